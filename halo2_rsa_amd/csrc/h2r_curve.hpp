// Short Weierstrass curves y^2 = x^3 + b with a = 0 and PRIME order over a 4 x 64-bit Montgomery field (h2r_field.hpp), for the
// commitments (h2r_msm.hpp).  A curve enters the code only as its coordinate field's FieldConsts and the small integer 3 b; the one
// instance today is bn256 G1 (b = 3 over Fq, of order r = the modulus of H2R_FIELD_BN254_FR).  Host and device share every formula
// (H2R_FD): h2r_curve_eval runs on the host exactly what the kernels inline.
//
// Points are homogeneous projective (X : Y : Z), coordinates in the Montgomery form of the coordinate field, the identity (0 : 1 : 0).  The
// formulas are the COMPLETE ones of Renes, Costello and Batina, "Complete addition formulas for prime order elliptic curves" (Eurocrypt
// 2016) for a = 0: algorithm 7 (addition), 8 (mixed addition) and 9 (doubling).  On a curve of prime order they have no exceptional
// case: P + P, P + (-P) and the identity on either side run through the same straight-line code, which is what a bucket that meets its
// own contents needs.  The product by 3 b is a short chain of additions (b3 is 9 here), never a field product.
// An affine point is (x, y); (0, 0) stands for the identity, as halo2curves encodes it (restated, not pinned).  Algorithm 8 has no
// encoding of an affine identity: callers skip (0, 0) operands (pt_add_affine does).
#pragma once

#include "h2r_field.hpp"

namespace h2r {

struct CurveConsts {
    FieldConsts fq;    // the coordinate field
    uint32_t b3;       // 3 b
    uint32_t pad_;
};
struct PtProj { Fe x, y, z; };
struct PtAff { Fe x, y; };

H2R_FD Fe fe_load_one(const FieldConsts &f) { return fe_words(f.one); }
H2R_FD PtProj pt_identity(const CurveConsts &c) { PtProj r; r.x = fe_zero(); r.y = fe_load_one(c.fq); r.z = fe_zero(); return r; }
#if defined(__HIPCC__)
// device only: a projective point in memory is its three coordinates back to back (96 bytes on a 16-byte boundary)
__device__ __forceinline__ PtProj pt_load(const uint8_t *p) { PtProj r; r.x = fe_load(p); r.y = fe_load(p + 32); r.z = fe_load(p + 64); return r; }
__device__ __forceinline__ void pt_store(uint8_t *p, const PtProj &x) { fe_store(p, x.x); fe_store(p + 32, x.y); fe_store(p + 64, x.z); }
#endif
H2R_FD bool pt_aff_is_identity(const PtAff &p) { return fe_is_zero(p.x) && fe_is_zero(p.y); }
// 3 b * t with additions
H2R_FD Fe fe_mul_b3(const Fe &t, const CurveConsts &c) { return fe_mul_small(t, c.b3, c.fq.p); }

// RCB16 algorithm 7: complete addition, a = 0 (12 products)
H2R_FD PtProj pt_add(const PtProj &p, const PtProj &q, const CurveConsts &c) {
    const FieldConsts &f = c.fq;
    Fe t0 = fe_mont_mul(p.x, q.x, f), t1 = fe_mont_mul(p.y, q.y, f), t2 = fe_mont_mul(p.z, q.z, f);
    Fe t3 = fe_mont_mul(fe_add(p.x, p.y, f.p), fe_add(q.x, q.y, f.p), f);
    t3 = fe_sub(t3, fe_add(t0, t1, f.p), f.p);
    Fe t4 = fe_mont_mul(fe_add(p.y, p.z, f.p), fe_add(q.y, q.z, f.p), f);
    t4 = fe_sub(t4, fe_add(t1, t2, f.p), f.p);
    Fe y3 = fe_mont_mul(fe_add(p.x, p.z, f.p), fe_add(q.x, q.z, f.p), f);
    y3 = fe_sub(y3, fe_add(t0, t2, f.p), f.p);
    t0 = fe_add(fe_add(t0, t0, f.p), t0, f.p);
    t2 = fe_mul_b3(t2, c);
    Fe z3 = fe_add(t1, t2, f.p);
    t1 = fe_sub(t1, t2, f.p);
    y3 = fe_mul_b3(y3, c);
    PtProj r;
    r.x = fe_sub(fe_mont_mul(t3, t1, f), fe_mont_mul(t4, y3, f), f.p);
    r.y = fe_add(fe_mont_mul(t1, z3, f), fe_mont_mul(y3, t0, f), f.p);
    r.z = fe_add(fe_mont_mul(z3, t4, f), fe_mont_mul(t0, t3, f), f.p);
    return r;
}
// RCB16 algorithm 8: complete mixed addition, a = 0 (11 products); q is an affine point of the curve, NOT (0, 0)
H2R_FD PtProj pt_add_mixed(const PtProj &p, const PtAff &q, const CurveConsts &c) {
    const FieldConsts &f = c.fq;
    Fe t0 = fe_mont_mul(p.x, q.x, f), t1 = fe_mont_mul(p.y, q.y, f);
    Fe t3 = fe_mont_mul(fe_add(q.x, q.y, f.p), fe_add(p.x, p.y, f.p), f);
    t3 = fe_sub(t3, fe_add(t0, t1, f.p), f.p);
    Fe t4 = fe_add(fe_mont_mul(q.y, p.z, f), p.y, f.p);
    Fe y3 = fe_add(fe_mont_mul(q.x, p.z, f), p.x, f.p);
    t0 = fe_add(fe_add(t0, t0, f.p), t0, f.p);
    const Fe t2 = fe_mul_b3(p.z, c);
    Fe z3 = fe_add(t1, t2, f.p);
    t1 = fe_sub(t1, t2, f.p);
    y3 = fe_mul_b3(y3, c);
    PtProj r;
    r.x = fe_sub(fe_mont_mul(t3, t1, f), fe_mont_mul(t4, y3, f), f.p);
    r.y = fe_add(fe_mont_mul(t1, z3, f), fe_mont_mul(y3, t0, f), f.p);
    r.z = fe_add(fe_mont_mul(z3, t4, f), fe_mont_mul(t0, t3, f), f.p);
    return r;
}
// p + q for an affine q that may be (0, 0): the identity is skipped like a zero digit
H2R_FD PtProj pt_add_affine(const PtProj &p, const PtAff &q, const CurveConsts &c) { return pt_aff_is_identity(q) ? p : pt_add_mixed(p, q, c); }
// RCB16 algorithm 9: doubling, a = 0 (6 products and 2 squarings)
H2R_FD PtProj pt_double(const PtProj &p, const CurveConsts &c) {
    const FieldConsts &f = c.fq;
    Fe t0 = fe_mont_mul(p.y, p.y, f);
    Fe z3 = fe_add(t0, t0, f.p); z3 = fe_add(z3, z3, f.p); z3 = fe_add(z3, z3, f.p);
    Fe t1 = fe_mont_mul(p.y, p.z, f);
    Fe t2 = fe_mul_b3(fe_mont_mul(p.z, p.z, f), c);
    PtProj r;
    r.x = fe_mont_mul(t2, z3, f);
    Fe y3 = fe_add(t0, t2, f.p);
    r.z = fe_mont_mul(t1, z3, f);
    t2 = fe_add(fe_add(t2, t2, f.p), t2, f.p);
    t0 = fe_sub(t0, t2, f.p);
    r.y = fe_add(r.x, fe_mont_mul(t0, y3, f), f.p);
    t1 = fe_mont_mul(p.x, p.y, f);
    r.x = fe_mont_mul(t0, t1, f);
    r.x = fe_add(r.x, r.x, f.p);
    return r;
}
// d * p for a window digit d < 256: double-and-add from the top bit (what lane d of the bucket kernel runs on its bucket)
H2R_FD PtProj pt_mul_digit(const PtProj &p, uint32_t d, const CurveConsts &c) {
    PtProj acc = pt_identity(c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 7; bit >= 0; --bit) {
        acc = pt_double(acc, c);
        if ((d >> bit) & 1u) acc = pt_add(acc, p, c);
    }
    return acc;
}
// eight doublings: one window of the Horner over the windows
H2R_FD PtProj pt_shift_window(PtProj p, const CurveConsts &c) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 8; ++i) p = pt_double(p, c);
    return p;
}
// (X : Y : Z) -> (X / Z, Y / Z), Montgomery form in and out; Z = 0 goes to (0, 0) by a branch and never reaches fe_inv
H2R_FD PtAff pt_to_affine(const PtProj &p, const CurveConsts &c) {
    PtAff r;
    if (fe_is_zero(p.z)) { r.x = fe_zero(); r.y = fe_zero(); return r; }
    const Fe zi = fe_to_mont(fe_inv(fe_from_mont(p.z, c.fq), c.fq), c.fq);
    r.x = fe_mont_mul(p.x, zi, c.fq); r.y = fe_mont_mul(p.y, zi, c.fq);
    return r;
}

// Host: the curve of a ctx field (H2R_FIELD_*), or nullptr where the field has none.  A later curve is one more row.
struct CurveRow { uint32_t field; uint64_t q[4]; uint32_t b3; };
inline const CurveConsts *curve_of_field(uint32_t field) {
    static const CurveRow rows[] = {
        // bn256 G1: y^2 = x^3 + 3 over Fq, order r (field 0 = H2R_FIELD_BN254_FR: the ctx's p is the group order)
        {0u, {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull}, 9u},
    };
    static const struct Table {
        CurveConsts c[sizeof rows / sizeof rows[0]];
        Table() { for (size_t i = 0; i < sizeof rows / sizeof rows[0]; ++i) { field_consts_init(rows[i].q, &c[i].fq); c[i].b3 = rows[i].b3; c[i].pad_ = 0; } }
    } table;
    for (size_t i = 0; i < sizeof rows / sizeof rows[0]; ++i) if (rows[i].field == field) return &table.c[i];
    return nullptr;
}

}  // namespace h2r
