// KZG parameters from a KNOWN tau: halo2's `ParamsKZG::setup(k, rng)` restated for the device -- g = [tau^i]G,
// g_lagrange = [l_i(tau)]G, [tau]G2.  A known tau is toxic waste: whoever holds it forges openings.  This route is for tests, benches and
// development keys, as the reference's own `setup` is.  Held to the Python models (tests/setup_ref.py, tests/msm_ref.py, tests/pairing_ref.py);
// byte parity with upstream's ParamsKZG is not claimed.
//   fixed_base_table_kernel   T[w][d] = [d 256^w]B for w < 32, d < 256: the lane (w, d) forms d W_w from the window's base W_w = [256^w]B
//                             (32 affine points the host made with the curve functions below, handed over in the kernel arguments) by
//                             pt_mul_digit and stores it affine.  Entries are 64 bytes, x then y in the MONTGOMERY form of the coordinate
//                             field whatever the ctx's representation is -- the form pt_add_mixed takes, so the multiplication never
//                             converts an entry --, (0, 0) for d = 0 and for every entry of the identity's table.
//   fixed_base_mul_kernel     out[i] = [s_i]B: one lane per scalar walks the 32 bytes of the integer the scalar means from the bottom and adds
//                             T[w][byte w] (pt_add_affine: a zero byte is skipped), at most 32 mixed additions and NO doubling, then one
//                             conversion to affine.  The 32 windows cover all 256 bits: a canonical value >= r multiplies like its residue.
//   setup_scalars_kernel      the two scalar families halo2's setup feeds the multiplication, one lane per element: tau^i as the product of
//                             the squaring chain's entries at the bits of i; l_i(tau) = w^i (tau^n - 1) / (n (tau - w^i)) with w^i formed
//                             the same way and one fe_inv per lane (the host refuses tau^n = 1, so the difference is never zero).
// No workgroup waits for another, no atomics, no status; every loop has a fixed trip count (fe_inv's is capped), a table index is a window
// and a byte, so a table of garbage gives unspecified bytes and never a fault.  Launches are sliced by workgroups of 256 (block0).
// [k]Q on the twist (h2r_g2_mul) is host code: affine double-and-add over h2r_pairing.hpp's Fq2, every exceptional case spelled out.
// Host and device share every formula (H2R_FD): h2r_fixed_base_eval runs on the host exactly what the kernels inline.
#pragma once

#include "h2r_curve.hpp"
#include "h2r_pairing.hpp"

namespace h2r {

constexpr uint32_t FB_WINDOWS = 32, FB_DIGITS = 256, FB_ENTRY_BYTES = 64;
constexpr uint32_t FB_TABLE_BYTES = FB_WINDOWS * FB_DIGITS * FB_ENTRY_BYTES;   // 524,288
constexpr uint32_t FB_MAX_POINTS = 1u << 24;
constexpr uint32_t SETUP_MAX_LOG = 24;                                         // n <= 2^24: an index has 24 bits
constexpr uint32_t SETUP_POWERS = 0, SETUP_LAGRANGE = 1;

H2R_FD PtProj pt_from_affine(const PtAff &p, const CurveConsts &c) {
    PtProj r = pt_identity(c);
    if (!pt_aff_is_identity(p)) { r.x = p.x; r.y = p.y; r.z = fe_load_one(c.fq); }
    return r;
}
// entry d of the window whose base is wb = [256^w]B (affine, Montgomery form): d wb, affine
H2R_FD PtAff fb_table_entry(const PtAff &wb, uint32_t d, const CurveConsts &c) { return pt_to_affine(pt_mul_digit(pt_from_affine(wb, c), d, c), c); }
// [k]B over a table: `entry(w, d)` hands out T[w][d] for d != 0.  k is the canonical integer; its bytes are shifted out of the bottom word,
// so nothing is indexed by the window.
template <class Entry> H2R_FD PtProj fb_walk(const Fe &k, Entry &&entry, const CurveConsts &c) {
    uint64_t k0 = k.v[0], k1 = k.v[1], k2 = k.v[2], k3 = k.v[3];
    PtProj acc = pt_identity(c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t w = 0; w < FB_WINDOWS; ++w) {
        const uint32_t d = (uint32_t)k0 & 0xffu;
        if (d) acc = pt_add_affine(acc, entry(w, d), c);
        k0 = (k0 >> 8) | (k1 << 56); k1 = (k1 >> 8) | (k2 << 56); k2 = (k2 >> 8) | (k3 << 56); k3 >>= 8;
    }
    return acc;
}
// base^i for i < 2^SETUP_MAX_LOG out of the squaring chain pw[b] = base^(2^b), Montgomery form
H2R_FD Fe setup_chain_power(uint32_t i, const Fe *pw, const FieldConsts &f) {
    Fe acc = fe_load_one(f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t b = 0; b < SETUP_MAX_LOG; ++b)
        if ((i >> b) & 1u) acc = fe_mont_mul(acc, pw[b], f);
    return acc;
}
// l_i(tau) = w^i c / (tau - w^i) with c = (tau^n - 1) / n, everything in Montgomery form; tau is outside the domain
H2R_FD Fe setup_lagrange_value(const Fe &wi, const Fe &tau, const Fe &c, const FieldConsts &f) {
    const Fe den = fe_sub(tau, wi, f.p);
    const Fe inv = fe_to_mont(fe_inv(fe_from_mont(den, f), f), f);
    return fe_mont_mul(fe_mont_mul(wi, c, f), inv, f);
}

// ---- host: the window bases, a base's validation --------------------------------------------------------------------------------------------
// W_0 = B, W_(w+1) = [256]W_w (eight doublings), affine in Montgomery form
inline void fb_window_bases(const PtAff &b, PtAff *wb, const CurveConsts &c) {
    PtProj p = pt_from_affine(b, c);
    for (uint32_t w = 0; w < FB_WINDOWS; ++w) { wb[w] = pt_to_affine(p, c); p = pt_shift_window(p, c); }
}
// (x, y) in Montgomery form: the identity (0, 0) or a point of the curve
inline bool pt_aff_on_curve(const PtAff &p, const CurveConsts &c) {
    if (pt_aff_is_identity(p)) return true;
    const FieldConsts &f = c.fq;
    const Fe b = fe_mul_small(fe_load_one(f), c.b3 / 3u, f.p);
    return fe_eq(fe_mont_mul(p.y, p.y, f), fe_add(fe_mont_mul(fe_mont_mul(p.x, p.x, f), p.x, f), b, f.p));
}

// ---- host: G2 on the twist, affine --------------------------------------------------------------------------------------------------------
struct G2Aff { Fq2 x, y; bool inf; };
inline G2Aff g2_identity() { G2Aff r; r.x = fq2_zero(); r.y = fq2_zero(); r.inf = true; return r; }
inline G2Aff g2_double(const G2Aff &p, const FieldConsts &f) {
    if (p.inf || fq2_is_zero(p.y)) return g2_identity();
    const Fq2 x2 = fq2_square(p.x, f);
    const Fq2 lam = fq2_mul(fq2_add(fq2_add(x2, x2, f), x2, f), fq2_inv(fq2_add(p.y, p.y, f), f), f);
    G2Aff r; r.inf = false;
    r.x = fq2_sub(fq2_sub(fq2_square(lam, f), p.x, f), p.x, f);
    r.y = fq2_sub(fq2_mul(lam, fq2_sub(p.x, r.x, f), f), p.y, f);
    return r;
}
inline G2Aff g2_add(const G2Aff &p, const G2Aff &q, const FieldConsts &f) {
    if (p.inf) return q;
    if (q.inf) return p;
    if (fq2_eq(p.x, q.x)) return fq2_eq(p.y, q.y) ? g2_double(p, f) : g2_identity();
    const Fq2 lam = fq2_mul(fq2_sub(q.y, p.y, f), fq2_inv(fq2_sub(q.x, p.x, f), f), f);
    G2Aff r; r.inf = false;
    r.x = fq2_sub(fq2_sub(fq2_square(lam, f), p.x, f), q.x, f);
    r.y = fq2_sub(fq2_mul(lam, fq2_sub(p.x, r.x, f), f), p.y, f);
    return r;
}
// [k]Q for any 256-bit k, double-and-add from the top
inline G2Aff g2_mul(const G2Aff &q, const uint64_t k[4], const FieldConsts &f) {
    G2Aff acc = g2_identity();
    for (int bit = 255; bit >= 0; --bit) {
        acc = g2_double(acc, f);
        if ((k[bit >> 6] >> (bit & 63)) & 1ull) acc = g2_add(acc, q, f);
    }
    return acc;
}
// 128 bytes in c's representation <-> a point; all zero is the identity.  H2R_E_SHAPE for a coordinate >= q, H2R_E_ASSERTION off E'
inline uint32_t g2_load(const uint8_t *p, G2Aff *out, const PairingConsts &c) {
    if (!pr_in_range(p, 4, c)) return (uint32_t)H2R_E_SHAPE;
    out->x = pr_ld2(p, c); out->y = pr_ld2(p + 64, c);
    out->inf = fq2_is_zero(out->x) && fq2_is_zero(out->y);
    if (!out->inf && !fq2_eq(fq2_square(out->y, c.fq), fq2_add(fq2_mul(fq2_square(out->x, c.fq), out->x, c.fq), c.b2, c.fq))) return (uint32_t)H2R_E_ASSERTION;
    return 0u;
}
inline void g2_store(uint8_t *p, const G2Aff &q, const PairingConsts &c) {
    if (q.inf) { std::memset(p, 0, PR_G2_BYTES); return; }
    pr_st2(p, q.x, c); pr_st2(p + 64, q.y, c);
}
inline void g2_generator(uint8_t *p, const PairingConsts &c) {
    for (uint32_t j = 0; j < 4; ++j) pr_st(p + 32 * j, fe_to_mont(fe_words(PR_G2_GENERATOR[j]), c.fq), c);
}

// ---- the kernels' arguments -----------------------------------------------------------------------------------------------------------------
struct FixedBaseTableArgs {
    uint8_t *table;                 // [32][256] entries of 64 bytes
    uint32_t block0, pad_;
    PtAff wb[FB_WINDOWS];           // the windows' bases, Montgomery form
    CurveConsts cv;
};
struct FixedBaseMulArgs {
    const uint8_t *table;
    const uint8_t *scalars;         // [n][4] u64, the ctx's representation
    uint8_t *out;                   // [n][2][4] u64, likewise
    uint32_t n, mont, block0, pad_;
    FieldConsts fr;                 // the scalars' field (the ctx's)
    CurveConsts cv;
};
struct SetupScalarsArgs {
    uint8_t *out;                   // [n][4] u64, the ctx's representation
    uint32_t n, mode, mont, block0;
    Fe pw[SETUP_MAX_LOG];           // tau^(2^b) (POWERS) or omega^(2^b) (LAGRANGE), Montgomery form
    Fe tau, c;                      // LAGRANGE: tau and (tau^n - 1) / n, Montgomery form
    FieldConsts fr;
};

#ifdef H2R_TU_SETUP

// grid (the windows [a.block0, a.block0 + blocks)): workgroup = window, lane = digit
__global__ __launch_bounds__(256) void fixed_base_table_kernel(FixedBaseTableArgs a) {
    const uint32_t w = a.block0 + blockIdx.x, d = threadIdx.x;
    if (w >= FB_WINDOWS) return;
    // the window's base is uniform; held in scalar registers next to the curve's constants through pt_mul_digit it makes the compiler spill
    // scalar registers, so it is moved to vector registers here (an empty statement that only names the register class)
    PtAff wb = a.wb[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) { asm volatile("" : "+v"(wb.x.v[k])); asm volatile("" : "+v"(wb.y.v[k])); }
    const PtAff e = fb_table_entry(wb, d, a.cv);
    uint8_t *o = a.table + ((uint64_t)w * FB_DIGITS + d) * FB_ENTRY_BYTES;
    fe_store(o, e.x); fe_store(o + 32, e.y);
}

// grid (blocks of 256 over n scalars)
__global__ __launch_bounds__(256) void fixed_base_mul_kernel(FixedBaseMulArgs a) {
    const uint64_t i = ((uint64_t)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.n) return;
    Fe k = fe_load(a.scalars + i * 32);
    if (a.mont) k = fe_from_mont(k, a.fr);
    const PtProj acc = fb_walk(k, [&](uint32_t w, uint32_t d) __attribute__((always_inline)) {
        const uint8_t *e = a.table + ((uint64_t)w * FB_DIGITS + d) * FB_ENTRY_BYTES;
        PtAff q; q.x = fe_load(e); q.y = fe_load(e + 32);
        return q;
    }, a.cv);
    PtAff r = pt_to_affine(acc, a.cv);
    if (!a.mont) { r.x = fe_from_mont(r.x, a.cv.fq); r.y = fe_from_mont(r.y, a.cv.fq); }
    fe_store(a.out + i * 64, r.x); fe_store(a.out + i * 64 + 32, r.y);
}

// grid (blocks of 256 over n elements)
__global__ __launch_bounds__(256) void setup_scalars_kernel(SetupScalarsArgs a) {
    const uint64_t i = ((uint64_t)a.block0 + blockIdx.x) * 256 + threadIdx.x;
    if (i >= a.n) return;
    Fe v = setup_chain_power((uint32_t)i, a.pw, a.fr);
    if (a.mode == SETUP_LAGRANGE) v = setup_lagrange_value(v, a.tau, a.c, a.fr);
    if (!a.mont) v = fe_from_mont(v, a.fr);
    fe_store(a.out + i * 32, v);
}

#endif  // H2R_TU_SETUP

}  // namespace h2r
