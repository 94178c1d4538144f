// The verifier of halo2's verify_proof (KZG, VerifierGWC, Blake2bRead) up to the pairing, for a batch of one-circuit proofs over the curve of
// the ctx's field (h2r_curve.hpp; today bn256 G1).  DESIGN.md section 2n.  A restatement, held to the Python model tests/verify_proof_ref.py
// and not pinned against upstream.  A proof is accepted iff e(L, [tau]G2) = e(R, G2) with
//     L = sum_p u^p W_p        R = sum_p u^p (z_p W_p + sum_i v^i C_{p,i} - [sum_i v^i e_{p,i}] G)
// over the point sets p = 0..3 at z_p = x, omega x, omega^-(bf+1) x, omega^-1 x; G2 and the pairing are the caller's.  Three kernels:
//   proof_decode_kernel     the proof's 32-byte items -> affine points (64 bytes) and scalars (32 bytes) in the ctx's representation.  One lane
//                           per (circuit, item), 64 circuits per workgroup, the item on grid.y: every lane of a workgroup decodes the same
//                           kind.  A point is x with bit 255 cleared, y = (x^3 + b)^((q+1)/4), checked by y^2 = x^3 + b, its sign by bit
//                           255; the exponent is a kernel argument walked bit by bit (uniform control flow, no table).  TWO launches: pass 0
//                           flags a scalar >= r or an abscissa >= q with H2R_E_SHAPE and writes nothing else, pass 1 skips every circuit
//                           that has a status and flags an abscissa of no point with H2R_E_ASSERTION.  So H2R_E_SHAPE WINS wherever in a
//                           proof the two occur, whatever the order in which lanes run; several lanes may store the same byte.
//   verify_scalars_kernel   the verifier's field side, one lane per circuit, 64 circuits per workgroup (the transcript kernel's geometry):
//                           l0(x), l_last(x), l_active(x) in closed form (the bf + 2 differences x - omega^i and x^n - 1 inverted by
//                           Montgomery's trick around ONE fe_inv, the prefix products in the lane's LDS column), the constraint expression
//                           at x folded with y -- constraint_fold (h2r_constraints.hpp: THE definition of the terms and their order, shared
//                           with the quotient kernel) over a source that reads evaluations instead of columns --, the expected h(x), and
//                           then one scalar per base of R and the four scalars u^p of L.
//   msm_terms_kernel        out[e] = sum_{t<T} s[e][t] P[e][t] for bases that differ per circuit: one workgroup of 256 per circuit, lane l
//                           takes the terms l, l + 256, ... (pt_mul_window2: any 256-bit scalar, a trip count that no scalar changes), the
//                           workgroup sums over LDS with the complete addition, lane 0 stores the affine sum, (0, 0) for the identity.
// THE BASE ORDER of R's scalars (h2r_verify_scalars' `right`, h2r_msm_terms' bases): the proof's points in proof order -- 5 advice, A' and S'
// interleaved per lookup argument, the S permutation Z, the A lookup Z, the random polynomial, the 4 pieces of h, W_0..W_3 -- then the key's F
// fixed and m sigma commitments, then G: 5 + 3A + S + 9 + F + m + 1 bases.  A commitment's scalar sums u^p v^i over its queries (i counts the
// queries of point set p in the open plan's order from 0), a piece j of h gets its query's times x^(n j), W_p gets u^p z_p, G minus the sum of
// u^p v^i e_{p,i}.
// No kernel waits for another workgroup, none uses atomics, no loop's trip count depends on a proof's bytes except fe_inv's.  Host and device
// share every formula (H2R_FD): h2r_verify_eval runs on the host exactly what the kernels inline.
#pragma once

#include <cstring>

#include "h2r_constraints.hpp"
#include "h2r_curve_ntt.hpp"
#include "h2r_transcript.hpp"

namespace h2r {

constexpr u32 VF_POINT = 1, VF_SCALAR = 2;          // a section's kind (= TR_POINT, TR_SCALAR)
constexpr u32 VF_MAX_SECTIONS = 16, VF_MAX_ITEMS = 1u << 16;
constexpr u32 VF_LANES = 64;                        // circuits of a decode / scalars workgroup: one wavefront
constexpr u32 VF_MAX_PLAN = 64;                     // entries of a plan
constexpr u32 VF_MAX_INDEX = 16;                    // columns of a group
constexpr u32 VF_MAX_BF = 13, VF_MAX_INV = VF_MAX_BF + 3;   // blinding factors; values inverted together
constexpr u32 VF_H_PIECES = 4, VF_POINT_SETS = ROTATIONS;   // point set p = x under rotation p (ROT_*: the bits of a plan mask)
constexpr u32 VF_MAX_TERMS = 4096, VF_TERM_LANES = 256;
// the groups of a plan entry
constexpr u32 VF_G_ADVICE = 0, VF_G_FIXED = 1, VF_G_RANDOM = 2, VF_G_SIGMA = 3, VF_G_PERM_Z = 4, VF_G_LOOKUP_Z = 5, VF_G_LOOKUP_A = 6, VF_G_LOOKUP_S = 7,
              VF_G_H = 8, VF_GROUPS = 9;

// 32 bytes of host or device memory <-> an element (device: two 16-byte accesses, as fe_load / fe_store)
H2R_FD Fe vf_ld(const u8 *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fe_load(p);
#else
    Fe r; std::memcpy(r.v, p, 32); return r;
#endif
}
H2R_FD void vf_st(u8 *p, const Fe &x) {
#if defined(__HIP_DEVICE_COMPILE__)
    fe_store(p, x);
#else
    std::memcpy(p, x.v, 32);
#endif
}

// ---- the decoder ----------------------------------------------------------------------------------------------------------------------------
// a^e for an exponent every lane shares (a kernel argument), Montgomery form in and out: 256 squarings, a product per set bit
H2R_FD Fe vf_pow_shared(const Fe &a, const u64 (&e)[4], const FieldConsts &f) {
    u64 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
    Fe acc = fe_words(f.one);
    H2R_ROLLED
    for (int bit = 0; bit < 256; ++bit) {
        acc = fe_mont_mul(acc, acc, f);
        if (e3 >> 63) acc = fe_mont_mul(acc, a, f);
        e3 = (e3 << 1) | (e2 >> 63); e2 = (e2 << 1) | (e1 >> 63); e1 = (e1 << 1) | (e0 >> 63); e0 <<= 1;
    }
    return acc;
}
// pass 0: the range of an item's 32 bytes
H2R_FD u32 vf_item_range(u32 kind, Fe raw, const TrConsts &c) {
    if (kind == VF_POINT) { raw.v[3] &= ~(1ull << 63); return ge_p(raw.v, c.fq.p) ? (u32)H2R_E_SHAPE : 0u; }
    return ge_p(raw.v, c.fr.p) ? (u32)H2R_E_SHAPE : 0u;
}
// pass 1 for a scalar in range: the ctx's representation
H2R_FD Fe vf_decode_scalar(const Fe &raw, const TrConsts &c) { return c.mont ? fe_to_mont(raw, c.fr) : raw; }
// pass 1 for a point whose abscissa is in range: 0 and (x, y) in the ctx's representation, or H2R_E_ASSERTION; sqrt_exp = (q + 1) / 4, b3 = 3 b
H2R_FD u32 vf_decode_point(Fe raw, const u64 (&sqrt_exp)[4], u32 b3, const TrConsts &c, Fe &x_out, Fe &y_out) {
    const u64 sign = raw.v[3] >> 63;
    raw.v[3] &= ~(1ull << 63);
    const FieldConsts &f = c.fq;
    const Fe xm = fe_to_mont(raw, f);
    // b in Montgomery form: 3 b * 3^-1 is not at hand, but b = b3 / 3 is a small integer
    const Fe rhs = fe_add(fe_mont_mul(fe_mont_mul(xm, xm, f), xm, f), fe_mul_small(fe_words(f.one), b3 / 3u, f.p), f.p);
    Fe ym = vf_pow_shared(rhs, sqrt_exp, f);
    if (!fe_eq(fe_mont_mul(ym, ym, f), rhs)) return (u32)H2R_E_ASSERTION;
    Fe yc = fe_from_mont(ym, f);
    if ((yc.v[0] & 1ull) != sign) { yc = fe_sub(fe_zero(), yc, f.p); ym = fe_sub(fe_zero(), ym, f.p); }
    x_out = c.mont ? xm : raw; y_out = c.mont ? ym : yc;
    return 0u;
}

struct DecodeArgs {
    const u8 *proof; u64 proof_stride;              // circuit e reads proof + e * proof_stride
    u8 *points; u64 points_stride;                  // [batch][num_points][64]
    u8 *scalars; u64 scalars_stride;                // [batch][num_scalars][32]
    u8 *status;                                     // nullable, never cleared
    u64 batch;
    u32 num_sections, num_items, pass, block0;
    u32 sec_end[VF_MAX_SECTIONS];                   // one past the section's last item
    u32 sec_out[VF_MAX_SECTIONS];                   // the section's first entry among the points / the scalars
    u8 sec_kind[VF_MAX_SECTIONS];
    u64 sqrt_exp[4];
    u32 b3, pad_;
    TrConsts c;
};

// ---- the scalars --------------------------------------------------------------------------------------------------------------------------
struct VfPlanEntry { u8 group, index, mask, pad_; };
struct VfStore { Fe *w; u32 stride; };             // element i at w[i * stride]: an array on the host, the lane's LDS column on the device
struct VerifyScalarsArgs {
    const u8 *evals; u64 evals_stride;              // [batch][num_evals][32], the ctx's representation
    const u64 *ch[7];                               // theta, beta, gamma, y, x, v, u: [batch][4], the ctx's representation
    u8 *right; u64 right_stride;                    // [batch][num_bases][32]
    u8 *left;                                       // [batch][4][32]
    u8 *status;                                     // nullable, never cleared
    u64 batch;
    u32 block0, mont, log_n, bf, num_open, num_bases, w_pos, g_pos;
    ConstraintShape cs;
    unsigned short ev_first[VF_GROUPS][VF_MAX_INDEX];   // a column's first evaluation
    u8 ev_mask[VF_GROUPS][VF_MAX_INDEX];                // ... and the point sets it is evaluated at (the eval plan)
    unsigned short base_pos[VF_GROUPS][VF_MAX_INDEX];   // a column's commitment among the bases (group h: its piece 0)
    VfPlanEntry open[VF_MAX_PLAN];
    Fe zmul[VF_POINT_SETS];                         // 1, omega, omega^-(bf+1), omega^-1: Montgomery form
    Fe ninv;                                        // 1 / n, Montgomery form
    FieldConsts f;
};

H2R_FD u32 vf_popc(u32 x) { u32 n = 0; for (; x; x &= x - 1) ++n; return n; }

// constraint_fold's column reads under the verifier's names: E(group, index, point set).  B answers E and the rest of a source.
template <class B> struct VfColumns : B {
    H2R_FD Fe adv(u32 c, u32 rot) const { return this->E(VF_G_ADVICE, c, rot); }
    H2R_FD Fe fix(u32 c) const { return this->E(VF_G_FIXED, c, ROT_CUR); }
    H2R_FD Fe sigma(u32 c) const { return this->E(VF_G_SIGMA, c, ROT_CUR); }
    H2R_FD Fe perm_value(u32 src) const { return adv(src, ROT_CUR); }   // (the verifier has no extra columns)
    H2R_FD Fe perm_z(u32 s, u32 rot) const { return this->E(VF_G_PERM_Z, s, rot); }
    H2R_FD Fe look_z(u32 k, u32 rot) const { return this->E(VF_G_LOOKUP_Z, k, rot); }
    H2R_FD Fe a_perm(u32 k, u32 rot) const { return this->E(VF_G_LOOKUP_A, k, rot); }
    H2R_FD Fe s_perm(u32 k) const { return this->E(VF_G_LOOKUP_S, k, ROT_CUR); }
};
// one circuit's evaluations (Montgomery form on the way out), its challenges, l0 / l_last / l_active at x and beta x
struct VfEvals : ConstraintField {
    const VerifyScalarsArgs &a; const u8 *ev;
    const Fe &theta_, &beta_, &gamma_, &y_, &bx; const Fe (&lag)[3];
    H2R_FD Fe E(u32 g, u32 i, u32 p) const {
        const u32 at = (u32)a.ev_first[g][i] + vf_popc((u32)a.ev_mask[g][i] & ((1u << p) - 1u));
        const Fe r = vf_ld(ev + (u64)at * 32);
        return a.mont ? r : fe_to_mont(r, f);
    }
    H2R_FD Fe l(u32 i) const { return lag[i]; }
    H2R_FD Fe ident(u32 c) const { return mul(a.cs.dpow[c], bx); }
    H2R_FD const Fe &theta() const { return theta_; }
    H2R_FD const Fe &beta() const { return beta_; }
    H2R_FD const Fe &gamma() const { return gamma_; }
    H2R_FD const Fe &y() const { return y_; }
};

// The scalars of one circuit.  ev: its evaluations, right / left: its outputs, tmp: VF_MAX_INV elements of the lane's own.  0, H2R_E_SHAPE for
// a challenge that is not canonical (nothing written), H2R_E_ASSERTION for x^n = 1 (nothing written).
H2R_FD u32 vf_scalars(const VerifyScalarsArgs &a, u64 e, const u8 *ev, u8 *right, u8 *left, const VfStore &tmp) {
    const FieldConsts &f = a.f;
    Fe theta, beta, gamma, y, x, v, u;
    {
        u32 bad = 0;
        auto take = [&](u32 k) __attribute__((always_inline)) {
            const Fe c = fe_words(a.ch[k] + e * 4);
            if (ge_p(c.v, f.p)) bad = 1u;
            return a.mont ? c : fe_to_mont(c, f);
        };
        theta = take(0); beta = take(1); gamma = take(2); y = take(3); x = take(4); v = take(5); u = take(6);
        if (bad) return (u32)H2R_E_SHAPE;
    }
    auto mul = [&](const Fe &p, const Fe &q) __attribute__((always_inline)) { return fe_mont_mul(p, q, f); };
    auto add = [&](const Fe &p, const Fe &q) __attribute__((always_inline)) { return fe_add(p, q, f.p); };
    auto sub = [&](const Fe &p, const Fe &q) __attribute__((always_inline)) { return fe_sub(p, q, f.p); };
    auto inv = [&](const Fe &p) __attribute__((always_inline)) { return fe_to_mont(fe_inv(fe_from_mont(p, f), f), f); };
    const Fe one = fe_words(f.one);
    Fe xn = x;
    H2R_ROLLED
    for (u32 l = 0; l < a.log_n; ++l) xn = mul(xn, xn);
    if (fe_eq(xn, one)) return (u32)H2R_E_ASSERTION;

    // ---- l0, l_last, l_active and 1 / (x^n - 1): t_0 = x^n - 1, t_1 = x - 1, t_(2+j) = x - omega^(u+j) for j <= bf (u + bf = n - 1) ----
    Fe lag[3], xn1_inv;                                                // l0, l_last, l_active at x
    {
        const u32 K = a.bf + 3;
        const Fe xn1 = sub(xn, one);
        Fe pr = xn1, w = a.zmul[ROT_LAST];                            // omega^u = omega^-(bf+1)
        tmp.w[0] = pr;
        pr = mul(pr, sub(x, one)); tmp.w[tmp.stride] = pr;
        H2R_ROLLED
        for (u32 j = 2; j < K; ++j) { pr = mul(pr, sub(x, w)); tmp.w[j * tmp.stride] = pr; w = mul(w, a.zmul[ROT_NEXT]); }
        Fe all = inv(pr);                                              // every factor is nonzero: x^n != 1
        const Fe zn = mul(xn1, a.ninv);
        Fe blind = fe_zero();
        w = a.zmul[ROT_PREV];                                         // omega^(n-1), then down to omega^u
        lag[1] = fe_zero();
        H2R_ROLLED
        for (u32 j = K - 1; j >= 2; --j) {
            const Fe t = sub(x, w), ti = mul(all, tmp.w[(j - 1) * tmp.stride]);
            all = mul(all, t);
            const Fe l = mul(mul(zn, w), ti);
            if (j == 2) lag[1] = l; else blind = add(blind, l);
            w = mul(w, a.zmul[ROT_PREV]);
        }
        lag[0] = mul(zn, mul(all, tmp.w[0]));                              // t_1's inverse
        xn1_inv = mul(all, sub(x, one));                               // t_0's
        lag[2] = sub(sub(one, lag[1]), blind);
    }

    const Fe bx = mul(beta, x);
    const VfColumns<VfEvals> src{{{f}, a, ev, theta, beta, gamma, y, bx, lag}};
    const Fe eh = mul(constraint_fold(a.cs, src), xn1_inv);            // the expected h(x): the constraint expression at x, folded with y

    // ---- the scalars: sums in the ctx's representation, in this circuit's own row ----
    auto repr = [&](const Fe &p) __attribute__((always_inline)) { return a.mont ? p : fe_from_mont(p, f); };
    auto bump = [&](u32 pos, const Fe &c) __attribute__((always_inline)) { u8 *o = right + (u64)pos * 32; vf_st(o, add(vf_ld(o), repr(c))); };
    H2R_ROLLED
    for (u32 i = 0; i < a.num_bases; ++i) vf_st(right + (u64)i * 32, fe_zero());
    Fe up = one, gsum = fe_zero();
    H2R_ROLLED
    for (u32 p = 0; p < VF_POINT_SETS; ++p) {
        Fe vp = one, esum = fe_zero();
        H2R_ROLLED
        for (u32 j = 0; j < a.num_open; ++j) {
            const VfPlanEntry q = a.open[j];
            if (!((q.mask >> p) & 1u)) continue;
            Fe coeff = mul(up, vp), val;
            const u32 pos = a.base_pos[q.group][q.index];
            if (q.group == VF_G_H) {
                val = eh;
                H2R_ROLLED
                for (u32 piece = 0; piece < VF_H_PIECES; ++piece) { bump(pos + piece, coeff); coeff = mul(coeff, xn); }
            } else {
                val = src.E(q.group, q.index, p);
                bump(pos, coeff);
            }
            esum = add(esum, mul(vp, val));
            vp = mul(vp, v);
        }
        vf_st(right + (u64)(a.w_pos + p) * 32, repr(mul(up, mul(x, a.zmul[p]))));
        gsum = add(gsum, mul(up, esum));
        vf_st(left + (u64)p * 32, repr(up));
        up = mul(up, u);
    }
    vf_st(right + (u64)a.g_pos * 32, repr(sub(fe_zero(), gsum)));
    return 0u;
}

// ---- the sum of terms -----------------------------------------------------------------------------------------------------------------------
struct MsmTermsArgs {
    const u8 *scalars; u64 s_elem_stride;           // [T][32] per circuit, or one copy (stride 0)
    const u8 *bases; u64 b_elem_stride;             // [T][64] likewise
    u8 *out;                                        // [batch][64]
    u8 *status;                                     // nullable, never cleared
    u32 T, elem0, mont, pad_;
    FieldConsts fr;
    CurveConsts cv;
};
// s * P of one term as it lies in memory (the ctx's representation); (0, 0) is the identity
H2R_FD PtProj vf_term(const u8 *s, const u8 *b, u32 mont, const FieldConsts &fr, const CurveConsts &cv) {
    Fe k = vf_ld(s);
    if (mont) k = fe_from_mont(k, fr);
    PtProj p;
    p.x = vf_ld(b); p.y = vf_ld(b + 32);
    if (fe_is_zero(p.x) && fe_is_zero(p.y)) p = pt_identity(cv);
    else {
        if (!mont) { p.x = fe_to_mont(p.x, cv.fq); p.y = fe_to_mont(p.y, cv.fq); }
        p.z = fe_load_one(cv.fq);
    }
    return pt_mul_window2(p, k.v, cv);
}
// the sum as it is stored
H2R_FD void vf_store_sum(u8 *o, const PtProj &acc, u32 mont, const CurveConsts &cv) {
    PtAff r = pt_to_affine(acc, cv);
    if (!mont) { r.x = fe_from_mont(r.x, cv.fq); r.y = fe_from_mont(r.y, cv.fq); }
    vf_st(o, r.x); vf_st(o + 32, r.y);
}

#ifdef H2R_TU_VERIFY

// grid (workgroups of 64 circuits of one launch, items), 64 lanes
__global__ __launch_bounds__(VF_LANES) void proof_decode_kernel(DecodeArgs a) {
    const u64 e = ((u64)a.block0 + blockIdx.x) * VF_LANES + threadIdx.x;
    const u32 item = blockIdx.y;
    if (e >= a.batch || item >= a.num_items) return;
    if (a.status && a.status[e]) return;                  // flagged on entry, or by pass 0: nothing is written
    u32 s = 0;
#pragma unroll 1
    while (s + 1 < a.num_sections && item >= a.sec_end[s]) ++s;
    const u32 kind = a.sec_kind[s], k = a.sec_out[s] + item - (s ? a.sec_end[s - 1] : 0u);
    const Fe raw = fe_load(a.proof + e * a.proof_stride + (u64)item * 32);
    if (a.pass == 0) {
        if (vf_item_range(kind, raw, a.c) && a.status) a.status[e] = (u8)H2R_E_SHAPE;
        return;
    }
    if (vf_item_range(kind, raw, a.c)) return;            // (no status array: the item is left out)
    if (kind == VF_SCALAR) { fe_store(a.scalars + e * a.scalars_stride + (u64)k * 32, vf_decode_scalar(raw, a.c)); return; }
    Fe x, y;
    if (vf_decode_point(raw, a.sqrt_exp, a.b3, a.c, x, y)) { if (a.status) a.status[e] = (u8)H2R_E_ASSERTION; return; }
    u8 *o = a.points + e * a.points_stride + (u64)k * 64;
    fe_store(o, x); fe_store(o + 32, y);
}

// grid (workgroups of 64 circuits of one launch), 64 lanes
__global__ __launch_bounds__(VF_LANES) void verify_scalars_kernel(VerifyScalarsArgs a) {
    __shared__ Fe tile[VF_MAX_INV * VF_LANES];             // element i of lane l at tile[i * 64 + l]
    const u64 e = ((u64)a.block0 + blockIdx.x) * VF_LANES + threadIdx.x;
    if (e >= a.batch) return;
    if (a.status && a.status[e]) return;
    const VfStore tmp{tile + threadIdx.x, VF_LANES};
    const u32 bad = vf_scalars(a, e, a.evals + e * a.evals_stride, a.right + e * a.right_stride, a.left + e * 128, tmp);
    if (bad && a.status) a.status[e] = (u8)bad;
}

// grid (circuits of one launch), 256 lanes
__global__ __launch_bounds__(VF_TERM_LANES) void msm_terms_kernel(MsmTermsArgs a) {
    __shared__ __align__(16) u8 sh[VF_TERM_LANES * CNTT_POINT_BYTES];
    const u32 tid = threadIdx.x;
    const u64 e = (u64)a.elem0 + blockIdx.x;
    if (a.status && a.status[e]) return;                  // the whole workgroup: nothing is written
    const u8 *s = a.scalars + e * a.s_elem_stride, *b = a.bases + e * a.b_elem_stride;
    PtProj acc = pt_identity(a.cv);
#pragma unroll 1
    for (u32 t = tid; t < a.T; t += VF_TERM_LANES) acc = pt_add(acc, vf_term(s + (u64)t * 32, b + (u64)t * 64, a.mont, a.fr, a.cv), a.cv);
    pt_store(sh + tid * CNTT_POINT_BYTES, acc);
    __syncthreads();
#pragma unroll 1
    for (u32 h = VF_TERM_LANES / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            acc = pt_add(acc, pt_load(sh + (tid + h) * CNTT_POINT_BYTES), a.cv);
            pt_store(sh + tid * CNTT_POINT_BYTES, acc);
        }
        __syncthreads();
    }
    if (tid == 0) vf_store_sum(a.out + e * 64, acc, a.mont, a.cv);
}

#endif  // H2R_TU_VERIFY

}  // namespace h2r
