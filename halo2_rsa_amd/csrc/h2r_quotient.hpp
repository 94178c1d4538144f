// The vanishing argument's quotient h on the extended domain: halo2's plonk::evaluation::evaluate_h for THIS circuit's constraint system (the
// one main gate, up to PERM_MAX_COLUMNS permutation columns in sets, the five lookup arguments), not a general expression evaluator.
// Third-party behaviour (halo2, not in the reference tree), restated in DESIGN.md section 2g; parity is pinned against a Python restatement
// (tests/quotient_ref.py, tests/test_quotient_gpu.py), not against upstream.  With n = 2^log_n, N = 2^log_ext, r = N / n,
// X_j = zeta * omega_ext^j the point of index j < N (natural order) and f<t>[j] = f[(j + t * r) mod N] the rotation of a column by t rows,
// acc starts at 0 and every term t does acc = acc * y + t, in this order (upstream's; part of the contract):
//   gate         sum_{i<5} s_i v_i + s_mul_ab v_0 v_1 + s_mul_cd v_2 v_3 + se_next v_4<+1> + s_const
//   permutation  l0 (1 - Z_0);  l_last (Z_{S-1}^2 - Z_{S-1});  for s = 1 .. S-1: l0 (Z_s - Z_{s-1}<-(blinding_factors + 1)>);
//                for s = 0 .. S-1: l_active (Z_s<+1> prod_{c in s} (v_c + beta sigma_c + gamma) - Z_s prod_{c in s} (v_c + delta^c beta X_j + gamma))
//   lookup k     (ascending over the selected arguments) with A_k = theta fixed[tag_k] + fixed[enable_k] v_(advice_k),
//                S = theta fixed[table_tag] + fixed[table_value]:
//                l0 (1 - Z_k);  l_last (Z_k^2 - Z_k);  l_active (Z_k<+1> (A'_k + beta)(S'_k + gamma) - Z_k (A_k + beta)(S + gamma));
//                l0 (A'_k - S'_k);  l_active (A'_k - S'_k)(A'_k - A'_k<-1>)
//   h[j] = acc / (X_j^n - 1); X_j^n takes r values, zeta^n * (omega_ext^n)^(j mod r), which the host inverts (fe_inv) into the arguments.
// One pointwise kernel: no workgroup waits for another, no workspace.  A workgroup of 256 threads takes QUOT_TILE consecutive points, a thread
// the QUOT_LANE_POINTS points tid + 256 q of them (adjacent lanes on adjacent elements in every load, rotated ones included: a rotation
// shifts a whole run); X_j of the first is built from the set bits of j (host passes omega_ext^(2^b)), the next ones by a product with
// omega_ext^256, as perm_product's omega^i.  beta * delta^c and the four challenges sit in LDS, computed once per workgroup.  Rotated reads are
// plain global reads at (j +- t r) mod N: N is a power of two, so the wrap at both ends of a column is one AND.  The terms are folded into acc
// as they are formed (Horner), so a handful of elements are live at any time.  The grid is (circuits, tiles): the workgroups of one tile of
// every circuit are dispatched next to each other, so the key columns' lines (shared by the circuits) have a chance of being found in L2.
// All arithmetic is in the Montgomery domain (fe_mont_mul / fe_add / fe_sub); a canonical ctx converts on load, and on the store inside the
// product with 1 / (X_j^n - 1) (the host passes that factor as a plain integer then); every result is the canonical representative.
// The kernel is defined in the one translation unit that launches it (h2r_tu_quotient.hip, H2R_TU_QUOTIENT).
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 QUOT_LANE_POINTS = 4;                 // points of a thread, 256 apart
constexpr u32 QUOT_TILE = 256 * QUOT_LANE_POINTS;   // points of a workgroup
constexpr u32 QUOT_STEP_BIT = 8;                    // a thread steps X_j by omega_ext^(2^8)
constexpr u32 QUOT_MAX_LOG = 24;
constexpr u32 QUOT_MAX_SCALE_LOG = 4;               // log_ext - log_n
constexpr u32 QUOT_MAX_FIXED = 16;
constexpr u32 QUOT_LOOKUP_ARGS = 5;
constexpr u32 QUOT_PERM_MAX_COLUMNS = 8;
constexpr u32 QUOT_GATE_FIXED = 9;                  // sa, sb, sc, sd, se, s_mul_ab, s_mul_cd, se_next, s_const

struct QuotCols { const u8 *base; u64 elem_stride, col_stride; };   // column c of circuit e at base + e * elem_stride + c * col_stride

struct QuotientArgs {
    QuotCols advice, extra, perm_z, a_perm, s_perm, look_z;   // per circuit
    QuotCols fixed, sigma, l;                                 // the proving key's: elem_stride = 0.  l: l0, l_last, l_active
    const u64 *theta, *beta, *gamma, *y;                      // [circuit][4], the ctx's representation
    u8 *status;                                               // nullable, never cleared
    u8 *h; u64 h_elem_stride;
    u32 log_ext, scale_log, mont, tile0;
    u32 last_rot;                                             // blinding_factors + 1
    u32 m, chunk_len, n_sets, lookup_mask;
    u8 gate_fixed[QUOT_GATE_FIXED], src[QUOT_PERM_MAX_COLUMNS];
    u8 lookup_advice[QUOT_LOOKUP_ARGS], lookup_tag[QUOT_LOOKUP_ARGS], lookup_enable[QUOT_LOOKUP_ARGS], table_tag, table_value;
    Fe dpow[QUOT_PERM_MAX_COLUMNS];                           // delta^c, Montgomery form
    Fe wpow[QUOT_MAX_LOG];                                    // omega_ext^(2^b), Montgomery form
    Fe zeta;                                                  // Montgomery form
    Fe xinv[1u << QUOT_MAX_SCALE_LOG];                        // 1 / (zeta^n (omega_ext^n)^i - 1): Montgomery form (a canonical ctx: the plain integer)
    FieldConsts f;
};

__host__ __device__ inline u32 quotient_tiles(u32 log_ext) { return (u32)(((1ull << log_ext) + QUOT_TILE - 1) / QUOT_TILE); }

#ifdef H2R_TU_QUOTIENT

// element j of a column in Montgomery form
__device__ __forceinline__ Fe quot_at(const u8 *col, u32 j, const QuotientArgs &a) { return fe_load_mont(col + (u64)j * 32, a.mont, a.f); }

// grid (circuits, tiles of one launch): the circuits of a tile next to each other
__global__ __launch_bounds__(256) void quotient_kernel(QuotientArgs a) {
    __shared__ Fe ch[4];                          // theta, beta, gamma, y: Montgomery form
    __shared__ Fe bl[QUOT_PERM_MAX_COLUMNS];      // beta * delta^c
    __shared__ u32 state;                         // 0: go, 1: skipped or refused
    const u32 tid = threadIdx.x, tile = a.tile0 + blockIdx.y;
    const u64 elem = blockIdx.x;
    if (tid == 0) {
        u32 st = a.status && a.status[elem] ? 1u : 0u;
        if (!st) {
            auto take = [&](const u64 *w, u32 k) __attribute__((always_inline)) {
                const Fe c = fe_words(w + elem * 4);
                if (ge_p(c.v, a.f.p)) st = 1u;
                else ch[k] = a.mont ? c : fe_to_mont(c, a.f);
            };
            take(a.theta, 0); take(a.beta, 1); take(a.gamma, 2); take(a.y, 3);
            if (st && a.status && tile == 0) a.status[elem] = (u8)H2R_E_SHAPE;   // not a canonical challenge: nothing is written for this circuit
        }
        state = st;
    }
    __syncthreads();
    if (state) return;
    if (tid < QUOT_PERM_MAX_COLUMNS) bl[tid] = tid < a.m ? fe_mont_mul(ch[1], a.dpow[tid], a.f) : fe_zero();
    __syncthreads();

    const u32 N = 1u << a.log_ext, mask = N - 1, r = 1u << a.scale_log;
    u32 j = tile * QUOT_TILE + tid;
    if (j >= N) return;
    Fe X = a.zeta;                                // X_j = zeta * omega_ext^j from the set bits of j
    for (u32 b = 0; b < a.log_ext; ++b)
        if ((j >> b) & 1u) X = fe_mont_mul(X, a.wpow[b], a.f);
    const Fe one = fe_words(a.f.one);
    const u8 *adv_e = a.advice.base + elem * a.advice.elem_stride, *ext_e = a.extra.base + elem * a.extra.elem_stride;
    const u8 *pz_e = a.perm_z.base + elem * a.perm_z.elem_stride;
    const u8 *ap_e = a.a_perm.base + elem * a.a_perm.elem_stride, *sp_e = a.s_perm.base + elem * a.s_perm.elem_stride;
    const u8 *lz_e = a.look_z.base + elem * a.look_z.elem_stride;
    u8 *h_e = a.h + elem * a.h_elem_stride;

#pragma unroll 1
    for (u32 q = 0; q < QUOT_LANE_POINTS && j < N; ++q, j += 256) {
        const u32 j_next = (j + r) & mask, j_prev = (j - r) & mask, j_last = (j - a.last_rot * r) & mask;
        auto adv = [&](u32 c, u32 jj) __attribute__((always_inline)) { return quot_at(adv_e + (u64)c * a.advice.col_stride, jj, a); };
        auto fix = [&](u32 c) __attribute__((always_inline)) { return quot_at(a.fixed.base + (u64)c * a.fixed.col_stride, j, a); };
        auto mul = [&](const Fe &x, const Fe &w) __attribute__((always_inline)) { return fe_mont_mul(x, w, a.f); };
        auto add = [&](const Fe &x, const Fe &w) __attribute__((always_inline)) { return fe_add(x, w, a.f.p); };
        auto sub = [&](const Fe &x, const Fe &w) __attribute__((always_inline)) { return fe_sub(x, w, a.f.p); };
        // ---- the gate (the first term: acc = 0 * y + gate) ----
        Fe acc;
        {
            acc = fe_zero();
#pragma unroll 1
            for (u32 pr = 0; pr < 2; ++pr) {   // (v_0, v_1) under sa, sb, s_mul_ab, then (v_2, v_3) under sc, sd, s_mul_cd
                const Fe va = adv(2 * pr, j), vb = adv(2 * pr + 1, j);
                acc = add(acc, add(mul(fix(a.gate_fixed[2 * pr]), va), mul(fix(a.gate_fixed[2 * pr + 1]), vb)));
                acc = add(acc, mul(fix(a.gate_fixed[5 + pr]), mul(va, vb)));
            }
            acc = add(acc, mul(fix(a.gate_fixed[4]), adv(4, j)));
            acc = add(acc, mul(fix(a.gate_fixed[7]), adv(4, j_next)));
            acc = add(acc, fix(a.gate_fixed[8]));
        }
        auto push = [&](const Fe &t) __attribute__((always_inline)) { acc = add(mul(acc, ch[3]), t); };
        const Fe l0 = quot_at(a.l.base, j, a), l_last = quot_at(a.l.base + a.l.col_stride, j, a);
        const Fe l_active = quot_at(a.l.base + 2 * a.l.col_stride, j, a);
        // ---- the permutation argument ----
        {
            auto Z = [&](u32 s, u32 jj) __attribute__((always_inline)) { return quot_at(pz_e + (u64)s * a.perm_z.col_stride, jj, a); };
            push(mul(l0, sub(one, Z(0, j))));
            {
                const Fe z = Z(a.n_sets - 1, j);
                push(mul(l_last, sub(mul(z, z), z)));
            }
            for (u32 s = 1; s < a.n_sets; ++s) push(mul(l0, sub(Z(s, j), Z(s - 1, j_last))));
            for (u32 s = 0; s < a.n_sets; ++s) {
                const u32 c0 = s * a.chunk_len, c1 = c0 + a.chunk_len < a.m ? c0 + a.chunk_len : a.m;
                Fe left = Z(s, j_next), right = Z(s, j);
                for (u32 c = c0; c < c1; ++c) {
                    const u32 src = a.src[c];
                    const Fe v = src < 5 ? adv(src, j) : quot_at(ext_e + (u64)(src - 5) * a.extra.col_stride, j, a);
                    const Fe vg = add(v, ch[2]);
                    left = mul(left, add(vg, mul(ch[1], quot_at(a.sigma.base + (u64)c * a.sigma.col_stride, j, a))));
                    right = mul(right, add(vg, mul(bl[c], X)));
                }
                push(mul(l_active, sub(left, right)));
            }
        }
        // ---- the lookup arguments ----
        if (a.lookup_mask) {
            const Fe sg = add(add(mul(ch[0], fix(a.table_tag)), fix(a.table_value)), ch[2]);   // S + gamma
            for (u32 k = 0; k < QUOT_LOOKUP_ARGS; ++k) {
                if (!((a.lookup_mask >> k) & 1u)) continue;
                const u8 *apc = ap_e + (u64)k * a.a_perm.col_stride, *spc = sp_e + (u64)k * a.s_perm.col_stride;
                const u8 *zc = lz_e + (u64)k * a.look_z.col_stride;
                const Fe z = quot_at(zc, j, a);
                push(mul(l0, sub(one, z)));
                push(mul(l_last, sub(mul(z, z), z)));
                const Fe ap = quot_at(apc, j, a), sp = quot_at(spc, j, a);
                {
                    const Fe ak = add(mul(ch[0], fix(a.lookup_tag[k])), mul(fix(a.lookup_enable[k]), adv(a.lookup_advice[k], j)));
                    const Fe left = mul(mul(quot_at(zc, j_next, a), add(ap, ch[1])), add(sp, ch[2]));
                    const Fe right = mul(mul(z, add(ak, ch[1])), sg);
                    push(mul(l_active, sub(left, right)));
                }
                const Fe d = sub(ap, sp);
                push(mul(l0, d));
                push(mul(l_active, mul(d, sub(ap, quot_at(apc, j_prev, a)))));
            }
        }
        const Fe h = mul(acc, a.xinv[j & (r - 1)]);
        st16(h_e + (u64)j * 32, h.v[0], h.v[1]);
        st16(h_e + (u64)j * 32 + 16, h.v[2], h.v[3]);
        X = mul(X, a.wpow[QUOT_STEP_BIT]);
    }
}

#endif  // H2R_TU_QUOTIENT

}  // namespace h2r
