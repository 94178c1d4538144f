// The vanishing argument's quotient h on the extended domain: halo2's plonk::evaluation::evaluate_h for THIS circuit's constraint system (the
// one main gate, up to PERM_MAX_COLUMNS permutation columns in sets, the five lookup arguments), not a general expression evaluator.
// Third-party behaviour (halo2, not in the reference tree), restated in DESIGN.md section 2g; parity is pinned against a Python restatement
// (tests/quotient_ref.py, tests/test_quotient_gpu.py), not against upstream.  With n = 2^log_n, N = 2^log_ext, r = N / n,
// X_j = zeta * omega_ext^j the point of index j < N (natural order) and f<t>[j] = f[(j + t * r) mod N] the rotation of a column by t rows,
// acc is constraint_fold (h2r_constraints.hpp: THE definition of the terms and their order, shared with the verifier) over the columns at j, and
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

#include "h2r_constraints.hpp"

namespace h2r {

constexpr u32 QUOT_LANE_POINTS = 4;                 // points of a thread, 256 apart
constexpr u32 QUOT_TILE = 256 * QUOT_LANE_POINTS;   // points of a workgroup
constexpr u32 QUOT_STEP_BIT = 8;                    // a thread steps X_j by omega_ext^(2^8)
constexpr u32 QUOT_MAX_LOG = 24;
constexpr u32 QUOT_MAX_SCALE_LOG = 4;               // log_ext - log_n

struct QuotCols { const u8 *base; u64 elem_stride, col_stride; };   // column c of circuit e at base + e * elem_stride + c * col_stride

struct QuotientArgs {
    QuotCols advice, extra, perm_z, a_perm, s_perm, look_z;   // per circuit
    QuotCols fixed, sigma, l;                                 // the proving key's: elem_stride = 0.  l: l0, l_last, l_active
    const u64 *theta, *beta, *gamma, *y;                      // [circuit][4], the ctx's representation
    u8 *status;                                               // nullable, never cleared
    u8 *h; u64 h_elem_stride;
    u32 log_ext, scale_log, mont, tile0;
    u32 last_rot;                                             // blinding_factors + 1
    ConstraintShape cs;
    Fe wpow[QUOT_MAX_LOG];                                    // omega_ext^(2^b), Montgomery form
    Fe zeta;                                                  // Montgomery form
    Fe xinv[1u << QUOT_MAX_SCALE_LOG];                        // 1 / (zeta^n (omega_ext^n)^i - 1): Montgomery form (a canonical ctx: the plain integer)
    FieldConsts f;
};

__host__ __device__ inline u32 quotient_tiles(u32 log_ext) { return (u32)(((1ull << log_ext) + QUOT_TILE - 1) / QUOT_TILE); }

#ifdef H2R_TU_QUOTIENT

// element j of a column in Montgomery form
__device__ __forceinline__ Fe quot_at(const u8 *col, u32 j, const QuotientArgs &a) { return fe_load_mont(col + (u64)j * 32, a.mont, a.f); }

// constraint_fold's source at one point: global loads of one circuit's columns at the point's four rotations, the challenges and beta * delta^c from LDS
struct QuotSrc : ConstraintField {
    const QuotientArgs &a;
    const Fe *ch, *bl;
    const u8 *adv_e, *ext_e, *pz_e, *ap_e, *sp_e, *lz_e;      // the circuit's column groups
    u32 at[ROTATIONS];                                        // the point's index under every rotation
    Fe X;
    __device__ __forceinline__ Fe col(const u8 *base, const QuotCols &g, u32 c, u32 rot) const { return quot_at(base + (u64)c * g.col_stride, at[rot], a); }
    __device__ __forceinline__ Fe adv(u32 c, u32 rot) const { return col(adv_e, a.advice, c, rot); }
    __device__ __forceinline__ Fe fix(u32 c) const { return col(a.fixed.base, a.fixed, c, ROT_CUR); }
    __device__ __forceinline__ Fe sigma(u32 c) const { return col(a.sigma.base, a.sigma, c, ROT_CUR); }
    __device__ __forceinline__ Fe l(u32 i) const { return col(a.l.base, a.l, i, ROT_CUR); }
    __device__ __forceinline__ Fe perm_value(u32 src) const { return src < 5 ? adv(src, ROT_CUR) : col(ext_e, a.extra, src - 5, ROT_CUR); }
    __device__ __forceinline__ Fe perm_z(u32 s, u32 rot) const { return col(pz_e, a.perm_z, s, rot); }
    __device__ __forceinline__ Fe look_z(u32 k, u32 rot) const { return col(lz_e, a.look_z, k, rot); }
    __device__ __forceinline__ Fe a_perm(u32 k, u32 rot) const { return col(ap_e, a.a_perm, k, rot); }
    __device__ __forceinline__ Fe s_perm(u32 k) const { return col(sp_e, a.s_perm, k, ROT_CUR); }
    __device__ __forceinline__ Fe ident(u32 c) const { return mul(bl[c], X); }
    __device__ __forceinline__ const Fe &theta() const { return ch[0]; }
    __device__ __forceinline__ const Fe &beta() const { return ch[1]; }
    __device__ __forceinline__ const Fe &gamma() const { return ch[2]; }
    __device__ __forceinline__ const Fe &y() const { return ch[3]; }
};

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
    if (tid < QUOT_PERM_MAX_COLUMNS) bl[tid] = tid < a.cs.m ? fe_mont_mul(ch[1], a.cs.dpow[tid], a.f) : fe_zero();
    __syncthreads();

    const u32 N = 1u << a.log_ext, mask = N - 1, r = 1u << a.scale_log;
    u32 j = tile * QUOT_TILE + tid;
    if (j >= N) return;
    QuotSrc s{{a.f}, a, ch, bl,
              a.advice.base + elem * a.advice.elem_stride, a.extra.base + elem * a.extra.elem_stride, a.perm_z.base + elem * a.perm_z.elem_stride,
              a.a_perm.base + elem * a.a_perm.elem_stride, a.s_perm.base + elem * a.s_perm.elem_stride, a.look_z.base + elem * a.look_z.elem_stride,
              {}, a.zeta};                        // X_j = zeta * omega_ext^j from the set bits of j
    for (u32 b = 0; b < a.log_ext; ++b)
        if ((j >> b) & 1u) s.X = s.mul(s.X, a.wpow[b]);
    u8 *h_e = a.h + elem * a.h_elem_stride;

#pragma unroll 1
    for (u32 q = 0; q < QUOT_LANE_POINTS && j < N; ++q, j += 256) {
        s.at[ROT_CUR] = j; s.at[ROT_NEXT] = (j + r) & mask; s.at[ROT_LAST] = (j - a.last_rot * r) & mask; s.at[ROT_PREV] = (j - r) & mask;
        const Fe h = s.mul(constraint_fold(a.cs, s), a.xinv[j & (r - 1)]);
        st16(h_e + (u64)j * 32, h.v[0], h.v[1]);
        st16(h_e + (u64)j * 32 + 16, h.v[2], h.v[3]);
        s.X = s.mul(s.X, a.wpow[QUOT_STEP_BIT]);
    }
}

#endif  // H2R_TU_QUOTIENT

}  // namespace h2r
