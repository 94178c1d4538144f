// The evaluation domain's transforms between Lagrange, coefficient and coset (extended) form: a number-theoretic transform over the ctx's
// field.  Third-party behaviour (halo2 poly::domain::EvaluationDomain, not in the reference tree), restated in DESIGN.md section 2f; parity is
// pinned against a Python restatement (tests/ntt_ref.py, tests/test_ntt_gpu.py), not against upstream.  With n = 2^log_n, m = 2^log_m <= n,
// omega a primitive n-th root of unity and g != 0 the coset shift, natural index order on both sides:
//   forward   out[j] = sum_{i < m} in[i] * (g * omega^j)^i,  j < n
//   inverse   out[i] = g^-i * n^-1 * sum_{j < n} in[j] * omega^(-i * j)                       (m = n)
// The log n butterfly stages are cut into P = ceil(log n / NTT_TILE_LOG) passes of s_1 >= s_2 >= ... stages (as even as they come), one launch
// of ntt_pass_kernel each; N_q = 2^(s_q), n_q = N_1 ... N_q.  Cooley-Tukey over the digits i = i_P + N_P * (i_{P-1} + N_{P-1} * ( ... i_1)),
// j = j_1 + N_1 * (j_2 + N_2 * ( ... j_P)): pass q is an N_q-point transform over digit q, and between two passes the element with the
// output digits J = j_1 + ... + n_{q-2} * j_{q-1} done and d = i_q next takes the factor omega_(n_q)^(d * J) (applied by pass q on its load).
//   pass 1    line r = i_P + N_P * ( ... i_2) of `in` (the elements r + (n / N_1) * d, d < N_1; rows >= m are zeros that are not loaded), times
//             g^i (forward), transformed, written to `out` at j_1 + N_1 * (i_2 + N_2 * i_3): the digit reversal happens here and only here
//   pass q    in place in `out`: the elements J + n_(q-1) * (d + N_q * h), d < N_q, of line (J, h); the last pass leaves natural order and
//             folds n^-1 * g^-p into its store (inverse)
// A workgroup of 256 threads holds a tile of NTT_TILE = 1 << NTT_TILE_LOG elements: 2^(NTT_TILE_LOG - s_q) ADJACENT lines (runs of that many
// adjacent elements in memory) times the N_q points of each, so every workgroup reads and writes its own element set and none waits for
// another.  In LDS the tile is four planes of 64-bit words (consecutive lanes on consecutive 8-byte words: no bank conflicts at the strides
// that matter); a line's points are stored bit-reversed and the stages run decimation-in-time, so they leave in natural order.
// Twiddles come from a table in the workspace that ntt_setup_kernel fills per call (Montgomery form; host passes base^(2^b), a thread builds
// its first power from the set bits of its index and steps by multiplication, as perm_product's omega^i):
//   stage[t]  = omega_(2^smax)^t, t < 2^(smax - 1): the butterflies' (stage t of an s-stage pass reads stage[k << (smax - 1 - t)])
//   wlo / whi = omega^e, omega^(4096 e), e < 4096: omega^E for any E < 2^24 in one product (the factors between passes)
//   glo / ghi = c * g^e, g^(4096 e) (forward) or c * n^-1 * g^-e, g^(-4096 e) (inverse), c = the conversion of a canonical ctx: the first
//               load and the last store of a canonical ctx convert within the same product
// All arithmetic is in the Montgomery domain (fe_mont_mul / fe_add / fe_sub); every result is the canonical representative, so the bytes do
// not depend on the order of operations.  The kernels are defined in the one translation unit that launches them (h2r_tu_ntt.hip, H2R_TU_NTT).
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 NTT_TILE_LOG = 10;                   // elements of a tile = 1 << NTT_TILE_LOG: 32 KB of LDS, 256 threads x 4 elements
constexpr u32 NTT_TILE = 1u << NTT_TILE_LOG;
constexpr u32 NTT_MAX_LOG = 24;
constexpr u32 NTT_MAX_PASSES = (NTT_MAX_LOG + NTT_TILE_LOG - 1) / NTT_TILE_LOG;
constexpr u32 NTT_SPLIT_LOG = 12;                  // the two-level power tables: E = lo + (hi << NTT_SPLIT_LOG)
constexpr u32 NTT_SPLIT = 1u << NTT_SPLIT_LOG;
constexpr u32 NTT_TABLES = 5;                      // stage, wlo, whi, glo, ghi: NTT_SPLIT entries each (stage uses the first NTT_TILE / 2)
constexpr u64 NTT_WORKSPACE_BYTES = (u64)NTT_TABLES * NTT_SPLIT * 32 + 256;
static_assert(2 * NTT_SPLIT_LOG >= NTT_MAX_LOG && NTT_TILE / 2 <= NTT_SPLIT, "the two-level tables cover every exponent");

enum : u32 { NTT_F_NONE = 0, NTT_F_CONST = 1, NTT_F_TABLE = 2 };   // how the first load / the last store is scaled

struct NttPlan { u32 passes, s[NTT_MAX_PASSES], smax; };
// stages per pass: as even as they come, the larger ones first
__host__ __device__ inline NttPlan ntt_plan(u32 log_n) {
    NttPlan pl;
    pl.passes = (log_n + NTT_TILE_LOG - 1) / NTT_TILE_LOG;
    u32 left = log_n;
    for (u32 q = 0; q < NTT_MAX_PASSES; ++q) {
        pl.s[q] = q < pl.passes ? (left + (pl.passes - q) - 1) / (pl.passes - q) : 0;
        left -= pl.s[q];
    }
    pl.smax = pl.s[0];
    return pl;
}
// workgroups of one column in pass q
__host__ __device__ inline u32 ntt_pass_tiles(u32 log_n, u32 s) {
    const u32 lines = 1u << (log_n - s), per = 1u << (NTT_TILE_LOG - s);
    return (lines + per - 1) / per;
}

struct NttSetupArgs {
    Fe pow2[NTT_TABLES][NTT_SPLIT_LOG];   // per table: base^(2^b), Montgomery form
    Fe first[NTT_TABLES];                 // per table: entry 0 (the constant every entry carries)
    u32 count[NTT_TABLES];                // entries to fill (a multiple of 4, <= NTT_SPLIT; 0: the table is not used)
    Fe *tab;                              // [NTT_TABLES][NTT_SPLIT]
    FieldConsts f;
};

struct NttArgs {
    const u8 *in; u64 in_elem_stride, in_col_stride;
    u8 *out; u64 out_elem_stride, out_col_stride;
    u32 log_n, log_m, pass, passes;
    u32 s[NTT_MAX_PASSES], smax;
    u32 load_mode, store_mode;            // NTT_F_*: the first pass's load, the last pass's store
    Fe load_const, store_const;
    const Fe *tab;                        // [NTT_TABLES][NTT_SPLIT]
    FieldConsts f;
};

#ifdef H2R_TU_NTT

// base^E of a two-level table pair, E < 2^24; `wide`: exponents reach beyond the low table (uniform per launch)
__device__ __forceinline__ Fe ntt_pow(const Fe *lo, const Fe *hi, u32 e, bool wide, const FieldConsts &f) {
    const Fe l = lo[e & (NTT_SPLIT - 1)];
    return wide ? fe_mont_mul(l, hi[e >> NTT_SPLIT_LOG], f) : l;
}

// grid (NTT_SPLIT / 1024, NTT_TABLES): a thread fills the four entries 4 * t .. 4 * t + 3 of one table
__global__ __launch_bounds__(256) void ntt_setup_kernel(NttSetupArgs a) {
    const u32 table = blockIdx.y, e0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (e0 >= a.count[table]) return;
    Fe x = a.first[table];
    for (u32 b = 2; b < NTT_SPLIT_LOG; ++b)
        if ((e0 >> b) & 1u) x = fe_mont_mul(x, a.pow2[table][b], a.f);
    Fe *dst = a.tab + (u64)table * NTT_SPLIT + e0;
    const Fe step = a.pow2[table][0];
    dst[0] = x;
    for (u32 k = 1; k < 4; ++k) { x = fe_mont_mul(x, step, a.f); dst[k] = x; }
}

// grid (ntt_pass_tiles, columns, elements)
__global__ __launch_bounds__(256) void ntt_pass_kernel(NttArgs a) {
    __shared__ u64 lds[4][NTT_TILE];
    const u32 tid = threadIdx.x, tile = blockIdx.x, q = a.pass;
    const u32 s = a.s[q], lr = NTT_TILE_LOG - s, R = 1u << lr, lines = 1u << (a.log_n - s);
    u32 lb = 0;                                              // log2 n_(q-1): the output digits that are done
    for (u32 k = 0; k < q; ++k) lb += a.s[k];
    const bool first = q == 0, last = q + 1 == a.passes;
    const Fe *stage = a.tab, *wlo = a.tab + NTT_SPLIT, *whi = a.tab + 2 * NTT_SPLIT, *glo = a.tab + 3 * NTT_SPLIT, *ghi = a.tab + 4 * NTT_SPLIT;
    u8 *dst = a.out + (u64)blockIdx.z * a.out_elem_stride + (u64)blockIdx.y * a.out_col_stride;
    const u8 *src = first ? a.in + (u64)blockIdx.z * a.in_elem_stride + (u64)blockIdx.y * a.in_col_stride : dst;
    const u32 line0 = tile << lr;
    auto put = [&](u32 e, const Fe &v) { lds[0][e] = v.v[0]; lds[1][e] = v.v[1]; lds[2][e] = v.v[2]; lds[3][e] = v.v[3]; };
    auto get = [&](u32 e) { Fe v; v.v[0] = lds[0][e]; v.v[1] = lds[1][e]; v.v[2] = lds[2][e]; v.v[3] = lds[3][e]; return v; };
    // where point d of line `line` lies in `out` during the passes after the first
    auto place = [&](u32 line, u32 d) { const u32 J = line & ((1u << lb) - 1), h = line >> lb; return J + ((d + (h << s)) << lb); };

    // ---- load: adjacent lines on adjacent lanes; point d of a line goes to the bit-reversed slot ----
    for (u32 k = 0; k < 4; ++k) {
        const u32 gi = tid + 256 * k, lam = gi & (R - 1), d = gi >> lr, line = line0 + lam;
        if (line >= lines) continue;   // (a transform smaller than a tile)
        Fe v = fe_zero();
        if (first) {
            const u32 i = line + d * lines;
            if (i < (1u << a.log_m)) {
                v = fe_load(src + (u64)i * 32);
                if (a.load_mode == NTT_F_CONST) v = fe_mont_mul(v, a.load_const, a.f);
                else if (a.load_mode == NTT_F_TABLE) v = fe_mont_mul(v, ntt_pow(glo, ghi, i, a.log_m > NTT_SPLIT_LOG, a.f), a.f);
            }
        } else {
            v = fe_load(src + (u64)place(line, d) * 32);
            const u32 e = (d * (line & ((1u << lb) - 1))) << (a.log_n - lb - s);   // omega_(n_q)^(d * J) as a power of omega
            v = fe_mont_mul(v, ntt_pow(wlo, whi, e, a.log_n > NTT_SPLIT_LOG, a.f), a.f);
        }
        put(((__brev(d) >> (32 - s)) << lr) | lam, v);
    }
    __syncthreads();
    // ---- s stages, decimation in time: stage t pairs the slots that differ in bit lr + t ----
    for (u32 t = 0; t < s; ++t) {
        const u32 beta = lr + t;
        for (u32 k = 0; k < 2; ++k) {
            const u32 b = tid + 256 * k;
            const u32 e0 = ((b >> beta) << (beta + 1)) | (b & ((1u << beta) - 1)), e1 = e0 | (1u << beta);
            if (line0 + (e0 & (R - 1)) >= lines) continue;
            const Fe x = get(e0);
            Fe y = get(e1);
            if (t) y = fe_mont_mul(y, stage[((e0 >> lr) & ((1u << t) - 1)) << (a.smax - 1 - t)], a.f);
            put(e0, fe_add(x, y, a.f.p));
            put(e1, fe_sub(x, y, a.f.p));
        }
        __syncthreads();
    }
    // ---- store: the first pass writes each line's points as one run (the digit reversal), the others go back where they came from ----
    const u32 s3 = a.passes == 3 ? a.s[2] : 0, s2 = a.passes >= 2 ? a.s[1] : 0;
    for (u32 k = 0; k < 4; ++k) {
        const u32 gi = tid + 256 * k;
        u32 lam, d, p;
        if (first) {
            d = gi & ((1u << s) - 1); lam = gi >> s;
            const u32 line = line0 + lam;
            if (line >= lines) continue;
            p = d + (((line >> s3) | ((line & ((1u << s3) - 1)) << s2)) << s);
        } else {
            lam = gi & (R - 1); d = gi >> lr;
            if (line0 + lam >= lines) continue;
            p = place(line0 + lam, d);
        }
        Fe v = get((d << lr) | lam);
        if (last) {
            if (a.store_mode == NTT_F_CONST) v = fe_mont_mul(v, a.store_const, a.f);
            else if (a.store_mode == NTT_F_TABLE) v = fe_mont_mul(v, ntt_pow(glo, ghi, p, a.log_n > NTT_SPLIT_LOG, a.f), a.f);
            st16(dst + (u64)p * 32, v.v[0], v.v[1]);
            st16(dst + (u64)p * 32 + 16, v.v[2], v.v[3]);
        } else {   // read again by the next pass: ordinary stores
            reinterpret_cast<ulonglong2 *>(dst + (u64)p * 32)[0] = make_ulonglong2(v.v[0], v.v[1]);
            reinterpret_cast<ulonglong2 *>(dst + (u64)p * 32)[1] = make_ulonglong2(v.v[2], v.v[3]);
        }
    }
}

#endif  // H2R_TU_NTT

}  // namespace h2r
