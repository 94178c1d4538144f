// halo2's lookup argument, the step after the permuted columns: the compressed INPUT column A in its original row order and the
// grand-product column Z of plonk::lookup::prover::commit_product.  Third-party algorithm (halo2, not in the reference tree), restated in
// DESIGN.md section 2d; parity is pinned against a Python restatement (tests/test_lookup_product.py), not against upstream.
//   A[i]  = tag(i) * theta + cell(i, column of the argument) on a lookup-enabled row of the image, 0 elsewhere
//   S[i]  = the compressed table: its n_rows rows (row 0 = (0, 0)), then 0 -- computed here from the configuration and theta, never read
//   Z[0]  = 1,  Z[i+1] = Z[i] * (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)),  i = 0 .. usable_rows - 1
// One inversion per column: with n_i = (A_i + beta)(S_i + gamma), d_i = (A'_i + beta)(S'_i + gamma) and D = prod d over all rows,
//   Z_i = (prod_{j < i} n_j) * (prod_{j >= i} d_j) * D^-1,
// and Z[usable_rows] = 1 exactly when prod n = D (a comparison).  Three launches, and NO workgroup ever waits for another one:
//   lookup_product_tiles_kernel   per tile of LOOKUP_PRODUCT_TILE rows of one column: prod n and prod d of the tile -> workspace
//   lookup_product_carry_kernel   per column, one wave: prefix of the tiles' n, suffix of their d, D != 0 and prod n == D (status), D^-1
//                                 (fe_inv; D is in Montgomery form), the tiles' carry-ins (the suffix one times D^-1) -> workspace
//   lookup_product_scan_kernel    per tile: n_i, d_i again, scans serial per lane (four consecutive rows), across the wave with __shfl,
//                                 across the four waves through LDS, seeded with the carry-ins; Z leaves through an LDS stage so that
//                                 every store instruction covers 1 KB of the column.  Rows behind usable_rows count as n = d = 1, so
//                                 the tile that holds row usable_rows - 1 also produces Z[usable_rows] (when usable_rows is a multiple
//                                 of the tile, its last thread writes that one element).
// All arithmetic is in the Montgomery domain (fe_mont_mul); a canonical ctx converts on load and on store, a Montgomery ctx nothing.
//   lookup_input_kernel           A: one workgroup per dense 256-row window of one column, one row per lane, lanes exchange halves so
//                                 that each 16-byte non-temporal store instruction covers whole 128-byte lines (lookup_fill_kernel's geometry).
// The kernels are defined in the one translation unit that launches them (h2r_tu_lookup_product.hip, H2R_TU_LOOKUP_PRODUCT); the lp_*
// device helpers are shared with the permutation argument's product (h2r_permutation_product.hpp, H2R_TU_PERM_PRODUCT).
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 LOOKUP_PRODUCT_TILE = 1024;          // rows of a column per workgroup of the product kernels: 256 threads x 4 consecutive rows
constexpr u32 LOOKUP_PRODUCT_LANE_ROWS = 4;
constexpr u32 LOOKUP_PRODUCT_HDR_BYTES = 64;       // per (element, argument) in the workspace: u32 skip, u32 go; then [tile]{Fe n, Fe d}
constexpr u32 LOOKUP_PRODUCT_STAGE_PITCH = 144;    // bytes of a thread's four Z rows in the LDS stage (128 + 16: the threads' rows start on different banks)

__host__ __device__ inline u32 lookup_product_tiles(u32 usable_rows) { return (usable_rows + LOOKUP_PRODUCT_TILE - 1) / LOOKUP_PRODUCT_TILE; }
__host__ __device__ inline u64 lookup_product_slot_bytes(u32 usable_rows) { return LOOKUP_PRODUCT_HDR_BYTES + 64ull * lookup_product_tiles(usable_rows); }

struct LookupInputArgs {
    AdviceDst img;                 // (read only) the image, rows [0, rows)
    const u8 *kinds; u64 rows;
    const u8 *status;              // nullable: elements with a nonzero status are skipped
    const u64 *theta;              // [elem][4], the ctx's representation
    u64 p[4];
    u32 usable_rows, first_row, arg_mask, n_lens;
    u32 tag[8];
    u8 ktab[256];                  // per row kind: (index of the composition tag + 1) | (index of the overflow tag + 1) << 4; 0 = lookup off
    u8 *out; u64 out_elem_stride;  // element e, argument k at + e * out_elem_stride + k * usable_rows * 32
};

struct LookupProductArgs {
    const u8 *a_in, *a_perm, *s_perm; u64 in_elem_stride;
    const u64 *theta, *beta, *gamma;   // [elem][4], the ctx's representation
    u32 usable_rows, n_tiles, arg_mask, mont;
    u32 n_rows, n_lens, tag[8], row_off[8];
    FieldConsts f;
    u8 *z; u64 z_elem_stride, z_col_stride;
    u8 *status;                    // nullable, never cleared
    u8 *ws;                        // [elem][5] slots of lookup_product_slot_bytes
};

#if defined(H2R_TU_LOOKUP_PRODUCT) || defined(H2R_TU_PERM_PRODUCT)

__device__ __forceinline__ Fe lp_load(const u8 *p) {
    const ulonglong2 lo = reinterpret_cast<const ulonglong2 *>(p)[0], hi = reinterpret_cast<const ulonglong2 *>(p)[1];
    Fe r; r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = hi.x; r.v[3] = hi.y;
    return r;
}
__device__ __forceinline__ Fe lp_words(const u64 *w) { Fe r; for (int k = 0; k < 4; ++k) r.v[k] = w[k]; return r; }

#ifdef H2R_TU_LOOKUP_PRODUCT
__global__ __launch_bounds__(256) void lookup_input_kernel(LookupInputArgs a) {
    __shared__ Fe tagth[8];
    __shared__ u8 ktab[256];
    const u32 tid = threadIdx.x, lane = tid & 63, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    if (a.status && a.status[elem]) return;
    const Fe theta = lp_words(a.theta + elem * 4);
    if (ge_p(theta.v, a.p)) return;   // not a canonical challenge: h2r_lookup_product_columns reports it, the columns stay untouched
    ktab[tid] = a.ktab[tid];
    if (tid < 8) tagth[tid] = tid < a.n_lens ? fe_mul_small(theta, a.tag[tid], a.p) : fe_zero();
    __syncthreads();
    const u32 usable = a.usable_rows;
    // a wave works on 64 consecutive rows: every lane computes one row, then the lanes exchange halves so that each of the two store
    // instructions writes 64 consecutive 16-byte units (rows base .. base+31, then base+32 .. base+63)
    const u32 base = blockIdx.x * 256 + (tid & ~63u), pos = base + lane;
    Fe av = fe_zero();
    if (pos < usable && pos >= a.first_row && (u64)(pos - a.first_row) < a.rows) {
        const u64 ir = pos - a.first_row;
        const u32 kt = ktab[a.kinds[ir]];
        const u32 ci = arg < 4 ? (kt & 15u) : (kt >> 4);
        if (ci) {   // the lookups read the PHYSICAL columns 0..3 (composition) and 0 (overflow), as h2r_lookup_hist_advice does
            const Fe cell = lp_load(a.img.base + elem * a.img.elem_stride + ir * a.img.row_pitch + (u64)(arg < 4 ? arg : 0u) * a.img.col_pitch);
            av = fe_add(tagth[ci - 1], cell, a.p);   // tag * theta + cell: the same sum in either representation
        }
    }
    u8 *out = a.out + elem * a.out_elem_stride + (u64)arg * usable * 32;
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
        const int srcl = 32 * hlf + (int)(lane >> 1);
        const bool hi = lane & 1;
        const u64 a0 = __shfl(av.v[0], srcl), a1 = __shfl(av.v[1], srcl), a2 = __shfl(av.v[2], srcl), a3 = __shfl(av.v[3], srcl);
        const u32 row = base + 32 * hlf + (lane >> 1);
        if (row < usable) st16(out + (u64)row * 32 + (hi ? 16 : 0), hi ? a2 : a0, hi ? a3 : a1);
    }
}

#endif  // H2R_TU_LOOKUP_PRODUCT

// ---- the grand product ---------------------------------------------------------------------------------------------------------
struct LpChallenges { Fe theta, beta, gamma; bool ok; };   // Montgomery form; ok: all three were canonical elements
// one challenge (four words in the ctx's representation) in Montgomery form; clears ok when it is not a canonical element
__device__ __forceinline__ Fe lp_challenge(const u64 *w, const FieldConsts &f, u32 mont, bool &ok) {
    Fe c = lp_words(w);
    if (ge_p(c.v, f.p)) ok = false;
    else if (!mont) c = fe_to_mont(c, f);
    return c;
}
__device__ __forceinline__ LpChallenges lp_challenges(const LookupProductArgs &a, u64 elem) {
    LpChallenges c;
    c.ok = true;
    c.theta = lp_challenge(a.theta + elem * 4, a.f, a.mont, c.ok); c.beta = lp_challenge(a.beta + elem * 4, a.f, a.mont, c.ok);
    c.gamma = lp_challenge(a.gamma + elem * 4, a.f, a.mont, c.ok);
    return c;
}
__device__ __forceinline__ Fe lp_one(const LookupProductArgs &a) { return lp_words(a.f.one); }
__device__ __forceinline__ Fe lp_shfl_up(const Fe &x, u32 d) { Fe r; for (int k = 0; k < 4; ++k) r.v[k] = __shfl_up(x.v[k], d); return r; }
__device__ __forceinline__ Fe lp_shfl_down(const Fe &x, u32 d) { Fe r; for (int k = 0; k < 4; ++k) r.v[k] = __shfl_down(x.v[k], d); return r; }
__device__ __forceinline__ Fe lp_shfl(const Fe &x, int src) { Fe r; for (int k = 0; k < 4; ++k) r.v[k] = __shfl(x.v[k], src); return r; }
// product of the lanes 0 .. lane (prefix) / lane .. 63 (suffix) of one wave
__device__ __forceinline__ Fe lp_wave_prefix(Fe x, u32 lane, const FieldConsts &f) {
    for (u32 d = 1; d < 64; d <<= 1) { const Fe m = fe_mont_mul(lp_shfl_up(x, d), x, f); if (lane >= d) x = m; }
    return x;
}
__device__ __forceinline__ Fe lp_wave_suffix(Fe x, u32 lane, const FieldConsts &f) {
    for (u32 d = 1; d < 64; d <<= 1) { const Fe m = fe_mont_mul(lp_shfl_down(x, d), x, f); if (lane + d < 64) x = m; }
    return x;
}
// n, d of row r of one column (Montgomery form); a row behind usable_rows counts as 1 / 1
__device__ __forceinline__ void lp_term(const LookupProductArgs &a, u64 col, u32 r, const LpChallenges &c, const Fe *tagth, Fe &n, Fe &d) {
    n = lp_one(a); d = n;
    if (r >= a.usable_rows) return;
    Fe A = lp_load(a.a_in + col + (u64)r * 32), Ap = lp_load(a.a_perm + col + (u64)r * 32), Sp = lp_load(a.s_perm + col + (u64)r * 32);
    if (!a.mont) { A = fe_to_mont(A, a.f); Ap = fe_to_mont(Ap, a.f); Sp = fe_to_mont(Sp, a.f); }
    Fe sg = c.gamma;
    if (r && r < a.n_rows) {   // a row of the table: tag * theta + value (row_off[0] = 1 and n_rows <= one tile: the host checks both)
        u32 i = 0;
        while (i + 1 < a.n_lens && r >= a.row_off[i + 1]) ++i;
        sg = fe_add(fe_add(tagth[i], fe_to_mont(fe_small(r - a.row_off[i]), a.f), a.f.p), c.gamma, a.f.p);
    }
    n = fe_mont_mul(fe_add(A, c.beta, a.f.p), sg, a.f);
    d = fe_mont_mul(fe_add(Ap, c.beta, a.f.p), fe_add(Sp, c.gamma, a.f.p), a.f);
}
// the four rows tile * TILE + 4 tid + j of a thread
__device__ __forceinline__ void lp_terms(const LookupProductArgs &a, u64 elem, u32 arg, u32 tile, u32 tid, const LpChallenges &c, const Fe *tagth,
                                         Fe (&n)[4], Fe (&d)[4]) {
    const u64 col = elem * a.in_elem_stride + (u64)arg * a.usable_rows * 32;
    const u32 r0 = tile * LOOKUP_PRODUCT_TILE + LOOKUP_PRODUCT_LANE_ROWS * tid;
    lp_term(a, col, r0, c, tagth, n[0], d[0]); lp_term(a, col, r0 + 1, c, tagth, n[1], d[1]);
    lp_term(a, col, r0 + 2, c, tagth, n[2], d[2]); lp_term(a, col, r0 + 3, c, tagth, n[3], d[3]);
}
__device__ __forceinline__ u8 *lp_slot(const LookupProductArgs &a, u64 elem, u32 arg) {
    return a.ws + (elem * 5 + arg) * lookup_product_slot_bytes(a.usable_rows);
}

#ifdef H2R_TU_LOOKUP_PRODUCT
__global__ __launch_bounds__(256) void lookup_product_tiles_kernel(LookupProductArgs a) {
    __shared__ Fe tagth[8];
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    u8 *slot = lp_slot(a, elem, arg);
    const bool skip = a.status && a.status[elem];   // the status on entry: the carry kernel, which writes statuses, reads this copy
    if (tile == 0 && tid == 0) reinterpret_cast<u32 *>(slot)[0] = skip ? 1u : 0u;
    if (skip) return;
    const LpChallenges c = lp_challenges(a, elem);
    if (!c.ok || a.n_rows > a.usable_rows) return;   // H2R_E_SHAPE, set by the carry kernel
    if (tid < 8) tagth[tid] = tid < a.n_lens ? fe_mul_small(c.theta, a.tag[tid], a.f.p) : fe_zero();
    __syncthreads();
    Fe n[4], d[4];
    lp_terms(a, elem, arg, tile, tid, c, tagth, n, d);
    Fe tn = fe_mont_mul(fe_mont_mul(n[0], n[1], a.f), fe_mont_mul(n[2], n[3], a.f), a.f);
    Fe td = fe_mont_mul(fe_mont_mul(d[0], d[1], a.f), fe_mont_mul(d[2], d[3], a.f), a.f);
    for (int s = 32; s; s >>= 1) {
        Fe on, od;
        for (int k = 0; k < 4; ++k) { on.v[k] = __shfl_xor(tn.v[k], s); od.v[k] = __shfl_xor(td.v[k], s); }
        tn = fe_mont_mul(tn, on, a.f); td = fe_mont_mul(td, od, a.f);
    }
    if (lane == 0) { wtot[0][wave] = tn; wtot[1][wave] = td; }
    __syncthreads();
    if (tid < 2) {
        const Fe x = fe_mont_mul(fe_mont_mul(wtot[tid][0], wtot[tid][1], a.f), fe_mont_mul(wtot[tid][2], wtot[tid][3], a.f), a.f);
        reinterpret_cast<Fe *>(slot + LOOKUP_PRODUCT_HDR_BYTES)[2 * tile + tid] = x;
    }
}

// one wave per column; lane l takes the tiles [l * per, (l + 1) * per)
__global__ __launch_bounds__(64) void lookup_product_carry_kernel(LookupProductArgs a) {
    const u32 lane = threadIdx.x, arg = blockIdx.x;
    const u64 elem = blockIdx.y;
    if (!((a.arg_mask >> arg) & 1u)) return;
    u8 *slot = lp_slot(a, elem, arg);
    u32 *hdr = reinterpret_cast<u32 *>(slot);
    Fe *tp = reinterpret_cast<Fe *>(slot + LOOKUP_PRODUCT_HDR_BYTES);
    if (hdr[0]) { if (lane == 0) hdr[1] = 0; return; }   // status nonzero on entry: skipped
    const LpChallenges c = lp_challenges(a, elem);
    if (!c.ok || a.n_rows > a.usable_rows) {
        if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_SHAPE; hdr[1] = 0; }
        return;
    }
    const u32 T = a.n_tiles, per = (T + 63) / 64;
    const u32 lo = lane * per < T ? lane * per : T, hi = lo + per < T ? lo + per : T;
    const Fe one = lp_one(a);
    Fe pn = one, pd = one;
    for (u32 t = lo; t < hi; ++t) { pn = fe_mont_mul(pn, tp[2 * t], a.f); pd = fe_mont_mul(pd, tp[2 * t + 1], a.f); }
    const Fe inc_n = lp_wave_prefix(pn, lane, a.f), inc_d = lp_wave_suffix(pd, lane, a.f);
    const Fe N = lp_shfl(inc_n, 63), D = lp_shfl(inc_d, 0);
    if (fe_is_zero(D)) {   // some (A' + beta)(S' + gamma) is zero: no Z
        if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_ASSERTION; hdr[1] = 0; }
        return;
    }
    if (lane == 0) {
        if (!fe_eq(N, D) && a.status) a.status[elem] = (u8)H2R_E_ASSERTION;   // Z[usable_rows] != 1: the column is written as computed
        hdr[1] = 1;
    }
    const Fe dinv = fe_to_mont(fe_inv(fe_from_mont(D, a.f), a.f), a.f);      // D is D * R: back to the integer, invert, forth
    Fe run_n = lp_shfl_up(inc_n, 1), run_d = lp_shfl_down(inc_d, 1);
    if (lane == 0) run_n = one;
    if (lane == 63) run_d = one;
    run_d = fe_mont_mul(run_d, dinv, a.f);
    for (u32 t = lo; t < hi; ++t) { const Fe x = tp[2 * t]; tp[2 * t] = run_n; run_n = fe_mont_mul(run_n, x, a.f); }
    for (u32 t = hi; t > lo; --t) { const Fe x = tp[2 * t - 1]; tp[2 * t - 1] = run_d; run_d = fe_mont_mul(run_d, x, a.f); }
}

__global__ __launch_bounds__(256) void lookup_product_scan_kernel(LookupProductArgs a) {
    __shared__ __attribute__((aligned(16))) u8 stage[256 * LOOKUP_PRODUCT_STAGE_PITCH];
    __shared__ Fe tagth[8];
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    const u8 *slot = lp_slot(a, elem, arg);
    if (!reinterpret_cast<const u32 *>(slot)[1]) return;   // skipped, refused, or a zero denominator
    const LpChallenges c = lp_challenges(a, elem);
    if (tid < 8) tagth[tid] = tid < a.n_lens ? fe_mul_small(c.theta, a.tag[tid], a.f.p) : fe_zero();
    __syncthreads();
    Fe n[4], d[4];
    lp_terms(a, elem, arg, tile, tid, c, tagth, n, d);
    // serial per lane: pn[j] = n_0 .. n_{j-1} (pn[0] = 1 is not kept), sd[j] = d_j .. d_3
    Fe pn[4], sd[4];
    pn[1] = n[0]; pn[2] = fe_mont_mul(pn[1], n[1], a.f); pn[3] = fe_mont_mul(pn[2], n[2], a.f);
    const Fe tn = fe_mont_mul(pn[3], n[3], a.f);
    sd[3] = d[3]; sd[2] = fe_mont_mul(d[2], sd[3], a.f); sd[1] = fe_mont_mul(d[1], sd[2], a.f); sd[0] = fe_mont_mul(d[0], sd[1], a.f);
    // across the wave, then across the workgroup's four waves through LDS
    const Fe inc_n = lp_wave_prefix(tn, lane, a.f), inc_d = lp_wave_suffix(sd[0], lane, a.f);
    if (lane == 63) wtot[0][wave] = inc_n;
    if (lane == 0) wtot[1][wave] = inc_d;
    __syncthreads();
    const Fe *tp = reinterpret_cast<const Fe *>(slot + LOOKUP_PRODUCT_HDR_BYTES);
    Fe carry_n = tp[2 * tile], carry_d = tp[2 * tile + 1];   // prod n of the tiles before this one; prod d of the tiles behind it, times D^-1
    for (u32 w = 0; w < wave; ++w) carry_n = fe_mont_mul(carry_n, wtot[0][w], a.f);
    for (u32 w = wave + 1; w < 4; ++w) carry_d = fe_mont_mul(carry_d, wtot[1][w], a.f);
    const Fe one = lp_one(a);
    Fe ex_n = lp_shfl_up(inc_n, 1), ex_d = lp_shfl_down(inc_d, 1);
    if (lane == 0) ex_n = one;
    if (lane == 63) ex_d = one;
    const Fe cp = fe_mont_mul(carry_n, ex_n, a.f), cs = fe_mont_mul(ex_d, carry_d, a.f);
    u8 *mine = stage + tid * LOOKUP_PRODUCT_STAGE_PITCH;
    auto put = [&](u32 j, const Fe &p, const Fe &s) {   // Z of the thread's row j = (prod n before it) * (prod d from it on, D^-1 included)
        Fe z = fe_mont_mul(p, fe_mont_mul(s, cs, a.f), a.f);
        if (!a.mont) z = fe_from_mont(z, a.f);
        reinterpret_cast<ulonglong2 *>(mine + 32 * j)[0] = make_ulonglong2(z.v[0], z.v[1]);
        reinterpret_cast<ulonglong2 *>(mine + 32 * j)[1] = make_ulonglong2(z.v[2], z.v[3]);
    };
    put(0, cp, sd[0]); put(1, fe_mont_mul(cp, pn[1], a.f), sd[1]); put(2, fe_mont_mul(cp, pn[2], a.f), sd[2]); put(3, fe_mont_mul(cp, pn[3], a.f), sd[3]);
    u8 *zc = a.z + elem * a.z_elem_stride + (u64)arg * a.z_col_stride;
    const u32 row0 = tile * LOOKUP_PRODUCT_TILE;
    if (tid == 255 && a.usable_rows == row0 + LOOKUP_PRODUCT_TILE) {   // usable_rows is a multiple of the tile: Z[usable_rows] = prod n * D^-1 has no tile of its own
        Fe z = fe_mont_mul(fe_mont_mul(cp, tn, a.f), cs, a.f);
        if (!a.mont) z = fe_from_mont(z, a.f);
        st16(zc + (u64)a.usable_rows * 32, z.v[0], z.v[1]);
        st16(zc + (u64)a.usable_rows * 32 + 16, z.v[2], z.v[3]);
    }
    __syncthreads();
    // rows row0 .. min(row0 + TILE - 1, usable_rows): the rows behind usable_rows - 1 were computed with n = d = 1, so row usable_rows is Z[usable_rows]
    const u32 left = a.usable_rows + 1 - row0, nw = left < LOOKUP_PRODUCT_TILE ? left : LOOKUP_PRODUCT_TILE;
    for (u32 q = tid; q < 2 * nw; q += 256) {
        const u32 r = q >> 1, h = q & 1u;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(stage + (r >> 2) * LOOKUP_PRODUCT_STAGE_PITCH + (r & 3u) * 32 + h * 16);
        st16(zc + (u64)(row0 + r) * 32 + h * 16, v.x, v.y);
    }
}

#endif  // H2R_TU_LOOKUP_PRODUCT

#endif  // H2R_TU_LOOKUP_PRODUCT || H2R_TU_PERM_PRODUCT

}  // namespace h2r
