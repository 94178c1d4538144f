// halo2's lookup argument, the step after the permuted columns: the compressed INPUT column A in its original row order and the
// grand-product column Z of plonk::lookup::prover::commit_product.  Third-party algorithm (halo2, not in the reference tree), restated in
// DESIGN.md section 2d; parity is pinned against a Python restatement (tests/test_lookup_product.py), not against upstream.
//   A[i]  = tag(i) * theta + cell(i, column of the argument) on a lookup-enabled row of the image, 0 elsewhere
//   S[i]  = the compressed table: its n_rows rows (row 0 = (0, 0)), then 0 -- computed here from the configuration and theta, never read
//   Z[0]  = 1,  Z[i+1] = Z[i] * (A[i] + beta)(S[i] + gamma) / ((A'[i] + beta)(S'[i] + gamma)),  i = 0 .. usable_rows - 1
// Z is the grand product of h2r_grand_product.hpp with n_i = (A_i + beta)(S_i + gamma), d_i = (A'_i + beta)(S'_i + gamma) and start = 1, one
// column per (circuit, argument); Z[usable_rows] = 1 exactly when prod n = D (a comparison).  The three launches:
//   lookup_product_tiles_kernel   copies the status on entry into the slot's header, then the tile's pair
//   lookup_product_carry_kernel   per column: refuses (H2R_E_SHAPE), or D != 0 and prod n == D (H2R_E_ASSERTION), the carry-ins, go
//   lookup_product_scan_kernel    writes Z where go is set
// and next to them
//   lookup_input_kernel           A: one workgroup per dense 256-row window of one column, one row per lane, lanes exchange halves so
//                                 that each 16-byte non-temporal store instruction covers whole 128-byte lines (lookup_fill_kernel's geometry).
// The kernels are defined in the one translation unit that launches them (h2r_tu_lookup_product.hip, H2R_TU_LOOKUP_PRODUCT).
#pragma once

#include "h2r_grand_product.hpp"

namespace h2r {

// DEPRECATED alias of GRAND_PRODUCT_TILE, used by no code of this tree.  The previous revision's tests read `LOOKUP_PRODUCT_TILE = <digits>;`
// out of this file and must still run against this library; delete the two lines in the revision after this one.
constexpr u32 LOOKUP_PRODUCT_TILE = 1024;
static_assert(LOOKUP_PRODUCT_TILE == GRAND_PRODUCT_TILE, "one tile for both grand products");
// per (element, argument) in the workspace: the header (u32 skip, u32 go), then [tile]{Fe n, Fe d}
__host__ __device__ inline u64 lookup_product_slot_bytes(u32 usable_rows) { return GRAND_PRODUCT_HDR_BYTES + 64ull * grand_product_tiles(usable_rows); }

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

#ifdef H2R_TU_LOOKUP_PRODUCT

__global__ __launch_bounds__(256) void lookup_input_kernel(LookupInputArgs a) {
    __shared__ Fe tagth[8];
    __shared__ u8 ktab[256];
    const u32 tid = threadIdx.x, lane = tid & 63, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    if (a.status && a.status[elem]) return;
    const Fe theta = fe_words(a.theta + elem * 4);
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
            const Fe cell = fe_load(a.img.base + elem * a.img.elem_stride + ir * a.img.row_pitch + (u64)(arg < 4 ? arg : 0u) * a.img.col_pitch);
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

// ---- the grand product ---------------------------------------------------------------------------------------------------------
struct LpChallenges { Fe theta, beta, gamma; bool ok; };   // Montgomery form; ok: all three were canonical elements
__device__ __forceinline__ LpChallenges lp_challenges(const LookupProductArgs &a, u64 elem) {
    LpChallenges c;
    c.ok = true;
    c.theta = grand_product_challenge(a.theta + elem * 4, a.f, a.mont, c.ok); c.beta = grand_product_challenge(a.beta + elem * 4, a.f, a.mont, c.ok);
    c.gamma = grand_product_challenge(a.gamma + elem * 4, a.f, a.mont, c.ok);
    return c;
}
// tag * theta of every bit length, once per workgroup (the caller synchronises)
__device__ __forceinline__ void lp_tag_thetas(const LookupProductArgs &a, const LpChallenges &c, u32 tid, Fe *tagth) {
    if (tid < 8) tagth[tid] = tid < a.n_lens ? fe_mul_small(c.theta, a.tag[tid], a.f.p) : fe_zero();
}
// n, d of row r of one column (Montgomery form); a row behind usable_rows counts as 1 / 1
__device__ __forceinline__ void lp_term(const LookupProductArgs &a, u64 col, u32 r, const LpChallenges &c, const Fe *tagth, Fe &n, Fe &d) {
    n = fe_words(a.f.one); d = n;
    if (r >= a.usable_rows) return;
    Fe A = fe_load(a.a_in + col + (u64)r * 32), Ap = fe_load(a.a_perm + col + (u64)r * 32), Sp = fe_load(a.s_perm + col + (u64)r * 32);
    if (!a.mont) { A = fe_to_mont(A, a.f); Ap = fe_to_mont(Ap, a.f); Sp = fe_to_mont(Sp, a.f); }   // (one branch: the three loads issue together)
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
    const u32 r0 = tile * GRAND_PRODUCT_TILE + GRAND_PRODUCT_LANE_ROWS * tid;
    lp_term(a, col, r0, c, tagth, n[0], d[0]); lp_term(a, col, r0 + 1, c, tagth, n[1], d[1]);
    lp_term(a, col, r0 + 2, c, tagth, n[2], d[2]); lp_term(a, col, r0 + 3, c, tagth, n[3], d[3]);
}
__device__ __forceinline__ u8 *lp_slot(const LookupProductArgs &a, u64 elem, u32 arg) {
    return a.ws + (elem * 5 + arg) * lookup_product_slot_bytes(a.usable_rows);
}
__device__ __forceinline__ Fe *lp_pairs(u8 *slot) { return reinterpret_cast<Fe *>(slot + GRAND_PRODUCT_HDR_BYTES); }

__global__ __launch_bounds__(256) void lookup_product_tiles_kernel(LookupProductArgs a) {
    __shared__ Fe tagth[8];
    const u32 tid = threadIdx.x, tile = blockIdx.x, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    u8 *slot = lp_slot(a, elem, arg);
    const bool skip = a.status && a.status[elem];   // the status on entry: the carry kernel, which writes statuses, reads this copy
    if (tile == 0 && tid == 0) reinterpret_cast<u32 *>(slot)[0] = skip ? 1u : 0u;
    if (skip) return;
    const LpChallenges c = lp_challenges(a, elem);
    if (!c.ok || a.n_rows > a.usable_rows) return;   // H2R_E_SHAPE, set by the carry kernel
    lp_tag_thetas(a, c, tid, tagth);
    __syncthreads();
    Fe n[4], d[4];
    lp_terms(a, elem, arg, tile, tid, c, tagth, n, d);
    grand_product_tile(n, d, lp_pairs(slot) + 2 * tile, a.f);
}

// one wave per column.  N and D are compared after the walk, so both stay live across its inversion: 96 VGPRs, the last count with 5 waves/SIMD.
// Occupancy buys nothing here (a launch is one wave per column); should it ever, hand fe_eq(N, D) out of the walk instead of N and D.
__global__ __launch_bounds__(64) void lookup_product_carry_kernel(LookupProductArgs a) {
    const u32 lane = threadIdx.x, arg = blockIdx.x;
    const u64 elem = blockIdx.y;
    if (!((a.arg_mask >> arg) & 1u)) return;
    u8 *slot = lp_slot(a, elem, arg);
    u32 *hdr = reinterpret_cast<u32 *>(slot);
    if (hdr[0]) { if (lane == 0) hdr[1] = 0; return; }   // status nonzero on entry: skipped
    const LpChallenges c = lp_challenges(a, elem);
    if (!c.ok || a.n_rows > a.usable_rows) {
        if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_SHAPE; hdr[1] = 0; }
        return;
    }
    Fe N, D, dinv;
    if (!grand_product_carry(lp_pairs(slot), a.n_tiles, lane, nullptr, a.f, N, D, dinv)) {   // some (A' + beta)(S' + gamma) is zero: no Z
        if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_ASSERTION; hdr[1] = 0; }
        return;
    }
    if (lane == 0) {
        if (!fe_eq(N, D) && a.status) a.status[elem] = (u8)H2R_E_ASSERTION;   // Z[usable_rows] != 1: the column is written as computed
        hdr[1] = 1;
    }
}

__global__ __launch_bounds__(256) void lookup_product_scan_kernel(LookupProductArgs a) {
    __shared__ Fe tagth[8];
    const u32 tid = threadIdx.x, tile = blockIdx.x, arg = blockIdx.y;
    const u64 elem = blockIdx.z;
    if (!((a.arg_mask >> arg) & 1u)) return;
    u8 *slot = lp_slot(a, elem, arg);
    if (!reinterpret_cast<const u32 *>(slot)[1]) return;   // skipped, refused, or a zero denominator
    const LpChallenges c = lp_challenges(a, elem);
    lp_tag_thetas(a, c, tid, tagth);
    __syncthreads();
    Fe n[4], d[4];
    lp_terms(a, elem, arg, tile, tid, c, tagth, n, d);
    grand_product_scan(n, d, lp_pairs(slot) + 2 * tile, a.z + elem * a.z_elem_stride + (u64)arg * a.z_col_stride, a.usable_rows, tile, a.mont, a.f);
}

#endif  // H2R_TU_LOOKUP_PRODUCT

}  // namespace h2r
