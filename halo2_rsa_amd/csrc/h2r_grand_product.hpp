// What the two grand products share: the lookup argument's Z (h2r_lookup_product.hpp) and the permutation argument's Z_s
// (h2r_permutation_product.hpp) are one algorithm, restated in DESIGN.md sections 2d and 2e.  For a column (or set) with a pair n_i, d_i per
// row, D = prod d over all rows and a first value `start`,
//   Z[0] = start,  Z[i+1] = Z[i] * n_i / d_i   <=>   Z[i] = start * (prod_{j < i} n_j) * (prod_{j >= i} d_j) * D^-1:
// one inversion per column.  Three launches, and NO workgroup ever waits for another one; the workspace holds one pair of Fe per tile of
// GRAND_PRODUCT_TILE rows, [tile]{n, d}, behind a header of GRAND_PRODUCT_HDR_BYTES:
//   tiles   per tile: prod n and prod d of its rows -> the tile's pair                                              (grand_product_tile)
//   carry   per column, one wave: prefix of the tiles' n, suffix of their d, D (zero: no Z), D^-1 (fe_inv; D is in Montgomery form); the
//           pairs become the tiles' carry-ins (start in the prefix one, D^-1 in the suffix one)                      (grand_product_carry)
//   scan    per tile: the rows' n, d again, scans serial per lane (four consecutive rows), across the wave with __shfl, across the four
//           waves through LDS, seeded with the carry-ins; Z leaves through an LDS stage so that every store instruction covers 1 KB of the
//           column.  Rows behind usable_rows count as n = d = 1, so the tile that holds row usable_rows - 1 also produces Z[usable_rows]
//           (when usable_rows is a multiple of the tile, its last thread writes that one element).                   (grand_product_scan)
// All arithmetic is in the Montgomery domain (fe_mont_mul); a canonical ctx converts on load and on store, a Montgomery ctx nothing.
// What an argument adds is its kernels' prologues (status and skip header, challenges, per-workgroup tables) and how a row's n, d are formed.
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 GRAND_PRODUCT_TILE = 1024;           // rows of a column per workgroup of the tiles and scan kernels: 256 threads x 4 consecutive rows
constexpr u32 GRAND_PRODUCT_LANE_ROWS = 4;
constexpr u32 GRAND_PRODUCT_HDR_BYTES = 64;        // of a workspace slot: u32 skip, u32 go (what the scan may write); then the tiles' pairs
constexpr u32 GRAND_PRODUCT_STAGE_PITCH = 144;     // bytes of a thread's four Z rows in the LDS stage (128 + 16: the threads' rows start on different banks)

__host__ __device__ inline u32 grand_product_tiles(u32 usable_rows) { return (usable_rows + GRAND_PRODUCT_TILE - 1) / GRAND_PRODUCT_TILE; }

#if defined(__HIPCC__)

// one challenge (four words in the ctx's representation) in Montgomery form; clears ok when it is not a canonical element
__device__ __forceinline__ Fe grand_product_challenge(const u64 *w, const FieldConsts &f, u32 mont, bool &ok) {
    Fe c = fe_words(w);
    if (ge_p(c.v, f.p)) ok = false;
    else if (!mont) c = fe_to_mont(c, f);
    return c;
}
// product of the lanes 0 .. lane (prefix) / lane .. 63 (suffix) of one wave
__device__ __forceinline__ Fe fe_wave_prefix(Fe x, u32 lane, const FieldConsts &f) {
    for (u32 d = 1; d < 64; d <<= 1) { const Fe m = fe_mont_mul(fe_shfl_up(x, d), x, f); if (lane >= d) x = m; }
    return x;
}
__device__ __forceinline__ Fe fe_wave_suffix(Fe x, u32 lane, const FieldConsts &f) {
    for (u32 d = 1; d < 64; d <<= 1) { const Fe m = fe_mont_mul(fe_shfl_down(x, d), x, f); if (lane + d < 64) x = m; }
    return x;
}

// tiles: the n, d of a thread's four rows -> pair[0] = prod n, pair[1] = prod d over the workgroup's 1,024 rows
__device__ __forceinline__ void grand_product_tile(const Fe (&n)[4], const Fe (&d)[4], Fe *pair, const FieldConsts &f) {
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Fe tn = fe_mont_mul(fe_mont_mul(n[0], n[1], f), fe_mont_mul(n[2], n[3], f), f);
    Fe td = fe_mont_mul(fe_mont_mul(d[0], d[1], f), fe_mont_mul(d[2], d[3], f), f);
    for (int s = 32; s; s >>= 1) {
        Fe on, od;
        for (int k = 0; k < 4; ++k) { on.v[k] = __shfl_xor(tn.v[k], s); od.v[k] = __shfl_xor(td.v[k], s); }
        tn = fe_mont_mul(tn, on, f); td = fe_mont_mul(td, od, f);
    }
    if (lane == 0) { wtot[0][wave] = tn; wtot[1][wave] = td; }
    __syncthreads();
    if (tid < 2) pair[tid] = fe_mont_mul(fe_mont_mul(wtot[tid][0], wtot[tid][1], f), fe_mont_mul(wtot[tid][2], wtot[tid][3], f), f);
}

// carry: one wave walks the T pairs tp of one column; lane l takes the tiles [l * per, (l + 1) * per) (none when there are fewer tiles than
// lanes).  N = prod n, D = prod d over all tiles.  D zero: returns false and leaves the pairs as they are.  Otherwise dinv = D^-1 and pair t
// becomes {start * prod n of the tiles before t, prod d of the tiles behind t * D^-1}; start == nullptr: 1.
__device__ __forceinline__ bool grand_product_carry(Fe *tp, u32 T, u32 lane, const Fe *start, const FieldConsts &f, Fe &N, Fe &D, Fe &dinv) {
    const u32 per = (T + 63) / 64;
    const u32 lo = lane * per < T ? lane * per : T, hi = lo + per < T ? lo + per : T;
    const Fe one = fe_words(f.one);
    Fe pn = one, pd = one;
    for (u32 t = lo; t < hi; ++t) { pn = fe_mont_mul(pn, tp[2 * t], f); pd = fe_mont_mul(pd, tp[2 * t + 1], f); }
    const Fe inc_n = fe_wave_prefix(pn, lane, f), inc_d = fe_wave_suffix(pd, lane, f);
    N = fe_shfl(inc_n, 63); D = fe_shfl(inc_d, 0);
    if (fe_is_zero(D)) return false;
    dinv = fe_to_mont(fe_inv(fe_from_mont(D, f), f), f);      // D is D * R: back to the integer, invert, forth
    Fe run_n = fe_shfl_up(inc_n, 1), run_d = fe_shfl_down(inc_d, 1);
    if (lane == 0) run_n = one;
    if (lane == 63) run_d = one;
    if (start) run_n = fe_mont_mul(run_n, *start, f);
    run_d = fe_mont_mul(run_d, dinv, f);
    for (u32 t = lo; t < hi; ++t) { const Fe x = tp[2 * t]; tp[2 * t] = run_n; run_n = fe_mont_mul(run_n, x, f); }
    for (u32 t = hi; t > lo; --t) { const Fe x = tp[2 * t - 1]; tp[2 * t - 1] = run_d; run_d = fe_mont_mul(run_d, x, f); }
    return true;
}

// scan: the n, d of a thread's four rows and the tile's carry-ins -> the rows tile * TILE .. of the column zc (32 bytes per row)
__device__ __forceinline__ void grand_product_scan(const Fe (&n)[4], const Fe (&d)[4], const Fe *carry, u8 *zc, u32 usable_rows, u32 tile, u32 mont,
                                                   const FieldConsts &f) {
    __shared__ __attribute__((aligned(16))) u8 stage[256 * GRAND_PRODUCT_STAGE_PITCH];
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // serial per lane: pn[j] = n_0 .. n_{j-1} (pn[0] = 1 is not kept), sd[j] = d_j .. d_3
    Fe pn[4], sd[4];
    pn[1] = n[0]; pn[2] = fe_mont_mul(pn[1], n[1], f); pn[3] = fe_mont_mul(pn[2], n[2], f);
    const Fe tn = fe_mont_mul(pn[3], n[3], f);
    sd[3] = d[3]; sd[2] = fe_mont_mul(d[2], sd[3], f); sd[1] = fe_mont_mul(d[1], sd[2], f); sd[0] = fe_mont_mul(d[0], sd[1], f);
    // across the wave, then across the workgroup's four waves through LDS
    const Fe inc_n = fe_wave_prefix(tn, lane, f), inc_d = fe_wave_suffix(sd[0], lane, f);
    if (lane == 63) wtot[0][wave] = inc_n;
    if (lane == 0) wtot[1][wave] = inc_d;
    __syncthreads();
    Fe carry_n = carry[0], carry_d = carry[1];   // start times prod n of the tiles before this one; prod d of the tiles behind it, times D^-1
    for (u32 w = 0; w < wave; ++w) carry_n = fe_mont_mul(carry_n, wtot[0][w], f);
    for (u32 w = wave + 1; w < 4; ++w) carry_d = fe_mont_mul(carry_d, wtot[1][w], f);
    const Fe one = fe_words(f.one);
    Fe ex_n = fe_shfl_up(inc_n, 1), ex_d = fe_shfl_down(inc_d, 1);
    if (lane == 0) ex_n = one;
    if (lane == 63) ex_d = one;
    const Fe cp = fe_mont_mul(carry_n, ex_n, f), cs = fe_mont_mul(ex_d, carry_d, f);
    u8 *mine = stage + tid * GRAND_PRODUCT_STAGE_PITCH;
    auto put = [&](u32 j, const Fe &p, const Fe &s) {   // Z of the thread's row j = (start, prod n before it) * (prod d from it on, D^-1 included)
        const Fe z = fe_mont_mul(p, fe_mont_mul(s, cs, f), f);
        fe_store(mine + 32 * j, mont ? z : fe_from_mont(z, f));
    };
    put(0, cp, sd[0]); put(1, fe_mont_mul(cp, pn[1], f), sd[1]); put(2, fe_mont_mul(cp, pn[2], f), sd[2]); put(3, fe_mont_mul(cp, pn[3], f), sd[3]);
    const u32 row0 = tile * GRAND_PRODUCT_TILE;
    if (tid == 255 && usable_rows == row0 + GRAND_PRODUCT_TILE) {   // usable_rows is a multiple of the tile: Z[usable_rows] has no tile of its own
        Fe z = fe_mont_mul(fe_mont_mul(cp, tn, f), cs, f);
        if (!mont) z = fe_from_mont(z, f);
        st16(zc + (u64)usable_rows * 32, z.v[0], z.v[1]);
        st16(zc + (u64)usable_rows * 32 + 16, z.v[2], z.v[3]);
    }
    __syncthreads();
    // rows row0 .. min(row0 + TILE - 1, usable_rows): the rows behind usable_rows - 1 were computed with n = d = 1, so row usable_rows is Z[usable_rows]
    const u32 left = usable_rows + 1 - row0, nw = left < GRAND_PRODUCT_TILE ? left : GRAND_PRODUCT_TILE;
    for (u32 q = tid; q < 2 * nw; q += 256) {
        const u32 r = q >> 1, h = q & 1u;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(stage + (r >> 2) * GRAND_PRODUCT_STAGE_PITCH + (r & 3u) * 32 + h * 16);
        st16(zc + (u64)(row0 + r) * 32 + h * 16, v.x, v.y);
    }
}

#endif  // __HIPCC__

}  // namespace h2r
