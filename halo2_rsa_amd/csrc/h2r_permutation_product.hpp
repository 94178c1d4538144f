// halo2's permutation (copy-constraint) argument: the grand-product columns Z of plonk::permutation::prover::commit.  Third-party algorithm
// (halo2, not in the reference tree), restated in DESIGN.md section 2e; parity is pinned against a Python restatement
// (tests/permutation_ref.py, tests/test_permutation_product.py), not against upstream.  Per circuit (= element) its own beta, gamma; m
// permutation columns in S = ceil(m / chunk_len) sets, set s = the columns [s * chunk_len, min(m, (s + 1) * chunk_len)); u = usable_rows:
//   v_c(i)     the value of column c at usable row i: a PHYSICAL column of the advice image (rows [first_row, first_row + rows), 0 elsewhere)
//              or a caller-supplied extra column
//   n_s(i)   = prod_{c in s} (v_c(i) + beta * delta^c * omega^i + gamma),   d_s(i) = prod_{c in s} (v_c(i) + beta * sigma_c(i) + gamma)
//   Z_0[0]   = 1,  Z_s[0] = Z_{s-1}[u],  Z_s[i+1] = Z_s[i] * n_s(i) / d_s(i),  i = 0 .. u - 1
// One inversion per set, as for the lookup argument's Z (h2r_lookup_product.hpp): with D_s = prod_i d_s(i), N_s = prod_i n_s(i) and
// start_s = prod_{t < s} N_t / D_t,
//   Z_s[i] = start_s * (prod_{j < i} n_s(j)) * (prod_{j >= i} d_s(j)) * D_s^-1,
// and Z_{S-1}[u] = 1 exactly when prod_s N_s = prod_s D_s (a comparison).  Three launches, and NO workgroup ever waits for another one:
//   perm_product_tiles_kernel   per tile of PERM_PRODUCT_TILE rows of one set: prod n and prod d of the tile -> workspace
//   perm_product_carry_kernel   per element, one wave that walks the sets in order: prefix of the tiles' n, suffix of their d, D_s != 0, D_s^-1
//                               (fe_inv; D_s is in Montgomery form), the tiles' carry-ins (start_s in the prefix one, D_s^-1 in the suffix one)
//                               -> workspace; after the last set prod N == prod D (status)
//   perm_product_scan_kernel    per tile: n, d again, scans serial per lane (four consecutive rows), across the wave with __shfl, across the
//                               four waves through LDS, seeded with the carry-ins; Z leaves through an LDS stage so that every store
//                               instruction covers 1 KB of the column.  Rows behind usable_rows count as n = d = 1, so the tile that holds
//                               row usable_rows - 1 also produces Z_s[usable_rows] (when usable_rows is a multiple of the tile, its last
//                               thread writes that one element).
// All arithmetic is in the Montgomery domain (fe_mont_mul); a canonical ctx converts on load and on store, a Montgomery ctx nothing.
// The kernels are defined in the one translation unit that launches them (h2r_tu_permutation_product.hip, H2R_TU_PERM_PRODUCT: next to the
// lookup product's kernels that unit became the slowest of the build); they share the lookup product's lp_* helpers (loads, shuffles,
// wave prefix / suffix, the challenge check).
#pragma once

#include "h2r_lookup_product.hpp"

namespace h2r {

constexpr u32 PERM_PRODUCT_TILE = 1024;            // rows of a set per workgroup: 256 threads x 4 consecutive rows
constexpr u32 PERM_PRODUCT_LANE_ROWS = 4;
constexpr u32 PERM_PRODUCT_HDR_BYTES = 64;         // per element in the workspace: u32 skip, u32 sets to write; then [set][tile]{Fe n, Fe d}
constexpr u32 PERM_PRODUCT_STAGE_PITCH = 144;      // bytes of a thread's four Z rows in the LDS stage (128 + 16: the threads' rows start on different banks)
constexpr u32 PERM_MAX_COLUMNS = 8;
constexpr u32 PERM_OMEGA_BITS = 28;                // omega^(2^b), b < 28: every row number below 2^28

__host__ __device__ inline u32 perm_product_tiles(u32 usable_rows) { return (usable_rows + PERM_PRODUCT_TILE - 1) / PERM_PRODUCT_TILE; }
__host__ __device__ inline u64 perm_product_slot_bytes(u32 usable_rows, u32 n_sets) {
    return PERM_PRODUCT_HDR_BYTES + 64ull * n_sets * perm_product_tiles(usable_rows);
}

struct PermProductArgs {
    AdviceDst img;                 // (read only) the image, rows [0, rows)
    u64 rows;
    const u8 *extra; u64 extra_elem_stride, extra_col_stride;
    const u8 *sigma; u64 sigma_col_stride;
    const u64 *beta, *gamma;       // [elem][4], the ctx's representation
    u32 usable_rows, first_row, n_tiles, mont;
    u32 m, chunk_len, n_sets;
    u8 src[PERM_MAX_COLUMNS];      // per permutation column: 0..4 = physical advice column, 5 + j = extra column j
    Fe dpow[PERM_MAX_COLUMNS];     // delta^c, Montgomery form
    Fe wpow[PERM_OMEGA_BITS];      // omega^(2^b), Montgomery form
    FieldConsts f;
    u8 *z; u64 z_elem_stride, z_col_stride;
    u8 *status;                    // nullable, never cleared
    u8 *ws;                        // [elem] slots of perm_product_slot_bytes
};

#ifdef H2R_TU_PERM_PRODUCT

struct PpChallenges { Fe beta, gamma; bool ok; };   // Montgomery form; ok: both were canonical elements
__device__ __forceinline__ PpChallenges pp_challenges(const PermProductArgs &a, u64 elem) {
    PpChallenges c;
    c.ok = true;
    c.beta = lp_challenge(a.beta + elem * 4, a.f, a.mont, c.ok); c.gamma = lp_challenge(a.gamma + elem * 4, a.f, a.mont, c.ok);
    return c;
}
__device__ __forceinline__ u8 *pp_slot(const PermProductArgs &a, u64 elem) { return a.ws + elem * perm_product_slot_bytes(a.usable_rows, a.n_sets); }
__device__ __forceinline__ Fe *pp_tiles(u8 *slot, const PermProductArgs &a, u32 set) {
    return reinterpret_cast<Fe *>(slot + PERM_PRODUCT_HDR_BYTES) + 2ull * set * a.n_tiles;
}
// beta * delta^c of every column, once per workgroup (the caller synchronises)
__device__ __forceinline__ void pp_beta_labels(const PermProductArgs &a, const PpChallenges &c, u32 tid, Fe *bl) {
    if (tid < PERM_MAX_COLUMNS) bl[tid] = tid < a.m ? fe_mont_mul(c.beta, a.dpow[tid], a.f) : fe_zero();
}
// n, d of row r of one set, the columns [c0, c1) (Montgomery form); w = omega^r; a row behind usable_rows counts as 1 / 1
__device__ __forceinline__ void pp_term(const PermProductArgs &a, const u8 *img, const u8 *ext, u32 r, u32 c0, u32 c1, const PpChallenges &c,
                                        const Fe *bl, const Fe &w, Fe &n, Fe &d) {
    n = lp_words(a.f.one); d = n;
    if (r >= a.usable_rows) return;
    const bool in_image = r >= a.first_row && (u64)(r - a.first_row) < a.rows;
    for (u32 col = c0; col < c1; ++col) {
        const u32 src = a.src[col];
        Fe v = fe_zero();   // (an unassigned cell)
        if (src < 5) { if (in_image) v = lp_load(img + (u64)(r - a.first_row) * a.img.row_pitch + (u64)src * a.img.col_pitch); }
        else v = lp_load(ext + (u64)(src - 5) * a.extra_col_stride + (u64)r * 32);
        Fe sg = lp_load(a.sigma + (u64)col * a.sigma_col_stride + (u64)r * 32);
        if (!a.mont) { v = fe_to_mont(v, a.f); sg = fe_to_mont(sg, a.f); }
        const Fe vg = fe_add(v, c.gamma, a.f.p);   // loaded once, used for both n and d
        const Fe nn = fe_add(vg, fe_mont_mul(bl[col], w, a.f), a.f.p), dd = fe_add(vg, fe_mont_mul(c.beta, sg, a.f), a.f.p);
        if (col == c0) { n = nn; d = dd; }
        else { n = fe_mont_mul(n, nn, a.f); d = fe_mont_mul(d, dd, a.f); }
    }
}
// the four rows tile * TILE + 4 tid + j of a thread
__device__ __forceinline__ void pp_terms(const PermProductArgs &a, u64 elem, u32 set, u32 tile, u32 tid, const PpChallenges &c, const Fe *bl,
                                         Fe (&n)[4], Fe (&d)[4]) {
    const u32 r0 = tile * PERM_PRODUCT_TILE + PERM_PRODUCT_LANE_ROWS * tid;
    Fe w0 = lp_words(a.f.one);   // omega^r0 from the set bits of r0 (a multiple of four; every usable row is below 2^28), then times omega per row
    if (r0 < a.usable_rows)
        for (u32 b = 2; b < PERM_OMEGA_BITS; ++b)
            if ((r0 >> b) & 1u) w0 = fe_mont_mul(w0, a.wpow[b], a.f);
    const u32 c0 = set * a.chunk_len, c1 = c0 + a.chunk_len < a.m ? c0 + a.chunk_len : a.m;
    const u8 *img = a.img.base + elem * a.img.elem_stride;
    const u8 *ext = a.extra + elem * a.extra_elem_stride;
    const Fe w1 = fe_mont_mul(w0, a.wpow[0], a.f), w2 = fe_mont_mul(w1, a.wpow[0], a.f), w3 = fe_mont_mul(w2, a.wpow[0], a.f);
    pp_term(a, img, ext, r0, c0, c1, c, bl, w0, n[0], d[0]); pp_term(a, img, ext, r0 + 1, c0, c1, c, bl, w1, n[1], d[1]);
    pp_term(a, img, ext, r0 + 2, c0, c1, c, bl, w2, n[2], d[2]); pp_term(a, img, ext, r0 + 3, c0, c1, c, bl, w3, n[3], d[3]);
}

__global__ __launch_bounds__(256) void perm_product_tiles_kernel(PermProductArgs a) {
    __shared__ Fe bl[PERM_MAX_COLUMNS];
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, set = blockIdx.y;
    const u64 elem = blockIdx.z;
    u8 *slot = pp_slot(a, elem);
    const bool skip = a.status && a.status[elem];   // the status on entry: the carry kernel, which writes statuses, reads this copy
    if (tile == 0 && set == 0 && tid == 0) reinterpret_cast<u32 *>(slot)[0] = skip ? 1u : 0u;
    if (skip) return;
    const PpChallenges c = pp_challenges(a, elem);
    if (!c.ok) return;   // H2R_E_SHAPE, set by the carry kernel
    pp_beta_labels(a, c, tid, bl);
    __syncthreads();
    Fe n[4], d[4];
    pp_terms(a, elem, set, tile, tid, c, bl, n, d);
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
        pp_tiles(slot, a, set)[2 * tile + tid] = x;
    }
}

// one wave per element, the sets in order; lane l takes the tiles [l * per, (l + 1) * per) of each set (none when there are fewer tiles than lanes)
__global__ __launch_bounds__(64) void perm_product_carry_kernel(PermProductArgs a) {
    const u32 lane = threadIdx.x;
    const u64 elem = blockIdx.x;
    u8 *slot = pp_slot(a, elem);
    u32 *hdr = reinterpret_cast<u32 *>(slot);
    if (hdr[0]) { if (lane == 0) hdr[1] = 0; return; }   // status nonzero on entry: skipped
    const PpChallenges c = pp_challenges(a, elem);
    if (!c.ok) {
        if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_SHAPE; hdr[1] = 0; }
        return;
    }
    const u32 T = a.n_tiles, per = (T + 63) / 64;
    const u32 lo = lane * per < T ? lane * per : T, hi = lo + per < T ? lo + per : T;
    const Fe one = lp_words(a.f.one);
    Fe start = one, all_n = one, all_d = one;   // Z_s[0]; prod N_t and prod D_t of the sets so far
    for (u32 s = 0; s < a.n_sets; ++s) {
        Fe *tp = pp_tiles(slot, a, s);
        Fe pn = one, pd = one;
        for (u32 t = lo; t < hi; ++t) { pn = fe_mont_mul(pn, tp[2 * t], a.f); pd = fe_mont_mul(pd, tp[2 * t + 1], a.f); }
        const Fe inc_n = lp_wave_prefix(pn, lane, a.f), inc_d = lp_wave_suffix(pd, lane, a.f);
        const Fe N = lp_shfl(inc_n, 63), D = lp_shfl(inc_d, 0);
        if (fe_is_zero(D)) {   // some v + beta * sigma + gamma of this set is zero: no Z from here on, the sets before it are written
            if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_ASSERTION; hdr[1] = s; }
            return;
        }
        const Fe dinv = fe_to_mont(fe_inv(fe_from_mont(D, a.f), a.f), a.f);      // D is D * R: back to the integer, invert, forth
        Fe run_n = lp_shfl_up(inc_n, 1), run_d = lp_shfl_down(inc_d, 1);
        if (lane == 0) run_n = one;
        if (lane == 63) run_d = one;
        run_n = fe_mont_mul(run_n, start, a.f);
        run_d = fe_mont_mul(run_d, dinv, a.f);
        for (u32 t = lo; t < hi; ++t) { const Fe x = tp[2 * t]; tp[2 * t] = run_n; run_n = fe_mont_mul(run_n, x, a.f); }
        for (u32 t = hi; t > lo; --t) { const Fe x = tp[2 * t - 1]; tp[2 * t - 1] = run_d; run_d = fe_mont_mul(run_d, x, a.f); }
        start = fe_mont_mul(start, fe_mont_mul(N, dinv, a.f), a.f);
        all_n = fe_mont_mul(all_n, N, a.f); all_d = fe_mont_mul(all_d, D, a.f);
    }
    if (lane == 0) {
        if (!fe_eq(all_n, all_d) && a.status) a.status[elem] = (u8)H2R_E_ASSERTION;   // Z_{S-1}[usable_rows] != 1: every column is written as computed
        hdr[1] = a.n_sets;
    }
}

__global__ __launch_bounds__(256) void perm_product_scan_kernel(PermProductArgs a) {
    __shared__ __attribute__((aligned(16))) u8 stage[256 * PERM_PRODUCT_STAGE_PITCH];
    __shared__ Fe bl[PERM_MAX_COLUMNS];
    __shared__ Fe wtot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, set = blockIdx.y;
    const u64 elem = blockIdx.z;
    u8 *slot = pp_slot(a, elem);
    if (set >= reinterpret_cast<const u32 *>(slot)[1]) return;   // skipped, refused, or a zero denominator in this set or one before it
    const PpChallenges c = pp_challenges(a, elem);
    pp_beta_labels(a, c, tid, bl);
    __syncthreads();
    Fe n[4], d[4];
    pp_terms(a, elem, set, tile, tid, c, bl, n, d);
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
    const Fe *tp = pp_tiles(slot, a, set);
    Fe carry_n = tp[2 * tile], carry_d = tp[2 * tile + 1];   // Z_s[0] times prod n of the tiles before this one; prod d of the tiles behind it, times D_s^-1
    for (u32 w = 0; w < wave; ++w) carry_n = fe_mont_mul(carry_n, wtot[0][w], a.f);
    for (u32 w = wave + 1; w < 4; ++w) carry_d = fe_mont_mul(carry_d, wtot[1][w], a.f);
    const Fe one = lp_words(a.f.one);
    Fe ex_n = lp_shfl_up(inc_n, 1), ex_d = lp_shfl_down(inc_d, 1);
    if (lane == 0) ex_n = one;
    if (lane == 63) ex_d = one;
    const Fe cp = fe_mont_mul(carry_n, ex_n, a.f), cs = fe_mont_mul(ex_d, carry_d, a.f);
    u8 *mine = stage + tid * PERM_PRODUCT_STAGE_PITCH;
    auto put = [&](u32 j, const Fe &p, const Fe &s) {   // Z of the thread's row j = (Z_s[0], prod n before it) * (prod d from it on, D_s^-1 included)
        Fe z = fe_mont_mul(p, fe_mont_mul(s, cs, a.f), a.f);
        if (!a.mont) z = fe_from_mont(z, a.f);
        reinterpret_cast<ulonglong2 *>(mine + 32 * j)[0] = make_ulonglong2(z.v[0], z.v[1]);
        reinterpret_cast<ulonglong2 *>(mine + 32 * j)[1] = make_ulonglong2(z.v[2], z.v[3]);
    };
    put(0, cp, sd[0]); put(1, fe_mont_mul(cp, pn[1], a.f), sd[1]); put(2, fe_mont_mul(cp, pn[2], a.f), sd[2]); put(3, fe_mont_mul(cp, pn[3], a.f), sd[3]);
    u8 *zc = a.z + elem * a.z_elem_stride + (u64)set * a.z_col_stride;
    const u32 row0 = tile * PERM_PRODUCT_TILE;
    if (tid == 255 && a.usable_rows == row0 + PERM_PRODUCT_TILE) {   // usable_rows is a multiple of the tile: Z_s[usable_rows] has no tile of its own
        Fe z = fe_mont_mul(fe_mont_mul(cp, tn, a.f), cs, a.f);
        if (!a.mont) z = fe_from_mont(z, a.f);
        st16(zc + (u64)a.usable_rows * 32, z.v[0], z.v[1]);
        st16(zc + (u64)a.usable_rows * 32 + 16, z.v[2], z.v[3]);
    }
    __syncthreads();
    // rows row0 .. min(row0 + TILE - 1, usable_rows): the rows behind usable_rows - 1 were computed with n = d = 1, so row usable_rows is Z_s[usable_rows]
    const u32 left = a.usable_rows + 1 - row0, nw = left < PERM_PRODUCT_TILE ? left : PERM_PRODUCT_TILE;
    for (u32 q = tid; q < 2 * nw; q += 256) {
        const u32 r = q >> 1, h = q & 1u;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(stage + (r >> 2) * PERM_PRODUCT_STAGE_PITCH + (r & 3u) * 32 + h * 16);
        st16(zc + (u64)(row0 + r) * 32 + h * 16, v.x, v.y);
    }
}

#endif  // H2R_TU_PERM_PRODUCT

}  // namespace h2r
