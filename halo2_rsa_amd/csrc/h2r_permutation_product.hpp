// halo2's permutation (copy-constraint) argument: the grand-product columns Z of plonk::permutation::prover::commit.  Third-party algorithm
// (halo2, not in the reference tree), restated in DESIGN.md section 2e; parity is pinned against a Python restatement
// (tests/permutation_ref.py, tests/test_permutation_product.py), not against upstream.  Per circuit (= element) its own beta, gamma; m
// permutation columns in S = ceil(m / chunk_len) sets, set s = the columns [s * chunk_len, min(m, (s + 1) * chunk_len)); u = usable_rows:
//   v_c(i)     the value of column c at usable row i: a PHYSICAL column of the advice image (rows [first_row, first_row + rows), 0 elsewhere)
//              or a caller-supplied extra column
//   n_s(i)   = prod_{c in s} (v_c(i) + beta * delta^c * omega^i + gamma),   d_s(i) = prod_{c in s} (v_c(i) + beta * sigma_c(i) + gamma)
//   Z_0[0]   = 1,  Z_s[0] = Z_{s-1}[u],  Z_s[i+1] = Z_s[i] * n_s(i) / d_s(i),  i = 0 .. u - 1
// Every Z_s is the grand product of h2r_grand_product.hpp with start_s = Z_{s-1}[u] = prod_{t < s} N_t / D_t (N_s = prod_i n_s(i), D_s =
// prod_i d_s(i)): one inversion per set, and Z_{S-1}[u] = 1 exactly when prod_s N_s = prod_s D_s (a comparison).  The three launches:
//   perm_product_tiles_kernel   copies the status on entry into the slot's header, then the tile's pair of one set
//   perm_product_carry_kernel   per element, one wave that walks the sets in order: refuses (H2R_E_SHAPE), or per set D_s != 0 and the
//                               carry-ins with start_s; after the last set prod N == prod D (H2R_E_ASSERTION); the number of sets to write
//   perm_product_scan_kernel    writes Z_s of the sets below that number
// The kernels are defined in the one translation unit that launches them (h2r_tu_permutation_product.hip, H2R_TU_PERM_PRODUCT: next to the
// lookup product's kernels that unit became the slowest of the build).
#pragma once

#include "h2r_grand_product.hpp"

namespace h2r {

// DEPRECATED alias of GRAND_PRODUCT_TILE, used by no code of this tree.  The previous revision's tests read `PERM_PRODUCT_TILE = <digits>;`
// out of this file and must still run against this library; delete the two lines in the revision after this one.
constexpr u32 PERM_PRODUCT_TILE = 1024;
static_assert(PERM_PRODUCT_TILE == GRAND_PRODUCT_TILE, "one tile for both grand products");
constexpr u32 PERM_MAX_COLUMNS = 8;
constexpr u32 PERM_OMEGA_BITS = 28;                // omega^(2^b), b < 28: every row number below 2^28

// per element in the workspace: the header (u32 skip, u32 sets to write), then [set][tile]{Fe n, Fe d}
__host__ __device__ inline u64 perm_product_slot_bytes(u32 usable_rows, u32 n_sets) {
    return GRAND_PRODUCT_HDR_BYTES + 64ull * n_sets * grand_product_tiles(usable_rows);
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
    c.beta = grand_product_challenge(a.beta + elem * 4, a.f, a.mont, c.ok); c.gamma = grand_product_challenge(a.gamma + elem * 4, a.f, a.mont, c.ok);
    return c;
}
__device__ __forceinline__ u8 *pp_slot(const PermProductArgs &a, u64 elem) { return a.ws + elem * perm_product_slot_bytes(a.usable_rows, a.n_sets); }
__device__ __forceinline__ Fe *pp_pairs(u8 *slot, const PermProductArgs &a, u32 set) {
    return reinterpret_cast<Fe *>(slot + GRAND_PRODUCT_HDR_BYTES) + 2ull * set * a.n_tiles;
}
// beta * delta^c of every column, once per workgroup (the caller synchronises)
__device__ __forceinline__ void pp_beta_labels(const PermProductArgs &a, const PpChallenges &c, u32 tid, Fe *bl) {
    if (tid < PERM_MAX_COLUMNS) bl[tid] = tid < a.m ? fe_mont_mul(c.beta, a.dpow[tid], a.f) : fe_zero();
}
// n, d of row r of one set, the columns [c0, c1) (Montgomery form); w = omega^r; a row behind usable_rows counts as 1 / 1
__device__ __forceinline__ void pp_term(const PermProductArgs &a, const u8 *img, const u8 *ext, u32 r, u32 c0, u32 c1, const PpChallenges &c,
                                        const Fe *bl, const Fe &w, Fe &n, Fe &d) {
    n = fe_words(a.f.one); d = n;
    if (r >= a.usable_rows) return;
    const bool in_image = r >= a.first_row && (u64)(r - a.first_row) < a.rows;
    for (u32 col = c0; col < c1; ++col) {
        const u32 src = a.src[col];
        Fe v = fe_zero();   // (an unassigned cell)
        if (src < 5) { if (in_image) v = fe_load(img + (u64)(r - a.first_row) * a.img.row_pitch + (u64)src * a.img.col_pitch); }
        else v = fe_load(ext + (u64)(src - 5) * a.extra_col_stride + (u64)r * 32);
        Fe sg = fe_load(a.sigma + (u64)col * a.sigma_col_stride + (u64)r * 32);
        if (!a.mont) { v = fe_to_mont(v, a.f); sg = fe_to_mont(sg, a.f); }   // (one branch: both loads issue together)
        const Fe vg = fe_add(v, c.gamma, a.f.p);   // loaded once, used for both n and d
        const Fe nn = fe_add(vg, fe_mont_mul(bl[col], w, a.f), a.f.p), dd = fe_add(vg, fe_mont_mul(c.beta, sg, a.f), a.f.p);
        if (col == c0) { n = nn; d = dd; }
        else { n = fe_mont_mul(n, nn, a.f); d = fe_mont_mul(d, dd, a.f); }
    }
}
// the four rows tile * TILE + 4 tid + j of a thread
__device__ __forceinline__ void pp_terms(const PermProductArgs &a, u64 elem, u32 set, u32 tile, u32 tid, const PpChallenges &c, const Fe *bl,
                                         Fe (&n)[4], Fe (&d)[4]) {
    const u32 r0 = tile * GRAND_PRODUCT_TILE + GRAND_PRODUCT_LANE_ROWS * tid;
    Fe w0 = fe_words(a.f.one);   // omega^r0 from the set bits of r0 (a multiple of four; every usable row is below 2^28), then times omega per row
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
    const u32 tid = threadIdx.x, tile = blockIdx.x, set = blockIdx.y;
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
    grand_product_tile(n, d, pp_pairs(slot, a, set) + 2 * tile, a.f);
}

// one wave per element, the sets in order
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
    const Fe one = fe_words(a.f.one);
    Fe start = one, all_n = one, all_d = one;   // Z_s[0]; prod N_t and prod D_t of the sets so far
    for (u32 s = 0; s < a.n_sets; ++s) {
        Fe N, D, dinv;
        if (!grand_product_carry(pp_pairs(slot, a, s), a.n_tiles, lane, &start, a.f, N, D, dinv)) {
            // some v + beta * sigma + gamma of this set is zero: no Z from here on, the sets before it are written
            if (lane == 0) { if (a.status) a.status[elem] = (u8)H2R_E_ASSERTION; hdr[1] = s; }
            return;
        }
        start = fe_mont_mul(start, fe_mont_mul(N, dinv, a.f), a.f);
        all_n = fe_mont_mul(all_n, N, a.f); all_d = fe_mont_mul(all_d, D, a.f);
    }
    if (lane == 0) {
        if (!fe_eq(all_n, all_d) && a.status) a.status[elem] = (u8)H2R_E_ASSERTION;   // Z_{S-1}[usable_rows] != 1: every column is written as computed
        hdr[1] = a.n_sets;
    }
}

__global__ __launch_bounds__(256) void perm_product_scan_kernel(PermProductArgs a) {
    __shared__ Fe bl[PERM_MAX_COLUMNS];
    const u32 tid = threadIdx.x, tile = blockIdx.x, set = blockIdx.y;
    const u64 elem = blockIdx.z;
    u8 *slot = pp_slot(a, elem);
    if (set >= reinterpret_cast<const u32 *>(slot)[1]) return;   // skipped, refused, or a zero denominator in this set or one before it
    const PpChallenges c = pp_challenges(a, elem);
    pp_beta_labels(a, c, tid, bl);
    __syncthreads();
    Fe n[4], d[4];
    pp_terms(a, elem, set, tile, tid, c, bl, n, d);
    grand_product_scan(n, d, pp_pairs(slot, a, set) + 2 * tile, a.z + elem * a.z_elem_stride + (u64)set * a.z_col_stride, a.usable_rows, tile, a.mont, a.f);
}

#endif  // H2R_TU_PERM_PRODUCT

}  // namespace h2r
