// The openings of halo2's create_proof after h exists: the evaluations of the committed polynomials at x and its rotations (poly::
// eval_polynomial), the witness polynomials of the GWC multi-open (poly::kzg::multiopen::ProverGWC: kate_division of sum_i v^i f_i by X - z
// per distinct point z) and the fold of h's pieces with x^n (vanishing::prover::evaluate).  Third-party behaviour (halo2, not in the
// reference tree), restated in DESIGN.md section 2h; parity is pinned against a Python restatement (tests/opening_ref.py,
// tests/test_open_gpu.py), not against upstream.  A column is n_coeffs coefficients f[0 .. n_coeffs) of 32 bytes; per circuit (= element)
// its own points z_p, p < num_points, and its own v; bit p of a column's mask = "queried at point p".
//   eval      evals[e][q] = sum_i f_c[i] z_p^i for the queries q = (c, p) in column order, points ascending within a column
//   witness   g_p = sum_{c in Q_p} v^idx(c) f_c  (Q_p: the columns with bit p, in column order; idx: the position within Q_p, from 0),
//             W_p[i - 1] = g_p[i] + z_p W_p[i] for i = n_coeffs - 1 .. 1, W_p[n_coeffs - 1] = 0, batch_evals[e][p] = g_p[0] + z_p W_p[0]
// Synthetic division is a suffix scan of the affine maps t -> g[i] + z t, and the evaluation is the value that falls out of its low end, so
// both calls have the shape of the grand products (h2r_grand_product.hpp): three launches, and NO workgroup ever waits for another one.
// (The scan here composes affine maps, not factors, so only the Fe helpers of h2r_field.hpp are shared with them.)
// With OPEN_TILE = 1,024 coefficients per tile, Z = z^1024, T_t = sum_{i in tile t} f[i] z^(i - 1024 t):
//   open_tiles_kernel   per (circuit, tile): a thread takes four consecutive coefficients (adjacent lanes load adjacent 128 bytes); per
//                       column and per masked point the lane's 4-term Horner, the wave with __shfl_down and z^4, z^8 .. z^128, the four
//                       waves through LDS with z^256: T_t -> workspace.  A column is read once for all of its points.  For the witness the
//                       same on g_p (grid.y = the point), formed on load by a Horner over the point's columns from the last one down.
//   open_carry_kernel   one wave per (circuit, query or point), the tiles from the top: K_t = T_(t+1) + Z K_(t+1); a lane takes a run of
//                       tiles, the wave combines the runs by shuffle with Z^run.  T_0 + Z K_0 is the evaluation (the batched one for the
//                       witness), written from here; for the witness K_t replaces T_t in the workspace.
//   open_scan_kernel    (witness) per (circuit, point, tile): g again, the suffix scan within the lane, across the wave and across the
//                       waves, seeded with K_t; W[i - 1] leaves through an LDS stage so that one store instruction covers 1 KB.
// Coefficients past n_coeffs in the last tile count as 0 and are not loaded.  z^(2^b), b <= 10, are formed by squaring once per workgroup
// (LDS); no inversion anywhere.  fold_kernel is pointwise: out[i] = sum_c s^c in[c][i] by a Horner over the columns from the top, a thread
// takes four elements 256 apart.
// All arithmetic is fe_mont_mul / fe_add / fe_sub in the Montgomery domain; a canonical ctx converts on load and on store (a Horner whose
// multiplier is in Montgomery form leaves a canonical accumulator canonical, so the fold and the sum that forms g convert nothing per
// column), small per-circuit values on their one store; every result is the canonical representative, so the bytes do not depend on the
// order of operations.  Every helper is force-inlined and takes the argument struct by reference: an outlined one would put the 2 KB
// struct in scratch.  The kernels are defined in the one translation unit that launches them (h2r_tu_open.hip,
// H2R_TU_OPEN).
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 OPEN_MAX_COLUMNS = 64;
constexpr u32 OPEN_MAX_POINTS = 4;
constexpr u32 OPEN_MAX_QUERIES = OPEN_MAX_COLUMNS * OPEN_MAX_POINTS;
constexpr u32 OPEN_MAX_COEFFS = 1u << 24;
constexpr u32 OPEN_LANE_COEFFS = 4;                 // consecutive coefficients of a thread
constexpr u32 OPEN_TILE = 256 * OPEN_LANE_COEFFS;   // coefficients of a workgroup
constexpr u32 OPEN_TILE_LOG = 10;
constexpr u32 OPEN_POW_BITS = OPEN_TILE_LOG + 1;    // z^(2^b), b = 0 .. 10
constexpr u32 OPEN_HDR_BYTES = 64;                  // per circuit in the workspace: u32 skipped on entry, u32 go (the scan's); then [slot][tile] Fe
constexpr u32 OPEN_STAGE_PITCH = 144;               // bytes of a thread's four W rows in the LDS stage (128 + 16: the threads' rows start on different banks)
constexpr u32 FOLD_LANE_ELEMS = 4;                  // elements of a thread, 256 apart
constexpr u32 FOLD_TILE = 256 * FOLD_LANE_ELEMS;

struct OpenCol { const u8 *base; u64 elem_stride; u32 mask, q0; };   // q0: the column's first query

struct OpenArgs {
    OpenCol cols[OPEN_MAX_COLUMNS];
    const u64 *points, *v;          // [circuit][num_points][4], [circuit][4] (witness), the ctx's representation
    u64 *evals;                     // eval: [circuit][n_queries][4]; witness: batch_evals [circuit][num_points][4], nullable
    u8 *status;                     // nullable, never cleared
    u8 *w; u64 w_elem_stride, w_point_stride;
    u8 *ws; u64 slot_bytes;         // [circuit] slots of slot_bytes
    u32 n_coeffs, n_tiles, num_cols, num_points, n_queries, mont, witness, elem0;
    u8 qpoint[OPEN_MAX_QUERIES];    // eval: the point of query q
    u8 point_cols[OPEN_MAX_POINTS]; // columns that are queried at point p
    FieldConsts f;
};

struct FoldArgs {
    const u8 *in; u64 in_elem_stride, in_col_stride;
    const u64 *s;                   // [circuit][4], the ctx's representation
    u8 *status;                     // nullable, never cleared
    u8 *out; u64 out_elem_stride;
    u32 n_coeffs, num_cols, mont, tile0;
    FieldConsts f;
};

__host__ __device__ inline u32 open_tiles_of(u32 n_coeffs) { return (n_coeffs + OPEN_TILE - 1) / OPEN_TILE; }
__host__ __device__ inline u64 open_slot_bytes(u32 n_coeffs, u32 slots) { return OPEN_HDR_BYTES + 32ull * slots * open_tiles_of(n_coeffs); }

#ifdef H2R_TU_OPEN

__device__ __forceinline__ u8 *open_slot(const OpenArgs &a, u64 elem) { return a.ws + elem * a.slot_bytes; }
__device__ __forceinline__ Fe *open_slot_tiles(u8 *slot, const OpenArgs &a, u32 s) { return reinterpret_cast<Fe *>(slot + OPEN_HDR_BYTES) + (u64)s * a.n_tiles; }
// every point of the circuit, and v for the witness, is a canonical element
__device__ __forceinline__ bool open_scalars_ok(const OpenArgs &a, u64 elem) {
    bool ok = true;
    for (u32 p = 0; p < a.num_points; ++p) {
        const Fe z = fe_words(a.points + (elem * a.num_points + p) * 4);
        if (ge_p(z.v, a.f.p)) ok = false;
    }
    if (a.witness) {
        const Fe v = fe_words(a.v + elem * 4);
        if (ge_p(v.v, a.f.p)) ok = false;
    }
    return ok;
}
// what a workgroup of the tiles / scan kernels starts with: z_p^(2^b) of every point and v, Montgomery form.  The caller synchronises.
__device__ __forceinline__ void open_prologue(const OpenArgs &a, u64 elem, u32 tid, Fe (*zp)[OPEN_POW_BITS], Fe *vm) {
    if (tid < a.num_points) {
        Fe z = fe_words(a.points + (elem * a.num_points + tid) * 4);
        if (!a.mont) z = fe_to_mont(z, a.f);
        for (u32 b = 0; b < OPEN_POW_BITS; ++b) { zp[tid][b] = z; z = fe_mont_mul(z, z, a.f); }
    }
    if (tid == 64 && a.witness) {
        const Fe v = fe_words(a.v + elem * 4);
        *vm = a.mont ? v : fe_to_mont(v, a.f);
    }
}
// the thread's four coefficients i0 .. i0 + 3 of one column, Montgomery form; past n_coeffs: 0, not loaded
__device__ __forceinline__ void open_coeffs(const OpenArgs &a, const u8 *col, u32 i0, Fe (&f)[4]) {
#pragma unroll
    for (u32 j = 0; j < OPEN_LANE_COEFFS; ++j) {
        f[j] = fe_zero();
        if (i0 + j < a.n_coeffs) f[j] = fe_load_mont(col + (u64)(i0 + j) * 32, a.mont, a.f);
    }
}
// g_p's four coefficients, Montgomery form: a Horner in v over the point's columns from the last one down
__device__ __forceinline__ void open_form_g(const OpenArgs &a, u64 elem, u32 p, u32 i0, const Fe &vm, Fe (&g)[4]) {
#pragma unroll
    for (u32 j = 0; j < OPEN_LANE_COEFFS; ++j) g[j] = fe_zero();
    if (i0 >= a.n_coeffs) return;
    bool first = true;
    for (u32 k = a.num_cols; k > 0; --k) {
        const OpenCol &c = a.cols[k - 1];
        if (!((c.mask >> p) & 1u)) continue;
        const u8 *col = c.base + elem * c.elem_stride;
#pragma unroll
        for (u32 j = 0; j < OPEN_LANE_COEFFS; ++j) {
            if (!first) g[j] = fe_mont_mul(g[j], vm, a.f);
            if (i0 + j < a.n_coeffs) g[j] = fe_add(g[j], fe_load(col + (u64)(i0 + j) * 32), a.f.p);
        }
        first = false;
    }
    if (!a.mont) {
#pragma unroll
        for (u32 j = 0; j < OPEN_LANE_COEFFS; ++j) g[j] = fe_to_mont(g[j], a.f);
    }
}
// sum_j f[j] z^j
__device__ __forceinline__ Fe open_horner4(const Fe (&f)[4], const Fe &z, const FieldConsts &fc) {
    Fe h = fe_add(fe_mont_mul(f[3], z, fc), f[2], fc.p);
    h = fe_add(fe_mont_mul(h, z, fc), f[1], fc.p);
    return fe_add(fe_mont_mul(h, z, fc), f[0], fc.p);
}
// lane 0: sum_l x_l z^(4 l) over the wave (zp = z^(2^b) of the point); the other lanes hold partial sums that nobody reads
__device__ __forceinline__ Fe open_wave_sum(Fe x, const Fe *zp, const FieldConsts &fc) {
    for (u32 s = 0; s < 6; ++s) x = fe_add(x, fe_mont_mul(fe_shfl_down(x, 1u << s), zp[2 + s], fc), fc.p);
    return x;
}
// the four waves' sums -> the tile's
__device__ __forceinline__ Fe open_tile_sum(const Fe *wt, const Fe *zp, const FieldConsts &fc) {
    Fe t = fe_add(fe_mont_mul(wt[3], zp[8], fc), wt[2], fc.p);
    t = fe_add(fe_mont_mul(t, zp[8], fc), wt[1], fc.p);
    return fe_add(fe_mont_mul(t, zp[8], fc), wt[0], fc.p);
}

// grid (tiles, 1 | points, circuits of one launch)
__global__ __launch_bounds__(256) void open_tiles_kernel(OpenArgs a) {
    __shared__ Fe zp[OPEN_MAX_POINTS][OPEN_POW_BITS];
    __shared__ Fe vm;
    __shared__ Fe wt[2][OPEN_MAX_POINTS][4];
    __shared__ u32 state;
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const u64 elem = (u64)a.elem0 + blockIdx.z;
    u8 *slot = open_slot(a, elem);
    if (tid == 0) {
        const bool skip = a.status && a.status[elem];       // the status on entry: the carry kernel, which writes statuses, reads this copy
        if (tile == 0 && blockIdx.y == 0) reinterpret_cast<u32 *>(slot)[0] = skip ? 1u : 0u;
        state = !skip && open_scalars_ok(a, elem) ? 0u : 1u;   // not canonical: H2R_E_SHAPE, set by the carry kernel
    }
    __syncthreads();
    if (state) return;
    open_prologue(a, elem, tid, zp, &vm);
    __syncthreads();
    const u32 i0 = tile * OPEN_TILE + OPEN_LANE_COEFFS * tid;
    if (a.witness) {
        const u32 p = blockIdx.y;
        if (!a.point_cols[p]) return;
        Fe g[4];
        open_form_g(a, elem, p, i0, vm, g);
        const Fe s = open_wave_sum(open_horner4(g, zp[p][0], a.f), zp[p], a.f);
        if (lane == 0) wt[0][p][wave] = s;
        __syncthreads();
        if (tid == 0) open_slot_tiles(slot, a, p)[tile] = open_tile_sum(wt[0][p], zp[p], a.f);
        return;
    }
    for (u32 c = 0; c < a.num_cols; ++c) {
        const u32 mask = a.cols[c].mask, buf = c & 1u;
        Fe f[4];
        open_coeffs(a, a.cols[c].base + elem * a.cols[c].elem_stride, i0, f);
        for (u32 p = 0; p < a.num_points; ++p) {
            if (!((mask >> p) & 1u)) continue;
            const Fe s = open_wave_sum(open_horner4(f, zp[p][0], a.f), zp[p], a.f);
            if (lane == 0) wt[buf][p][wave] = s;
        }
        // one barrier per column: the sums of column c + 1 go to the other half of wt, and those of column c + 2 are written behind the
        // next barrier, after the threads below have read this half
        __syncthreads();
        if (tid < a.num_points && ((mask >> tid) & 1u)) {
            const u32 q = a.cols[c].q0 + (u32)__popc(mask & ((1u << tid) - 1u));
            open_slot_tiles(slot, a, q)[tile] = open_tile_sum(wt[buf][tid], zp[tid], a.f);
        }
    }
}

// one wave per (circuit, query | point): grid (slots, circuits of one launch).  Lane l takes the tiles [l * per, (l + 1) * per)
__global__ __launch_bounds__(64) void open_carry_kernel(OpenArgs a) {
    const u32 lane = threadIdx.x, s = blockIdx.x;
    const u64 elem = (u64)a.elem0 + blockIdx.y;
    u8 *slot = open_slot(a, elem);
    u32 *hdr = reinterpret_cast<u32 *>(slot);
    if (hdr[0]) { if (lane == 0 && s == 0) hdr[1] = 0; return; }   // status nonzero on entry: skipped
    if (!open_scalars_ok(a, elem)) {
        if (lane == 0 && s == 0) { if (a.status) a.status[elem] = (u8)H2R_E_SHAPE; hdr[1] = 0; }
        return;
    }
    if (lane == 0 && s == 0) hdr[1] = 1;
    const u32 p = a.witness ? s : a.qpoint[s];
    if (a.witness && !a.point_cols[p]) return;
    Fe Z = fe_words(a.points + (elem * a.num_points + p) * 4);
    if (!a.mont) Z = fe_to_mont(Z, a.f);
    for (u32 b = 0; b < OPEN_TILE_LOG; ++b) Z = fe_mont_mul(Z, Z, a.f);   // z^1024
    const u32 T = a.n_tiles, per = (T + 63) / 64;
    const u32 lo = lane * per < T ? lane * per : T, hi = lo + per < T ? lo + per : T;
    Fe *tp = open_slot_tiles(slot, a, s);
    Fe run = fe_zero();                        // sum_{t in the run} T_t Z^(t - lo)
    for (u32 t = hi; t > lo; --t) run = fe_add(fe_mont_mul(run, Z, a.f), tp[t - 1], a.f.p);
    Fe pw = fe_words(a.f.one);               // Z^per: every run before the last nonempty one has `per` tiles
    for (u32 b = 32 - (u32)__clz(per); b > 0; --b) {
        pw = fe_mont_mul(pw, pw, a.f);
        if ((per >> (b - 1)) & 1u) pw = fe_mont_mul(pw, Z, a.f);
    }
    Fe inc = run;                              // suffix scan: inc_l = sum_{m >= l} run_m (Z^per)^(m - l)
    for (u32 d = 1; d < 64; d <<= 1) {
        const Fe m = fe_add(inc, fe_mont_mul(fe_shfl_down(inc, d), pw, a.f), a.f.p);
        if (lane + d < 64) inc = m;
        pw = fe_mont_mul(pw, pw, a.f);
    }
    if (a.witness) {
        Fe k = fe_shfl_down(inc, 1);         // K of the run's top tile: what lies above the run
        if (lane == 63) k = fe_zero();
        for (u32 t = hi; t > lo; --t) { const Fe x = tp[t - 1]; tp[t - 1] = k; k = fe_add(fe_mont_mul(k, Z, a.f), x, a.f.p); }
    }
    if (lane == 0 && a.evals) {                // T_0 + Z K_0
        const Fe r = a.mont ? inc : fe_from_mont(inc, a.f);
        u64 *o = a.evals + (elem * (a.witness ? a.num_points : a.n_queries) + s) * 4;
        for (int k = 0; k < 4; ++k) o[k] = r.v[k];
    }
}

// grid (tiles, points, circuits of one launch)
__global__ __launch_bounds__(256) void open_scan_kernel(OpenArgs a) {
    __shared__ __attribute__((aligned(16))) u8 stage[256 * OPEN_STAGE_PITCH];
    __shared__ Fe zp[OPEN_MAX_POINTS][OPEN_POW_BITS];
    __shared__ Fe vm;
    __shared__ Fe wt[4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, p = blockIdx.y;
    const u64 elem = (u64)a.elem0 + blockIdx.z;
    u8 *slot = open_slot(a, elem);
    if (!reinterpret_cast<const u32 *>(slot)[1] || !a.point_cols[p]) return;   // skipped or refused; a point that no column queries
    open_prologue(a, elem, tid, zp, &vm);
    __syncthreads();
    const Fe *z = zp[p];
    const u32 row0 = tile * OPEN_TILE, i0 = row0 + OPEN_LANE_COEFFS * tid;
    Fe g[4];
    open_form_g(a, elem, p, i0, vm, g);
    // across the wave: inc_l = sum_{m >= l} (the lane's 4-term Horner)_m z^(4 (m - l)); across the waves through LDS
    Fe inc = open_horner4(g, z[0], a.f);
    for (u32 s = 0; s < 6; ++s) {
        const Fe m = fe_add(inc, fe_mont_mul(fe_shfl_down(inc, 1u << s), z[2 + s], a.f), a.f.p);
        if (lane + (1u << s) < 64) inc = m;
    }
    if (lane == 0) wt[wave] = inc;
    __syncthreads();
    Fe cw = open_slot_tiles(slot, a, p)[tile];   // K_t, then what lies above this wave: W[the wave's top coefficient]
    for (u32 w = 3; w > wave; --w) cw = fe_add(fe_mont_mul(cw, z[8], a.f), wt[w], a.f.p);
    Fe cin = fe_shfl_down(inc, 1);             // what lies above the lane's four coefficients: W[i0 + 3]
    if (lane == 63) cin = cw;
    else {
        Fe zl = z[2];                            // z^(4 (63 - lane)), 63 - lane >= 1
        bool have = false;
        for (u32 b = 0; b < 6; ++b) {
            if (!(((63 - lane) >> b) & 1u)) continue;
            zl = have ? fe_mont_mul(zl, z[2 + b], a.f) : z[2 + b];
            have = true;
        }
        cin = fe_add(cin, fe_mont_mul(cw, zl, a.f), a.f.p);
    }
    // W[i0 + 2], W[i0 + 1], W[i0], W[i0 - 1]: the thread's rows 3, 2, 1, 0 of the stage (row r of the tile is W[row0 - 1 + r])
    u8 *mine = stage + tid * OPEN_STAGE_PITCH;
    auto step = [&](const Fe &above, const Fe &gj, u32 row) __attribute__((always_inline)) {   // W[i - 1] = g[i] + z W[i] into the thread's stage row
        const Fe w = fe_add(fe_mont_mul(above, z[0], a.f), gj, a.f.p);
        const Fe o = a.mont ? w : fe_from_mont(w, a.f);
        reinterpret_cast<ulonglong2 *>(mine + 32 * row)[0] = make_ulonglong2(o.v[0], o.v[1]);
        reinterpret_cast<ulonglong2 *>(mine + 32 * row)[1] = make_ulonglong2(o.v[2], o.v[3]);
        return w;
    };
    step(step(step(step(cin, g[3], 3), g[2], 2), g[1], 1), g[0], 0);
    u8 *wc = a.w + elem * a.w_elem_stride + (u64)p * a.w_point_stride;
    if (tid == 255 && a.n_coeffs == row0 + OPEN_TILE) {   // n_coeffs is a multiple of the tile: W[n_coeffs - 1] = 0 has no tile of its own
        st16(wc + (u64)(a.n_coeffs - 1) * 32, 0, 0);
        st16(wc + (u64)(a.n_coeffs - 1) * 32 + 16, 0, 0);
    }
    __syncthreads();
    // rows whose index row0 - 1 + r lies in [0, n_coeffs): row 0 of tile 0 is the remainder (the carry kernel's), and the coefficients past
    // n_coeffs - 1 were computed from zeros, so W[n_coeffs - 1] = 0 comes out of the tile that holds index n_coeffs
    for (u32 q = tid; q < 2 * OPEN_TILE; q += 256) {
        const u32 r = q >> 1, h = q & 1u;
        const u64 idx = (u64)row0 + r;           // W index + 1
        if (idx == 0 || idx > a.n_coeffs) continue;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(stage + (r >> 2) * OPEN_STAGE_PITCH + (r & 3u) * 32 + h * 16);
        st16(wc + (idx - 1) * 32 + h * 16, v.x, v.y);
    }
}

// grid (circuits, tiles of one launch): out[i] = sum_c s^c in[c][i]
__global__ __launch_bounds__(256) void fold_kernel(FoldArgs a) {
    __shared__ Fe sm;          // s, Montgomery form
    __shared__ u32 state;      // 0: go, 1: skipped or refused
    const u32 tid = threadIdx.x, tile = a.tile0 + blockIdx.y;
    const u64 elem = blockIdx.x;
    if (tid == 0) {
        u32 st = a.status && a.status[elem] ? 1u : 0u;
        if (!st) {
            const Fe s = fe_words(a.s + elem * 4);
            if (ge_p(s.v, a.f.p)) {
                st = 1u;
                if (a.status && tile == 0) a.status[elem] = (u8)H2R_E_SHAPE;   // not a canonical scalar: nothing is written for this circuit
            } else sm = a.mont ? s : fe_to_mont(s, a.f);
        }
        state = st;
    }
    __syncthreads();
    if (state) return;
    const Fe s = sm;
    const u8 *in = a.in + elem * a.in_elem_stride;
    u8 *out = a.out + elem * a.out_elem_stride;
    u32 i = tile * FOLD_TILE + tid;
#pragma unroll 1
    for (u32 q = 0; q < FOLD_LANE_ELEMS && i < a.n_coeffs; ++q, i += 256) {
        // (the accumulator stays in the representation of the columns: s is the only Montgomery-form factor of every product)
        Fe acc = fe_load(in + (u64)(a.num_cols - 1) * a.in_col_stride + (u64)i * 32);
        for (u32 c = a.num_cols - 1; c > 0; --c) acc = fe_add(fe_mont_mul(acc, s, a.f), fe_load(in + (u64)(c - 1) * a.in_col_stride + (u64)i * 32), a.f.p);
        st16(out + (u64)i * 32, acc.v[0], acc.v[1]);
        st16(out + (u64)i * 32 + 16, acc.v[2], acc.v[3]);
    }
}

#endif  // H2R_TU_OPEN

}  // namespace h2r
