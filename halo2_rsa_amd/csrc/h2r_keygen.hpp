// Key generation on the device: the fixed columns of an image's row kinds and the sigma columns of its copy pairs.  DESIGN.md section 2p.
// Both belong to one circuit SHAPE and are built once; what they feed (the commitments of the verifying key) must not depend on launch
// geometry or on the order in which atomics arrive, so every step below has one result whatever the schedule.
//
// keygen_fixed_kernel: a gather.  One lane per (row, column) of the 15 fixed columns (nine gate selectors in h2r_fixed_row's order, the
//   table's tag and value, the composition arguments' tag / enable, the overflow argument's tag / enable), grid (row tile of 256, column):
//   adjacent lanes take adjacent rows of one column, a wavefront stores 2 KB contiguous.  The per-kind rows come from the host's
//   h2r_advice_fixed_row_ex as a table of 256 kinds x 13 values in the ctx's representation (KgKind); the table's rows as small integers.
//   A kind without a fixed row raises the status byte (H2R_E_SHAPE) and leaves zeros.
//
// sigma: sigma_c[r] = the label delta^c' omega^r' of the NEXT cell of (c, r)'s copy class in ascending (column, row) order, cyclically.
//   Cell id = c * 2^k + r < 2^27.  The launches, none of which waits for another workgroup:
//   init      label[id] = id, touched[id] = 0
//   mark      per pair: refusals into the status byte; touched[] = 1 for both cells of a kept pair (equal-valued plain stores)
//   hook      per pair: the roots ra, rb of both cells (label[] followed down to label[x] == x); where they differ atomicMin(label[max], min)
//             and the `changed` word is raised.  Labels only decrease and stay inside their class.
//   compress  per pair: both cells take their root (atomicMin again: a label never rises).  The host reads `changed` after each hook +
//             compress round and stops at the first round that changed nothing: then every pair's cells share a root, a root is the
//             smallest id of its class (every chain descends to it), and every touched cell carries it.  The fixed point is unique, so
//             the labels do not depend on the order of the atomics.
//   count / tile_scan / compact   the touched cells in id order: per tile of 1,024 ids a count, one workgroup's exclusive scan over
//             the tiles, an order-preserving scan inside the tile -> vals[] = ids ascending, keys[] = their labels
//   sort      a STABLE least-significant-digit radix sort of (key, val) by key, 8-bit digits: per pass a histogram per tile of 1,024
//             entries (LDS integer adds), a digit-major exclusive scan over the tiles by one workgroup, and a scatter that ranks equal
//             digits inside the tile in entry order -- by ballots inside a wavefront, wave after wave through an LDS counter, no
//             atomics -- so that equal keys keep their ascending ids
//   identity  sigma = the cells' own labels: one power per lane, then three steps of omega^256
//   scatter   per sorted entry: the successor is the right neighbour if it has the same key, else the key itself (the class's smallest
//             id, its first entry); its label is computed from (c', r') by a power and stored at the entry's own cell
// Arithmetic in the Montgomery domain; a canonical ctx converts on store.
#pragma once

#include "h2r_field.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 KG_NUM_FIXED = 15, KG_KIND_VALUES = 13, KG_LANES = 256, KG_TILE = 1024, KG_MAX_COLUMNS = 8;
constexpr u32 KG_MAX_LOG_N = 24;                    // ids below 8 * 2^24 = 2^27
constexpr u32 KG_ABSENT = 15;                       // col_map's nibble of a physical column that is no permutation column
constexpr u32 KG_CTRL_WORDS = 64;                   // ctrl[0] = changed, ctrl[1] = the number of touched cells
// launch_keygen_sigma's phases (a launch with an empty grid -- no pairs, no touched cells -- is the caller's to leave out)
enum { KG_PHASE_INIT = 0, KG_PHASE_MARK, KG_PHASE_HOOK, KG_PHASE_COMPRESS, KG_PHASE_COUNT, KG_PHASE_TILE_SCAN, KG_PHASE_COMPACT, KG_PHASE_SORT_HIST,
       KG_PHASE_SORT_SCAN, KG_PHASE_SORT_SCATTER, KG_PHASE_IDENTITY, KG_PHASE_SCATTER };

// a kind's values in the ctx's representation: sa .. s_const, tag_composition, its enable, tag_overflow, its enable
struct KgKind { Fe v[KG_KIND_VALUES]; u32 valid, pad_[7]; };
struct KgTableRow { u32 tag, value; };

struct KeygenFixedArgs {
    const u8 *kinds; u64 rows;      // the image's row kinds (device)
    u32 first_row, log_n, table_rows, mont;
    const KgKind *tab;              // [256] (device)
    const KgTableRow *table;        // [table_rows] (device)
    u8 *out; u64 col_stride;        // column c at out + c * col_stride, 2^log_n rows of 32 bytes
    u8 *status;                     // one byte, never cleared
    FieldConsts f;
};

struct KeygenSigmaArgs {
    const h2r_copy *copies; u64 n_copies;
    u32 first_row, usable_rows, log_n, m;
    u32 n_cells, n_tiles;           // m << log_n; tiles of KG_TILE ids
    u32 n_touched, sort_tiles;      // (from the compaction on) the sorted list's length and its tiles of KG_TILE entries
    u32 shift, src;                 // of one sort pass: the digit's shift, which of the two buffers is read
    u32 col_map, mont;              // nibble p = the permutation column of physical column p, or KG_ABSENT
    u32 *label, *touched, *tile_count, *ctrl, *hist;
    u32 *keys[2], *vals[2];
    Fe dpow[KG_MAX_COLUMNS];        // delta^c, Montgomery form
    Fe wpow[KG_MAX_LOG_N];          // omega^(2^b), Montgomery form
    FieldConsts f;
    u8 *sigma; u64 col_stride;
    u8 *status;                     // one byte, never cleared
};

#ifdef H2R_TU_KEYGEN

__global__ __launch_bounds__(KG_LANES) void keygen_fixed_kernel(KeygenFixedArgs a) {
    const u64 r = (u64)blockIdx.x * KG_LANES + threadIdx.x;
    const u32 col = blockIdx.y;
    if (r >= (1ull << a.log_n)) return;
    Fe x = fe_zero();
    if (col == 9 || col == 10) {                     // the table: from row 0 on
        if (r < a.table_rows) {
            const KgTableRow t = a.table[r];
            x = fe_small(col == 9 ? t.tag : t.value);
            if (a.mont) x = fe_to_mont(x, a.f);
        }
    } else if (r >= a.first_row && r - a.first_row < a.rows) {
        const KgKind *k = a.tab + a.kinds[r - a.first_row];
        if (!k->valid) { if (col == 0) *a.status = (u8)H2R_E_SHAPE; }
        else x = fe_load(reinterpret_cast<const u8 *>(&k->v[col < 9 ? col : col - 2]));
    }
    fe_store(a.out + (u64)col * a.col_stride + r * 32, x);
}

// ---- sigma ----------------------------------------------------------------------------------------------------------------------------
// a pair's two cell ids: 0 = dropped (an operand outside the image), 1 = kept, 2 = refused
__device__ __forceinline__ u32 kg_pair(const KeygenSigmaArgs &a, u64 i, u32 &ca, u32 &cb) {
    const h2r_copy p = a.copies[i];
    if (p.src_row == H2R_COPY_SRC_A || p.src_row == H2R_COPY_SRC_B || p.src_row == H2R_COPY_SRC_N) return 0;
    const u64 r = (u64)p.row + a.first_row, sr = (u64)p.src_row + a.first_row;
    if (r >= a.usable_rows || sr >= a.usable_rows || p.col >= 5 || p.src_col >= 5) return 2;
    const u32 c = (a.col_map >> (4 * p.col)) & 15u, sc = (a.col_map >> (4 * p.src_col)) & 15u;
    if (c == KG_ABSENT || sc == KG_ABSENT) return 2;
    ca = (c << a.log_n) + (u32)r; cb = (sc << a.log_n) + (u32)sr;
    return 1;
}
// label[] followed down to a root: labels only decrease along the chain, so the walk ends
__device__ __forceinline__ u32 kg_find(const u32 *label, u32 x) {
    for (;;) {
        const u32 l = __atomic_load_n(label + x, __ATOMIC_RELAXED);
        if (l == x) return x;
        x = l;
    }
}
// exclusive prefix of one value per thread over the workgroup's 256 threads; total: their sum
__device__ __forceinline__ u32 kg_block_scan(u32 x, u32 &total) {
    __shared__ u32 wsum[4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 inc = x;
    for (u32 d = 1; d < 64; d <<= 1) { const u32 y = __shfl_up(inc, d); if (lane >= d) inc += y; }
    __syncthreads();                                 // (a second scan in one kernel: the sums of the first have been read)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u32 base = 0;
    for (u32 w = 0; w < wave; ++w) base += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + inc - x;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_init_kernel(KeygenSigmaArgs a) {
    const u32 id = blockIdx.x * KG_LANES + threadIdx.x;
    if (id < KG_CTRL_WORDS) a.ctrl[id] = 0;
    if (id >= a.n_cells) return;
    a.label[id] = id; a.touched[id] = 0;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_mark_kernel(KeygenSigmaArgs a) {
    const u64 i = (u64)blockIdx.x * KG_LANES + threadIdx.x;
    if (i >= a.n_copies) return;
    u32 ca, cb;
    const u32 what = kg_pair(a, i, ca, cb);
    if (what == 2) *a.status = (u8)H2R_E_SHAPE;
    if (what != 1) return;
    a.touched[ca] = 1; a.touched[cb] = 1;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_hook_kernel(KeygenSigmaArgs a) {
    const u64 i = (u64)blockIdx.x * KG_LANES + threadIdx.x;
    if (i >= a.n_copies) return;
    u32 ca, cb;
    if (kg_pair(a, i, ca, cb) != 1) return;
    const u32 ra = kg_find(a.label, ca), rb = kg_find(a.label, cb);
    if (ra == rb) return;
    atomicMin(a.label + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    a.ctrl[0] = 1;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_compress_kernel(KeygenSigmaArgs a) {
    const u64 i = (u64)blockIdx.x * KG_LANES + threadIdx.x;
    if (i >= a.n_copies) return;
    u32 c[2];
    if (kg_pair(a, i, c[0], c[1]) != 1) return;
    for (int s = 0; s < 2; ++s) {
        const u32 r = kg_find(a.label, c[s]);
        if (r != c[s]) atomicMin(a.label + c[s], r);
    }
}

// the thread's four consecutive ids of a tile and their touched flags
__device__ __forceinline__ u32 kg_flags(const KeygenSigmaArgs &a, u32 id0, u32 (&fl)[4]) {
    u32 n = 0;
    for (u32 j = 0; j < 4; ++j) { fl[j] = id0 + j < a.n_cells ? a.touched[id0 + j] : 0u; n += fl[j]; }
    return n;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_count_kernel(KeygenSigmaArgs a) {
    u32 fl[4], total;
    const u32 n = kg_flags(a, blockIdx.x * KG_TILE + 4 * threadIdx.x, fl);
    kg_block_scan(n, total);
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = total;
}

// one workgroup: tile_count[] becomes its exclusive prefix, ctrl[1] the total
__global__ __launch_bounds__(KG_LANES) void keygen_sigma_tile_scan_kernel(KeygenSigmaArgs a) {
    const u32 per = (a.n_tiles + KG_LANES - 1) / KG_LANES;
    const u32 lo = threadIdx.x * per < a.n_tiles ? threadIdx.x * per : a.n_tiles, hi = lo + per < a.n_tiles ? lo + per : a.n_tiles;
    u32 sum = 0, total;
    for (u32 t = lo; t < hi; ++t) sum += a.tile_count[t];
    u32 run = kg_block_scan(sum, total);
    for (u32 t = lo; t < hi; ++t) { const u32 c = a.tile_count[t]; a.tile_count[t] = run; run += c; }
    if (threadIdx.x == 0) a.ctrl[1] = total;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_compact_kernel(KeygenSigmaArgs a) {
    u32 fl[4], total;
    const u32 id0 = blockIdx.x * KG_TILE + 4 * threadIdx.x;
    const u32 n = kg_flags(a, id0, fl);
    u32 pos = a.tile_count[blockIdx.x] + kg_block_scan(n, total);
    for (u32 j = 0; j < 4; ++j)
        if (fl[j]) { a.vals[0][pos] = id0 + j; a.keys[0][pos] = a.label[id0 + j]; ++pos; }
}

// entry j * 256 + tid of the tile, j < 4: the order the scatter ranks in
__global__ __launch_bounds__(KG_LANES) void keygen_sigma_sort_hist_kernel(KeygenSigmaArgs a) {
    __shared__ u32 h[256];
    const u32 tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    for (u32 j = 0; j < 4; ++j) {
        const u32 i = blockIdx.x * KG_TILE + j * KG_LANES + tid;
        if (i < a.n_touched) atomicAdd(&h[(a.keys[a.src][i] >> a.shift) & 255u], 1u);
    }
    __syncthreads();
    a.hist[blockIdx.x * 256 + tid] = h[tid];
}

// one workgroup, thread d = digit d: hist[tile][d] becomes the position of the tile's first entry with that digit (digit-major)
__global__ __launch_bounds__(KG_LANES) void keygen_sigma_sort_scan_kernel(KeygenSigmaArgs a) {
    const u32 d = threadIdx.x;
    u32 run = 0, total;
    for (u32 t = 0; t < a.sort_tiles; ++t) { const u32 c = a.hist[t * 256 + d]; a.hist[t * 256 + d] = run; run += c; }
    const u32 base = kg_block_scan(run, total);
    for (u32 t = 0; t < a.sort_tiles; ++t) a.hist[t * 256 + d] += base;
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_sort_scatter_kernel(KeygenSigmaArgs a) {
    __shared__ u32 cnt[256];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cnt[tid] = a.hist[blockIdx.x * 256 + tid];
    __syncthreads();
    const u32 *keys = a.keys[a.src], *vals = a.vals[a.src];
    u32 *keys_out = a.keys[a.src ^ 1u], *vals_out = a.vals[a.src ^ 1u];
    for (u32 j = 0; j < 4; ++j) {
        const u32 i = blockIdx.x * KG_TILE + j * KG_LANES + tid;
        const bool valid = i < a.n_touched;
        const u32 key = valid ? keys[i] : 0u, val = valid ? vals[i] : 0u, d = (key >> a.shift) & 255u;
        // the lanes of this wavefront with the same digit
        unsigned long long peers = __ballot(valid);
        for (u32 b = 0; b < 8; ++b) { const unsigned long long bb = __ballot(valid && ((d >> b) & 1u)); peers &= ((d >> b) & 1u) ? bb : ~bb; }
        const u32 rank = __popcll(peers & ((1ull << lane) - 1ull)), same = __popcll(peers);
        u32 pos = 0;
        for (u32 w = 0; w < 4; ++w) {                 // wave after wave: entry order
            if (wave == w && valid) pos = cnt[d] + rank;
            __syncthreads();
            if (wave == w && valid && rank == 0) cnt[d] += same;
            __syncthreads();
        }
        if (valid) { keys_out[pos] = key; vals_out[pos] = val; }
    }
}

// delta^c omega^r in Montgomery form
__device__ __forceinline__ Fe kg_label(const KeygenSigmaArgs &a, u32 c, u32 r) {
    Fe w = a.dpow[0];
    for (u32 k = 1; k < KG_MAX_COLUMNS; ++k) if (k == c) w = a.dpow[k];
    for (u32 b = 0; b < a.log_n; ++b)
        if ((r >> b) & 1u) w = fe_mont_mul(w, a.wpow[b], a.f);
    return w;
}

// grid (row tiles of 1,024, columns): rows tile * 1024 + j * 256 + tid
__global__ __launch_bounds__(KG_LANES) void keygen_sigma_identity_kernel(KeygenSigmaArgs a) {
    const u32 c = blockIdx.y, n = 1u << a.log_n;
    u32 r = blockIdx.x * KG_TILE + threadIdx.x;
    if (r >= n) return;
    Fe w = kg_label(a, c, r);
    u8 *col = a.sigma + (u64)c * a.col_stride;
    for (u32 j = 0; j < 4 && r < n; ++j, r += KG_LANES) {
        fe_store(col + (u64)r * 32, a.mont ? w : fe_from_mont(w, a.f));
        w = fe_mont_mul(w, a.wpow[8], a.f);          // (rows 256 apart exist only where log_n > 8)
    }
}

__global__ __launch_bounds__(KG_LANES) void keygen_sigma_scatter_kernel(KeygenSigmaArgs a) {
    const u32 i = blockIdx.x * KG_LANES + threadIdx.x;
    if (i >= a.n_touched) return;
    const u32 *keys = a.keys[a.src], *vals = a.vals[a.src];
    const u32 key = keys[i], cell = vals[i];
    const u32 next = (i + 1 < a.n_touched && keys[i + 1] == key) ? vals[i + 1] : key;
    const u32 mask = (1u << a.log_n) - 1u;
    const Fe w = kg_label(a, next >> a.log_n, next & mask);
    fe_store(a.sigma + (u64)(cell >> a.log_n) * a.col_stride + (u64)(cell & mask) * 32, a.mont ? w : fe_from_mont(w, a.f));
}

#endif  // H2R_TU_KEYGEN

}  // namespace h2r
