// The integer arithmetic every prover-stage export (h2r_api.hip: lookup, permutation, NTT, quotient, openings, fold, MSM) runs on a
// caller's buffers before a kernel may touch them: alignment, the layout and reach of a block of columns, overlap of two ranges, and
// how many items fit one launch.  Pure host code, no HIP, so that tests/cpp/test_stage_args.cpp can run it without a device.
#pragma once
#include <cstdint>

namespace h2r_stage_args {
using u64 = uint64_t;
using u128 = unsigned __int128;

// a base or one of its strides is not a multiple of 16 bytes (the kernels move 16 bytes per lane)
template <class... Strides> inline bool misaligned(const void *base, Strides... strides) {
    return ((static_cast<u64>(reinterpret_cast<uintptr_t>(base)) | ... | static_cast<u64>(strides)) & 15) != 0;
}

// num_cols x batch columns of `col` bytes: column c of element e starts at base + e * elem_stride + c * col_stride.  A single column
// per element is {base, col, elem_stride, col, 1, batch}; columns shared by every element have elem_stride = 0 (ask extent() only).
struct ColumnBlock {
    const void *base = nullptr;
    u64 col = 0, elem_stride = 0, col_stride = 0;
    uint32_t num_cols = 0;
    u64 batch = 0;
    // strides that hold a column, and columns that do not overlap each other: [element][column] (the element stride covers an
    // element's columns) or [column][element] (the column stride covers every element's)
    bool disjoint() const {
        if (elem_stride < col || col_stride < col) return false;
        const u128 elem_major = (u128)(num_cols - 1) * col_stride + col, col_major = batch ? (u128)(batch - 1) * elem_stride + col : 0;
        return elem_stride >= elem_major || col_stride >= col_major;
    }
    // bytes from the first column's first byte to the last column's last one
    u128 extent() const { return batch ? (u128)(batch - 1) * elem_stride + (u128)(num_cols - 1) * col_stride + col : 0; }
};

// [a0, a0 + a_bytes) and [b0, b0 + b_bytes) share a byte (the interval test: an empty range counts only strictly inside the other)
inline bool overlaps(const void *a0, u128 a_bytes, const void *b0, u128 b_bytes) {
    const u128 a = reinterpret_cast<uintptr_t>(a0), b = reinterpret_cast<uintptr_t>(b0);
    return a < b + b_bytes && b < a + a_bytes;
}
inline bool overlaps(const ColumnBlock &a, const void *b0, u128 b_bytes) { return overlaps(a.base, a.extent(), b0, b_bytes); }
inline bool overlaps(const ColumnBlock &a, const ColumnBlock &b) { return overlaps(a, b.base, b.extent()); }

// The launch limits: a global size (threads) below 2^32, at most 65,535 in a grid dimension; workgroups of 256 threads.
constexpr u64 kMaxGlobalThreads = (1ull << 32) - 1, kMaxGridDim = 65535, kBlockThreads = 256;
// The largest number of items one launch takes, where an item costs `blocks_per_item` workgroups and the items go into one grid
// dimension: min(items, max_grid_dim, floor(max_global_threads / 256 / blocks_per_item)).  0: even one item is too large.
inline u64 slice_items(u64 blocks_per_item, u64 items, u64 max_global_threads = kMaxGlobalThreads, u64 max_grid_dim = kMaxGridDim) {
    const u64 fit = blocks_per_item ? max_global_threads / kBlockThreads / blocks_per_item : items;
    const u64 cap = fit < max_grid_dim ? fit : max_grid_dim;
    return items < cap ? items : cap;
}
// fn(first, count) over [0, total) in slices of at most `per` items, in order; stops at, and returns, the first status that is not 0
template <class Fn> inline int32_t for_each_slice(u64 total, u64 per, Fn &&fn) {
    for (u64 first = 0, count; per && first < total; first += count)
        if (const int32_t rc = fn(first, count = total - first < per ? total - first : per)) return rc;
    return 0;
}
}  // namespace h2r_stage_args
