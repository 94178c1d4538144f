// Stand-alone host test of the prover stages' buffer arithmetic (halo2_rsa_amd/csrc/h2r_stage_args.hpp): alignment, column blocks,
// overlap, launch slices.  The formulas the header replaced are restated below as plain reference functions, as every stage export
// spelled them before, and compared with it over an enumerated grid.  No device, no library: g++ -std=c++17 -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "h2r_stage_args.hpp"

using namespace h2r_stage_args;

static int g_fail = 0;
#define REQUIRE(x) do { if (!(x)) { if (g_fail < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_fail; } } while (0)

// ---- the references: the former ntt_columns_disjoint / ntt_extent, the written-out interval test, the five slice formulas ----------------
static bool ref_disjoint(u64 col, u64 elem_stride, u64 col_stride, uint32_t num_cols, u64 batch) {
    if (elem_stride < col || col_stride < col) return false;
    const u128 elem_major = (u128)(num_cols - 1) * col_stride + col, col_major = batch ? (u128)(batch - 1) * elem_stride + col : 0;
    return elem_stride >= elem_major || col_stride >= col_major;
}
static u128 ref_extent(u64 col, u64 elem_stride, u64 col_stride, uint32_t num_cols, u64 batch) {
    return batch ? (u128)(batch - 1) * elem_stride + (u128)(num_cols - 1) * col_stride + col : 0;
}
static bool ref_overlaps(u128 a0, u128 a1, u128 b0, u128 b1) { return a0 < b1 && b0 < a1; }
// the Z layout test of the two product calls as it was: 64-bit, so it wraps for huge strides (z_col_stride >= zcol was checked before it)
static bool ref_z_layout_u64(u64 zcol, u64 es, u64 cs, u64 S, u64 batch) {
    const bool elem_major = es >= (S - 1) * cs + zcol;
    const bool col_major = batch == 0 || (es >= zcol && cs >= (batch - 1) * es + zcol);
    return elem_major || col_major;
}
static const u64 kMaxBlocks = ((1ull << 32) - 1) / 256;
static u64 ref_lookup_elems(u64 blocks_per_elem) {   // lookup input, lookup product, permutation product (the loops took min(per, what is left))
    const u64 per = ((1ull << 32) - 1) / (blocks_per_elem * 256);
    return per < 65535 ? per : 65535;
}
static void ref_ntt(u64 tiles, u64 num_cols, u64 batch, u64 *cols_per, u64 *elems_per) {   // columns, then elements
    *cols_per = std::min<u64>({num_cols, 65535, kMaxBlocks / tiles});
    *elems_per = *cols_per ? std::min<u64>({batch, 65535, kMaxBlocks / (tiles * *cols_per)}) : 0;
}
static u64 ref_quotient_tiles(u64 tiles, u64 batch) { return std::min<u64>({tiles, 65535, kMaxBlocks / batch}); }
static u64 ref_fold_tiles(u64 tiles, u64 batch) { return std::min<u64>({tiles, 65535, kMaxBlocks / batch}); }
static u64 ref_open_elems(u64 n_tiles, u64 points, bool witness, u64 batch) {
    const u64 per_elem = n_tiles * (witness ? points : 1u);
    return std::min<u64>({batch, 65535, kMaxBlocks / per_elem});
}
static u64 ref_msm_elems(u64 slices, u64 windows, u64 cols, u64 batch) { return std::min<u64>({batch, 65535, kMaxBlocks / (slices * windows * cols)}); }

static const void *ptr(u64 a) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(a)); }

// no two of the block's columns share a byte (small blocks only)
static bool brute_disjoint(const ColumnBlock &b) {
    std::vector<u64> starts;
    for (u64 e = 0; e < b.batch; ++e)
        for (u64 c = 0; c < b.num_cols; ++c) starts.push_back(e * b.elem_stride + c * b.col_stride);
    std::sort(starts.begin(), starts.end());
    for (size_t i = 1; i < starts.size(); ++i)
        if (starts[i] - starts[i - 1] < b.col) return false;
    return true;
}

static void check_block(u64 base, u64 col, u64 es, u64 cs, uint32_t nc, u64 batch) {
    const ColumnBlock b{ptr(base), col, es, cs, nc, batch};
    REQUIRE(b.disjoint() == ref_disjoint(col, es, cs, nc, batch));
    REQUIRE(b.extent() == ref_extent(col, es, cs, nc, batch));
    if (es < (1ull << 20) && cs < (1ull << 20)) {
        if (b.disjoint()) REQUIRE(brute_disjoint(b));
        // the former 64-bit test of Z agrees wherever it did not wrap, and elements exist (it let batch == 0 through unseen)
        if (cs >= col && batch) REQUIRE(ref_z_layout_u64(col, es, cs, nc, batch) == b.disjoint());
    }
    // against a second block of one column behind, at, and just inside this one's end: the interval test in 128-bit
    for (u64 other : {base, base + 16, (u64)((u128)base + b.extent() - 16), (u64)((u128)base + b.extent()), base - 2048, base - 32}) {
        const ColumnBlock o{ptr(other), 32, 32, 32, 1, 1};
        const bool want = ref_overlaps(base, (u128)base + ref_extent(col, es, cs, nc, batch), other, (u128)other + 32);
        REQUIRE(overlaps(b, o) == want && overlaps(o, b) == want);
        REQUIRE(overlaps(b, ptr(other), 32) == want && overlaps(ptr(other), 32, b.base, b.extent()) == want);
    }
}

static void test_blocks() {
    const u64 bases[] = {0x7f0000000000ull, 1ull << 63, (1ull << 63) - 16, ~0ull - 15};
    for (u64 col : {32ull, 2048ull})
        for (uint32_t nc : {1u, 2u, 5u})
            for (u64 batch : {0ull, 1ull, 2ull, 3ull}) {
                // strides at, just below and just above a column, small multiples of one, and near 2^63 and 2^64 - 16
                std::vector<u64> plain = {0, col - 16, col, col + 16, 2 * col, 3 * col - 16, 3 * col, 5 * col, 5 * col + 16, 10 * col,
                                          (1ull << 63) - 16, 1ull << 63, (1ull << 63) + 16, ~0ull - 15};
                for (u64 base : bases)
                    for (u64 a : plain) {
                        for (u64 b : plain) check_block(base, col, a, b, nc, batch);
                        // ... and at, just below and just above the bound the other stride sets, in both arrangements
                        const u128 em = (u128)(nc - 1) * a + col, cm = batch ? (u128)(batch - 1) * a + col : 0;
                        for (int d : {-16, 0, 16}) {
                            if (em + d <= ~0ull) check_block(base, col, (u64)(em + d), a, nc, batch);   // [element][column]: a = col_stride
                            if (cm + d <= ~0ull) check_block(base, col, a, (u64)(cm + d), nc, batch);   // [column][element]: a = elem_stride
                        }
                    }
            }
    // an empty range at the other's first byte shares nothing (batch == 0 makes every range of a call empty), touching ranges share nothing, one byte does
    REQUIRE(!overlaps(ptr(4096), 0, ptr(4096), 64) && !overlaps(ptr(4096), 64, ptr(4096), 0) && !overlaps(ptr(4096), 0, ptr(4096), 0));
    REQUIRE(!overlaps(ptr(4096), 64, ptr(4160), 64) && overlaps(ptr(4096), 65, ptr(4160), 64) && overlaps(ptr(4160), 64, ptr(4096), 65));
    REQUIRE(overlaps(ptr(~0ull - 15), 16, ptr(~0ull), 1) && !overlaps(ptr(~0ull - 15), 15, ptr(~0ull), (u128)1 << 100));
    // the one input class whose answer changed: three sets, strides of 2^63.  The 64-bit sum 2 * 2^63 + zcol wrapped to zcol.
    REQUIRE(ref_z_layout_u64(32608, 1ull << 63, 1ull << 63, 3, 2));
    REQUIRE(!(ColumnBlock{ptr(4096), 32608, 1ull << 63, 1ull << 63, 3, 2}.disjoint()));
}

static void test_alignment() {
    REQUIRE(!misaligned(ptr(4096)) && !misaligned(ptr(4096), 16ull) && !misaligned(ptr(4096), 0ull, 32ull, 48ull));
    REQUIRE(misaligned(ptr(4104)) && misaligned(ptr(4096), 8ull) && misaligned(ptr(4096), 16ull, 4ull) && misaligned(ptr(4096), 16ull, 32ull, 1ull));
    REQUIRE(!misaligned(ptr(~0ull - 15), ~0ull - 15) && misaligned(ptr(~0ull - 15), ~0ull - 14) && misaligned(nullptr, (uint32_t)24));
}

static void test_slices_small_limits() {
    const u64 G = 1ull << 12, D = 7;   // 16 workgroups of 256 threads per launch, 7 in the sliced dimension
    for (u64 bpi = 1; bpi <= 20; ++bpi)
        for (u64 items = 0; items <= 40; ++items) {
            const u64 per = slice_items(bpi, items, G, D);
            if (items) REQUIRE((per == 0) == (bpi * 256 > G));   // 0 exactly when one item exceeds the global size
            else REQUIRE(per == 0);
            REQUIRE(per <= items && per <= D && per * bpi * 256 <= G);
            if (per < items && per < D) REQUIRE((per + 1) * bpi * 256 > G);   // ... and the largest such number
            u64 next = 0, calls = 0;
            const int32_t rc = for_each_slice(items, per, [&](u64 first, u64 count) {
                REQUIRE(first == next && count >= 1 && count <= per);
                REQUIRE(count == per || first + count == items);   // only the last slice is short
                next = first + count; ++calls;
                return 0;
            });
            REQUIRE(rc == 0 && next == (per ? items : 0) && calls == (per ? (items + per - 1) / per : 0));
        }
    // no workgroups per item: only the grid dimension binds
    REQUIRE(slice_items(0, 100, G, D) == D && slice_items(0, 3, G, D) == 3);
    // the first status that is not 0 ends the walk and comes back
    u64 calls = 0;
    REQUIRE(for_each_slice(10, 3, [&](u64 first, u64) { ++calls; return first == 3 ? -7 : 0; }) == -7 && calls == 2);
    REQUIRE(for_each_slice(~0ull, ~0ull - 1, [&](u64, u64) { return 0; }) == 0);   // (no wrap of `first`)
}

static u64 g_rng = 0x9e3779b97f4a7c15ull;   // xorshift64, fixed seed
static u64 rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static u64 rnd_bits(unsigned max_bits) { return (rnd() >> (64 - 1 - rnd() % max_bits)) | 1; }   // >= 1, of every width up to max_bits

static void test_slices_default_limits() {
    u64 multi = 0, none = 0;
    for (int i = 0; i < 400; ++i) {
        const u64 blocks = rnd_bits(26), items = rnd_bits(22) - (i % 50 == 0), batch = 1 + rnd() % 65535;
        const u64 lookup = ref_lookup_elems(blocks);
        REQUIRE(slice_items(blocks, items) == std::min(items, lookup) && (slice_items(blocks, items ? items : 1) == 0) == (lookup == 0));
        u64 cols_per, elems_per;
        const u64 tiles = rnd_bits(25), num_cols = rnd_bits(18);
        ref_ntt(tiles, num_cols, items, &cols_per, &elems_per);
        REQUIRE(slice_items(tiles, num_cols) == cols_per);
        if (cols_per) REQUIRE(slice_items(tiles * cols_per, items) == elems_per);
        REQUIRE(slice_items(batch, items) == ref_quotient_tiles(items, batch) && slice_items(batch, items) == ref_fold_tiles(items, batch));
        const u64 n_tiles = rnd_bits(22), points = 1 + rnd() % 4;
        REQUIRE(slice_items(n_tiles, items) == ref_open_elems(n_tiles, points, false, items));
        REQUIRE(slice_items(n_tiles * points, items) == ref_open_elems(n_tiles, points, true, items));
        const u64 slices = rnd_bits(14), cols = 1 + rnd() % 32;
        REQUIRE(slice_items(slices * 32 * cols, items) == ref_msm_elems(slices, 32, cols, items));
        const u64 per = slice_items(blocks, items);
        multi += per && per < items; none += items && !per;
    }
    REQUIRE(multi >= 20 && none >= 20);   // the inputs reach the multi-slice launches and the refusals
}

int main() {
    test_alignment();
    test_blocks();
    test_slices_small_limits();
    test_slices_default_limits();
    if (g_fail) { std::printf("STAGE_ARGS_FAILED %d\n", g_fail); return 1; }
    std::printf("STAGE_ARGS_OK\n");
    return 0;
}
