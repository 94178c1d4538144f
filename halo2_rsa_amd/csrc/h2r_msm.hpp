// The commitments of halo2's create_proof: multi-scalar multiplications sum_i s_i P_i over the curve of the ctx's field (h2r_curve.hpp;
// today bn256 G1 for H2R_FIELD_BN254_FR), for many columns of scalars over one array of bases.  DESIGN.md section 2i.
// Pippenger with unsigned windows of MSM_WINDOW_BITS = 8 bits, MSM_WINDOWS = 32 windows; the n points are cut into slices of MSM_SLICE.
// Two launches, and NO workgroup ever waits for another one:
//   msm_bucket_kernel   one workgroup of 256 threads per (slice, window, column, circuit): sum_b b * B_b of the slice's points whose digit in
//                       the window is b -> one projective partial of 96 bytes in the workspace.
//   msm_fold_kernel     one workgroup per (column, circuit): the slices' partials summed per window, a Horner over the windows from the top
//                       (8 doublings each), one conversion to affine, 64 bytes stored.
// THE SKEW BOUND.  The columns a prover commits are not uniform (permuted lookup columns repeat values in long runs, advice cells are short
// integers, selector-like columns are 0 / 1), so no lane owns a bucket while the points are accumulated.  The bucket kernel counting-sorts
// the slice's NON-ZERO digits in LDS (histogram with LDS atomics, prefix sum, 16-bit local indices through the histogram's running copy);
// lane t then takes the t-th run of R = ceil(M / 256) entries of the sorted list (M <= MSM_SLICE non-zero digits): at most
// MSM_SLICE / 256 = 64 mixed additions, whatever the digits are.  Within a run the digits ascend: a group of equal digits that neither
// starts at the run's first entry nor ends at its last lies whole inside the lane and goes straight to its bucket in LDS; the run's first
// and last group (which may continue in the neighbours) become the lane's two entries of a list of 512 (key = digit, point), whose equal
// keys are adjacent.  A segmented inclusive scan over that list (Hillis-Steele keyed by digit: 9 strides x 2 entries per lane = at most 18
// complete additions) leaves each group's sum in its last entry, which stores it to the bucket.  Then lane b forms b * B_b by double-and-add
// (8 doublings, at most 8 additions) and the workgroup tree-reduces (8 additions).  A lane therefore performs at most 64 + 18 + 16 + 8 point
// operations per workgroup: a function of MSM_SLICE and the window width alone.  Zero digits and (0, 0) bases only shorten the list.
// In the fold a lane sums ceil(num_slices / 8) partials of one window (num_slices = ceil(n / MSM_SLICE): a function of n alone), three
// additions combine the eight lanes of a window, and one lane runs the Horner: 248 doublings and 31 additions, a latency tail per call
// that the columns and circuits of a call share -- the call is built for many columns at once.
// All arithmetic is fe_mont_mul / fe_add / fe_sub over the coordinate field in the Montgomery domain, complete formulas throughout; a
// canonical ctx converts a base on load and the result on store.  A scalar's digit is a byte of the integer the 32 bytes mean: the byte
// itself for a canonical ctx, a byte of w * R^-1 mod p for a Montgomery ctx (one field product per scalar per (window, slice) workgroup,
// against eleven per mixed addition).  Results are the canonical representatives of the affine coordinates, (0, 0) for the identity: the
// bytes do not depend on the order of additions (the order in which the sort's running copy hands out positions is not fixed).
// Every helper is force-inlined; no scratch.  The kernels are defined in the one translation unit that launches them (h2r_tu_msm.hip).
#pragma once

#include "h2r_curve.hpp"
#include "h2r_kernels.hpp"

namespace h2r {

constexpr u32 MSM_MAX_COLUMNS = 64;
constexpr u32 MSM_MAX_POINTS = 1u << 24;
constexpr u32 MSM_WINDOW_BITS = 8;
constexpr u32 MSM_WINDOWS = 32;
constexpr u32 MSM_SLICE = 16384;                 // points of a bucket workgroup (16-bit local indices: at most 65,536)
constexpr u32 MSM_PARTIAL_BYTES = 96;            // a projective point
constexpr u32 MSM_FOLD_GROUPS = 8;               // lanes of the fold that share one window's slices

struct MsmCol { const u8 *base; u64 elem_stride; };
struct MsmArgs {
    MsmCol cols[MSM_MAX_COLUMNS];
    const u8 *bases;                // [n][2][4] u64, the ctx's representation
    u8 *status;                     // nullable, never cleared
    u64 *out;                       // [circuit][num_cols][2][4]
    u8 *ws;                         // [circuit][num_cols][window][slice] partials
    u32 n, num_cols, num_slices, mont, elem0, pad_;
    FieldConsts fr;                 // the scalars' field (the ctx's)
    CurveConsts cv;
};

__host__ __device__ inline u32 msm_slices_of(u32 n) { return (n + MSM_SLICE - 1) / MSM_SLICE; }
__host__ __device__ inline u64 msm_workspace_bytes(u32 n, u32 num_cols, u64 batch) {
    return 256 + batch * num_cols * MSM_WINDOWS * msm_slices_of(n) * (u64)MSM_PARTIAL_BYTES;
}

#ifdef H2R_TU_MSM

__device__ __forceinline__ u8 *msm_partial(const MsmArgs &a, u64 elem, u32 col, u32 window, u32 slice) {
    return a.ws + (((elem * a.num_cols + col) * MSM_WINDOWS + window) * a.num_slices + slice) * MSM_PARTIAL_BYTES;
}
// the digit of scalar j of the slice in `window`: a byte of the integer the 32 bytes mean
__device__ __forceinline__ u32 msm_digit(const MsmArgs &a, const u8 *scal, u32 j, u32 window) {
    if (!a.mont) return scal[(u64)j * 32 + window];
    const Fe s = fe_from_mont(fe_load(scal + (u64)j * 32), a.fr);
    const u32 k = window >> 3;
    const u64 w = k == 0 ? s.v[0] : k == 1 ? s.v[1] : k == 2 ? s.v[2] : s.v[3];
    return (u32)(w >> ((window & 7u) * 8)) & 0xffu;
}
__device__ __forceinline__ PtAff msm_load_base(const MsmArgs &a, u64 i) {
    PtAff b; b.x = fe_load(a.bases + i * 64); b.y = fe_load(a.bases + i * 64 + 32);
    if (!a.mont) { b.x = fe_to_mont(b.x, a.cv.fq); b.y = fe_to_mont(b.y, a.cv.fq); }   // ((0, 0) stays (0, 0))
    return b;
}

// grid (num_slices * 32, num_cols, circuits of one launch)
__global__ __launch_bounds__(256) void msm_bucket_kernel(MsmArgs a) {
    __shared__ u32 hist[256];        // the counts, then the running copy of the start offsets
    __shared__ u32 scan[256];
    __shared__ u32 pkey[512];
    __shared__ __align__(16) u8 bucket[256 * MSM_PARTIAL_BYTES];
    __shared__ __align__(16) u8 pool[MSM_SLICE * 3];   // digits (1 byte) and sorted indices (2 bytes); afterwards the 512 entries of the scan
    static_assert(MSM_SLICE * 3 >= 512 * MSM_PARTIAL_BYTES && MSM_SLICE <= 65536, "the scan's entries reuse the sort's arrays; 16-bit indices");
    u8 *digits = pool;
    unsigned short *sorted = reinterpret_cast<unsigned short *>(pool + MSM_SLICE);
    // (the window is rotated by slice, column and circuit: short scalars leave most windows empty, and workgroup ids that are congruent
    // modulo 8 share an XCD -- a fixed window per id would put all of a call's loaded workgroups on one eighth of the device)
    const u32 tid = threadIdx.x, slice = blockIdx.x / MSM_WINDOWS, col = blockIdx.y;
    const u32 window = (blockIdx.x + slice + col + blockIdx.z) % MSM_WINDOWS;
    const u64 elem = (u64)a.elem0 + blockIdx.z;
    if (a.status && a.status[elem]) return;               // nonzero on entry: skipped, nothing is written
    const u32 i0 = slice * MSM_SLICE, cnt = min(MSM_SLICE, a.n - i0);
    const u8 *scal = a.cols[col].base + elem * a.cols[col].elem_stride + (u64)i0 * 32;
    const PtProj ident = pt_identity(a.cv);

    hist[tid] = 0;
    pt_store(bucket + tid * MSM_PARTIAL_BYTES, ident);
    __syncthreads();
    for (u32 j = tid; j < cnt; j += 256) {
        const u32 d = msm_digit(a, scal, j, window);
        digits[j] = (u8)d;
        if (d) atomicAdd(&hist[d], 1u);
    }
    __syncthreads();
    const u32 mine = hist[tid];
    scan[tid] = mine;
    __syncthreads();
    for (u32 s = 1; s < 256; s <<= 1) {
        const u32 t = tid >= s ? scan[tid - s] : 0u;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
    }
    const u32 M = scan[255];                              // non-zero digits of the slice
    hist[tid] = scan[tid] - mine;                         // where digit tid's entries start
    __syncthreads();
    for (u32 j = tid; j < cnt; j += 256) {
        const u32 d = digits[j];
        if (d) sorted[atomicAdd(&hist[d], 1u)] = (unsigned short)j;
    }
    __syncthreads();

    // the lane's run of the sorted list
    const u32 R = (M + 255) / 256, lo = min(tid * R, M), hi = min(lo + R, M);
    PtProj acc = ident, head = ident;
    u32 cur = 0, head_key = 0;
#pragma unroll 1
    for (u32 k = lo; k < hi; ++k) {
        const u32 idx = sorted[k], d = digits[idx];
        if (d != cur) {
            if (cur) {
                if (!head_key) { head = acc; head_key = cur; }                 // the run's first group: it may continue in the lane before
                else pt_store(bucket + cur * MSM_PARTIAL_BYTES, acc);     // a group that lies whole inside this lane
            }
            cur = d; acc = ident;
        }
        acc = pt_add_affine(acc, msm_load_base(a, (u64)i0 + idx), a.cv);
    }
    __syncthreads();                                      // the sort's arrays are dead from here on
    {   // entries 2 tid and 2 tid + 1 of the list: (first group, last group); a run of one group adds (its digit, identity)
        u8 *e0 = pool + (2 * tid) * MSM_PARTIAL_BYTES, *e1 = e0 + MSM_PARTIAL_BYTES;
        if (!head_key) { pt_store(e0, acc); pt_store(e1, ident); pkey[2 * tid] = cur; pkey[2 * tid + 1] = cur; }   // (cur = 0: an empty run)
        else { pt_store(e0, head); pt_store(e1, acc); pkey[2 * tid] = head_key; pkey[2 * tid + 1] = cur; }
    }
    __syncthreads();
    // segmented inclusive scan keyed by digit; the upper half of a stride first: its reads of the lower half see the stride's old values
#pragma unroll 1
    for (u32 step = 0; step < 18; ++step) {
        const u32 s = 1u << (step >> 1), i = tid + ((step & 1u) ? 0u : 256u);
        const u32 key = pkey[i];
        const bool need = i >= s && key != 0 && pkey[i - s] == key;
        PtProj left = ident;
        if (need) left = pt_load(pool + (i - s) * MSM_PARTIAL_BYTES);
        __syncthreads();
        if (need) pt_store(pool + i * MSM_PARTIAL_BYTES, pt_add(pt_load(pool + i * MSM_PARTIAL_BYTES), left, a.cv));
        __syncthreads();
    }
    for (u32 h = 0; h < 2; ++h) {   // a group's last entry holds its sum
        const u32 i = tid + 256 * h, key = pkey[i];
        if (key && (i == 511 || pkey[i + 1] != key)) pt_store(bucket + key * MSM_PARTIAL_BYTES, pt_load(pool + i * MSM_PARTIAL_BYTES));
    }
    __syncthreads();
    // lane b: b * B_b, then the workgroup's sum
    acc = pt_mul_digit(pt_load(bucket + tid * MSM_PARTIAL_BYTES), tid, a.cv);
    pt_store(bucket + tid * MSM_PARTIAL_BYTES, acc);
    __syncthreads();
#pragma unroll 1
    for (u32 s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            acc = pt_add(acc, pt_load(bucket + (tid + s) * MSM_PARTIAL_BYTES), a.cv);
            pt_store(bucket + tid * MSM_PARTIAL_BYTES, acc);
        }
        __syncthreads();
    }
    if (tid == 0) pt_store(msm_partial(a, elem, col, window, slice), acc);
}

// grid (num_cols, circuits of one launch)
__global__ __launch_bounds__(256) void msm_fold_kernel(MsmArgs a) {
    __shared__ __align__(16) u8 sh[256 * MSM_PARTIAL_BYTES];
    const u32 tid = threadIdx.x, window = tid % MSM_WINDOWS, g = tid / MSM_WINDOWS, col = blockIdx.x;
    static_assert(MSM_WINDOWS * MSM_FOLD_GROUPS == 256, "a lane per (window, group)");
    const u64 elem = (u64)a.elem0 + blockIdx.y;
    if (a.status && a.status[elem]) return;               // skipped: no workspace result is consumed
    PtProj acc = pt_identity(a.cv);
#pragma unroll 1
    for (u32 s = g; s < a.num_slices; s += MSM_FOLD_GROUPS) acc = pt_add(acc, pt_load(msm_partial(a, elem, col, window, s)), a.cv);
    pt_store(sh + tid * MSM_PARTIAL_BYTES, acc);
    __syncthreads();
#pragma unroll 1
    for (u32 s = MSM_FOLD_GROUPS / 2; s >= 1; s >>= 1) {
        if (g < s) {
            acc = pt_add(acc, pt_load(sh + (tid + s * MSM_WINDOWS) * MSM_PARTIAL_BYTES), a.cv);
            pt_store(sh + tid * MSM_PARTIAL_BYTES, acc);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    acc = pt_load(sh + (MSM_WINDOWS - 1) * MSM_PARTIAL_BYTES);
#pragma unroll 1
    for (u32 w = MSM_WINDOWS - 1; w > 0; --w) acc = pt_add(pt_shift_window(acc, a.cv), pt_load(sh + (w - 1) * MSM_PARTIAL_BYTES), a.cv);
    PtAff r = pt_to_affine(acc, a.cv);
    if (!a.mont) { r.x = fe_from_mont(r.x, a.cv.fq); r.y = fe_from_mont(r.y, a.cv.fq); }
    u8 *o = reinterpret_cast<u8 *>(a.out) + (elem * a.num_cols + col) * 64;
    fe_store(o, r.x); fe_store(o + 32, r.y);
}

#endif  // H2R_TU_MSM

}  // namespace h2r
