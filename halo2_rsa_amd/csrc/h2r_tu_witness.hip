// libh2r.so, translation unit "witness": the witness kernels outside the mul_mod records -- aux / fresh / check / link (h2r_kernels.hpp),
// sha256_kernel (h2r_sha256.hpp), decompose / key_expand, refresh / is_equal_muled / pad_limbs (h2r_muled.hpp) -- the arena's fill and
// restore kernels and the queue probe, and their launchers.
#define H2R_TU_WITNESS
#include "h2r_internal.hpp"
#include "h2r_muled.hpp"
#include "h2r_sha256.hpp"

using namespace h2r;

extern "C" {   // plain names in the code object
// a streaming fill in the product kernels' store pattern (16 bytes per lane, non-temporal, whole 4 KB runs per workgroup step,
// XCD-contiguous blocks): what h2r_image_arena_create times on a candidate region
__global__ __launch_bounds__(256) void arena_fill_kernel(u8 *p, u64 bytes) {
    const u64 per_block = 64ull << 10;
    const u64 b = xcd_contiguous_block(blockIdx.x, gridDim.x);
    u8 *q = p + b * per_block;
    const u64 n = bytes - b * per_block < per_block ? bytes - b * per_block : per_block;
    for (u64 o = (u64)threadIdx.x * 16; o + 16 <= n; o += 4096) st16(q + o, 0x0123456789abcdefull ^ o, b);
}
// h2r_arena_restore_constants: the constant planes of every record slot of a region, from the constant record (4 bytes per thread and step;
// every plane starts on a 16-byte boundary of the record and is a whole number of words)
__global__ __launch_bounds__(256) void arena_restore_kernel(u8 *base, u64 elem_stride, u64 off_records, u64 record_stride, u32 T, u64 n_records,
                                                            const u8 *cr, ArenaConstPlanes pl) {
    for (u64 k = blockIdx.x; k < n_records; k += gridDim.x) {
        const u64 elem = k / T, t = k - elem * T;
        u8 *rec = base + elem * elem_stride + off_records + t * record_stride;
        for (int p = 0; p < 7; ++p)
            for (u32 o = threadIdx.x * 4; o < pl.bytes[p]; o += 256 * 4)
                *reinterpret_cast<u32 *>(rec + pl.off[p] + o) = *reinterpret_cast<const u32 *>(cr + pl.off[p] + o);
    }
}
__global__ void queue_probe_kernel(unsigned long long ticks, unsigned long long *stamp) {   // one wave that holds its queue for `ticks` of the 100 MHz wall clock
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (stamp && threadIdx.x == 0) { stamp[0] = t0; stamp[1] = wall_clock64(); }   // when it ran, on the device's own clock
}
}  // extern "C"

namespace h2r {

namespace {
// a kernel whose dynamic LDS request may pass the default limit
void allow_lds(const void *kernel, u32 bytes) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    (void)hipGetLastError();
}
}  // namespace

hipError_t launch_aux_shape(u32 w, u32 lds, const AuxArgs &aa, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    auto go = [&](auto kernel) { hipExtLaunchKernelGGL(kernel, dim3((unsigned)aa.batch), dim3(64), lds, st, ea, eb, 0, aa); };
    if (aa.key_idx) { if (w == 64) go(&aux_kernel<64, true>); else go(&aux_kernel<32, true>); }
    else { if (w == 64) go(&aux_kernel<64>); else go(&aux_kernel<32>); }
    return hipGetLastError();
}

hipError_t launch_fresh_shape(u32 w, const FreshArgs &fa, hipStream_t st) {
    if (w == 64) hipLaunchKernelGGL((fresh_kernel<64>), dim3((unsigned)fa.batch), dim3(64), 0, st, fa);
    else hipLaunchKernelGGL((fresh_kernel<32>), dim3((unsigned)fa.batch), dim3(64), 0, st, fa);
    return hipGetLastError();
}

hipError_t launch_sha256(const Sha256Args &sa, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(sha256_kernel, dim3((unsigned)((sa.batch + 63) / 64)), dim3(64), 0, st, ea, eb, 0, sa);
    return hipGetLastError();
}

hipError_t launch_check_shape(u32 w, const CheckArgs &ca, hipStream_t st) {
    if (w == 64) hipLaunchKernelGGL((check_kernel<64>), dim3((unsigned)ca.n_items), dim3(256), 0, st, ca);
    else hipLaunchKernelGGL((check_kernel<32>), dim3((unsigned)ca.n_items), dim3(256), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_link_shape(u32 w, const LinkArgs &la, u64 batch, hipStream_t st) {
    if (w == 64) hipLaunchKernelGGL((link_kernel<64>), dim3((unsigned)batch), dim3(64), 0, st, la);
    else hipLaunchKernelGGL((link_kernel<32>), dim3((unsigned)batch), dim3(64), 0, st, la);
    return hipGetLastError();
}

hipError_t launch_decompose(const DecompArgs &da, u32 blocks, hipStream_t st) {
    hipLaunchKernelGGL(decompose_kernel, dim3(blocks), dim3(256), (da.comp_len + 256) * sizeof(u32), st, da);
    return hipGetLastError();
}

hipError_t launch_key_expand(const u32 *raw, u32 raw_stride, u32 num_keys, const u32 *key_idx, u64 batch, u32 kreal, u32 *n_out, hipStream_t st) {
    hipLaunchKernelGGL(key_expand_kernel, dim3((unsigned)((batch * kreal + 255) / 256)), dim3(256), 0, st, raw, raw_stride, num_keys, key_idx, batch, kreal, n_out);
    return hipGetLastError();
}

hipError_t launch_refresh(const RefreshArgs &ra, u32 stage, hipStream_t st) {
    if (stage > 40 * 1024) allow_lds(reinterpret_cast<const void *>(&refresh_kernel), stage);
    hipLaunchKernelGGL(refresh_kernel, dim3((unsigned)ra.batch), dim3(256), stage, st, ra);
    return hipGetLastError();
}

hipError_t launch_is_equal_muled(const EqMuledArgs &ea, u32 stage, hipStream_t st) {
    if (stage > 36 * 1024) allow_lds(reinterpret_cast<const void *>(&is_equal_muled_kernel), stage);
    hipLaunchKernelGGL(is_equal_muled_kernel, dim3((unsigned)ea.batch), dim3(256), stage, st, ea);
    return hipGetLastError();
}

hipError_t launch_pad_limbs(const PadArgs &pa, hipStream_t st) {
    const u64 blocks = (pa.batch * pa.L + 255) / 256;
    hipLaunchKernelGGL(pad_limbs_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, pa);
    return hipGetLastError();
}

hipError_t launch_arena_fill(u8 *p, u64 bytes, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(arena_fill_kernel, dim3((unsigned)((bytes + (64ull << 10) - 1) >> 16)), dim3(256), 0, st, ea, eb, 0, p, bytes);
    return hipGetLastError();
}

hipError_t launch_arena_restore(u32 blocks, u8 *base, u64 elem_stride, u64 off_records, u64 record_stride, u32 T, u64 n_records, const u8 *cr,
                                const ArenaConstPlanes &pl, hipStream_t st) {
    hipLaunchKernelGGL(arena_restore_kernel, dim3(blocks), dim3(256), 0, st, base, elem_stride, off_records, record_stride, T, n_records, cr, pl);
    return hipGetLastError();
}

hipError_t launch_queue_probe(unsigned long long ticks, unsigned long long *stamp, hipStream_t st) {
    hipLaunchKernelGGL(queue_probe_kernel, dim3(1), dim3(64), 0, st, ticks, stamp);
    return hipGetLastError();
}

}  // namespace h2r
