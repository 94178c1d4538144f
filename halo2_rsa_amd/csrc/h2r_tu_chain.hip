// libh2r.so, translation unit "chain": the dependent mul_mod chain per element -- recip_kernel, key_table_kernel, chain_kernel,
// chain_dual_kernel (h2r_kernels.hpp) -- for the calls without keys; the launcher itself is h2r_chain_launch.hpp.
#include "h2r_chain_launch.hpp"

namespace h2r {
namespace {

template <int K, int NW>
hipError_t launch_key_table_t(const u32 *n_keys, u32 kreal, u64 num_keys, u32 *raw, u32 raw_stride, u32 *pre, u8 *key_status, hipStream_t st) {
    const u64 grid = num_keys + 1 < (1ull << 20) ? num_keys + 1 : (1ull << 20);   // (the sentinel entry is a key of its own)
    hipLaunchKernelGGL((key_table_kernel<K, NW>), dim3((unsigned)grid), dim3(64 * NW), 0, st, n_keys, kreal, num_keys, raw, raw_stride, pre, key_status);
    return hipGetLastError();
}
}  // namespace

// The digits K of the chain build that serves integers of `kreal` digits: what a key table's entries are computed for.
u32 chain_digits(u32 kreal) { return kreal <= 8 ? 8 : kreal <= 16 ? 16 : kreal <= 32 ? 32 : kreal <= 64 ? 64 : kreal <= 96 ? 96 : 128; }

hipError_t launch_key_table_shape(const u32 *n_keys, u32 kreal, u64 num_keys, u32 *raw, u32 raw_stride, u32 *pre, u8 *key_status, hipStream_t st) {
    switch (chain_digits(kreal)) {   // the workgroup of recip_kernel for the same K
        case 8: return launch_key_table_t<8, 1>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
        case 16: return launch_key_table_t<16, 1>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
        case 32: return launch_key_table_t<32, 4>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
        case 64: return launch_key_table_t<64, 4>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
        case 96: return launch_key_table_t<96, 6>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
        default: return launch_key_table_t<128, 8>(n_keys, kreal, num_keys, raw, raw_stride, pre, key_status, st);
    }
}

hipError_t launch_chain_shape(u32 num_cus, const ChainArgs &ca, bool co_running, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    if (ca.key_idx) return launch_chain_shape_keyed(num_cus, ca, co_running, st, ea, eb);   // h2r_tu_chain_keyed.hip
    return launch_chain_shape_t<false>(num_cus, ca, co_running, st, ea, eb);
}

}  // namespace h2r
