// libh2r.so, translation unit "lookup": the lookup argument's multiplicities and permuted columns -- hist_kernel / perm_kernel over the
// records (h2r_kernels.hpp), the per-argument histograms, the A' / S' set-up and fill (h2r_lookup.hpp) -- and their launchers.
#define H2R_TU_LOOKUP
#include "h2r_internal.hpp"
#include "h2r_lookup.hpp"

namespace h2r {

hipError_t launch_hist(const HistArgs &ha, hipStream_t st) {
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)ha.num_elems), dim3(256), ha.hist_len * sizeof(u32), st, ha);
    return hipGetLastError();
}

hipError_t launch_perm(bool staged, u32 lds, const PermArgs &pa, hipStream_t st) {
    if (staged) {
        if (lds > 48 * 1024) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&perm_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipGetLastError();
        }
        hipLaunchKernelGGL(perm_kernel<true>, dim3((unsigned)pa.h.num_elems), dim3(256), lds, st, pa);
    } else
        hipLaunchKernelGGL(perm_kernel<false>, dim3((unsigned)pa.h.num_elems), dim3(256), lds, st, pa);
    return hipGetLastError();
}

hipError_t launch_lookup_hist_records(const LookupHistArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lookup_hist_records_kernel, dim3((unsigned)a.num_elems), dim3(256), LOOKUP_ARGS * a.n_rows * sizeof(u32), st, a);
    return hipGetLastError();
}

hipError_t launch_lookup_hist_values(const LookupValuesArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lookup_hist_values_kernel, dim3((unsigned)a.num_elems), dim3(256), LOOKUP_ARGS * a.n_rows * sizeof(u32), st, a);
    return hipGetLastError();
}

hipError_t launch_lookup_hist_fresh(const LookupFreshArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lookup_hist_fresh_kernel, dim3((unsigned)a.num_elems), dim3(64), LOOKUP_ARGS * a.n_rows * sizeof(u32), st, a);
    return hipGetLastError();
}

hipError_t launch_lookup_setup(const LookupSetupArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(lookup_setup_kernel, dim3((unsigned)(a.num_elems * LOOKUP_ARGS)), dim3(256), lookup_setup_lds_bytes(a.n_rows), st, a);
    return hipGetLastError();
}

hipError_t launch_lookup_fill(const LookupFillArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const unsigned chunks = (a.usable_rows + a.rows_per_block - 1) / a.rows_per_block;
    hipExtLaunchKernelGGL(lookup_fill_kernel, dim3(chunks, LOOKUP_ARGS, (unsigned)a.num_elems), dim3(256), (unsigned)lookup_slot_bytes(a.n_rows), st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
