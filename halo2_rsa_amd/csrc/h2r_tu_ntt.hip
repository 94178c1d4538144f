// libh2r.so, translation unit "ntt": the evaluation domain's transforms (h2r_ntt.hpp) and their launchers.
#define H2R_TU_NTT
#include "h2r_internal.hpp"
#include "h2r_ntt.hpp"

namespace h2r {

hipError_t launch_ntt_setup(const NttSetupArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(ntt_setup_kernel, dim3(NTT_SPLIT / 1024, NTT_TABLES), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_ntt_pass(const NttArgs &a, u32 num_cols, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(ntt_pass_kernel, dim3(ntt_pass_tiles(a.log_n, a.s[a.pass]), num_cols, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
