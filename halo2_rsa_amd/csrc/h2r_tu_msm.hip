// libh2r.so, translation unit "msm": the commitments' multi-scalar multiplications over the curve of the ctx's field (h2r_msm.hpp, h2r_curve.hpp) and their launchers.
#define H2R_TU_MSM
#include "h2r_internal.hpp"
#include "h2r_msm.hpp"

namespace h2r {

hipError_t launch_msm(u32 phase, const MsmArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    if (phase == 0) hipExtLaunchKernelGGL(msm_bucket_kernel, dim3(a.num_slices * MSM_WINDOWS, a.num_cols, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    else hipExtLaunchKernelGGL(msm_fold_kernel, dim3(a.num_cols, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
