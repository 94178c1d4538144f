// libh2r.so, translation unit "curve_ntt": the transform over the points of the curve of the ctx's field that forms the Lagrange-basis commitment key (h2r_curve_ntt.hpp, h2r_curve.hpp) and its launchers.
#define H2R_TU_CURVE_NTT
#include "h2r_internal.hpp"
#include "h2r_curve_ntt.hpp"

namespace h2r {

hipError_t launch_curve_ntt(u32 phase, const CurveNttArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    if (phase == 0) hipExtLaunchKernelGGL(curve_ntt_twiddle_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    else if (phase == 1) hipExtLaunchKernelGGL(curve_ntt_load_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    else if (phase == 2) hipExtLaunchKernelGGL(curve_ntt_stage_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    else hipExtLaunchKernelGGL(curve_ntt_store_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
