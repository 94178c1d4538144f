// libh2r.so, translation unit "open": the evaluations at x, the GWC witness polynomials and the fold of h's pieces (h2r_open.hpp) and their launchers.
#define H2R_TU_OPEN
#include "h2r_internal.hpp"
#include "h2r_open.hpp"

namespace h2r {

hipError_t launch_open(u32 phase, const OpenArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const u32 ny = a.witness ? a.num_points : 1u;
    if (phase == 0) hipExtLaunchKernelGGL(open_tiles_kernel, dim3(a.n_tiles, ny, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    else if (phase == 1) hipExtLaunchKernelGGL(open_carry_kernel, dim3(a.witness ? a.num_points : a.n_queries, num_elems), dim3(64), 0, st, ea, eb, 0, a);
    else hipExtLaunchKernelGGL(open_scan_kernel, dim3(a.n_tiles, ny, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_fold(const FoldArgs &a, u32 num_tiles, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(fold_kernel, dim3(num_elems, num_tiles), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
