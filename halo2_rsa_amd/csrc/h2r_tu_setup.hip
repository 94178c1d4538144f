// libh2r.so, translation unit "setup": KZG parameters from a known tau -- the fixed-base table of a G1 point, the fixed-base multiplication of a
// column of scalars, the scalar families tau^i and l_i(tau) (h2r_setup.hpp, h2r_curve.hpp) -- and its launchers.
#define H2R_TU_SETUP
#include "h2r_internal.hpp"
#include "h2r_setup.hpp"

namespace h2r {

hipError_t launch_fixed_base_table(const FixedBaseTableArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(fixed_base_table_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}
hipError_t launch_fixed_base_mul(const FixedBaseMulArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(fixed_base_mul_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}
hipError_t launch_setup_scalars(const SetupScalarsArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(setup_scalars_kernel, dim3(num_blocks), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
