// libh2r.so, translation unit "quotient": the vanishing argument's quotient on the extended domain (h2r_quotient.hpp) and its launcher.
#define H2R_TU_QUOTIENT
#include "h2r_internal.hpp"
#include "h2r_quotient.hpp"

namespace h2r {

hipError_t launch_quotient(const QuotientArgs &a, u32 num_tiles, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(quotient_kernel, dim3(num_elems, num_tiles), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
