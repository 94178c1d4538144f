// libh2r.so, translation unit "random": the counter-based generator of the prover's blinding values (h2r_random.hpp) and its launcher.
#define H2R_TU_RANDOM
#include "h2r_internal.hpp"
#include "h2r_random.hpp"

namespace h2r {

hipError_t launch_random(const RandomArgs &a, u32 num_tiles, u32 num_cols, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(random_kernel, dim3(num_tiles, num_cols, num_elems), dim3(RND_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
