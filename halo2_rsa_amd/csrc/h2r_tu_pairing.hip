// libh2r.so, translation unit "pairing": the verifier's verdict -- the Miller values and final exponentiations of a batch of pairing
// products against prepared G2 tables (h2r_pairing.hpp) -- and its launcher.
#define H2R_TU_PAIRING
#include "h2r_internal.hpp"
#include "h2r_pairing.hpp"

namespace h2r {

hipError_t launch_pairing(const PairingArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(pairing_kernel, dim3(num_blocks), dim3(PR_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
