// libh2r.so, translation unit "verify": the verifier's kernels up to the pairing -- the proof decoder, the scalars of the accumulators, the
// sum of terms over per-circuit bases (h2r_verify.hpp) -- and their launchers.
#define H2R_TU_VERIFY
#include "h2r_internal.hpp"
#include "h2r_verify.hpp"

namespace h2r {

hipError_t launch_proof_decode(const DecodeArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(proof_decode_kernel, dim3(num_blocks, a.num_items), dim3(VF_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_verify_scalars(const VerifyScalarsArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(verify_scalars_kernel, dim3(num_blocks), dim3(VF_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_msm_terms(const MsmTermsArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(msm_terms_kernel, dim3(num_elems), dim3(VF_TERM_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
