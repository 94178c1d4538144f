// libh2r.so, translation unit "transcript": the Fiat-Shamir transcript's round kernel (h2r_transcript.hpp) and its launcher.
#define H2R_TU_TRANSCRIPT
#include "h2r_internal.hpp"
#include "h2r_transcript.hpp"

namespace h2r {

hipError_t launch_transcript(const TranscriptArgs &a, u32 num_blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    hipExtLaunchKernelGGL(transcript_kernel, dim3(num_blocks), dim3(TR_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

}  // namespace h2r
