// libh2r.so, translation unit "step": every instantiation of step_kernel (h2r_kernels.hpp) -- the records of call k and the
// chains of call k+1 in one launch -- for the calls without keys; the launcher itself is h2r_step_launch.hpp.
#include "h2r_step_launch.hpp"

namespace h2r {

hipError_t launch_step_shape(const StepShape &s, u32 num_cus, const ChainArgs &ca, const TraceArgs &ta, const AuxArgs *aa, const AuxArgs *va,
                             const Sha256Args *sha, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    if (ca.key_idx) return launch_step_shape_keyed(s, num_cus, ca, ta, aa, va, sha, st, ea, eb);   // h2r_tu_step_keyed.hip
    return launch_step_shape_t<false>(s, num_cus, ca, ta, aa, va, sha, st, ea, eb);
}
u32 step_shared_bytes_shape(const StepShape &s) {
    if (s.L == 32) return (u32)sizeof(StepShared<64, 4, 64, 32>);
    if (s.L == 16) return (u32)std::max(sizeof(StepShared<32, 4, 64, 16>), sizeof(StepShared<32, 4, 64, 16, true>));
    if (s.L == 128) return (u32)sizeof(StepShared<128, 8, 32, 128>);
    if (s.L == 64) return (u32)sizeof(StepShared<128, 8, 64, 64>);
    return (u32)sizeof(StepShared<96, 6, 64, 48>);
}

}  // namespace h2r
