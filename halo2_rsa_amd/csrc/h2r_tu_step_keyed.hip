// libh2r.so, translation unit "step, keyed": the step launches of keyed calls (step_kernel<.., KEYED>: the chain role takes the
// modulus and its Barrett constants from the key table, the witness roles its raw limbs).
#include "h2r_step_launch.hpp"

namespace h2r {

hipError_t launch_step_shape_keyed(const StepShape &s, u32 num_cus, const ChainArgs &ca, const TraceArgs &ta, const AuxArgs *aa, const AuxArgs *va,
                                   const Sha256Args *sha, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    return launch_step_shape_t<true>(s, num_cus, ca, ta, aa, va, sha, st, ea, eb);
}

}  // namespace h2r
