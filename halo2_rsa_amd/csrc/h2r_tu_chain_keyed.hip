// libh2r.so, translation unit "chain, keyed": the chain kernels of keyed calls (chain_element<.., KEYED>: the modulus and its Barrett
// constants come from the key table) -- every build launch_chain_shape picks among, but the two-chains-per-element one.
#include "h2r_chain_launch.hpp"

namespace h2r {

hipError_t launch_chain_shape_keyed(u32 num_cus, const ChainArgs &ca, bool co_running, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    return launch_chain_shape_t<true>(num_cus, ca, co_running, st, ea, eb);
}

}  // namespace h2r
