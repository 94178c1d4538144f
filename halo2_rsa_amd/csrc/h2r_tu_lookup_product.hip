// libh2r.so, translation unit "lookup product": the lookup argument's input columns A and grand-product columns Z
// (h2r_lookup_product.hpp) and their launchers.
#define H2R_TU_LOOKUP_PRODUCT
#include "h2r_internal.hpp"
#include "h2r_lookup_product.hpp"

namespace h2r {

hipError_t launch_lookup_input(const LookupInputArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const unsigned chunks = (a.usable_rows + 255) / 256;
    hipExtLaunchKernelGGL(lookup_input_kernel, dim3(chunks, 5, num_elems), dim3(256), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_lookup_product(u32 phase, const LookupProductArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    switch (phase) {
        case 0: hipExtLaunchKernelGGL(lookup_product_tiles_kernel, dim3(a.n_tiles, 5, num_elems), dim3(256), 0, st, ea, eb, 0, a); break;
        case 1: hipExtLaunchKernelGGL(lookup_product_carry_kernel, dim3(5, num_elems), dim3(64), 0, st, ea, eb, 0, a); break;
        default: hipExtLaunchKernelGGL(lookup_product_scan_kernel, dim3(a.n_tiles, 5, num_elems), dim3(256), 0, st, ea, eb, 0, a); break;
    }
    return hipGetLastError();
}

}  // namespace h2r
