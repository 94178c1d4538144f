// libh2r.so, translation unit "permutation product": the permutation argument's grand-product columns Z
// (h2r_permutation_product.hpp) and their launcher.
#define H2R_TU_PERM_PRODUCT
#include "h2r_internal.hpp"
#include "h2r_permutation_product.hpp"

namespace h2r {

hipError_t launch_perm_product(u32 phase, const PermProductArgs &a, u32 num_elems, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    switch (phase) {
        case 0: hipExtLaunchKernelGGL(perm_product_tiles_kernel, dim3(a.n_tiles, a.n_sets, num_elems), dim3(256), 0, st, ea, eb, 0, a); break;
        case 1: hipExtLaunchKernelGGL(perm_product_carry_kernel, dim3(num_elems), dim3(64), 0, st, ea, eb, 0, a); break;
        default: hipExtLaunchKernelGGL(perm_product_scan_kernel, dim3(a.n_tiles, a.n_sets, num_elems), dim3(256), 0, st, ea, eb, 0, a); break;
    }
    return hipGetLastError();
}

}  // namespace h2r
