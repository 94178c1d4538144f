// libh2r.so, translation unit "keygen": the fixed columns of an image's row kinds, the sigma columns of its copy pairs (h2r_keygen.hpp)
// and their launchers.
#define H2R_TU_KEYGEN
#include "h2r_internal.hpp"
#include "h2r_keygen.hpp"

namespace h2r {

hipError_t launch_keygen_fixed(const KeygenFixedArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const u32 tiles = (u32)(((1ull << a.log_n) + KG_LANES - 1) / KG_LANES);
    hipExtLaunchKernelGGL(keygen_fixed_kernel, dim3(tiles, KG_NUM_FIXED), dim3(KG_LANES), 0, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_keygen_sigma(u32 phase, const KeygenSigmaArgs &a, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const u32 pair_blocks = (u32)((a.n_copies + KG_LANES - 1) / KG_LANES);
    const dim3 lanes(KG_LANES);
    switch (phase) {
        case KG_PHASE_INIT: {
            const u32 cells = a.n_cells > KG_CTRL_WORDS ? a.n_cells : KG_CTRL_WORDS;
            hipExtLaunchKernelGGL(keygen_sigma_init_kernel, dim3((cells + KG_LANES - 1) / KG_LANES), lanes, 0, st, ea, eb, 0, a);
            break;
        }
        case KG_PHASE_MARK: hipExtLaunchKernelGGL(keygen_sigma_mark_kernel, dim3(pair_blocks), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_HOOK: hipExtLaunchKernelGGL(keygen_sigma_hook_kernel, dim3(pair_blocks), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_COMPRESS: hipExtLaunchKernelGGL(keygen_sigma_compress_kernel, dim3(pair_blocks), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_COUNT: hipExtLaunchKernelGGL(keygen_sigma_count_kernel, dim3(a.n_tiles), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_TILE_SCAN: hipExtLaunchKernelGGL(keygen_sigma_tile_scan_kernel, dim3(1), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_COMPACT: hipExtLaunchKernelGGL(keygen_sigma_compact_kernel, dim3(a.n_tiles), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_SORT_HIST: hipExtLaunchKernelGGL(keygen_sigma_sort_hist_kernel, dim3(a.sort_tiles), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_SORT_SCAN: hipExtLaunchKernelGGL(keygen_sigma_sort_scan_kernel, dim3(1), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_SORT_SCATTER: hipExtLaunchKernelGGL(keygen_sigma_sort_scatter_kernel, dim3(a.sort_tiles), lanes, 0, st, ea, eb, 0, a); break;
        case KG_PHASE_IDENTITY:
            hipExtLaunchKernelGGL(keygen_sigma_identity_kernel, dim3((u32)(((1ull << a.log_n) + KG_TILE - 1) / KG_TILE), a.m), lanes, 0, st, ea, eb, 0, a);
            break;
        case KG_PHASE_SCATTER: hipExtLaunchKernelGGL(keygen_sigma_scatter_kernel, dim3((a.n_touched + KG_LANES - 1) / KG_LANES), lanes, 0, st, ea, eb, 0, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace h2r
