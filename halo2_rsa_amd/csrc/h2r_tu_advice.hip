// libh2r.so, translation unit "advice": the advice image from records and programs -- advice_kernel / emit_kernel (h2r_kernels.hpp),
// var_rows_kernel (h2r_varrows.hpp), the row programs (h2r_rowprog.hpp), the layout permutation (h2r_copymap.hpp), the MockProver's row /
// copy checks and the image's lookup histogram (h2r_check.hpp) -- and their launchers.
#define H2R_TU_ADVICE
#include <type_traits>

#include "h2r_internal.hpp"
#include "h2r_varrows.hpp"
#include "h2r_rowprog.hpp"
#include "h2r_copymap.hpp"
#include "h2r_check.hpp"

namespace h2r {

hipError_t launch_advice_shape(u32 w, const AdviceArgs &aa, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    if (w == 64) hipExtLaunchKernelGGL((advice_kernel<64>), dim3((unsigned)aa.n_items), dim3(256), 0, st, ea, eb, 0, aa);
    else hipExtLaunchKernelGGL((advice_kernel<32>), dim3((unsigned)aa.n_items), dim3(256), 0, st, ea, eb, 0, aa);
    return hipGetLastError();
}

hipError_t launch_emit_shape(u32 w, const EmitArgs &a, u32 blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    const unsigned lds = EMIT_SEG_CAP + 64;
    if (w == 64) hipExtLaunchKernelGGL((emit_kernel<64>), dim3(blocks), dim3(256), lds, st, ea, eb, 0, a);
    else hipExtLaunchKernelGGL((emit_kernel<32>), dim3(blocks), dim3(256), lds, st, ea, eb, 0, a);
    return hipGetLastError();
}

hipError_t launch_var_rows_shape(u32 w, const VarRowsArgs &va, u32 blocks, hipStream_t st) {
    if (w == 64) hipLaunchKernelGGL((var_rows_kernel<64>), dim3(blocks), dim3(256), 0, st, va);
    else hipLaunchKernelGGL((var_rows_kernel<32>), dim3(blocks), dim3(256), 0, st, va);
    return hipGetLastError();
}

hipError_t launch_rowprog_shape(u32 w, u32 sr, const RowProgArgs &ra, u32 blocks, hipStream_t st, hipEvent_t ea, hipEvent_t eb) {
    auto go = [&](auto lw_c, auto sr_c) {
        constexpr int LW = decltype(lw_c)::value; constexpr u32 SR = decltype(sr_c)::value;
        hipExtLaunchKernelGGL((rowprog_kernel<LW, SR>), dim3(blocks), dim3(SR), 0, st, ea, eb, 0, ra);
    };
    using I64 = std::integral_constant<int, 64>; using I32 = std::integral_constant<int, 32>;
    const bool w64 = w == 64;
    if (sr == 64) { if (w64) go(I64{}, std::integral_constant<u32, 64>{}); else go(I32{}, std::integral_constant<u32, 64>{}); }
    else if (sr == 128) { if (w64) go(I64{}, std::integral_constant<u32, 128>{}); else go(I32{}, std::integral_constant<u32, 128>{}); }
    else { if (w64) go(I64{}, std::integral_constant<u32, 256>{}); else go(I32{}, std::integral_constant<u32, 256>{}); }
    return hipGetLastError();
}

hipError_t launch_rowprog_inv_shape(u32 w, u32 nt, const RowProgArgs &ra, u32 blocks, hipStream_t st) {
    const bool w64 = w == 64;
    if (nt == 64) {
        if (w64) hipLaunchKernelGGL((rowprog_inv_kernel<64, 64>), dim3(blocks), dim3(64), 0, st, ra);
        else hipLaunchKernelGGL((rowprog_inv_kernel<32, 64>), dim3(blocks), dim3(64), 0, st, ra);
    } else {
        if (w64) hipLaunchKernelGGL((rowprog_inv_kernel<64>), dim3(blocks), dim3(256), 0, st, ra);
        else hipLaunchKernelGGL((rowprog_inv_kernel<32>), dim3(blocks), dim3(256), 0, st, ra);
    }
    return hipGetLastError();
}

hipError_t launch_advice_layout(const LayoutArgs &la, u32 blocks, hipStream_t st) {
    hipLaunchKernelGGL(advice_layout_kernel, dim3(blocks), dim3(256), 0, st, la);
    return hipGetLastError();
}

hipError_t launch_advice_check_rows(const AdviceCheckArgs &ca, u32 blocks, hipStream_t st) {
    hipLaunchKernelGGL(advice_check_rows_kernel, dim3(blocks), dim3(256), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_advice_check_copies(const AdviceCheckArgs &ca, u32 blocks, hipStream_t st) {
    hipLaunchKernelGGL(advice_check_copies_kernel, dim3(blocks), dim3(256), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_advice_hist(const AdviceHistArgs &ha, u32 blocks, hipStream_t st) {
    hipLaunchKernelGGL(advice_hist_kernel, dim3(blocks), dim3(256), 5u * ha.n_rows * sizeof(u32), st, ha);
    return hipGetLastError();
}

}  // namespace h2r
