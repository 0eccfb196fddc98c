// grad_wide.hip - the backward kernels of the wide shapes (one wave per SIMD, 512 registers): positive and complex RNN from 101 units,
// float64 GRU 69..100 units.
// In grad.hip's translation unit (compiled with -amdgpu-mfma-vgpr-form, build.py) hipcc 7.2 crashes on several of these in
// 'AMDGPU Rewrite AGPR-Copy-MFMA' - which ones changes with unrelated edits of the kernel; rounds 2-3 ran three of them with 8 waves per
// workgroup instead - 256 registers per wave, 1.3 - 2.7 KB of spills per lane (the float64 GRU's backward kernel at 100 units: 12 ms
// where the 68-unit one takes 1.6).  This unit is compiled WITHOUT that option (accumulators in AGPRs), which the pass survives.
#include "grad_kernels.h"
#include "models.h"
#include "shapes.h"

namespace rnnwf {

namespace {
// the kernel of a one-layer row with NOUT head rows, where the row is a wide one (models.h: kGradWide)
template <int NOUT>
struct Wide {
    template <typename T, int NFULL, int>
    struct Row {
        static GradKernel kernel() {
            if constexpr (kGradWide<T, NFULL>) return gru_bwd_kernel<T, NFULL, kGradWaves, NOUT>;
            else return nullptr;
        }
    };
};
}  // namespace

GradKernel grad_wide_kernel(const rnnwf_handle* h) {
    GradKernel kern = nullptr;
    auto pick = [&](auto row) { kern = decltype(row)::kernel(); };
    if (h->model == RNNWF_MODEL_CRNN_U1) with_layer_kernels<Wide<3>::Row>(CrnnKernels(), h, pick);
    else with_layer_kernels<Wide<1>::Row>(GruKernels(), h, pick);
    return kern;
}

}  // namespace rnnwf
