// shapes.h - every shape with kernels: one table per family (handle.h: KernelRow, SplitRow, KernelTable), written once.  Every
// width-class dispatch of the host code walks one of these - the forward passes, the observable passes, the gradient, stochastic
// reconfiguration and the tables device-resident training replays (train.hip) - so a row added or changed here is added or changed
// for all of them.  A row instantiates its kernels in every translation unit that walks its table.
#pragma once
#include <type_traits>

#include "handle.h"

namespace rnnwf {

template <typename T, int NL, int NFULL, int WAVES> using KR = KernelRow<T, NL, NFULL, WAVES>;

// ---- positive GRU (GRU1D, GRU1D_PARITY, GRU1D_F64): (element type, layers, NFULL) -> waves per workgroup of the base and flip kernels
// (prnn.hip); its rows are also the gradient's shapes (grad.hip, grad_wide.hip) and, the one-layer ones, those of the observable passes
// (observable.h) and of stochastic reconfiguration (sr.hip, up to NFULL = 4)
using GruKernels = KernelTable<
    KR<double, 1, 1, 4>, KR<double, 1, 2, 4>, KR<double, 1, 3, 4>, KR<double, 1, 4, 8>, KR<double, 1, 6, 4>,
    KR<double, 2, 1, 4>, KR<double, 2, 2, 8>, KR<double, 2, 3, 4>, KR<double, 2, 4, 4>,
    KR<double, 3, 1, 4>, KR<double, 3, 2, 4>, KR<double, 3, 3, 4>, KR<double, 3, 4, 4>,
    KR<double, 4, 1, 4>, KR<double, 4, 2, 4>, KR<double, 4, 3, 4>, KR<double, 4, 4, 4>,
    KR<float, 1, 1, 4>, KR<float, 1, 2, 4>, KR<float, 1, 3, 4>, KR<float, 1, 4, 4>, KR<float, 1, 6, 8>, KR<float, 1, 8, 4>, KR<float, 1, 12, 4>, KR<float, 1, 16, 4>,
    KR<float, 2, 1, 4>, KR<float, 2, 2, 4>, KR<float, 2, 3, 8>, KR<float, 2, 4, 4>, KR<float, 2, 6, 4>,
    KR<float, 3, 1, 4>, KR<float, 3, 2, 8>, KR<float, 3, 3, 8>, KR<float, 3, 4, 4>, KR<float, 3, 6, 4>,
    KR<float, 4, 1, 4>, KR<float, 4, 2, 4>, KR<float, 4, 3, 4>, KR<float, 4, 4, 4>, KR<float, 4, 6, 4>>;
// The one-layer observable passes (observable.h: Gru1Launch) run at the row's waves per workgroup with one exception - f64 at 53..68
// units (NFULL = 4): 4, not 8.  At 8 the swap kernel spills 20 bytes per lane to scratch (profiles/renyi_kernel_resources.txt); at 4
// no kernel of the four passes uses scratch (profiles/{renyi,corr,renyi_regions,pauli}_kernel_resources.txt).
template <typename T, int NFULL, int WAVES>
constexpr int kGru1Waves = std::is_same<T, double>::value && NFULL == 4 ? 4 : WAVES;

// ---- complex RNN (CRNN_U1, f32): (layers, NFULL) -> waves per workgroup of the base and swap kernels (crnn.hip); also the gradient's
// shapes and, the one-layer rows, those of the Pauli and region-Renyi passes (crnn_observable.h)
using CrnnKernels = KernelTable<
    KR<float, 1, 1, 4>, KR<float, 1, 2, 4>, KR<float, 1, 3, 4>, KR<float, 1, 4, 4>, KR<float, 1, 6, 8>, KR<float, 1, 8, 4>, KR<float, 1, 12, 4>, KR<float, 1, 16, 4>,
    KR<float, 2, 1, 4>, KR<float, 2, 2, 4>, KR<float, 2, 3, 8>, KR<float, 2, 4, 4>, KR<float, 2, 6, 4>,
    KR<float, 3, 1, 4>, KR<float, 3, 2, 8>, KR<float, 3, 3, 8>, KR<float, 3, 4, 4>, KR<float, 3, 6, 4>,
    KR<float, 4, 1, 4>, KR<float, 4, 2, 4>, KR<float, 4, 3, 4>, KR<float, 4, 4, 4>, KR<float, 4, 6, 4>>;

// ---- 2D RNN (MDRNN2D, f64, one layer, 1..84 units): forward passes and gradient (mdrnn.hip), Pauli and region-Renyi passes
// (mdrnn_observable.h)
using MdKernels = KernelTable<KR<double, 1, 1, 4>, KR<double, 1, 2, 4>, KR<double, 1, 3, 4>, KR<double, 1, 4, 4>, KR<double, 1, 5, 4>>;

// ---- LSTM cell (LSTM1D_F64, one layer, NFULL 1..4: <= 20, 36, 52, 68 units): waves per workgroup of the flip pass - 8 where one
// workgroup fills a CU's LDS (two per SIMD); the base pass's differ at 68 units (lstm.hip: LLaunch::BWAVES)
using LstmKernels = KernelTable<KR<double, 1, 1, 4>, KR<double, 1, 2, 4>, KR<double, 1, 3, 8>, KR<double, 1, 4, 8>>;

// ---- bf16x3 engine, one layer: the flip pass of the positive RNN and the swap pass of the complex RNN, which share the layouts of each
// width.  MODE 0..2: split.hip (MODE 2, 37..50 units: the K-packed layout of the ping-pong kernels); MODE 3: the riders form, 53..100
// units (split_stream.hip).  NFULL <- <NF32, RJ, WAVES, MODE[, HMIN, HMAX]>
using SplitKernels = KernelTable<SplitRow<1, 0, 10, 4, 1>, SplitRow<2, 1, 2, 4, 1>, SplitRow<3, 1, 9, 4, 2, 0, 50>, SplitRow<3, 1, 10, 4, 0, 51>,
                                 SplitRow<4, 2, 2, 4, 3>, SplitRow<6, 3, 2, 4, 3>>;

// ---- cooperative base pass on the bf16 matrix core (split.hip: BfBase; f32, one layer, up to 52 units).  Its workgroup is the
// layout's (layout.h: BaseBfLayout), not a number of waves per item: WAVES = 0
using BaseBfKernels = KernelTable<KR<float, 1, 1, 0>, KR<float, 1, 2, 0>, KR<float, 1, 3, 0>>;

}  // namespace rnnwf
