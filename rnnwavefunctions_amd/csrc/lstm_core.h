// lstm_core.h - one step of tf.nn.rnn_cell.LSTMCell (TF 1.x defaults) for 16 chains per wave, float64, on the f64 MFMA.
//
// Reference arithmetic: the default cell of 2DTFIM_1DRNN/RNNwavefunction.py:9, built as
// MultiRNNCell([LSTMCell(units[n])]) (:37) - no peepholes, no projection, no clipping, forget_bias = 1, activation tanh:
//     z = [x, h] K + b;   i, j, f, o = split(z, 4, axis=1)
//     c' = sigmoid(f + 1) c + sigmoid(i) tanh(j);   h' = sigmoid(o) tanh(c')
// x is a one-hot (or the zero vector at the first site), so its rows of K are row selections that fold, together with the
// bias, into the accumulator initialisation (table BINIT, three variants as in GruLayout).  The forget bias is folded there
// too: the packed f rows of BINIT hold b_f + x K_f + 1 (pack: pack_lstm_image), so the step adds nothing after the products.
// That rounds (b + xK + 1) + hK instead of the reference's (xK + hK + b) + 1 - a difference of one rounding of a
// pre-activation, far below the 1e-11 N tolerance of log P (docs/lstm.md).
//
// Layout (LstmLayout<NFULL>, hidden size padded to HP = 16 NFULL + 4):
//   tile g NFULL + m (g = 0 i, 1 j, 2 f, 3 o), m < NFULL : units 16 m .. 16 m + 15 of gate g
//   tile 4 NFULL ("mixed")                              : register r = gate r of unit 16 NFULL + q (all four registers used)
// with the f64 C/D map row = q + 4 r (layout.h: row_to_qr<double>).  K runs over h only: KT = 4 NFULL + 1 k-steps.
// c is held in exactly h's register layout (c[kt] of lane (c, q) = cell state of unit 4 kt + q): neither state crosses lanes.
#pragma once
#include "gru_core.h"

namespace rnnwf {

template <int NFULL_>
struct LstmLayout {
    using T = double;
    static constexpr int NFULL = NFULL_;
    static constexpr int HP = 16 * NFULL + 4;       // padded hidden size
    static constexpr int KT = 4 * NFULL + 1;        // k-steps of 4
    static constexpr int NT = 4 * NFULL + 1;        // 16-row output tiles: four gates x NFULL groups + the mixed tile
    static constexpr int VW = 16 / (int)sizeof(T);  // A values per 16-byte LDS vector
    static constexpr int NG = (KT - 1) / VW;        // full vectors per (tile, lane)
    static constexpr size_t OFF_AVEC = 0;                                            // [NT][NG][64] x 16 B
    static constexpr size_t OFF_AREM = OFF_AVEC + (size_t)NT * NG * 64 * 16;         // [NT][64] T   (kt = KT-1)
    static constexpr size_t OFF_BINIT = OFF_AREM + (size_t)NT * 64 * sizeof(T);      // [3][NT][4 q][4 r] T
    static constexpr size_t SZ_BINIT_VARIANT = ((size_t)NT * 16 + 4) * sizeof(T);    // +4 T pad: de-alias banks
    static constexpr int WD_Q = ((KT + 3) / 4) * 4;                                  // head weights per lane quarter
    static constexpr size_t OFF_WD = OFF_BINIT + 3 * SZ_BINIT_VARIANT;               // [4 q][KT] T, WD_Q per q
    static constexpr size_t OFF_BD = OFF_WD + (size_t)4 * WD_Q * sizeof(T);          // [1] T (padded to 32 B)
    static constexpr size_t BYTES = ((OFF_BD + 32 + 15) / 16) * 16;
    static_assert(BYTES <= 160 * 1024, "the LSTM weight image must fit the 160 KiB of LDS (<= 68 units)");
};

template <int NFULL>
struct LstmCore {
    using L = LstmLayout<NFULL>;
    using T = double;
    using F = Frag<T>;
    using A = Act<T>;
    using V4 = typename F::V4;
    using VA = typename F::VA;
    static constexpr int KT = L::KT, NT = L::NT, NG = L::NG, VW = L::VW;

    static __device__ __forceinline__ const char* stage(char* lds, const void* wimg) {
        const uint4* src = reinterpret_cast<const uint4*>(wimg);
        uint4* dst = reinterpret_cast<uint4*>(lds);
        for (int i = threadIdx.x; i < (int)(L::BYTES / 16); i += blockDim.x) dst[i] = src[i];
        __syncthreads();
        return lds;
    }

    // c' and h' of one unit from its four accumulators (the f row carries the forget bias already)
    static __device__ __forceinline__ void gate(T ai, T aj, T af, T ao, T& c, T& h) {
#pragma clang fp contract(off)
        const T ig = A::sigmoid_scaled(ai);
        const T jt = A::tanh_scaled(aj);
        const T fg = A::sigmoid_scaled(af);
        const T og = A::sigmoid_scaled(ao);
        c = fma_(fg, c, ig * jt);
        h = og * A::tanh_scaled(c);
    }

    // h[kt], c[kt] of lane (c, q): unit 4 kt + q of chain c.  sig: input spin of this step (-1: zero vector).
    // One unit group at a time: the four gate tiles of group m (group 0 with the mixed tile as a fifth) go through the MFMA
    // chain, then their gates update c in place and write h' into hn; h is replaced once every product has read it.  Live
    // accumulators: 5 tiles instead of NT (17 at 68 units, whose 136 registers beside h, c and the fragments spilled).
    static __device__ __forceinline__ void step(const char* lds, int sig, T (&h)[KT], T (&c)[KT], int lane) {
        const int q = lane >> 4;
        // the image never changes: without the barrier the compiler hoists the fragment loads out of the site loop
        asm volatile("" ::: "memory");
        const char* binit = lds + L::OFF_BINIT + (size_t)(sig + 1) * L::SZ_BINIT_VARIANT + (size_t)q * 4 * sizeof(T);
        const VA* av = reinterpret_cast<const VA*>(lds + L::OFF_AVEC) + lane;
        const T* ar = reinterpret_cast<const T*>(lds + L::OFF_AREM) + lane;
        T hn[KT];
#pragma unroll
        for (int m = 0; m < NFULL; ++m) {
            const int nt = m == 0 ? 5 : 4;                                     // group 0 carries the mixed tile
            auto tile = [&](int k) { return k < 4 ? k * NFULL + m : NT - 1; };  // k = gate i, j, f, o; 4: mixed
            asm volatile("" ::: "memory");
            V4 acc[5];
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k < nt) acc[k] = *reinterpret_cast<const V4*>(binit + (size_t)tile(k) * 16 * sizeof(T));
            // MFMA chain and gate arithmetic in separate scheduling regions (f64 MFMA and VALU do not overlap on gfx950)
            __builtin_amdgcn_sched_barrier(0);
            // fragments one k-group ahead, one scheduling region per k-group: left to itself the scheduler issues every load of
            // the group's chain up front (160 registers of fragments at 68 units) and the kernel spills
            VA a[2][5];
            auto fetch = [&](int g, VA (&dst)[5]) {
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (k < nt) dst[k] = av[(tile(k) * NG + g) * 64];
            };
            fetch(0, a[0]);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                asm volatile("" ::: "memory");
                if (g + 1 < NG) fetch(g + 1, a[(g + 1) & 1]);
#pragma unroll
                for (int j = 0; j < VW; ++j)
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        if (k < nt) acc[k] = F::mfma(a[g & 1][k][j], h[g * VW + j], acc[k]);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k < nt) acc[k] = F::mfma(ar[tile(k) * 64], h[KT - 1], acc[k]);
            __builtin_amdgcn_sched_barrier(0);
            // two units per scheduling region: sixteen exponentials interleaved at once hold ~100 temporaries
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gate(acc[0][r], acc[1][r], acc[2][r], acc[3][r], c[4 * m + r], hn[4 * m + r]);
                if (r & 1) __builtin_amdgcn_sched_barrier(0);
            }
            if (m == 0) gate(acc[4][0], acc[4][1], acc[4][2], acc[4][3], c[KT - 1], hn[KT - 1]);
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = hn[kt];
    }

    // the logit difference d = z1 - z0 of the Dense(2) head on h', reduced over the four lane quarters (GruCore::head's arithmetic)
    static __device__ __forceinline__ T head(const char* lds, const T (&h)[KT], int lane) {
#pragma clang fp contract(off)
        const int q = lane >> 4;
        asm volatile("" ::: "memory");
        const T* wd = reinterpret_cast<const T*>(lds + L::OFF_WD) + q * L::WD_Q;
        T z = T(0);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) z = fma_(h[kt], wd[kt], z);
        z += __shfl_xor(z, 16);
        z += __shfl_xor(z, 32);
        return z + *reinterpret_cast<const T*>(lds + L::OFF_BD);
    }
};

}  // namespace rnnwf
