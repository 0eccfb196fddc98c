// lstm_corr_kernels.h - the three recurrent kernels of the LSTM wave function's all-pair correlation pass (rnnwf_correlations_lstm,
// lstm_corr.hip; docs/correlations_lstm.md), on LstmCore<NFULL> (lstm_core.h).  They are the LSTM counterparts of the base pass +
// prnn_site_both_kernel, of prnn_trunk_kernel and of prnn_branch_kernel (corr_kernels.h, whose header has the method) and write
// CorrArgs' arrays in exactly that file's layouts: from the suffix sums on run corr_kernels.h's own kernels.
//
//   lstm_corr_base_kernel : the teacher-forced base pass of this entry, 16 chains per wave: checkpoints (h, c) after every site but
//                           the last, as lstm_site_terms_kernel writes them, and per site bsel[n] = t_n(s_n),
//                           both[n] = t_n(1-s_n) - t_n(s_n).  The LSTM's base kernels hold both log-probabilities: no replay kernel.
//   lstm_trunk_kernel     : tile (i, 16-chain block), i = 0..N-2, persistent, longest first: restores (h, c) of hck[i], feeds 1-s_i,
//                           teacher-forces sites i+1..N-1 on the chain's own spins; at every site n tsel / toth[(i,n)] and, for
//                           n <= N-2, the state (h, c) to tck[(i,n)].  N(N-1)/2 cell evaluations per chain.
//   lstm_branch_kernel    : tile (i, j, block), j <= N-2, j ascending (longest first): restores (h, c) of tck[(i,j)], feeds 1-s_j,
//                           teacher-forces j+1..N-1, tail[(i,j)] = sum_{n>j} t^(ij)_n(s_n).  N(N-1)(N-2)/6 evaluations per chain.
//
// Device layouts (lstm_pauli_kernels.h's and corr_kernels.h's):
//   bits  [W = ceil(N/32)][ns] u32        spin n of chain s = bit (n & 31) of bits[n >> 5][s]
//   hck   [N-1][nsb][2 KT][64] f64        state after site n in B-fragment order: rows 0..KT-1 h, rows KT..2KT-1 c
//   tck   [N(N-1)/2][nsb][2 KT][64] f64   row pair_index(i, n): trunk i after site n, the same order (rows with n = N-1: unused)
//   bsel, both [N][ns]; tsel, toth, tail [N(N-1)/2][ns] f64
// A ragged last block repeats chain ns-1 and stores no per-chain value for it; its state rows lie inside the block's own rows.
#pragma once
#include "corr_kernels.h"
#include "lstm_core.h"

namespace rnnwf {

// (h, c) of lane `lane` from / to row `row` of a state array [rows][nsb][2 KT][64]
template <int KT>
__device__ __forceinline__ void lstm_load_state(double (&h)[KT], double (&cs)[KT], const void* base, int64_t row, int64_t nsb, int64_t sb,
                                                int lane) {
    const double* src = reinterpret_cast<const double*>(base) + ((row * nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        h[kt] = src[kt * 64];
        cs[kt] = src[(KT + kt) * 64];
    }
}

template <int KT>
__device__ __forceinline__ void lstm_store_state(const double (&h)[KT], const double (&cs)[KT], void* base, int64_t row, int64_t nsb,
                                                 int64_t sb, int lane) {
    double* dst = reinterpret_cast<double*>(base) + ((row * nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        dst[kt * 64] = h[kt];
        dst[(KT + kt) * 64] = cs[kt];
    }
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_corr_base_kernel(CorrArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;                 // waves per workgroup: WAVES, or fewer for small batches (launch_shrinking)
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    for (int64_t sb = gw; sb < a.nsb; sb += nw) {
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;     // a ragged last block repeats the last chain; its lanes write nothing
        double h[KT], cs[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = cs[kt] = 0.0;
        int sig_in = -1;
        uint32_t word = 0;
        for (int n = 0; n < N; ++n) {
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc];     // bit 0: the spin of site n
            const int sig = (int)(word & 1);
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            const double sel = sig ? lp1 : lp0, oth = sig ? lp0 : lp1;
            if (valid && q == 0) {
                a.bsel[(int64_t)n * a.ns + s] = sel;
                a.both[(int64_t)n * a.ns + s] = oth - sel;
            }
            if (n < N - 1) lstm_store_state<KT>(h, cs, const_cast<void*>(a.hck), n, a.nsb, sb, lane);      // this kernel's to write
            sig_in = sig;
        }
    }
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_trunk_kernel(CorrArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    // tiles longest chain first (i ascending), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        const int i = __builtin_amdgcn_readfirstlane((int)(tile / a.nsb));      // the tile is the wave's
        const int64_t sb = tile - (int64_t)i * a.nsb;
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        double h[KT], cs[KT];
        lstm_load_state<KT>(h, cs, a.hck, i, a.nsb, sb, lane);
        uint32_t word = a.bits[(int64_t)(i >> 5) * a.ns + sc] >> (i & 31);      // bit 0: the chain's own spin i
        int sig_in = 1 - (int)(word & 1);                                        // the flipped spin feeds site i+1
        int64_t p = pair_index(i, i + 1, N);
        for (int n = i + 1; n < N; ++n, ++p) {
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc];
            const int sig = (int)(word & 1);
            C::step(img, sig_in, h, cs, lane);
            if (n < N - 1) lstm_store_state<KT>(h, cs, a.tck, p, a.nsb, sb, lane);      // no branch starts at the last site
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            if (valid && q == 0) {
                a.tsel[p * a.ns + s] = sig ? lp1 : lp0;
                a.toth[p * a.ns + s] = sig ? lp0 : lp1;
            }
            sig_in = sig;
        }
    }
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_branch_kernel(CorrArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    // tile = (j (j - 1) / 2 + i) nsb + block, 0 <= i < j <= N-2: longest tail first (j ascending), every wave strides through them
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        const int64_t m = tile / a.nsb;
        const int64_t sb = tile - m * a.nsb;
        int j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)m)) * 0.5f);
        while ((int64_t)j * (j - 1) / 2 > m) --j;
        while ((int64_t)(j + 1) * j / 2 <= m) ++j;
        j = __builtin_amdgcn_readfirstlane(j);                                   // the tile is the wave's
        const int i = __builtin_amdgcn_readfirstlane((int)(m - (int64_t)j * (j - 1) / 2));
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        const int64_t p = pair_index(i, j, N);
        double h[KT], cs[KT];
        lstm_load_state<KT>(h, cs, a.tck, p, a.nsb, sb, lane);
        uint32_t word = a.bits[(int64_t)(j >> 5) * a.ns + sc] >> (j & 31);      // bit 0: the chain's own spin j
        int sig_in = 1 - (int)(word & 1);                                        // the second flipped spin feeds site j+1
        double lp = 0.0;
        for (int n = j + 1; n < N; ++n) {
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc];
            const int sig = (int)(word & 1);
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            lp += sig ? lp1 : lp0;
            sig_in = sig;
        }
        if (valid && q == 0) a.tail[p * a.ns + s] = lp;
    }
}

}  // namespace rnnwf
