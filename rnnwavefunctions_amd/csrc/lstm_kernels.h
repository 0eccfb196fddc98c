// lstm_kernels.h - the two recurrent kernels of the LSTM wave function (model LSTM1D_F64), the LSTM counterparts of
// prnn_base_kernel / prnn_flip_kernel (gru_kernels.h):
//
//   lstm_base_kernel : one pass over all N sites (raster order ny*Nx + nx, 2DTFIM_1DRNN/RNNwavefunction.py:74-80,118-123)
//                      for every chain, 16 chains per wave: ancestral sampling or teacher-forced evaluation; optionally
//                      checkpoints (h, c) after every site and the "flip base" log-probabilities of the flip pass.
//   lstm_flip_kernel : for every (flipped site i, block of 16 chains) re-evaluates sites i+1..N-1 from checkpoint i.
//
// Device layouts (all coalesced per wave):
//   bits [W = ceil(N/32)][ns] u32   spin n of chain s = bit (n & 31) of bits[n >> 5][s]
//   hck  [N-1][nsb][2 KT][64] f64  state after site n in B-fragment order: rows 0..KT-1 h, rows KT..2KT-1 c
//   lpq  [N+1][ns]            f64  row 0: log P(s); row k+1: log P(s with site k flipped)
#pragma once
#include "lstm_core.h"

namespace rnnwf {

struct LstmArgs {
    const void* wimg;            // packed weight image (LstmLayout)
    int32_t N;                   // sites
    int64_t ns;                  // chains in this launch
    int64_t nsb;                 // ceil(ns / 16)
    uint32_t* bits;              // in (teacher) / out (sampling)
    double* hck;                 // nullptr: no checkpoints
    double* lpq;                 // nullptr: no flip base
    double* out_lp;              // [ns] log P of the chain (may be nullptr)
    uint64_t seed, step;
    int64_t sample_offset;
    int32_t sampling;            // 1: draw spins, 0: read them from bits
    int64_t ntiles;              // flip pass: (N-1) * nsb
};

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_base_kernel(LstmArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;                 // waves per workgroup: WAVES, or fewer for small batches (lstm.hip)
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    for (int64_t sb = gw; sb < a.nsb; sb += nw) {
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        double h[KT], cs[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = cs[kt] = 0.0;
        int sig_in = -1;
        uint32_t word = 0;
        double cum = 0.0;
        for (int n = 0; n < N; ++n) {
            if (!a.sampling && (n & 31) == 0) word = a.bits[(int64_t)(n >> 5) * a.ns + sc];
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            int sig;
            if (a.sampling) {
                // tf.multinomial(log p): class 0 iff u * total < p0 (the rule and Philox stream of the GRU sampler)
                const float u = philox_uniform(a.seed, a.step, (uint64_t)(a.sample_offset + sc), n);
                sig = ((double)u < prob0(z)) ? 0 : 1;
                word |= (uint32_t)sig << (n & 31);
                if (((n & 31) == 31 || n == N - 1) && valid && q == 0) a.bits[(int64_t)(n >> 5) * a.ns + s] = word;
                if ((n & 31) == 31) word = 0;
            } else {
                sig = (word >> (n & 31)) & 1;
            }
            if (a.lpq && valid && q == 0) a.lpq[(int64_t)(n + 1) * a.ns + s] = cum + (sig ? lp0 : lp1);
            cum += sig ? lp1 : lp0;
            if (a.hck && n < N - 1) {
                double* dst = a.hck + (((int64_t)n * a.nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    dst[kt * 64] = h[kt];
                    dst[(KT + kt) * 64] = cs[kt];
                }
            }
            sig_in = sig;
        }
        if (valid && q == 0) {
            if (a.lpq) a.lpq[s] = cum;
            if (a.out_lp) a.out_lp[s] = cum;
        }
    }
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_flip_kernel(LstmArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;                 // waves per workgroup: WAVES, or fewer for small batches (lstm.hip)
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    // tiles ordered longest chain first (i ascending); every wave strides through them and gets the same mix of lengths
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        const int i = (int)(tile / a.nsb);
        const int64_t sb = tile - (int64_t)i * a.nsb;
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        double h[KT], cs[KT];
        {
            const double* src = a.hck + (((int64_t)i * a.nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                h[kt] = src[kt * 64];
                cs[kt] = src[(KT + kt) * 64];
            }
        }
        auto spin = [&](int n) { return (int)((a.bits[(int64_t)(n >> 5) * a.ns + sc] >> (n & 31)) & 1); };
        int sig_in = 1 - spin(i);                  // the flipped spin feeds site i+1
        double lp = 0.0;
        for (int n = i + 1; n < N; ++n) {
            const int sig = spin(n);
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            lp += sig ? lp1 : lp0;
            sig_in = sig;
        }
        if (valid && q == 0) a.lpq[(int64_t)(i + 1) * a.ns + s] += lp;
    }
}

}  // namespace rnnwf
