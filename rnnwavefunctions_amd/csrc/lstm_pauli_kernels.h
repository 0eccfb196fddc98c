// lstm_pauli_kernels.h - the two recurrent kernels of the LSTM wave function's Pauli pass (rnnwf_pauli_step_lstm, lstm_pauli.hip;
// docs/pauli_lstm.md), on LstmCore<NFULL> (lstm_core.h).  They are the LSTM counterparts of the base pass + prnn_site_terms_kernel
// and of prnn_masked_tail_kernel<..., PAIRED = false> (chain_kernels.h); from the log-ratios on the pass runs pauli_kernels.h's
// kernels, which read the same layouts.
//
//   lstm_site_terms_kernel  : the teacher-forced base pass of this entry, 16 chains per wave: checkpoints (h, c) after every site
//                             but the last, log P per chain, and the per-site terms log p(sigma_n | sigma_<n) that
//                             pauli_log_ratio_kernel adds up for a chain's own suffix.  log P is added as lstm_base_kernel adds it
//                             (the same terms in the same order): it equals rnnwf_log_prob's bit for bit.
//   lstm_masked_tail_kernel : tail of every chain and distinct flip mask - tile (mask, 16-chain block), persistent, one tile per wave
//                             at a time.  f >= 1: restores the chain's own (h, c) of hck[f-1], feeds its own spin f-1 and
//                             teacher-forces sites f..N-1 on own_word ^ mask_word.  f = 0: starts as the base pass does, from the
//                             zero state and the zero input, and runs all N sites.
//                             PAIRED (lstm_renyi.hip, docs/renyi_lstm.md): chains (2p, 2p + 1) are a replica pair and a masked site
//                             takes the partner's spin, (own_word & ~mask_word) | (partner_word & mask_word); the host normalises
//                             the masks so that site 0 is never masked, 1 <= f <= N-1.  The start is the !PAIRED form's,
//                             wave-uniform selects on f > 0 included (docs/renyi_stack.md, "Resources").
//
// Device layouts (lstm_kernels.h's and pauli_kernels.h's):
//   bits  [W = ceil(N/32)][ns] u32   spin n of chain s = bit (n & 31) of bits[n >> 5][s]
//   hck   [N-1][nsb][2 KT][64] f64   state after site n in B-fragment order: rows 0..KT-1 h, rows KT..2KT-1 c
//   terms [N][ns] f64, logp [ns] f64, tail [M][ns] f64
//   mask  [M][W] u32, no mask empty; order [M]: the masks longest chain first; first [M]: 0 <= f <= N-1
//   PAIRED: mask [R][W] the normalised region masks, order [nact] the regions that have a tail, first [R]: 1 <= f <= N-1 for those
#pragma once
#include "chain_kernels.h"
#include "lstm_core.h"

namespace rnnwf {

struct LstmTermsArgs {
    const void* wimg;            // packed weight image (LstmLayout)
    int32_t N;
    int64_t ns;                  // chains of this pass
    int64_t nsb;                 // ceil(ns / 16)
    const uint32_t* bits;        // [W][ns] packed spins
    double* hck;                 // out: the checkpoints
    double* terms;               // out: [N][ns]
    double* out_lp;              // out: [ns]
};

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) lstm_site_terms_kernel(LstmTermsArgs a) {
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
        double cum = 0.0;
        for (int n = 0; n < N; ++n) {
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc];     // bit 0: the spin of site n
            const int sig = (int)(word & 1);
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            const double term = sig ? lp1 : lp0;
            if (valid && q == 0) a.terms[(int64_t)n * a.ns + s] = term;
            cum += term;
            if (n < N - 1) {
                double* dst = a.hck + (((int64_t)n * a.nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    dst[kt * 64] = h[kt];
                    dst[(KT + kt) * 64] = cs[kt];
                }
            }
            sig_in = sig;
        }
        if (valid && q == 0) a.out_lp[s] = cum;
    }
}

template <int NFULL, int WAVES, bool PAIRED = false>
__global__ void __launch_bounds__(WAVES * 64) lstm_masked_tail_kernel(MaskArgs a) {
    using C = LstmCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wpb = blockDim.x >> 6;                 // waves per workgroup: WAVES, or fewer for small batches (launch_shrinking)
    const int64_t gw = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * wpb;
    const int N = a.N;
    // tiles longest chain first (the host's order), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        // the tile is the wave's: row, first site and mask words live in scalar registers
        const int t = __builtin_amdgcn_readfirstlane((int)(tile / a.nsb));
        const int64_t sb = tile - (int64_t)t * a.nsb;
        const int r = a.order[t];
        const int f = a.first[r];
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        const uint32_t* mrow = a.mask + (int64_t)r * a.W;
        // 32 sites of the changed chain at once, the mask word the same for the whole wave (PAIRED: ns is even, a valid chain's
        // partner is valid)
        auto changed_word = [&](int k) {
            if constexpr (PAIRED) {
                // the partner s ^ 1 is the neighbouring lane of the quad (c ^ 1): its word by DPP quad_perm [1,0,3,2], no second
                // load and no second address in vector registers.  A chain beyond ns has its partner beyond ns too (ns is even);
                // both read chain ns - 1 and neither is stored.
                const uint32_t m = mrow[k];
                const uint32_t own = a.bits[(int64_t)k * a.ns + sc];
                const uint32_t par = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, false);
                return (own & ~m) | (par & m);
            } else {
                return a.bits[(int64_t)k * a.ns + sc] ^ mrow[k];
            }
        };
        // branch-free start (f is wave-uniform): for f = 0 the load of hck[0] is discarded (PAIRED: the host never emits f = 0)
        const int g = f > 0 ? f - 1 : 0;
        double h[KT], cs[KT];
        {
            const double* src = reinterpret_cast<const double*>(a.hck) + (((int64_t)g * a.nsb + sb) * 2 * KT) * 64 + lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                h[kt] = f > 0 ? src[kt * 64] : 0.0;
                cs[kt] = f > 0 ? src[(KT + kt) * 64] : 0.0;
            }
        }
        uint32_t word = changed_word(g >> 5) >> (g & 31);      // f >= 1: bit 0 is the chain's own spin f-1 (no site below f is changed)
        int sig_in = f > 0 ? (int)(word & 1) : -1;
        double lp = 0.0;
        for (int n = f; n < N; ++n) {
            word = (n & 31) ? word >> 1 : changed_word(n >> 5);
            const int sig = (int)(word & 1);
            C::step(img, sig_in, h, cs, lane);
            const double z = C::head(img, h, lane);
            double lp0, lp1;
            log_softmax2(z, lp0, lp1);
            lp += sig ? lp1 : lp0;
            sig_in = sig;
        }
        if (valid && q == 0) a.tail[(int64_t)r * a.ns + s] = lp;
    }
}

}  // namespace rnnwf
