// stack_chain_kernels.h - the kernels that restart a STACK of GRU layers from the base pass's checkpoints (pauli_stack.hip,
// docs/pauli_stack.md): chain_kernels.h's masked tail and renyi_kernels.h's site-term replay over the layer stack S (gru_core.h:
// GruStack, NL = 2..4).  Arguments, wave prologue and tile order are chain_kernels.h's (MaskArgs, SwapArgs, WaveTile); the
// checkpoints are the stack's, hck[N][nsb][NL][KT][64] (S::ROW values per lane and site, all N sites), as prnn_ml_base_kernel
// writes them.
//
//   prnn_ml_masked_tail_kernel : tail of every chain and distinct mask - tile (mask, 16-chain block).  f >= 1: restores EVERY
//                                layer's state from row f - 1, feeds the chain's own spin f - 1 and teacher-forces sites f..N-1 on
//                                own_word ^ mask_word.  f = 0: zero states, input -1, all N sites.
//                                PAIRED (renyi_stack.hip, docs/renyi_stack.md): chains (2p, 2p + 1) are a pair and a masked site
//                                takes the partner's spin, (own_word & ~mask_word) | (partner_word & mask_word); the host
//                                normalises the masks so that site 0 is never masked, 1 <= f <= N-1.  The start is the !PAIRED
//                                form's, wave-uniform selects on f > 0 included: without them the checkpoint loads are hoisted
//                                and <float, 1, 4, 4> needs 100 vector registers for 82 (5 -> 4 waves per SIMD).
//   prnn_ml_site_terms_kernel  : log p(sigma_n | sigma_<n) of every chain and site 1..N-1: the head on the top layer's checkpoint
//                                of site n - the stack keeps the state after the last site too, so no site takes a step here.
// Both run the base pass's step form (S::BASE_BIAS_LAST) and head on the states prnn_ml_base_kernel stored, and pauli_log_ratio_kernel
// adds the replayed terms in the tail's order: what should cancel against the base pass's own terms cancels exactly.
#pragma once
#include "renyi_kernels.h"

namespace rnnwf {

template <typename T, int NFULL, int NL, int WAVES, bool PAIRED = false>
__global__ void __launch_bounds__(WAVES * 64) prnn_ml_masked_tail_kernel(MaskArgs a) {
    using S = GruStack<T, NFULL, NL, 1>;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = S::stage(lds, a.wimg);       // the layers that fit LDS; the others are read from a.wimg (layout.h: MlSpill)
    const WaveTile<WAVES> w;
    const int N = a.N;
    // tiles longest chain first (the host's order), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = w.gw; tile < a.ntiles; tile += w.nw) {
        // the tile is the wave's: row, first site and mask words live in scalar registers
        const int t = __builtin_amdgcn_readfirstlane((int)(tile / a.nsb));
        const int64_t sb = tile - (int64_t)t * a.nsb;
        const int r = a.order[t];
        const int f = a.first[r];
        const int64_t s = sb * kChains + w.c;
        const int64_t sc = s < a.ns ? s : a.ns - 1;
        const uint32_t* mrow = a.mask + (int64_t)r * a.W;
        // 32 sites of the changed chain at once, the mask word the same for the whole wave (PAIRED: ns is even, a valid chain's
        // partner is valid).  Bit 0 of `word` is the next site's spin.
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
        // branch-free start (f is wave-uniform): for f = 0 the load of row 0 is discarded (PAIRED: the host never emits f = 0)
        const int g = f > 0 ? f - 1 : 0;
        T h[S::NL][S::KT];
        {
            const T* src = reinterpret_cast<const T*>(a.hck) + (((int64_t)g * a.nsb + sb) * S::ROW) * 64 + w.lane;
#pragma unroll
            for (int l = 0; l < S::NL; ++l)
#pragma unroll
                for (int kt = 0; kt < S::KT; ++kt) h[l][kt] = f > 0 ? src[(l * S::KT + kt) * 64] : T(0);
        }
        uint32_t word = changed_word(g >> 5) >> (g & 31);
        int sig_in = f > 0 ? (int)(word & 1) : -1;
        double lp = 0.0;
        for (int n = f; n < N; ++n) {
            word = (n & 31) ? word >> 1 : changed_word(n >> 5);
            const int sig = (int)(word & 1);
            S::template step<S::BASE_BIAS_LAST>(img, a.wimg, sig_in, h, w.lane);
            T z[1];
            S::head(img, h, w.lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            lp += (double)(sig ? lp1 : lp0);
            sig_in = sig;
        }
        if (s < a.ns && w.q == 0) a.tail[(int64_t)r * a.ns + s] = lp;
    }
}

template <typename T, int NFULL, int NL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_ml_site_terms_kernel(SwapArgs a) {
    using S = GruStack<T, NFULL, NL, 1>;
    constexpr int KT = S::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = S::stage(lds, a.wimg);
    const WaveTile<WAVES> w;
    const int N = a.N;
    for (int64_t sb = w.gw; sb < a.nsb; sb += w.nw) {
        const int64_t s = sb * kChains + w.c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        // the top layer's part of row n: + n nsb ROW 64
        const T* ck = reinterpret_cast<const T*>(a.hck) + (sb * S::ROW + (S::NL - 1) * KT) * 64 + w.lane;
        for (int n = 1; n < N; ++n) {
            T h[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = ck[((int64_t)n * a.nsb * S::ROW + kt) * 64];
            T z[1];
            S::C0::head(img, h, w.lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            if (valid && w.q == 0) a.terms[(int64_t)n * a.ns + s] = (double)(spin_of(a.bits, a.ns, sc, n) ? lp1 : lp0);
        }
    }
}

}  // namespace rnnwf
