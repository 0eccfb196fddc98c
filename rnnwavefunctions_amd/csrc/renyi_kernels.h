// renyi_kernels.h - the second Renyi entropy of the positive GRU RNN by the replica swap trick (docs/renyi.md).
//
// Pairs (sigma, tau) = chains (2p, 2p + 1), so both halves of a pair sit in the same 16-chain block and, in the B-fragment
// checkpoint layout of prnn_base_kernel (hck[N-1][nsb][KT][64], chain = lane & 15), the partner's state is at lane ^ 1.
// For a cut l (A = sites 0..l-1):
//     log r_l = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)] = 1/2 (d_2p(l) + d_2p+1(l)),
//     d_s(l) = tail_s(l) - suffix_s(l)
// where tail_s(l) is the log-probability of chain s's own spins l..N-1 after the PARTNER's first l spins and suffix_s(l) that
// of the same spins after its own (the shared prefixes cancel).
//
//   prnn_swap_kernel        : tail_s(l) for every chain and cut 1..N-1 - tile i = l-1 restores the partner's hck[l-1], feeds the
//                             partner's spin l-1 and teacher-forces the chain's own spins l..N-1 (prnn_flip_kernel with another
//                             restart state and first input).
//   prnn_site_terms_kernel  : log p(sigma_n | sigma_<n) of every chain and site 1..N-1, replayed from the checkpoints (site n's
//                             head reads hck[n]; the last site takes one step from hck[N-2]).
//   renyi_assemble_kernel   : log r_l of every pair and cut; per (cut, 256 pairs) the sums of r and r^2.
//   renyi_sums_kernel       : those partial sums reduced per cut, in a fixed order (no atomics: a repeated call is bit-identical).
// The arguments, the wave prologue, the site loop and the block reduction are chain_kernels.h's.  The swap and replay kernels run the base pass's step form (step<true>, bias last) and head on the states the base pass stored,
// and the assembly adds the replayed terms in the swap kernel's order: a chain paired with itself gives d = 0 exactly.
#pragma once
#include "chain_kernels.h"

namespace rnnwf {

constexpr int kRenyiThreads = kSumThreads;   // pairs per block of the assembly

struct SwapArgs : ChainArgs {   // ns = 2 x pairs
    double* tail;                // [N-1][ns]: row l-1 = tail_s(l)
    double* terms;               // [N][ns]: row n = log p(sigma_n | sigma_<n) (row 0 not written)
    int64_t ntiles;              // (N-1) * nsb
};

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_swap_kernel(SwapArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);       // LDS, or the global image where it exceeds LDS (GruLayout::SPILL)
    const WaveTile<WAVES> w;
    const int N = a.N;
    // tiles longest chain first (i ascending), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = w.gw; tile < a.ntiles; tile += w.nw) {
        const int i = (int)(tile / a.nsb);
        const int64_t sb = tile - (int64_t)i * a.nsb;
        const int64_t s = sb * kChains + w.c;
        const int64_t sc = s < a.ns ? s : a.ns - 1;
        T h[KT];
        w.load_state(h, a.hck, i, a.nsb, sb, w.lane ^ 1);
        // the partner's spin l-1 feeds site l (ns is even: a valid chain's partner is valid)
        const double lp = teacher_forced_tail<C>(img, h, spin_of(a.bits, a.ns, sc ^ 1, i), i + 1, N, w.lane,
                                                 [&](int n) { return spin_of(a.bits, a.ns, sc, n); });
        if (s < a.ns && w.q == 0) a.tail[(int64_t)i * a.ns + s] = lp;
    }
}

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_site_terms_kernel(SwapArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const WaveTile<WAVES> w;
    const int N = a.N;
    for (int64_t sb = w.gw; sb < a.nsb; sb += w.nw) {
        const int64_t s = sb * kChains + w.c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        const T* ck = reinterpret_cast<const T*>(a.hck) + (sb * KT) * 64 + w.lane;      // + n nsb KT 64: hck[n]
        T h[KT];
        auto term = [&](int n) {
            T z[1];
            C::head(img, h, w.lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            if (valid && w.q == 0) a.terms[(int64_t)n * a.ns + s] = (double)(spin_of(a.bits, a.ns, sc, n) ? lp1 : lp0);
        };
        for (int n = 1; n < N - 1; ++n) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = ck[((int64_t)n * a.nsb * KT + kt) * 64];
            term(n);
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = ck[((int64_t)(N - 2) * a.nsb * KT + kt) * 64];
        C::template step<true>(img, spin_of(a.bits, a.ns, sc, N - 2), h, w.lane);
        term(N - 1);
    }
}

// (inline, as is renyi_sums_kernel: renyi.hip and renyi_regions.hip both include this header)
// grid (ceil(npairs / 256), N + 1): thread = pair, blockIdx.y = cut.  log_ratio [N+1][npairs]; part [N+1][gridDim.x][2]
inline __global__ void __launch_bounds__(kRenyiThreads) renyi_assemble_kernel(const double* tail, const double* terms, int N, int64_t ns,
                                                                      double* log_ratio, double* part) {
    __shared__ double r1[kRenyiThreads], r2[kRenyiThreads];
    const int l = blockIdx.y;
    const int64_t np = ns / 2, p = (int64_t)blockIdx.x * kRenyiThreads + threadIdx.x;
    double r = 0.0;
    if (p < np) {
        double lr = 0.0;                           // cuts 0 and N: no swap, r = 1
        if (l > 0 && l < N) {
            double sa = 0.0, sb = 0.0;             // own suffixes, summed in the swap kernel's order
            for (int n = l; n < N; ++n) {
                sa += terms[(int64_t)n * ns + 2 * p];
                sb += terms[(int64_t)n * ns + 2 * p + 1];
            }
            const double da = tail[(int64_t)(l - 1) * ns + 2 * p] - sa, db = tail[(int64_t)(l - 1) * ns + 2 * p + 1] - sb;
            lr = 0.5 * (da + db);
        }
        log_ratio[(int64_t)l * np + p] = lr;
        r = exp(lr);                               // log r > 709: +inf, and so is this cut's sum (docs/renyi.md)
    }
    block_sum2(r, r * r, r1, r2);
    if (threadIdx.x == 0) {
        double* o = part + ((int64_t)l * gridDim.x + blockIdx.x) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

// one block per cut: sums[l] = the partial sums of renyi_assemble_kernel over its blocks, each thread a fixed stride, then a tree
inline __global__ void __launch_bounds__(kRenyiThreads) renyi_sums_kernel(const double* part, int64_t nblk, double* sums) {
    __shared__ double r1[kRenyiThreads], r2[kRenyiThreads];
    const int l = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t k = threadIdx.x; k < nblk; k += kRenyiThreads) {
        a += part[((int64_t)l * nblk + k) * 2];
        b += part[((int64_t)l * nblk + k) * 2 + 1];
    }
    block_sum2(a, b, r1, r2);
    if (threadIdx.x == 0) {
        sums[2 * l] = r1[0];
        sums[2 * l + 1] = r2[0];
    }
}

}  // namespace rnnwf
