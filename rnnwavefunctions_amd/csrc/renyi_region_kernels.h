// renyi_region_kernels.h - the second Renyi entropy of ARBITRARY regions of the positive GRU RNN by the replica swap trick
// (docs/renyi_regions.md).  renyi_kernels.h covers the regions that are a prefix of the site order; here A is any site set, given
// as a mask, normalised by the host so that site 0 is not in A (r_A = r_complement) and A is not empty; f >= 1 is its first site.
//
// Pairs (sigma, tau) = chains (2p, 2p + 1) as in renyi_kernels.h: the partner of chain s is s ^ 1, in the same 16-chain block.
// The mixed chain of s is m_n = (n in A ? the partner's spin : its own).  It shares the sites 0..f-1 with s, so
//     log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)],
//     tail_s = sum_{n >= f} log p(m_n | m_<n),   suffix_s = sum_{n >= f} log p(s_n | s_<n)   (the shared prefixes cancel).
//
//   prnn_region_swap_kernel      : tail_s of every chain and region - tile (region, 16-chain block) restores the chain's OWN hck[f-1],
//                                  feeds its own spin f-1 and teacher-forces m_f..m_{N-1}.  For A = {l..N-1} this is, operation for
//                                  operation, the chain prnn_swap_kernel evaluates for the partner at cut l.
//   renyi_region_assemble_kernel : log r_A of every pair and region from the tails and prnn_site_terms_kernel's replayed terms; per
//                                  (region, 256 pairs) the sums of r and r^2.  renyi_sums_kernel (renyi_kernels.h) reduces them.
#pragma once
#include "renyi_kernels.h"

namespace rnnwf {

struct RegionArgs {
    const void* wimg;            // packed weight image (GruLayout)
    int32_t N;
    int32_t W;                   // ceil(N / 32): spin and mask words per chain / region
    int64_t ns;                  // chains of this pass: 2 x pairs
    int64_t nsb;                 // ceil(ns / 16)
    const uint32_t* bits;        // [W][ns] packed spins
    const void* hck;             // [N-1][nsb][KT][64] T: the base pass's checkpoints
    const uint32_t* mask;        // [R][W]: bit n & 31 of word n >> 5 set = site n in A (normalised: bit 0 of word 0 clear)
    const int32_t* order;        // [nact]: the regions that are not empty, longest mixed chain first (f ascending, ties by index)
    const int32_t* first;        // [R]: f of every region, 0 = empty after normalisation (no tile, log r = 0)
    double* tail;                // [R][ns]: row r = tail_s of region r (rows of empty regions are not written)
    int64_t ntiles;              // nact * nsb
};

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_region_swap_kernel(RegionArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);       // LDS, or the global image where it exceeds LDS (GruLayout::SPILL)
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int64_t gw = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int N = a.N;
    // tiles longest chain first (the host's order), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        // the tile is the wave's: region, first site and mask words live in scalar registers
        const int t = __builtin_amdgcn_readfirstlane((int)(tile / a.nsb));
        const int64_t sb = tile - (int64_t)t * a.nsb;
        const int r = a.order[t];
        const int f = a.first[r];                  // 1 <= f <= N-1
        const int64_t s = sb * kChains + c;
        const int64_t sc = s < a.ns ? s : a.ns - 1;
        T h[KT];
        {
            const T* src = reinterpret_cast<const T*>(a.hck) + (((int64_t)(f - 1) * a.nsb + sb) * KT) * 64 + lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = src[kt * 64];
        }
        const uint32_t* mrow = a.mask + (int64_t)r * a.W;
        // 32 sites of the mixed chain at once: (own & ~mask) | (partner & mask), the mask word the same for the whole wave (ns is
        // even: a valid chain's partner is valid).  Bit 0 of `mixed` is the next site's spin.
        auto mixed_word = [&](int w) {
            const uint32_t m = mrow[w];
            const uint32_t own = a.bits[(int64_t)w * a.ns + sc], par = a.bits[(int64_t)w * a.ns + (sc ^ 1)];
            return (own & ~m) | (par & m);
        };
        uint32_t mixed = mixed_word((f - 1) >> 5) >> ((f - 1) & 31);
        int sig_in = (int)(mixed & 1);             // own spin f-1 (site f-1 is not in A)
        double lp = 0.0;
        for (int n = f; n < N; ++n) {
            mixed = (n & 31) ? mixed >> 1 : mixed_word(n >> 5);
            const int sig = (int)(mixed & 1);
            C::template step<true>(img, sig_in, h, lane);
            T z[1];
            C::head(img, h, lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            lp += (double)(sig ? lp1 : lp0);
            sig_in = sig;
        }
        if (s < a.ns && q == 0) a.tail[(int64_t)r * a.ns + s] = lp;
    }
}

// grid (ceil(npairs / 256), R): thread = pair, blockIdx.y = region.  log_ratio [R][npairs]; part [R][gridDim.x][2]
__global__ void __launch_bounds__(kRenyiThreads) renyi_region_assemble_kernel(const double* tail, const double* terms,
                                                                             const int32_t* first, int N, int64_t ns,
                                                                             double* log_ratio, double* part) {
    __shared__ double r1[kRenyiThreads], r2[kRenyiThreads];
    const int reg = blockIdx.y;
    const int f = first[reg];
    const int64_t np = ns / 2, p = (int64_t)blockIdx.x * kRenyiThreads + threadIdx.x;
    double r = 0.0;
    if (p < np) {
        double lr = 0.0;                           // empty after normalisation: no swap, r = 1
        if (f > 0) {
            double sa = 0.0, sb = 0.0;             // own suffixes, summed in the region kernel's order
            for (int n = f; n < N; ++n) {
                sa += terms[(int64_t)n * ns + 2 * p];
                sb += terms[(int64_t)n * ns + 2 * p + 1];
            }
            const double da = tail[(int64_t)reg * ns + 2 * p] - sa, db = tail[(int64_t)reg * ns + 2 * p + 1] - sb;
            lr = 0.5 * (da + db);
        }
        log_ratio[(int64_t)reg * np + p] = lr;
        r = exp(lr);                               // log r > 709: +inf, and so is this region's sum
    }
    r1[threadIdx.x] = r;
    r2[threadIdx.x] = r * r;
    __syncthreads();
    for (int w = kRenyiThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            r1[threadIdx.x] += r1[threadIdx.x + w];
            r2[threadIdx.x] += r2[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + ((int64_t)reg * gridDim.x + blockIdx.x) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

}  // namespace rnnwf
