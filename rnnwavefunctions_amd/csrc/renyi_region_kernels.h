// renyi_region_kernels.h - the second Renyi entropy of ARBITRARY regions of the positive GRU RNN by the replica swap trick
// (docs/renyi_regions.md).  renyi_kernels.h covers the regions that are a prefix of the site order; here A is any site set, given
// as a mask, normalised by the host so that site 0 is not in A (r_A = r_complement) and A is not empty; f >= 1 is its first site.
//
// Pairs (sigma, tau) = chains (2p, 2p + 1) as in renyi_kernels.h: the partner of chain s is s ^ 1, in the same 16-chain block.
// The mixed chain of s is m_n = (n in A ? the partner's spin : its own).  It shares the sites 0..f-1 with s, so
//     log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)],
//     tail_s = sum_{n >= f} log p(m_n | m_<n),   suffix_s = sum_{n >= f} log p(s_n | s_<n)   (the shared prefixes cancel).
//
//   prnn_masked_tail_kernel      : (chain_kernels.h, PAIRED) tail_s of every chain and region - tile (region, 16-chain block) restores
//                                  the chain's OWN hck[f-1], feeds its own spin f-1 and teacher-forces m_f..m_{N-1}.  For A = {l..N-1}
//                                  this is, operation for operation, the chain prnn_swap_kernel evaluates for the partner at cut l.
//                                  MaskArgs: mask [R][W] (normalised: bit 0 of word 0 clear), order [nact] the regions that are not
//                                  empty, first [R] with 0 = empty after normalisation (no tile, log r = 0).
//   renyi_region_assemble_kernel : log r_A of every pair and region from the tails and prnn_site_terms_kernel's replayed terms; per
//                                  (region, 256 pairs) the sums of r and r^2.  renyi_sums_kernel (renyi_kernels.h) reduces them.
#pragma once
#include "renyi_kernels.h"

namespace rnnwf {

// (inline, as renyi_kernels.h's: renyi_regions.hip and mdrnn_renyi.hip both include this header)
// grid (ceil(npairs / 256), R): thread = pair, blockIdx.y = region.  log_ratio [R][npairs]; part [R][gridDim.x][2]
inline __global__ void __launch_bounds__(kRenyiThreads) renyi_region_assemble_kernel(const double* tail, const double* terms,
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
    block_sum2(r, r * r, r1, r2);
    if (threadIdx.x == 0) {
        double* o = part + ((int64_t)reg * gridDim.x + blockIdx.x) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

}  // namespace rnnwf
