// pauli_kernels.h - expectation values of Pauli strings and local energies of arbitrary real spin-1/2 Hamiltonians for the positive
// GRU RNN (docs/pauli.md).  A term is O = (prod_{i in S} sz_i)(prod_{i in F} sx_i); with s = 2 sigma - 1 and sigma ~ P = psi^2
//     v(sigma) = prod_{i in S} s_i * exp(1/2 [log P(sigma ^ F) - log P(sigma)]),   E[v] = <psi|O|psi>.
// sigma ^ F shares the sites 0..f-1 with sigma (f = first site of F), so
//     log P(sigma ^ F) - log P(sigma) = tail - suffix,   tail = sum_{n >= f} log p((sigma ^ F)_n | (sigma ^ F)_<n),
//                                                        suffix = sum_{n >= f} log p(sigma_n | sigma_<n).
//
//   prnn_masked_tail_kernel: (chain_kernels.h, not PAIRED) tail of every chain and distinct flip mask - tile (mask, 16-chain block).
//                           f >= 1: restores the chain's own hck[f-1], feeds its own spin f-1 and teacher-forces sites f..N-1 on
//                           own_word ^ mask_word.  f = 0: starts as the base pass does and runs all N sites.
//                           MaskArgs: mask [M][W], no mask empty; order [M]; first [M], 0 <= f <= N-1.
//   pauli_log_ratio_kernel: 1/2 (tail - suffix) per (mask, chain); the suffix is prnn_site_terms_kernel's replayed terms added in
//                           the flip kernel's order (f >= 1) or the base pass's log P (f = 0, the same additions in the same order).
//   pauli_term_kernel     : v of every (term, chain): sign by popcount parity of spin word & sign word; per (term, 256 chains) the
//                           sums of v and v^2, reduced by renyi_sums_kernel in a fixed order (no atomics).
//   pauli_eloc_kernel     : E_loc(sigma) = sum_k coeff_k v_k(sigma), terms in the caller's order.
#pragma once
#include "renyi_kernels.h"

namespace rnnwf {

constexpr int kPauliThreads = kRenyiThreads;   // chains per block of the assembly kernels (renyi_sums_kernel reduces their partial sums)

// (inline, as is renyi_sums_kernel: pauli.hip and mdrnn_pauli.hip both include this header)
// grid (ceil(ns / 256), M): thread = chain, blockIdx.y = mask.  log_ratio [M][ns]
inline __global__ void __launch_bounds__(kPauliThreads) pauli_log_ratio_kernel(const double* tail, const double* terms, const double* logp,
                                                                       const int32_t* first, int N, int64_t ns, double* log_ratio) {
    const int m = blockIdx.y;
    const int f = first[m];
    const int64_t s = (int64_t)blockIdx.x * kPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double own;
    if (f > 0) {
        own = 0.0;                                 // own suffix, summed in the flip kernel's order
        for (int n = f; n < N; ++n) own += terms[(int64_t)n * ns + s];
    } else {
        own = logp[s];                             // the base pass added the same terms from site 0 on
    }
    log_ratio[(int64_t)m * ns + s] = 0.5 * (tail[(int64_t)m * ns + s] - own);
}

// v_k(sigma): the sign from the packed spins, the ratio from the term's mask row (tmask < 0: diagonal term, ratio 1)
__device__ __forceinline__ double pauli_value(const uint32_t* bits, const uint32_t* sgn, const double* log_ratio, int tmask, int W,
                                              int64_t ns, int64_t s) {
    int odd = 0;                                   // parity of the number of sites of S with s_i = -1
    for (int w = 0; w < W; ++w) {
        const uint32_t sw = sgn[w];
        odd ^= __popc(sw) ^ __popc(bits[(int64_t)w * ns + s] & sw);
    }
    const double r = tmask < 0 ? 1.0 : exp(log_ratio[(int64_t)tmask * ns + s]);     // log r > 709: +inf, and so is every sum it enters
    return (odd & 1) ? -r : r;
}

// grid nterms * nblk (nblk = ceil(ns / 256)): block = (term k, 256 chains).  part [nterms][nblk][2]
inline __global__ void __launch_bounds__(kPauliThreads) pauli_term_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                  const double* log_ratio, int W, int64_t ns, int64_t nblk, double* part) {
    __shared__ double r1[kPauliThreads], r2[kPauliThreads];
    const int64_t k = blockIdx.x / nblk, b = blockIdx.x - k * nblk;
    const int64_t s = b * kPauliThreads + threadIdx.x;
    const double v = s < ns ? pauli_value(bits, sgn + k * W, log_ratio, tmask[k], W, ns, s) : 0.0;
    block_sum2(v, v * v, r1, r2);
    if (threadIdx.x == 0) {
        double* o = part + (k * nblk + b) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

// grid ceil(ns / 256): thread = chain; the terms in the caller's order
inline __global__ void __launch_bounds__(kPauliThreads) pauli_eloc_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                  const double* coeff, const double* log_ratio, int nterms, int W,
                                                                  int64_t ns, double* eloc) {
    const int64_t s = (int64_t)blockIdx.x * kPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double e = 0.0;
    for (int k = 0; k < nterms; ++k) e += coeff[k] * pauli_value(bits, sgn + (int64_t)k * W, log_ratio, tmask[k], W, ns, s);
    eloc[s] = e;
}

}  // namespace rnnwf
