// pauli_train_kernels.h - the assembly of rnnwf_pauli_train_steps (pauli.hip) and rnnwf_pauli_train_steps_2d (mdrnn_pauli.hip, whose
// tails, site terms and log P have the same layout; docs/pauli_train.md), each instantiating it under its own flags: the kernels of pauli_kernels.h
// with the amplitude ratio evaluated once per (flip mask, chain) instead of once per (term, chain) and per kernel.  Terms that share a
// mask (XX and YY of a bond) and the two consumers (E_loc, per-term sums) read one table.
//
//   pauli_ratio_kernel     : r = exp(1/2 (tail - suffix)) per (mask, chain) - pauli_log_ratio_kernel's suffix, subtraction and
//                            halving, then pauli_value's exp, in one thread: the value pauli_value forms from the stored log-ratio.
//   pauli_table_eloc_kernel: pauli_eloc_kernel with r read from the table: the terms in the caller's order, the same
//                            e += coeff[k] * v.
//   pauli_table_term_kernel: pauli_term_kernel with r read from the table; its partial sums are reduced by renyi_sums_kernel, which
//                            writes the iteration's row of the call's table of per-term sums.
// Every result equals the kernel's it replaces bit for bit (tests/test_gpu_pauli_train.py, tests/test_gpu_pauli_train_2d.py).  log r > 709 gives r = +inf as there.
#pragma once
#include "pauli_kernels.h"

namespace rnnwf {

// grid (ceil(ns / 256), M): thread = chain, blockIdx.y = mask.  ratio [M][ns]
inline __global__ void __launch_bounds__(kPauliThreads) pauli_ratio_kernel(const double* tail, const double* terms, const double* logp,
                                                                   const int32_t* first, int N, int64_t ns, double* ratio) {
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
    const double log_ratio = 0.5 * (tail[(int64_t)m * ns + s] - own);
    ratio[(int64_t)m * ns + s] = exp(log_ratio);   // log r > 709: +inf, and so is every sum it enters
}

// v_k(sigma): the sign from the packed spins, the ratio from the term's row of the table (tmask < 0: diagonal term, ratio 1)
__device__ __forceinline__ double pauli_table_value(const uint32_t* bits, const uint32_t* sgn, const double* ratio, int tmask, int W,
                                                    int64_t ns, int64_t s) {
    int odd = 0;                                   // parity of the number of sites of S with s_i = -1
    for (int w = 0; w < W; ++w) {
        const uint32_t sw = sgn[w];
        odd ^= __popc(sw) ^ __popc(bits[(int64_t)w * ns + s] & sw);
    }
    const double r = tmask < 0 ? 1.0 : ratio[(int64_t)tmask * ns + s];
    return (odd & 1) ? -r : r;
}

// grid nterms * nblk (nblk = ceil(ns / 256)): block = (term k, 256 chains).  part [nterms][nblk][2]
inline __global__ void __launch_bounds__(kPauliThreads) pauli_table_term_kernel(const uint32_t* bits, const uint32_t* sgn,
                                                                        const int32_t* tmask, const double* ratio, int W, int64_t ns,
                                                                        int64_t nblk, double* part) {
    __shared__ double r1[kPauliThreads], r2[kPauliThreads];
    const int64_t k = blockIdx.x / nblk, b = blockIdx.x - k * nblk;
    const int64_t s = b * kPauliThreads + threadIdx.x;
    const double v = s < ns ? pauli_table_value(bits, sgn + k * W, ratio, tmask[k], W, ns, s) : 0.0;
    block_sum2(v, v * v, r1, r2);
    if (threadIdx.x == 0) {
        double* o = part + (k * nblk + b) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

// grid ceil(ns / 256): thread = chain; the terms in the caller's order
inline __global__ void __launch_bounds__(kPauliThreads) pauli_table_eloc_kernel(const uint32_t* bits, const uint32_t* sgn,
                                                                        const int32_t* tmask, const double* coeff, const double* ratio,
                                                                        int nterms, int W, int64_t ns, double* eloc) {
    const int64_t s = (int64_t)blockIdx.x * kPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double e = 0.0;
    for (int k = 0; k < nterms; ++k) e += coeff[k] * pauli_table_value(bits, sgn + (int64_t)k * W, ratio, tmask[k], W, ns, s);
    eloc[s] = e;
}

}  // namespace rnnwf
