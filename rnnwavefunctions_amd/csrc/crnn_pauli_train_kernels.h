// crnn_pauli_train_kernels.h - the assembly of rnnwf_pauli_train_steps_complex (crnn_pauli.hip, docs/pauli_train.md): the kernels of
// crnn_pauli_kernels.h with the amplitude ratio psi(sigma ^ F) / psi(sigma) evaluated once per (flip mask, chain) instead of once per
// (term, chain) and per kernel.
//
//   crnn_pauli_ratio_kernel     : crnn_pauli_log_ratio_kernel's d = tail - suffix, then crnn_pauli_value's exp(d.re) (cos d.im,
//                                 sin d.im), in one thread; a flipped configuration outside the zero-magnetisation sector gives
//                                 exactly (0, 0), selected before the transcendental functions as there.
//   crnn_pauli_table_eloc_kernel: crnn_pauli_eloc_kernel with the ratio read from the table (no contraction, as there).
//   crnn_pauli_table_term_kernel: crnn_pauli_term_kernel with the ratio read from the table; renyi_sums_kernel reduces its partial
//                                 sums into the iteration's row of the call's table of per-term sums.
// Every result equals the kernel's it replaces bit for bit (tests/test_gpu_pauli_train.py).
#pragma once
#include "crnn_pauli_kernels.h"

namespace rnnwf {

// grid (ceil(ns / 256), M): thread = chain, blockIdx.y = mask.  ratio [M][ns]
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_ratio_kernel(const double2* tail, const double2* terms, const double2* tot,
                                                                          const int32_t* first, int N, int64_t ns, double2* ratio) {
    const int m = blockIdx.y;
    const int f = first[m];
    const int64_t s = (int64_t)blockIdx.x * kCPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double2 own;
    if (f > 0) {
        own = make_double2(0.0, 0.0);              // own suffix, summed in the tail kernel's order
        for (int n = f; n < N; ++n) {
            const double2 t = terms[(int64_t)n * ns + s];
            own.x += t.x;
            own.y += t.y;
        }
    } else {
        own = tot[s];                              // the base pass added the same terms from site 0 on
    }
    const double2 t = tail[(int64_t)m * ns + s];
    const bool zero = t.x == -__builtin_inf();     // sigma ^ F is outside the sector: psi = 0 exactly; no 0 * inf below
    const double mag = exp(zero ? 0.0 : t.x - own.x), ph = zero ? 0.0 : t.y - own.y;
    ratio[(int64_t)m * ns + s] = zero ? make_double2(0.0, 0.0) : make_double2(mag * cos(ph), mag * sin(ph));
}

// v_k(sigma): the sign from the SAMPLED packed spins, the ratio from the term's row of the table (tmask < 0: diagonal term, ratio 1)
__device__ __forceinline__ double2 crnn_pauli_table_value(const uint32_t* bits, const uint32_t* sgn, const double2* ratio, int tmask, int W,
                                                          int64_t ns, int64_t s) {
    int odd = 0;                                   // parity of the number of sites of S with s_i = -1
    for (int w = 0; w < W; ++w) {
        const uint32_t sw = sgn[w];
        odd ^= __popc(sw) ^ __popc(bits[(int64_t)w * ns + s] & sw);
    }
    const double2 v = tmask >= 0 ? ratio[(int64_t)tmask * ns + s] : make_double2(1.0, 0.0);
    return (odd & 1) ? make_double2(-v.x, -v.y) : v;
}

// grid nterms * nblk (nblk = ceil(ns / 256)): block = (term k, 256 chains).  part [nterms][2][nblk][2], as crnn_pauli_term_kernel's
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_table_term_kernel(const uint32_t* bits, const uint32_t* sgn,
                                                                               const int32_t* tmask, const double2* ratio, int W,
                                                                               int64_t ns, int64_t nblk, double* part) {
    __shared__ double r1[kCPauliThreads], r2[kCPauliThreads], r3[kCPauliThreads], r4[kCPauliThreads];
    const int64_t k = blockIdx.x / nblk, b = blockIdx.x - k * nblk;
    const int64_t s = b * kCPauliThreads + threadIdx.x;
    const double2 v = s < ns ? crnn_pauli_table_value(bits, sgn + k * W, ratio, tmask[k], W, ns, s) : make_double2(0.0, 0.0);
    block_sum2(v.x, v.y, r1, r2);
    block_sum2(v.x * v.x, v.y * v.y, r3, r4);
    if (threadIdx.x == 0) {
        double* o = part + ((2 * k) * nblk + b) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
        o += nblk * 2;
        o[0] = r3[0];
        o[1] = r4[0];
    }
}

// grid ceil(ns / 256): thread = chain; the terms in the caller's order.  coeff [nterms] (re, im)
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_table_eloc_kernel(const uint32_t* bits, const uint32_t* sgn,
                                                                               const int32_t* tmask, const double2* coeff,
                                                                               const double2* ratio, int nterms, int W, int64_t ns,
                                                                               float2* eloc) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * kCPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < nterms; ++k) {
        const double2 v = crnn_pauli_table_value(bits, sgn + (int64_t)k * W, ratio, tmask[k], W, ns, s);
        const double2 c = coeff[k];
        re += c.x * v.x - c.y * v.y;
        im += c.x * v.y + c.y * v.x;
    }
    eloc[s] = make_float2((float)re, (float)im);
}

}  // namespace rnnwf
