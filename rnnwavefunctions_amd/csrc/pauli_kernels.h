// pauli_kernels.h - expectation values of Pauli strings and local energies of arbitrary real spin-1/2 Hamiltonians for the positive
// GRU RNN (docs/pauli.md).  A term is O = (prod_{i in S} sz_i)(prod_{i in F} sx_i); with s = 2 sigma - 1 and sigma ~ P = psi^2
//     v(sigma) = prod_{i in S} s_i * exp(1/2 [log P(sigma ^ F) - log P(sigma)]),   E[v] = <psi|O|psi>.
// sigma ^ F shares the sites 0..f-1 with sigma (f = first site of F), so
//     log P(sigma ^ F) - log P(sigma) = tail - suffix,   tail = sum_{n >= f} log p((sigma ^ F)_n | (sigma ^ F)_<n),
//                                                        suffix = sum_{n >= f} log p(sigma_n | sigma_<n).
//
//   prnn_flip_mask_kernel : tail of every chain and distinct flip mask - tile (mask, 16-chain block).  f >= 1: restores the chain's
//                           own hck[f-1], feeds its own spin f-1 and teacher-forces sites f..N-1 on own_word ^ mask_word (the region
//                           kernel of renyi_region_kernels.h with one spin word instead of two).  f = 0: starts as the base pass
//                           does, from the zero state and the zero input, and runs all N sites - no special case downstream, and
//                           the arithmetic of site 0 is the base pass's own.
//   pauli_log_ratio_kernel: 1/2 (tail - suffix) per (mask, chain); the suffix is prnn_site_terms_kernel's replayed terms added in
//                           the flip kernel's order (f >= 1) or the base pass's log P (f = 0, the same additions in the same order).
//   pauli_term_kernel     : v of every (term, chain): sign by popcount parity of spin word & sign word; per (term, 256 chains) the
//                           sums of v and v^2, reduced by renyi_sums_kernel in a fixed order (no atomics).
//   pauli_eloc_kernel     : E_loc(sigma) = sum_k coeff_k v_k(sigma), terms in the caller's order.
#pragma once
#include "renyi_kernels.h"

namespace rnnwf {

constexpr int kPauliThreads = kRenyiThreads;   // chains per block of the assembly kernels (renyi_sums_kernel reduces their partial sums)

struct FlipMaskArgs {
    const void* wimg;            // packed weight image (GruLayout)
    int32_t N;
    int32_t W;                   // ceil(N / 32): spin and mask words per chain / mask
    int64_t ns;                  // chains of this pass
    int64_t nsb;                 // ceil(ns / 16)
    const uint32_t* bits;        // [W][ns] packed spins
    const void* hck;             // [N-1][nsb][KT][64] T: the base pass's checkpoints
    const uint32_t* mask;        // [M][W]: bit n & 31 of word n >> 5 set = site n flipped; no mask is empty
    const int32_t* order;        // [M]: the masks longest chain first (f ascending, ties by index)
    const int32_t* first;        // [M]: f of every mask, 0 <= f <= N-1
    double* tail;                // [M][ns]
    int64_t ntiles;              // M * nsb
};

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_flip_mask_kernel(FlipMaskArgs a) {
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
        // the tile is the wave's: mask, first site and mask words live in scalar registers
        const int t = __builtin_amdgcn_readfirstlane((int)(tile / a.nsb));
        const int64_t sb = tile - (int64_t)t * a.nsb;
        const int m = a.order[t];
        const int f = a.first[m];                  // 0 <= f <= N-1
        const int64_t s = sb * kChains + c;
        const int64_t sc = s < a.ns ? s : a.ns - 1;
        const uint32_t* mrow = a.mask + (int64_t)m * a.W;
        // 32 sites of the flipped chain at once, the mask word the same for the whole wave.  Bit 0 of `word` is the next site's spin.
        auto flipped_word = [&](int w) { return a.bits[(int64_t)w * a.ns + sc] ^ mrow[w]; };
        // branch-free start (f is wave-uniform): f >= 1 restores hck[f-1] and feeds the own spin f-1 (no site below f is flipped);
        // f = 0 is the base pass's start, zero state and zero input - the load of hck[0] is then discarded
        const int g = f > 0 ? f - 1 : 0;
        T h[KT];
        {
            const T* src = reinterpret_cast<const T*>(a.hck) + (((int64_t)g * a.nsb + sb) * KT) * 64 + lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = f > 0 ? src[kt * 64] : T(0);
        }
        uint32_t word = flipped_word(g >> 5) >> (g & 31);
        int sig_in = f > 0 ? (int)(word & 1) : -1;
        double lp = 0.0;
        for (int n = f; n < N; ++n) {
            word = (n & 31) ? word >> 1 : flipped_word(n >> 5);
            const int sig = (int)(word & 1);
            C::template step<true>(img, sig_in, h, lane);
            T z[1];
            C::head(img, h, lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            lp += (double)(sig ? lp1 : lp0);
            sig_in = sig;
        }
        if (s < a.ns && q == 0) a.tail[(int64_t)m * a.ns + s] = lp;
    }
}

// grid (ceil(ns / 256), M): thread = chain, blockIdx.y = mask.  log_ratio [M][ns]
__global__ void __launch_bounds__(kPauliThreads) pauli_log_ratio_kernel(const double* tail, const double* terms, const double* logp,
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
__global__ void __launch_bounds__(kPauliThreads) pauli_term_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                  const double* log_ratio, int W, int64_t ns, int64_t nblk, double* part) {
    __shared__ double r1[kPauliThreads], r2[kPauliThreads];
    const int64_t k = blockIdx.x / nblk, b = blockIdx.x - k * nblk;
    const int64_t s = b * kPauliThreads + threadIdx.x;
    const double v = s < ns ? pauli_value(bits, sgn + k * W, log_ratio, tmask[k], W, ns, s) : 0.0;
    r1[threadIdx.x] = v;
    r2[threadIdx.x] = v * v;
    __syncthreads();
    for (int w = kPauliThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            r1[threadIdx.x] += r1[threadIdx.x + w];
            r2[threadIdx.x] += r2[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + (k * nblk + b) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
    }
}

// grid ceil(ns / 256): thread = chain; the terms in the caller's order
__global__ void __launch_bounds__(kPauliThreads) pauli_eloc_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                  const double* coeff, const double* log_ratio, int nterms, int W,
                                                                  int64_t ns, double* eloc) {
    const int64_t s = (int64_t)blockIdx.x * kPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double e = 0.0;
    for (int k = 0; k < nterms; ++k) e += coeff[k] * pauli_value(bits, sgn + (int64_t)k * W, log_ratio, tmask[k], W, ns, s);
    eloc[s] = e;
}

}  // namespace rnnwf
