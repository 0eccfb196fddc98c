// chain_kernels.h - what the kernels of the four observable passes share (renyi_kernels.h, renyi_region_kernels.h, corr_kernels.h,
// pauli_kernels.h): all of them restart one-layer GRU chains from the base pass's checkpoints and teacher-force them to the last site.
//
//   ChainArgs               : the arguments every such kernel takes - weight image, packed spins, checkpoints (observable.h fills them)
//   spin_of                 : one spin of the packed bits
//   WaveTile                : a wave's place in the launch (one 16-chain tile per wave at a time) and its restart from a stored state
//   teacher_forced_tail     : the site loop of the swap, masked and branch kernels
//   block_sum2              : the 256-thread tree of the assembly kernels
//   prnn_masked_tail_kernel : the tails of chains changed under a site mask - swapped with the partner (Renyi-2 of regions) or flipped
//                             (Pauli strings)
#pragma once
#include "gru_core.h"

namespace rnnwf {

constexpr int kSumThreads = 256;     // threads per block of every kernel that reduces with block_sum2

struct ChainArgs {
    const void* wimg;            // packed weight image (GruLayout)
    int32_t N;
    int32_t W;                   // ceil(N / 32): spin (and mask) words per chain
    int64_t ns;                  // chains of this pass
    int64_t nsb;                 // ceil(ns / 16)
    const uint32_t* bits;        // [W][ns] packed spins
    const void* hck;             // [N-1][nsb][KT][64] T: the base pass's checkpoints
};

__device__ __forceinline__ int spin_of(const uint32_t* bits, int64_t ns, int64_t s, int n) {
    return (int)((bits[(int64_t)(n >> 5) * ns + s] >> (n & 31)) & 1);
}

// Lane (chain c = lane & 15 of the tile, quarter q), global wave index and wave count of a launch of WAVES waves per workgroup
template <int WAVES>
struct WaveTile {
    const int lane, c, q;
    const int64_t gw, nw;
    __device__ __forceinline__ WaveTile()
        : lane(threadIdx.x & 63), c(lane & 15), q(lane >> 4), gw((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)),
          nw((int64_t)gridDim.x * WAVES) {}
    // h <- row `row` of a [rows][nsb][KT][64] state array (the checkpoint layout), 16-chain block sb; from_lane = lane for the
    // chain's own state, lane ^ 1 for its pair partner's
    template <typename T, int KT>
    static __device__ __forceinline__ void load_state(T (&h)[KT], const void* base, int64_t row, int64_t nsb, int64_t sb, int from_lane) {
        const T* src = reinterpret_cast<const T*>(base) + ((row * nsb + sb) * KT) * 64 + from_lane;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = src[kt * 64];
    }
};

// Sites n0..N-1 teacher-forced from state h and input spin sig_in: the sum of log p(next_spin(n) | ...) in f64.  The base pass's step
// form (step<true>, bias last) and head, so that what should cancel against the base pass's own terms cancels exactly.
template <class C, typename T, class NextSpin>
__device__ __forceinline__ double teacher_forced_tail(const char* img, T (&h)[C::KT], int sig_in, int n0, int N, int lane,
                                                      NextSpin&& next_spin) {
    double lp = 0.0;
    for (int n = n0; n < N; ++n) {
        const int sig = next_spin(n);
        C::template step<true>(img, sig_in, h, lane);
        T z[1];
        C::head(img, h, lane, z);
        T lp0, lp1;
        log_softmax2(z[0], lp0, lp1);
        lp += (double)(sig ? lp1 : lp0);
        sig_in = sig;
    }
    return lp;
}

// r1[0], r2[0] <- the sums of v and v2 over the block's kSumThreads threads, a binary tree in a fixed order (no atomics: a repeated
// call is bit-identical); thread 0 reads them
__device__ __forceinline__ void block_sum2(double v, double v2, double* r1, double* r2) {
    r1[threadIdx.x] = v;
    r2[threadIdx.x] = v2;
    __syncthreads();
    for (int w = kSumThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            r1[threadIdx.x] += r1[threadIdx.x + w];
            r2[threadIdx.x] += r2[threadIdx.x + w];
        }
        __syncthreads();
    }
}

struct MaskArgs : ChainArgs {
    const uint32_t* mask;        // [rows][W]: bit n & 31 of word n >> 5 set = site n swapped / flipped
    const int32_t* order;        // [ntiles / nsb]: the rows that have a tail, longest chain first (f ascending, ties by index)
    const int32_t* first;        // [rows]: first masked site f of every row
    double* tail;                // [rows][ns]: row r = tail_s under mask r (rows without a tile are not written)
    int64_t ntiles;              // rows in `order` * nsb
};

// tail_s of every chain s and mask row: the log-probability of sites f..N-1 of the chain changed under the mask, f the mask's first
// site.  Tile (row, 16-chain block).
//   PAIRED  (renyi_region_kernels.h): chains (2p, 2p + 1) are a pair, a masked site takes the partner's spin.  The host normalises
//           the masks so that site 0 is never masked: 1 <= f <= N-1, and rows that are empty after that have no tile.
//   !PAIRED (pauli_kernels.h): a masked site is flipped.  No mask is empty, 0 <= f <= N-1.
// f >= 1 restores the chain's OWN hck[f-1] and feeds its own spin f-1 (no site below f is changed).  f = 0 starts as the base pass
// does, from the zero state and the zero input, and runs all N sites - no special case downstream, and the arithmetic of site 0 is
// the base pass's own.
template <typename T, int NFULL, int WAVES, bool PAIRED>
__global__ void __launch_bounds__(WAVES * 64) prnn_masked_tail_kernel(MaskArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);       // LDS, or the global image where it exceeds LDS (GruLayout::SPILL)
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
                const uint32_t m = mrow[k];
                const uint32_t own = a.bits[(int64_t)k * a.ns + sc], par = a.bits[(int64_t)k * a.ns + (sc ^ 1)];
                return (own & ~m) | (par & m);
            } else {
                return a.bits[(int64_t)k * a.ns + sc] ^ mrow[k];
            }
        };
        T h[KT];
        uint32_t word;
        int sig_in;
        if constexpr (PAIRED) {
            w.load_state(h, a.hck, f - 1, a.nsb, sb, w.lane);
            word = changed_word((f - 1) >> 5) >> ((f - 1) & 31);
            sig_in = (int)(word & 1);
        } else {
            // branch-free start (f is wave-uniform): for f = 0 the load of hck[0] is discarded
            const int g = f > 0 ? f - 1 : 0;
            const T* src = reinterpret_cast<const T*>(a.hck) + (((int64_t)g * a.nsb + sb) * KT) * 64 + w.lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = f > 0 ? src[kt * 64] : T(0);
            word = changed_word(g >> 5) >> (g & 31);
            sig_in = f > 0 ? (int)(word & 1) : -1;
        }
        const double lp = teacher_forced_tail<C>(img, h, sig_in, f, N, w.lane, [&](int n) {
            word = (n & 31) ? word >> 1 : changed_word(n >> 5);
            return (int)(word & 1);
        });
        if (s < a.ns && w.q == 0) a.tail[(int64_t)r * a.ns + s] = lp;
    }
}

}  // namespace rnnwf
