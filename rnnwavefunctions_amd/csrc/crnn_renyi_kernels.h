// crnn_renyi_kernels.h - the second Renyi entropy of arbitrary regions for the complex RNN with the U(1) mask (model CRNN_U1, one
// layer; docs/renyi_complex.md), by the replica swap trick on pairs (sigma, tau) = chains (2p, 2p + 1):
//     log r_A = (tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)   (complex, f64; no factor 1/2: log psi carries it already)
//     r = exp(re) (cos im, sin im),   exp(-S2(A)) = E[Re r],   E[Im r] = 0.
// tail_s is the sum of crnn_site's terms over the sites n >= f of the mixed chain (own & ~A) | (partner & A), f the first site of A
// (the host normalises the masks to site 0 not in A), suffix_s the same sum of the chain's own terms.  Both chains lie in the
// zero-magnetisation sector, so the two mixed chains do iff popcount(sigma & A) = popcount(tau & A); otherwise r = 0 exactly.  That
// is known from the packed spins before any cell is evaluated: only the surviving pairs are evaluated, compacted into full
// 16-chain tiles.
//
//   crnn_survivor_list_kernel: per region, the surviving chains in ascending order (ballot + fixed-order block scan, no atomics).
//   crnn_tile_scan_kernel    : tile_begin[t] of the regions in the host's order (longest mixed chain first); the tile count stays
//                              on the device.  Survivor and tile counts per region as f64 beside the sums.
//   crnn_paired_tail_kernel  : tile = 16 surviving chains of one region.  Lane (c, q) gathers its chain's own hck[f-1] from that
//                              chain's block, feeds its own spin f-1, counts the ups of its own sites below f and teacher-forces
//                              the sites f..N-1 of the mixed chain (crnn_teacher_forced_tail: crnn_masked_tail_kernel's site loop).
//   crnn_renyi_log_ratio_kernel: log r per (region, pair); (-inf, 0) for a pair outside the sector without reading a tail.
//   crnn_renyi_value_kernel  : r, selected on -inf before exp / cos / sin; per (region, 256 pairs) the sums of Re r, Im r and their
//                              squares, reduced by renyi_sums_kernel in a fixed order.
#pragma once
#include "crnn_pauli_kernels.h"

namespace rnnwf {

constexpr int kCRenyiThreads = kRenyiThreads;   // pairs per block of the list and assembly kernels

struct CRenyiArgs : ChainArgs {  // ns = 2 x pairs
    const uint32_t* mask;        // [R][W]: bit n & 31 of word n >> 5 set = site n in A (normalised: site 0 never)
    const int32_t* order;        // [nact]: the non-empty regions, longest mixed chain first (f ascending, ties by index)
    const int32_t* first;        // [R]: first site f of A, 0 = empty region
    int32_t nact;
    int32_t* surv;               // [nact][ns]: row t = the surviving chains of region order[t], ascending
    int32_t* cnt;                // [nact]: their number (even)
    int32_t* tile_begin;         // [nact + 1]: first tile of region order[t]; [nact] = the tile count
    double2* tail;               // [R][ns]: tail of chain s under region r (survivors only)
};

// pair p of region row mrow survives: both mixed chains lie in the sector
__device__ __forceinline__ bool crnn_pair_survives(const uint32_t* bits, const uint32_t* mrow, int W, int64_t ns, int64_t p) {
    int d = 0;
    for (int k = 0; k < W; ++k) {
        const uint32_t m = mrow[k];
        d += __popc(bits[(int64_t)k * ns + 2 * p] & m) - __popc(bits[(int64_t)k * ns + 2 * p + 1] & m);
    }
    return d == 0;
}

// grid nact: block t lists the survivors of region order[t], 256 pairs at a time; ranks by wave ballot, wave offsets in wave order
static __global__ void __launch_bounds__(kCRenyiThreads) crnn_survivor_list_kernel(CRenyiArgs a) {
    __shared__ int wsum[kCRenyiThreads / 64];
    const int t = blockIdx.x;
    const uint32_t* mrow = a.mask + (int64_t)a.order[t] * a.W;
    int32_t* row = a.surv + (int64_t)t * a.ns;
    const int64_t np = a.ns / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;                                  // surviving pairs so far, the same in every thread
    for (int64_t p0 = 0; p0 < np; p0 += kCRenyiThreads) {
        const int64_t p = p0 + threadIdx.x;
        const bool sv = p < np && crnn_pair_survives(a.bits, mrow, a.W, a.ns, p);
        const unsigned long long ball = __ballot(sv);
        if (lane == 0) wsum[wv] = __popcll(ball);
        __syncthreads();
        int off = base, all = 0;
        for (int i = 0; i < kCRenyiThreads / 64; ++i) {
            off += i < wv ? wsum[i] : 0;
            all += wsum[i];
        }
        if (sv) {
            const int at = 2 * (off + __popcll(ball & ((1ull << lane) - 1ull)));
            row[at] = (int32_t)(2 * p);
            row[at + 1] = (int32_t)(2 * p + 1);
        }
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.cnt[t] = 2 * base;
}

// one block: tile_begin = exclusive prefix of ceil(cnt / 16) over the regions in the host's order.  counts [2][R] f64: row 0 the
// surviving pairs, row 1 the tiles of every region (0 for an empty region: the host knows those)
static __global__ void __launch_bounds__(kCRenyiThreads) crnn_tile_scan_kernel(CRenyiArgs a, int R, double* counts) {
    __shared__ int part[kCRenyiThreads];
    for (int r = threadIdx.x; r < R; r += kCRenyiThreads)
        if (a.first[r] == 0) counts[r] = counts[R + r] = 0.0;
    const int per = (a.nact + kCRenyiThreads - 1) / kCRenyiThreads;
    const int t0 = min((int)threadIdx.x * per, (int)a.nact), t1 = min(t0 + per, (int)a.nact);
    int mine = 0;
    for (int t = t0; t < t1; ++t) mine += (a.cnt[t] + kChains - 1) / kChains;
    part[threadIdx.x] = mine;
    __syncthreads();
    int at = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) at += part[i];
    for (int t = t0; t < t1; ++t) {
        const int c = a.cnt[t], nt = (c + kChains - 1) / kChains, r = a.order[t];
        a.tile_begin[t] = at;
        counts[r] = (double)(c / 2);
        counts[R + r] = (double)nt;
        at += nt;
    }
    if (threadIdx.x == kCRenyiThreads - 1) a.tile_begin[a.nact] = at;      // the last thread's end is the total
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) crnn_paired_tail_kernel(CRenyiArgs a) {
    using C = GruCore<float, NFULL, 3>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);       // LDS, or the global image where it exceeds LDS (GruLayout::SPILL)
    const WaveTile<WAVES> w;
    const int N = a.N;
    const int ntiles = a.tile_begin[a.nact];       // written by crnn_tile_scan_kernel in front of this launch: no host round trip
    // tiles longest chain first (the host's region order), every wave strides through them
    for (int64_t tl = w.gw; tl < ntiles; tl += w.nw) {
        // the tile is the wave's: region, first site and mask words live in scalar registers
        const int tile = __builtin_amdgcn_readfirstlane((int)tl);
        int lo = 0, hi = a.nact;                   // tile_begin[lo] <= tile < tile_begin[hi]; empty regions have no tile
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.tile_begin[mid] <= tile) lo = mid; else hi = mid;
        }
        const int t = __builtin_amdgcn_readfirstlane(lo);
        const int r = a.order[t];
        const int f = a.first[r];                  // >= 1
        const int nsv = a.cnt[t];                  // >= 1: the region has a tile
        const int j = (tile - a.tile_begin[t]) * kChains + w.c;
        const bool live = j < nsv;                 // lanes beyond the last survivor repeat it and store nothing
        // (a 32-bit chain index: scalar row base + lane offset addressing, and one register less than the masked-tail kernel's int64)
        const uint32_t s = (uint32_t)a.surv[(int64_t)t * a.ns + (live ? j : nsv - 1)];
        const uint32_t* mrow = a.mask + (int64_t)r * a.W;
        // the chain's own hck[f-1], from its own block: once per tile, against N - f steps
        float h[KT];
        {
            const float* src = reinterpret_cast<const float*>(a.hck) + ((int64_t)(f - 1) * a.nsb * KT) * 64;
            const uint32_t at = (s >> 4) * (uint32_t)(KT * 64) + ((uint32_t)(w.q << 4) | (s & 15u));
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = src[at + (uint32_t)(kt * 64)];
        }
        // ups among the chain's own sites below f (none of them is in A)
        int num_up = 0;
        for (int k = 0; k < (f >> 5); ++k) num_up += __popc((a.bits + (int64_t)k * a.ns)[s]);
        num_up += __popc((a.bits + (int64_t)(f >> 5) * a.ns)[s] & ((1u << (f & 31)) - 1u));
        // 32 sites of the mixed chain at once (ns is even: the partner s ^ 1 is a chain of the pass)
        auto mixed_word = [&](int k) {
            const uint32_t m = mrow[k];
            const uint32_t* brow = a.bits + (int64_t)k * a.ns;
            return (brow[s] & ~m) | (brow[s ^ 1u] & m);
        };
        uint32_t word = mixed_word((f - 1) >> 5) >> ((f - 1) & 31);      // bit 0 = the own spin f-1
        const double2 lpsi = crnn_teacher_forced_tail<C>(img, h, (int)(word & 1), num_up, f, N, w.lane, [&](int n) {
            word = (n & 31) ? word >> 1 : mixed_word(n >> 5);
            return (int)(word & 1);
        });
        if (live && w.q == 0) (a.tail + (int64_t)r * a.ns)[s] = lpsi;
    }
}

// grid (ceil(npairs / 256), R): thread = pair, blockIdx.y = region.  log_ratio [R][npairs]
static __global__ void __launch_bounds__(kCRenyiThreads) crnn_renyi_log_ratio_kernel(CRenyiArgs a, const double2* terms, double2* log_ratio) {
    const int r = blockIdx.y;
    const int f = a.first[r];
    const int64_t np = a.ns / 2, p = (int64_t)blockIdx.x * kCRenyiThreads + threadIdx.x;
    if (p >= np) return;
    double2 lr = make_double2(0.0, 0.0);           // empty region: no swap, r = 1
    if (f > 0) {
        lr = make_double2(-__builtin_inf(), 0.0);  // a mixed chain outside the sector: psi = 0 exactly, no tail was computed
        if (crnn_pair_survives(a.bits, a.mask + (int64_t)r * a.W, a.W, a.ns, p)) {
            double2 sa = make_double2(0.0, 0.0), sb = sa;      // own suffixes, summed in the tail kernel's order
            for (int n = f; n < a.N; ++n) {
                const double2 ta = terms[(int64_t)n * a.ns + 2 * p], tb = terms[(int64_t)n * a.ns + 2 * p + 1];
                sa.x += ta.x;
                sa.y += ta.y;
                sb.x += tb.x;
                sb.y += tb.y;
            }
            const double2 ta = a.tail[(int64_t)r * a.ns + 2 * p], tb = a.tail[(int64_t)r * a.ns + 2 * p + 1];
            lr = make_double2((ta.x - sa.x) + (tb.x - sb.x), (ta.y - sa.y) + (tb.y - sb.y));
        }
    }
    log_ratio[(int64_t)r * np + p] = lr;
}

// grid (nblk, R), nblk = ceil(npairs / 256): block = (256 pairs, region).  part [R][2][nblk][2]: half 0 = the sums of (Re r, Im r),
// half 1 = of their squares - renyi_sums_kernel over 2 R rows then leaves {sum Re r, sum Im r, sum Re^2, sum Im^2} per region
static __global__ void __launch_bounds__(kCRenyiThreads) crnn_renyi_value_kernel(const double2* log_ratio, int64_t np, double* part) {
    __shared__ double r1[kCRenyiThreads], r2[kCRenyiThreads], r3[kCRenyiThreads], r4[kCRenyiThreads];
    const int64_t r = blockIdx.y, nblk = gridDim.x, p = (int64_t)blockIdx.x * kCRenyiThreads + threadIdx.x;
    double2 v = make_double2(0.0, 0.0);
    if (p < np) {
        const double2 d = log_ratio[r * np + p];
        const bool zero = d.x == -__builtin_inf();             // selected before the trigonometric functions: no 0 * inf
        const double mag = exp(zero ? 0.0 : d.x), ph = zero ? 0.0 : d.y;
        v = zero ? make_double2(0.0, 0.0) : make_double2(mag * cos(ph), mag * sin(ph));
    }
    block_sum2(v.x, v.y, r1, r2);
    block_sum2(v.x * v.x, v.y * v.y, r3, r4);
    if (threadIdx.x == 0) {
        double* o = part + ((2 * r) * nblk + blockIdx.x) * 2;
        o[0] = r1[0];
        o[1] = r2[0];
        o += nblk * 2;
        o[0] = r3[0];
        o[1] = r4[0];
    }
}

}  // namespace rnnwf
