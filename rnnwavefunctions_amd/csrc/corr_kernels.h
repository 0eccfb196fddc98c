// corr_kernels.h - two-point correlation functions of the positive GRU RNN: <sz_i>, <sz_i sz_j>, <sx_i>, <sx_i sx_j> for every
// site and pair in one call (docs/correlations.md).  psi = sqrt(P), samples sigma ~ P, s = 2 sigma - 1.
//
//     log r_i  = 1/2 [log P(sigma^(i))  - log P(sigma)]        <sx_i>      = E[r_i]
//     log r_ij = 1/2 [log P(sigma^(ij)) - log P(sigma)], i < j <sx_i sx_j> = E[r_ij]
// With t_n the base chain's log-probability of site n, t^(i)_n that of the chain with spin i flipped ("trunk i") and t^(ij)_n that
// of the chain with i and j flipped ("branch (i, j)") - the prefix 0..i-1 cancels and branch (i, j) shares sites i+1..j with trunk i:
//     log P(sigma^(ij)) - log P(sigma) = [t_i(1-s_i) - t_i(s_i)] + sum_{i<n<j} [t^(i)_n(s_n) - t_n(s_n)] + [t^(i)_j(1-s_j) - t_j(s_j)]
//                                      + sum_{n>j} [t^(ij)_n(s_n) - t_n(s_n)]
// Pair (i, n), i < n, has the lexicographic index pair_index(i, n, N) in 0 .. N(N-1)/2 - 1 everywhere below.
//
//   prnn_site_both_kernel : both outcomes of every site of the base chain, replayed from the base pass's checkpoints:
//                           bsel[n] = t_n(s_n), both[n] = t_n(1-s_n) - t_n(s_n)   (prnn_site_terms_kernel with both outcomes kept)
//   prnn_trunk_kernel     : tile (i, 16-chain block) as the flip pass: restore hck[i], feed 1-s_i, teacher-force i+1..N-1; at every
//                           site n the trunk state goes to tck[(i,n)][nsb][KT][64] (the checkpoint layout) and the site's two
//                           log-probabilities to tsel / toth.  N(N-1)/2 cell evaluations per chain.
//   prnn_branch_kernel    : tile (i, j, block), j <= N-2, longest first (j ascending): restore tck[(i,j)], feed 1-s_j, teacher-force
//                           j+1..N-1, tail[(i,j)] = sum_{n>j} t^(ij)_n(s_n).  N(N-1)(N-2)/6 cell evaluations per chain.
//   corr_suffix_kernel    : suf[j] = sum_{n>j} bsel[n], added from the last site down.
//   corr_assemble_kernel  : thread (chain, i): log r_i and log r_ij for every j > i, in f64, in the order written there.
//   corr_sums_kernel      : one block per row (site or pair): the sums over the chains, each thread a fixed stride, then a tree
//                           (no atomics: a repeated call is bit-identical).
//   corr_diag_kernel      : sum s_i s_j from the packed spins, in integers (exact).
// The four kernels from the suffix sums on read CorrArgs' arrays of doubles and the packed spins alone: lstm_corr.hip runs them
// behind the LSTM's recurrent kernels (lstm_corr_kernels.h), hence `inline`.
// Trunk and branch run the base pass's step form (step<true>, bias last) and head on states the base pass or the trunk stored, so
// what should cancel (zero weights; a branch whose flips do not reach the tail) cancels to rounding of the f64 sums only.
#pragma once
#include "chain_kernels.h"

namespace rnnwf {

constexpr int kCorrThreads = 256;

struct CorrArgs : ChainArgs {
    void* tck;                   // [N(N-1)/2][nsb][KT][64] T: trunk states, row pair_index(i, n) = trunk i after site n (n = N-1: unused)
    double* bsel;                // [N][ns]
    double* both;                // [N][ns]
    double* tsel;                // [N(N-1)/2][ns]: t^(i)_n(s_n)
    double* toth;                // [N(N-1)/2][ns]: t^(i)_n(1-s_n)
    double* tail;                // [N(N-1)/2][ns]: branch tails (rows with j = N-1: not written, not read)
    int64_t ntiles;              // trunk: (N-1) nsb; branch: (N-1)(N-2)/2 nsb
};

__host__ __device__ __forceinline__ int64_t pair_index(int i, int n, int N) {
    return (int64_t)i * (2 * N - i - 1) / 2 + (n - i - 1);
}

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_site_both_kernel(CorrArgs a) {
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
            const int sig = spin_of(a.bits, a.ns, sc, n);
            const double sel = (double)(sig ? lp1 : lp0), oth = (double)(sig ? lp0 : lp1);
            if (valid && w.q == 0) {
                a.bsel[(int64_t)n * a.ns + s] = sel;
                a.both[(int64_t)n * a.ns + s] = oth - sel;
            }
        };
        for (int n = 0; n < N - 1; ++n) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = ck[((int64_t)n * a.nsb * KT + kt) * 64];
            term(n);
        }
        // the last site's state is not checkpointed: one step from hck[N-2] (N = 1: from the zero state)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) h[kt] = N > 1 ? ck[((int64_t)(N - 2) * a.nsb * KT + kt) * 64] : T(0);
        C::template step<true>(img, N > 1 ? spin_of(a.bits, a.ns, sc, N - 2) : -1, h, w.lane);
        term(N - 1);
    }
}

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_trunk_kernel(CorrArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const WaveTile<WAVES> w;
    const int N = a.N;
    // tiles longest chain first (i ascending), every wave strides through them: each wave receives the same mix of lengths
    for (int64_t tile = w.gw; tile < a.ntiles; tile += w.nw) {
        const int i = (int)(tile / a.nsb);
        const int64_t sb = tile - (int64_t)i * a.nsb;
        const int64_t s = sb * kChains + w.c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        T h[KT];
        w.load_state(h, a.hck, i, a.nsb, sb, w.lane);
        int sig_in = 1 - spin_of(a.bits, a.ns, sc, i);      // the flipped spin feeds site i+1
        int64_t p = pair_index(i, i + 1, N);
        for (int n = i + 1; n < N; ++n, ++p) {
            const int sig = spin_of(a.bits, a.ns, sc, n);
            C::template step<true>(img, sig_in, h, w.lane);
            if (n < N - 1) {                                   // no branch starts at the last site
                T* dst = reinterpret_cast<T*>(a.tck) + ((p * a.nsb + sb) * KT) * 64 + w.lane;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) dst[kt * 64] = h[kt];
            }
            T z[1];
            C::head(img, h, w.lane, z);
            T lp0, lp1;
            log_softmax2(z[0], lp0, lp1);
            if (valid && w.q == 0) {
                a.tsel[p * a.ns + s] = (double)(sig ? lp1 : lp0);
                a.toth[p * a.ns + s] = (double)(sig ? lp0 : lp1);
            }
            sig_in = sig;
        }
    }
}

template <typename T, int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) prnn_branch_kernel(CorrArgs a) {
    using C = GruCore<T, NFULL, 1>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const WaveTile<WAVES> w;
    const int N = a.N;
    // tile = (j (j - 1) / 2 + i) nsb + block, 0 <= i < j <= N-2: longest tail first (j ascending), every wave strides through them
    for (int64_t tile = w.gw; tile < a.ntiles; tile += w.nw) {
        const int64_t m = tile / a.nsb;
        const int64_t sb = tile - m * a.nsb;
        int j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)m)) * 0.5f);
        while ((int64_t)j * (j - 1) / 2 > m) --j;
        while ((int64_t)(j + 1) * j / 2 <= m) ++j;
        const int i = (int)(m - (int64_t)j * (j - 1) / 2);
        const int64_t s = sb * kChains + w.c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        const int64_t p = pair_index(i, j, N);
        T h[KT];
        w.load_state(h, a.tck, p, a.nsb, sb, w.lane);
        // the second flipped spin feeds site j+1
        const double lp = teacher_forced_tail<C>(img, h, 1 - spin_of(a.bits, a.ns, sc, j), j + 1, N, w.lane,
                                                 [&](int n) { return spin_of(a.bits, a.ns, sc, n); });
        if (valid && w.q == 0) a.tail[p * a.ns + s] = lp;
    }
}

// suf [N][ns]: suf[j] = sum_{n>j} bsel[n], added from site N-1 down.  One thread per chain.
inline __global__ void __launch_bounds__(kCorrThreads) corr_suffix_kernel(const double* bsel, int N, int64_t ns, double* suf) {
    const int64_t s = (int64_t)blockIdx.x * kCorrThreads + threadIdx.x;
    if (s >= ns) return;
    double acc = 0.0;
    for (int j = N - 1; j >= 0; --j) {
        suf[(int64_t)j * ns + s] = acc;
        acc += bsel[(int64_t)j * ns + s];
    }
}

// grid (ceil(ns / 256), N): thread = chain, blockIdx.y = i.  lr [N + N(N-1)/2][ns]: rows 0..N-1 log r_i, row N + pair_index(i, j)
// log r_ij.  With x = both[i] and mid_j = sum_{i<n<j} (tsel[(i,n)] - bsel[n]), added with n ascending:
//     log r_ij = 1/2 (((x + mid_j) + (toth[(i,j)] - bsel[j])) + (tail[(i,j)] - suf[j]))       (j = N-1: no tail term)
//     log r_i  = 1/2 (x + mid_N)
inline __global__ void __launch_bounds__(kCorrThreads) corr_assemble_kernel(CorrArgs a, const double* suf, double* lr) {
    const int N = a.N, i = blockIdx.y;
    const int64_t ns = a.ns, s = (int64_t)blockIdx.x * kCorrThreads + threadIdx.x;
    if (s >= ns) return;
    const double x = a.both[(int64_t)i * ns + s];
    double mid = 0.0;
    int64_t p = pair_index(i, i + 1, N);
    for (int j = i + 1; j < N; ++j, ++p) {
        const double bj = a.bsel[(int64_t)j * ns + s];
        double v = (x + mid) + (a.toth[p * ns + s] - bj);
        if (j < N - 1) v += a.tail[p * ns + s] - suf[(int64_t)j * ns + s];
        lr[((int64_t)N + p) * ns + s] = 0.5 * v;
        mid += a.tsel[p * ns + s] - bj;
    }
    lr[(int64_t)i * ns + s] = 0.5 * (x + mid);
}

// one block per row of lr.  Row i < N: x_sums[i] = {sum r_i, sum r_i^2}.  Row N + pair_index(i, j): xx_sums[i][j] = {sum r_ij,
// sum r_ij^2, sum r_ij r_i, sum r_ij r_j, sum r_i r_j}.  Thread t adds chains t, t + 256, ... in that order, then a binary tree over
// the 256 threads.  exp of log r > 709 is +inf, and so are the sums it enters (docs/correlations.md).
inline __global__ void __launch_bounds__(kCorrThreads) corr_sums_kernel(const double* lr, int N, int64_t ns, double* x_sums, double* xx_sums) {
    __shared__ double red[5][kCorrThreads];
    const int64_t row = blockIdx.x;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int i = (int)row, j = -1;
    if (row >= N) {
        const int64_t p = row - N;
        i = 0;
        while (pair_index(i + 1, i + 2, N) <= p && i + 2 < N) ++i;      // first pair of trunk i+1 still <= p: p belongs to a later trunk
        j = (int)(p - pair_index(i, i + 1, N)) + i + 1;
    }
    for (int64_t s = threadIdx.x; s < ns; s += kCorrThreads) {
        if (j < 0) {
            const double r = exp(lr[row * ns + s]);
            acc[0] += r;
            acc[1] += r * r;
        } else {
            const double r = exp(lr[row * ns + s]), ri = exp(lr[(int64_t)i * ns + s]), rj = exp(lr[(int64_t)j * ns + s]);
            acc[0] += r;
            acc[1] += r * r;
            acc[2] += r * ri;
            acc[3] += r * rj;
            acc[4] += ri * rj;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = kCorrThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j < 0) {
            x_sums[2 * i] = red[0][0];
            x_sums[2 * i + 1] = red[1][0];
        } else {
            double* o = xx_sums + ((int64_t)i * N + j) * 5;
            for (int k = 0; k < 5; ++k) o[k] = red[k][0];
        }
    }
}

// grid (N, N): block (j, i), j >= i (the others return): zz[i][j] = zz[j][i] = sum_s s_i s_j = ns - 2 #{s: sigma_i != sigma_j}, and
// from the diagonal block z[i] = 2 #{s: sigma_i = 1} - ns.  Integer counts: exact, whatever the order.
inline __global__ void __launch_bounds__(kCorrThreads) corr_diag_kernel(const uint32_t* bits, int N, int64_t ns, double* z, double* zz) {
    __shared__ long long red[kCorrThreads];
    const int j = blockIdx.x, i = blockIdx.y;
    if (j < i) return;
    long long cnt = 0;
    for (int64_t s = threadIdx.x; s < ns; s += kCorrThreads) {
        const int si = spin_of(bits, ns, s, i);
        cnt += (i == j) ? si : (si ^ spin_of(bits, ns, s, j));
    }
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = kCorrThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (i == j) {
            z[i] = (double)(2 * red[0] - (long long)ns);
            zz[(int64_t)i * N + i] = (double)ns;
        } else {
            const double v = (double)((long long)ns - 2 * red[0]);
            zz[(int64_t)i * N + j] = v;
            zz[(int64_t)j * N + i] = v;
        }
    }
}

}  // namespace rnnwf
