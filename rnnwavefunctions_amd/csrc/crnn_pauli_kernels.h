// crnn_pauli_kernels.h - expectation values of Pauli strings and local energies of arbitrary spin-1/2 Hamiltonians for the complex
// RNN with the U(1) mask (model CRNN_U1, one layer; docs/pauli_complex.md).  A term is O = (prod_{i in S} sz_i)(prod_{i in F} sx_i);
// with s = 2 sigma - 1 and sigma ~ |psi|^2
//     v(sigma) = prod_{i in S} s_i * psi(sigma ^ F) / psi(sigma) = sign * exp(d.re) * (cos d.im + i sin d.im),   E[v] = <psi|O|psi>,
//     d = log psi(sigma ^ F) - log psi(sigma)   (complex, f64; the imaginary part is never reduced modulo 2 pi).
// log psi is the sum of crnn_site's terms (log-amplitude with the U(1) mask, phase).  sigma ^ F shares the sites 0..f-1 with sigma
// (f = first site of F), so d = tail - suffix over the sites n >= f, in both components.  A flipped configuration outside the
// zero-magnetisation sector has tail.re = -inf: its log-ratio is (-inf, 0) and its v exactly (0, 0); nothing forms inf - inf.
//
//   crnn_site_terms_kernel : the own (log-amplitude, phase) term of every chain and site 1..N-1, replayed from the checkpoints (site
//                            n's head reads hck[n]; the last site takes one step from hck[N-2]) - prnn_site_terms_kernel's shape.
//   crnn_masked_tail_kernel: tail of every chain and distinct flip mask - tile (mask, 16-chain block), prnn_masked_tail_kernel's
//                            shape (not PAIRED).  f >= 1: restores the chain's own hck[f-1], feeds its own spin f-1, counts the ups of
//                            its own sites below f and teacher-forces sites f..N-1 on own_word ^ mask_word.  f = 0: starts as the
//                            base pass does and runs all N sites.
//   crnn_pauli_log_ratio_kernel: tail - suffix per (mask, chain); the suffix is the replayed terms added in the tail kernel's order
//                            (f >= 1) or the base pass's total (f = 0, the same additions in the same order).
//   crnn_pauli_term_kernel : v of every (term, chain): sign by popcount parity of the SAMPLED spin word & sign word; per (term, 256
//                            chains) the sums of Re v, Im v and of their squares, reduced by renyi_sums_kernel in a fixed order.
//   crnn_pauli_eloc_kernel : E_loc(sigma) = sum_k coeff_k v_k(sigma), complex, f64, terms in the caller's order; rounded once to
//                            complex64.
#pragma once
#include "crnn_kernels.h"
#include "renyi_kernels.h"

namespace rnnwf {

constexpr int kCPauliThreads = kRenyiThreads;   // chains per block of the assembly kernels

struct CPauliArgs : ChainArgs {
    double2* terms;              // [N][ns]: row n = the own (log-amplitude, phase) term of site n (row 0 not written)
    const uint32_t* mask;        // [M][W]: bit n & 31 of word n >> 5 set = site n flipped; no mask empty
    const int32_t* order;        // [M]: the masks longest chain first (f ascending, ties by index)
    const int32_t* first;        // [M]: first flipped site f, 0 <= f <= N-1
    double2* tail;               // [M][ns]: sum over the sites n >= f of the flipped chain's terms
    int64_t ntiles;              // M * nsb
};

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) crnn_site_terms_kernel(CPauliArgs a) {
    using C = GruCore<float, NFULL, 3>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    const WaveTile<WAVES> w;
    const int N = a.N;
    for (int64_t sb = w.gw; sb < a.nsb; sb += w.nw) {
        const int64_t s = sb * kChains + w.c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        const float* ck = reinterpret_cast<const float*>(a.hck) + (sb * KT) * 64 + w.lane;      // + n nsb KT 64: hck[n]
        float h[KT];
        uint32_t word = a.bits[sc];                   // bit 0 = the spin of the site before the next term's
        int num_up = 0;                               // ups among the chain's own sites below the next term's
        auto term = [&](int n) {
            num_up += (int)(word & 1);
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc];
            float z[3];
            C::head(img, h, w.lane, z);
            float la0, la1, w0, ph0, ph1;
            crnn_site(z, n, N, num_up, la0, la1, w0, ph0, ph1);
            const int sig = (int)(word & 1);
            if (valid && w.q == 0) a.terms[(int64_t)n * a.ns + s] = make_double2((double)(sig ? la1 : la0), (double)(sig ? ph1 : ph0));
        };
        // one head for every site (a second inlined copy behind the loop costs the 260-unit row 224 bytes of scratch)
        for (int n = 1; n < N; ++n) {
            const int row = n < N - 1 ? n : N - 2;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = ck[((int64_t)row * a.nsb * KT + kt) * 64];
            if (n == N - 1) C::template step<true>(img, (int)(word & 1), h, w.lane);      // bit 0 = spin N-2
            term(n);
        }
    }
}

// Sites n0..N-1 teacher-forced from state h, input spin sig_in and num_up ups below n0: the f64 sums of the sites' log-amplitudes
// and phases (teacher_forced_tail for the complex cell; shared with crnn_paired_tail_kernel of crnn_renyi_kernels.h).  The base
// pass's step form (step<true>, bias last) and head.
template <class C, class NextSpin>
__device__ __forceinline__ double2 crnn_teacher_forced_tail(const char* img, float (&h)[C::KT], int sig_in, int num_up, int n0, int N, int lane,
                                                            NextSpin&& next_spin) {
    double re = 0.0, im = 0.0;
    for (int n = n0; n < N; ++n) {
        const int sig = next_spin(n);
        C::template step<true>(img, sig_in, h, lane);
        float z[3];
        C::head(img, h, lane, z);
        float la0, la1, w0, ph0, ph1;
        crnn_site(z, n, N, num_up, la0, la1, w0, ph0, ph1);
        re += (double)(sig ? la1 : la0);                     // -inf from the site where the count overshoots, and stays -inf
        im += (double)(sig ? ph1 : ph0);
        num_up += sig;
        sig_in = sig;
    }
    return make_double2(re, im);
}

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) crnn_masked_tail_kernel(CPauliArgs a) {
    using C = GruCore<float, NFULL, 3>;
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
        // branch-free start (f is wave-uniform): for f = 0 the load of hck[0] is discarded
        const int g = f > 0 ? f - 1 : 0;
        float h[KT];
        {
            const float* src = reinterpret_cast<const float*>(a.hck) + (((int64_t)g * a.nsb + sb) * KT) * 64 + w.lane;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) h[kt] = f > 0 ? src[kt * 64] : 0.0f;
        }
        // ups among the chain's own sites below f (none of them is flipped)
        int num_up = 0;
        for (int k = 0; k < (f >> 5); ++k) num_up += __popc(a.bits[(int64_t)k * a.ns + sc]);
        num_up += __popc(a.bits[(int64_t)(f >> 5) * a.ns + sc] & ((1u << (f & 31)) - 1u));
        // 32 sites of the flipped chain at once, the mask word the same for the whole wave.  Bit 0 of `word` is the next site's spin.
        uint32_t word = (a.bits[(int64_t)(g >> 5) * a.ns + sc] ^ mrow[g >> 5]) >> (g & 31);
        int sig_in = f > 0 ? (int)(word & 1) : -1;
        const double2 lpsi = crnn_teacher_forced_tail<C>(img, h, sig_in, num_up, f, N, w.lane, [&](int n) {
            word = (n & 31) ? word >> 1 : a.bits[(int64_t)(n >> 5) * a.ns + sc] ^ mrow[n >> 5];
            return (int)(word & 1);
        });
        if (s < a.ns && w.q == 0) a.tail[(int64_t)r * a.ns + s] = lpsi;
    }
}

// grid (ceil(ns / 256), M): thread = chain, blockIdx.y = mask.  log_ratio [M][ns]
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_log_ratio_kernel(const double2* tail, const double2* terms, const double2* tot,
                                                                              const int32_t* first, int N, int64_t ns, double2* log_ratio) {
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
    const bool out = t.x == -__builtin_inf();      // sigma ^ F is outside the sector: psi = 0 exactly
    log_ratio[(int64_t)m * ns + s] = out ? make_double2(-__builtin_inf(), 0.0) : make_double2(t.x - own.x, t.y - own.y);
}

// v_k(sigma): the sign from the SAMPLED packed spins, the ratio from the term's mask row (tmask < 0: diagonal term, ratio 1)
__device__ __forceinline__ double2 crnn_pauli_value(const uint32_t* bits, const uint32_t* sgn, const double2* log_ratio, int tmask, int W,
                                                    int64_t ns, int64_t s) {
    int odd = 0;                                   // parity of the number of sites of S with s_i = -1
    for (int w = 0; w < W; ++w) {
        const uint32_t sw = sgn[w];
        odd ^= __popc(sw) ^ __popc(bits[(int64_t)w * ns + s] & sw);
    }
    double2 v = make_double2(1.0, 0.0);
    if (tmask >= 0) {
        const double2 d = log_ratio[(int64_t)tmask * ns + s];
        const bool zero = d.x == -__builtin_inf();             // selected before the trigonometric functions: no 0 * inf
        const double mag = exp(zero ? 0.0 : d.x), ph = zero ? 0.0 : d.y;
        v = zero ? make_double2(0.0, 0.0) : make_double2(mag * cos(ph), mag * sin(ph));
    }
    return (odd & 1) ? make_double2(-v.x, -v.y) : v;
}

// grid nterms * nblk (nblk = ceil(ns / 256)): block = (term k, 256 chains).  part [nterms][2][nblk][2]: half 0 = the sums of (Re v,
// Im v), half 1 = of their squares - renyi_sums_kernel over 2 nterms rows then leaves {sum Re v, sum Im v, sum Re^2, sum Im^2} per term
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_term_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                         const double2* log_ratio, int W, int64_t ns, int64_t nblk,
                                                                         double* part) {
    __shared__ double r1[kCPauliThreads], r2[kCPauliThreads], r3[kCPauliThreads], r4[kCPauliThreads];
    const int64_t k = blockIdx.x / nblk, b = blockIdx.x - k * nblk;
    const int64_t s = b * kCPauliThreads + threadIdx.x;
    const double2 v = s < ns ? crnn_pauli_value(bits, sgn + k * W, log_ratio, tmask[k], W, ns, s) : make_double2(0.0, 0.0);
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
static __global__ void __launch_bounds__(kCPauliThreads) crnn_pauli_eloc_kernel(const uint32_t* bits, const uint32_t* sgn, const int32_t* tmask,
                                                                         const double2* coeff, const double2* log_ratio, int nterms, int W,
                                                                         int64_t ns, float2* eloc) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * kCPauliThreads + threadIdx.x;
    if (s >= ns) return;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < nterms; ++k) {
        const double2 v = crnn_pauli_value(bits, sgn + (int64_t)k * W, log_ratio, tmask[k], W, ns, s);
        const double2 c = coeff[k];
        re += c.x * v.x - c.y * v.y;
        im += c.x * v.y + c.y * v.x;
    }
    eloc[s] = make_float2((float)re, (float)im);
}

}  // namespace rnnwf
