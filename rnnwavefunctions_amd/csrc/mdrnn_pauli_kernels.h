// mdrnn_pauli_kernels.h - Pauli-string expectations and generic local energies for the 2D RNN (model MDRNN2D, float64) on the
// zig-zag path (docs/pauli_2d.md).  Everything here is in VISIT order: position p = ny Nx + j, column nx = j on even rows and
// Nx-1-j on odd rows; the host maps the caller's lattice-indexed masks before they arrive.
//
// For a flip mask F with first flipped position f, sigma' = sigma ^ F shares the positions < f with sigma, and the base pass's
// state after position p depends on the spins before p only.  So the states hs[0..f] are those of sigma' as well, and
//     log P(sigma') - log P(sigma) = tail - suffix,   tail   = sum_{p >= f} log p_p(sigma'_p | sigma'_<p),
//                                                     suffix = sum_{p >= f} log p_p(sigma_p  | sigma_<p).
//
//   mdrnn_site_terms_kernel : log p_p(sigma_p | sigma_<p) of every chain and position, the head replayed on the stored hs[p] - no
//                             cell step.  pauli_log_ratio_kernel (pauli_kernels.h) adds them from f on, in the tail's order.
//   mdrnn_masked_tail_kernel: the tail of every (distinct mask, 16-chain block): mdrnn_flip_kernel (mdrnn_kernels.h) with i := f,
//                             the spin words own ^ mask instead of one flipped bit, and position f's own term from head(hs[f]) at
//                             the flipped outcome.  States at positions <= f are the base pass's; EVERY position > f is
//                             recomputed and stored to its column slot, also where no flipped spin reaches it: the state above
//                             (nx, ny+1) is then always the last one written to column nx, whatever the mask.
//                             <..., PAIRED = true>: the same tail for the mixed chain of a replica pair (Renyi-2 of regions).
// The cell, the head and the state layout are MdCore's, unchanged.
#pragma once
#include "mdrnn_kernels.h"

namespace rnnwf {

struct MdPauliArgs {
    const void* wimg;
    int32_t N, Nx;
    int32_t rem;                   // num_units - 16 NFULL (1..4)
    int32_t W;                     // words per mask: ceil(N / 32)
    int64_t ns, nsb;
    const uint32_t* bits;          // [W][ns] spins in visit order
    const double* hs;              // [N][nsb][KP][64] double2: the base pass's states
    double* ring;                  // masked tails: [total waves][Nx][KP][64] double2, one private slot per lattice column
    double* terms;                 // [N][ns]: row p = log p_p(sigma_p | sigma_<p)
    const uint32_t* mask;          // [M][W] distinct non-empty flip masks (PAIRED: the normalised region masks), visit order
    const int32_t* order;          // [M] the masks f ascending (longest tail first), ties by index
    const int32_t* first;          // [M] first flipped position f, 0 <= f <= N-1
    double* tail;                  // [M][ns]
    int64_t ntiles;                // M * nsb
};

template <int NFULL, int WAVES>
__global__ void __launch_bounds__(WAVES * 64, NFULL <= 3 ? 2 : 1) mdrnn_site_terms_kernel(MdPauliArgs a) {
    using C = MdCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int64_t gw = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int N = a.N;
    for (int64_t sb = gw; sb < a.nsb; sb += nw) {
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        for (int p = 0; p < N; ++p) {
            double h[KT];
            C::load_state(a.hs + (((int64_t)p * a.nsb + sb) * C::KP) * 128 + 2 * lane, h);
            double lp0, lp1, p0;
            C::head(lds, h, lane, lp0, lp1, p0);
            if (valid && q == 0) a.terms[(int64_t)p * a.ns + s] = md_spin(a.bits, a.ns, sc, p) ? lp1 : lp0;
        }
    }
}

// PAIRED (mdrnn_renyi.hip, docs/renyi_2d.md): chains (2p, 2p + 1) are a replica pair and a masked position takes the PARTNER's spin
// instead of the flipped one - the mixed chain of the swap estimator.  The host normalises the masks so that position 0 is never
// masked (1 <= f <= N-1) and passes hold whole pairs (ns even).  Everything but the spin words is the same: hs[f] is the chain's own.
template <int NFULL, int WAVES, bool PAIRED = false>
__global__ void __launch_bounds__(WAVES * 64, NFULL <= 3 ? 2 : 1) mdrnn_masked_tail_kernel(MdPauliArgs a) {
    using C = MdCore<NFULL>;
    constexpr int KT = C::KT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    C::stage(lds, a.wimg);
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    // the wave index as a scalar: tile, mask and block bookkeeping then live in SGPRs (the 17..20-unit row needs its 128 VGPRs)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t gw = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int N = a.N;
    const int W = a.W;
    const int Nx = a.Nx;
    double* ring = a.ring + (int64_t)gw * Nx * C::KP * 128 + 2 * lane;
    uint32_t* words = reinterpret_cast<uint32_t*>(lds + C::L::BYTES) + wave * 8 * 64 + lane;
    for (int64_t tile = gw; tile < a.ntiles; tile += nw) {
        // mask, f and the mask words are the same for the whole wave
        const int64_t mo = tile / a.nsb;
        const int64_t sb = tile - mo * a.nsb;
        const int m = __builtin_amdgcn_readfirstlane(a.order[mo]);
        const int f = __builtin_amdgcn_readfirstlane(a.first[m]);
        const uint32_t* mw = a.mask + (int64_t)m * W;
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        // the changed configuration's spin words, [word][lane] in the wave's LDS slot (as mdrnn_flip_kernel).  PAIRED: ns is even,
        // so sc ^ 1 < ns also for the clamped lanes of a ragged block
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            uint32_t word = 0u;
            if (w < W) {
                const uint32_t own = a.bits[(int64_t)w * a.ns + sc];
                if constexpr (PAIRED)
                    word = (own & ~mw[w]) | (a.bits[(int64_t)w * a.ns + (sc ^ 1)] & mw[w]);
                else
                    word = own ^ mw[w];
            }
            words[w * 64] = word;
        }
        double hv[KT], hn[KT];
        C::load_state(a.hs + (((int64_t)f * a.nsb + sb) * C::KP) * 128 + 2 * lane, hn);   // state after position f: spins < f only
        // position f's own term at the flipped outcome: no step, f = 0 and f = N-1 included
        double lp;
        {
            double lp0, lp1, p0;
            C::head(lds, hn, lane, lp0, lp1, p0);
            lp = ((words[(f >> 5) * 64] >> (f & 31)) & 1) ? lp1 : lp0;
        }
        // positions f+1..N-1: mdrnn_flip_kernel's loop with i := f
        int ny = (f + 1) / Nx, j = (f + 1) - ny * Nx;
        auto bits_of = [&](int p, int jj, int nyy, int& sh, int& sv, int& so) {
            const int pv = nyy > 0 ? p - 2 * jj - 1 : -1;
            sh = jj == 0 ? -1 : (int)((words[((p - 1) >> 5) * 64] >> ((p - 1) & 31)) & 1);
            sv = pv >= 0 ? (int)((words[(pv >> 5) * 64] >> (pv & 31)) & 1) : -1;
            so = (int)((words[(p >> 5) * 64] >> (p & 31)) & 1);
        };
        int sig_h = -1, sig_v = -1, sig_o = 0;
        if (f + 1 < N) bits_of(f + 1, j, ny, sig_h, sig_v, sig_o);
        for (int p = f + 1; p < N; ++p) {
            const bool first = j == 0;
            const int pv = ny > 0 ? p - 2 * j - 1 : -1;
            const int nx = (ny & 1) ? Nx - 1 - j : j;
            // h_v operand: zero (first row), the state just computed (row turn), a base-pass state (pv <= f) or one this
            // chain produced (its column slot).  A row turn copies hn into hv before hn is cleared.
            if (pv < 0) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) hv[kt] = 0.0;
            } else if (pv == p - 1) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) hv[kt] = hn[kt];
            } else if (pv <= f) {
                C::load_state(a.hs + (((int64_t)pv * a.nsb + sb) * C::KP) * 128 + 2 * lane, hv);
            } else {
                C::load_state(ring + (int64_t)nx * C::KP * 128, hv);
            }
            if (first) {                           // no horizontal neighbour: uniform, once per row
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) hn[kt] = 0.0;
            }
            const int sh = sig_h, sv = sig_v, so = sig_o;
            int jn = j + 1, nyn = ny;
            if (jn == Nx) { jn = 0; ++nyn; }
            if (p + 1 < N) bits_of(p + 1, jn, nyn, sig_h, sig_v, sig_o);      // next step's bits, in flight during this one
            C::step(lds, sh, sv, hn, hv, hn, lane, a.rem);
            double lp0, lp1, p0;
            C::head(lds, hn, lane, lp0, lp1, p0);
            lp += so ? lp1 : lp0;
            // the last row has no vertical successor: nothing reads its states
            if (p < N - Nx) C::store_state(ring + (int64_t)nx * C::KP * 128, hn);
            j = jn; ny = nyn;
        }
        if (valid && q == 0) a.tail[(int64_t)m * a.ns + s] = lp;
    }
}

}  // namespace rnnwf
