// sr_kernels.h - kernels of stochastic reconfiguration (docs/sr.md) on the per-sample log-derivative matrix
//
//   J[ns][D],  D = PCOLS QCOLS + HEAD_ROW:  row s = O_s = d log psi(sigma_s) / d theta = 1/2 d log P / d theta  in IMAGE order, the
//   order of the gradient image h->gradW ([dW | head row], grad.hip), element type of the model.
//   Complex RNN (docs/sr_complex.md): J[2 ns][D_c], D_c = PCOLS QCOLS + 3 HEAD_ROW, row s = Re O_s, row ns + s = Im O_s; the rows
//   [0, ns) and [ns, 2 ns) are centred with their own column means (HALVES).
//   2D RNN (docs/sr_2d.md): J[ns][D_2], D_2 = PCOLS QCOLS + 2 HEAD_ROW of MdGradLayout, from the rows mdrnn_bwd_kernel<SR> left.
//   LSTM (docs/sr_lstm.md): J[ns][D_l], D_l = PCOLS QCOLS + HEAD_ROW of LstmGradLayout, from the rows lstm_bwd_kernel<SR> left.
//
//   sr_outer_kernel  : O_s = 1/2 sum_n p_{n ns + s} (x) q_{n ns + s} from the rows gru_bwd_kernel<SR> left in P and Q (unit weights),
//                      plus 1/2 of the sample's head row; image elements that no parameter reads (padding) are written as zeros.
//   sr_colsum_kernel : out[k] = scale sum_s w_s J[s][k] in f64 - the column mean (w = 1, scale = 1 / ns) and J^T y.
//   sr_gram_kernel   : (J - mean) M (J - mean)^T (M: the parameters per image element) in f64 on the f64 MFMA, operands converted and centred on the fly; the lower triangle is
//                      computed and mirrored.
// Every sum has a fixed order (no atomics): the same batch gives the same bits.
#pragma once
#include "grad_kernels.h"
#include "lstm_grad_kernels.h"
#include "mdrnn_grad_kernels.h"

namespace rnnwf {

// One workgroup per sample; the P tiles go round the waves (14 x 4 tiles at 50 units would be 224 accumulator registers in one wave)
// and the Q tiles are taken QCH at a time so that a pass holds at most 64 accumulator registers - the N rows of P are read again per
// pass, from L2.
// The tiles of a gradient image G (GradLayout, or MdGradLayout of the 2D RNN: P and Q of different widths, two head rows) over the
// WAVES = WP x WQ waves of a workgroup: wave w owns the P tiles wp, wp + WP, ... (wp = w mod WP) and the QW consecutive Q tiles from
// wq QW on (wq = w / WP), taken QCH at a time.  WQ = 1: every wave owns every Q tile.  HALF: the rows carry d log P, O = 1/2 of them.
template <typename T, class G_, int NOUT_, int WAVES_, int WQ_, bool HALF_>
struct SrTiles {
    using Elem = T;
    using G = G_;
    static constexpr int NOUT = NOUT_;                     // head rows: 1, 3 (complex RNN) or 2 (2D RNN)
    static constexpr bool HALF = HALF_;
    static constexpr int PT = G::PCOLS / 16, QT = G::QCOLS / 16;
    static constexpr int FRAG_REGS = 4 * (int)sizeof(T) / 4;
    static constexpr int WAVES = WAVES_, WQ = WQ_, WP = WAVES / WQ;
    static constexpr int MP = (PT + WP - 1) / WP;
    static constexpr int QW = (QT + WQ - 1) / WQ;
    static constexpr int QCH = 64 / (MP * FRAG_REGS) < 1 ? 1 : 64 / (MP * FRAG_REGS) > QW ? QW : 64 / (MP * FRAG_REGS);
    static constexpr int PASSES = (QW + QCH - 1) / QCH;
    static constexpr int64_t DW0 = (int64_t)G::PCOLS * G::QCOLS;
    static constexpr int64_t D = DW0 + NOUT * G::HEAD_ROW;
    static_assert(WP * WQ == WAVES && WP <= PT && (WQ - 1) * QW < QT, "every wave owns a tile");
    static_assert(MP * QCH * FRAG_REGS <= 64 || QCH == 1, "at most 64 accumulator registers per pass");
    static_assert(NOUT * G::HEAD_ROW <= WAVES * 64, "one thread per head element");
};

// The GRU families: 8 waves where 4 would own more than 112 registers of full rows of tiles; no split of the Q tiles.
template <typename T, int NFULL>
constexpr int kSrGruWaves = ((GradLayout<NFULL, T>::PCOLS / 16 + 3) / 4) * (GradLayout<NFULL, T>::QCOLS / 16) * (4 * (int)sizeof(T) / 4) > 112 ? 8 : 4;
template <typename T, int NFULL, int NOUT_ = 1>            // NOUT 3: the complex RNN's three head rows, which carry their 1/2 already
struct SrShape : SrTiles<T, GradLayout<NFULL, T>, NOUT_, kSrGruWaves<T, NFULL>, 1, NOUT_ == 1> {
    static constexpr int NF = NFULL;
};
// The 2D RNN (docs/sr_2d.md): NT x 2 NT tiles of 8 registers.  Two rows of waves share the P tiles, the Q tiles are split over
// two (up to 52 units) or four (53..84 units: eight waves) columns of waves.
template <int NFULL>
struct MdSrShape : SrTiles<double, MdGradLayout<NFULL>, 2, NFULL <= 3 ? 4 : 8, NFULL <= 3 ? 2 : 4, true> {
    static constexpr int NF = NFULL;
};

// The LSTM (docs/sr_lstm.md): (4 NFULL + 1) x (NFULL + 1) tiles of 8 registers, a P-heavy image - the P tiles go round four (up to 20
// units) or eight waves and no wave splits the Q tiles: 2 x 2, 2 x 3 and 2 x 4 tiles per wave in one pass, 3 x 5 in three passes of
// 2, 2 and 1 Q tiles at 53..68 units.
template <int NFULL>
struct LstmSrShape : SrTiles<double, LstmGradLayout<NFULL>, 1, NFULL == 1 ? 4 : 8, 1, true> {
    static constexpr int NF = NFULL;
};

// K = N is short: the last group of four sites is padded with zeros (its rows are read from site 0 and zeroed), no branch.
// NOUT = 3 (complex RNN): P holds the rows of one seed of gru_bwd_kernel<SR>, which already carry the 1/2 of log a = 1/2 log p
// (no factor here), head its three head rows, J the first row of that seed's half.
template <class S>
__global__ void __launch_bounds__((S::WAVES * 64)) sr_outer_kernel(const typename S::Elem* __restrict__ P, const typename S::Elem* __restrict__ Q,
                                                                 const typename S::Elem* __restrict__ head, const uint8_t* __restrict__ used,
                                                                 int N, int64_t ns, typename S::Elem* __restrict__ J) {
    using T = typename S::Elem;
    constexpr int NOUT = S::NOUT;
    const T scale = S::HALF ? T(0.5) : T(1);
    using G = typename S::G;
    using V4 = typename Frag<T>::V4;
    constexpr int PT = S::PT, MP = S::MP, WP = S::WP, QCH = S::QCH, QW = S::QW;
    constexpr bool SPLIT = S::WQ > 1;                      // the Q tiles are split over columns of waves
    const int lane = threadIdx.x & 63;
    const int wid = SPLIT ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;      // SPLIT: in a scalar register
    const int wave = SPLIT ? wid % WP : wid;
    // this wave's Q tiles are q0 .. q0 + qn - 1; the last column of waves may own fewer than QW: it skips a pass without a tile of
    // its own (a branch the whole wave takes) and multiplies its last tile again for the missing tiles of a pass it has one in
    const int q0 = SPLIT ? (wid / WP) * QW : 0;
    const int qn = SPLIT ? (S::QT - q0 < QW ? S::QT - q0 : QW) : QW;
    const int li = lane & 15, lk = lane >> 4;
    const int kgroups = (N + 3) / 4;
    for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
        T* out = J + s * S::D;
#pragma unroll
        for (int pass = 0; pass < S::PASSES; ++pass) {
            const int t0 = pass * QCH;
            if (SPLIT && t0 >= qn) continue;
            V4 acc[MP][QCH];
#pragma unroll
            for (int i = 0; i < MP; ++i)
#pragma unroll
                for (int t = 0; t < QCH; ++t) acc[i][t] = V4{T(0), T(0), T(0), T(0)};
            for (int kg = 0; kg < kgroups; ++kg) {
                const int n = 4 * kg + lk;
                const bool ok = n < N;
                const int64_t row = (int64_t)(ok ? n : 0) * ns + s;
                const T* prow = P + row * G::PCOLS + li;
                const T* qrow = Q + row * G::QCOLS + 16 * q0 + li;
                T qv[QCH], pv[MP];
#pragma unroll
                for (int t = 0; t < QCH; ++t) {
                    if constexpr (SPLIT) {                            // a tile past the wave's share: the last one again, dropped on store
                        qv[t] = qrow[16 * (t0 + t < qn ? t0 + t : qn - 1)];
                    } else {
                        qv[t] = t0 + t < QW ? qrow[16 * (t0 + t)] : T(0);
                    }
                }
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    const int pt = wave + WP * i;                 // a wave without an i-th tile multiplies the last tile again and drops it
                    pv[i] = prow[16 * (pt < PT ? pt : PT - 1)];
                }
#pragma unroll
                for (int t = 0; t < QCH; ++t) qv[t] = ok ? qv[t] : T(0);
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    const T p = ok ? pv[i] : T(0);
#pragma unroll
                    for (int t = 0; t < QCH; ++t)
                        if (t0 + t < QW) acc[i][t] = Frag<T>::mfma(p, qv[t], acc[i][t]);
                }
            }
#pragma unroll
            for (int i = 0; i < MP; ++i) {
                const int pt = wave + WP * i;
                if (pt >= PT) continue;
#pragma unroll
                for (int t = 0; t < QCH; ++t) {
                    if (t0 + t >= QW || t0 + t >= qn) continue;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int fr = sizeof(T) == 4 ? 4 * lk + rr : lk + 4 * rr;      // C/D fragment row of (lane quarter lk, register rr)
                        const int idx = (16 * pt + fr) * G::QCOLS + 16 * (q0 + t0 + t) + li;
                        out[idx] = used[idx] ? scale * acc[i][t][rr] : T(0);
                    }
                }
            }
        }
        if ((int)threadIdx.x < NOUT * G::HEAD_ROW) {
            const int idx = (int)S::DW0 + threadIdx.x;
            out[idx] = used[idx] ? scale * head[s * NOUT * G::HEAD_ROW + threadIdx.x] : T(0);
        }
    }
}

// 64 columns per workgroup of 4 waves: wave g adds the g-th quarter of the rows in order, wave 0 the four sums.  w == nullptr: w_s = 1.
template <typename T>
__global__ void __launch_bounds__(256) sr_colsum_kernel(const T* __restrict__ J, int64_t ns, int64_t D, const double* __restrict__ w,
                                                        double scale, double* __restrict__ out) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t chunk = (ns + 3) / 4, s0 = g * chunk, s1 = s0 + chunk < ns ? s0 + chunk : ns;
    const int64_t nblocks = (D + 63) / 64;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t col = b * 64 + lane;
        double v = 0.0;
        if (col < D)
            for (int64_t s = s0; s < s1; ++s) v += (w ? w[s] : 1.0) * (double)J[s * D + col];
        part[g][lane] = v;
        __syncthreads();
        if (g == 0 && col < D) out[col] = scale * (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
        __syncthreads();
    }
}

// gram = (J - mean)(J - mean)^T, [ns][ns] f64.  One workgroup per 32 x 32 block (bi, bj <= bi) of the lower triangle: 2 x 2 MFMA
// tiles per wave, the four waves take a quarter of the columns of J each (16 columns per step: a lane loads four consecutive
// elements of its row, element j is k-step j - both operands use the same order) and wave 0 adds the four partial blocks in order.
// Element (r, c), r >= c, is stored to (r, c) and (c, r): symmetric by construction.  D is a multiple of 4.
// mult[k]: how many flat parameters read image element k (0 padding, 2 the head's logit-difference row, which the two columns of
// wf_dense share with opposite signs) - the product is the flat-order one, sum over PARAMETERS.
// HALVES (complex RNN): ns is the order 2 x samples; the rows from ns / 2 on are centred with the second mean vector, mean + D.
template <typename T, bool HALVES = false>
__global__ void __launch_bounds__(256) sr_gram_kernel(const T* __restrict__ J, const double* __restrict__ mean, const uint8_t* __restrict__ mult,
                                                      int64_t ns, int64_t D, int64_t nblocks, double* __restrict__ gram) {
    typedef double V4 __attribute__((ext_vector_type(4)));
    typedef T T4 __attribute__((ext_vector_type(4)));
    __shared__ V4 red[3][2][2][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int64_t ksteps = (D + 15) / 16, ks0 = wave * ksteps / 4, ks1 = (wave + 1) * ksteps / 4;
    for (int64_t item = blockIdx.x; item < nblocks; item += gridDim.x) {
        int64_t bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= item) ++bi;
        const int64_t bj = item - bi * (bi + 1) / 2;
        const T* arow[2];
        const T* brow[2];
        const double* amean[2];
        const double* bmean[2];
        bool aok[2], bok[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int64_t ra = 32 * bi + 16 * x + li, rb = 32 * bj + 16 * x + li;
            aok[x] = ra < ns;
            bok[x] = rb < ns;
            arow[x] = J + (aok[x] ? ra : 0) * D;                   // rows past ns are read from row 0 and zeroed
            brow[x] = J + (bok[x] ? rb : 0) * D;
            amean[x] = mean + (HALVES && 2 * ra >= ns ? D : 0);
            bmean[x] = mean + (HALVES && 2 * rb >= ns ? D : 0);
        }
        V4 acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = V4{0.0, 0.0, 0.0, 0.0};
        for (int64_t ks = ks0; ks < ks1; ++ks) {
            const int64_t k = 16 * ks + 4 * lk;
            const bool kok = k < D;
            const int64_t kc = kok ? k : 0;
            V4 ma[2], mb[2];
            ma[0] = *reinterpret_cast<const V4*>(amean[0] + kc);
            if constexpr (HALVES) {
                ma[1] = *reinterpret_cast<const V4*>(amean[1] + kc);
                mb[0] = *reinterpret_cast<const V4*>(bmean[0] + kc);
                mb[1] = *reinterpret_cast<const V4*>(bmean[1] + kc);
            } else {
                ma[1] = mb[0] = mb[1] = ma[0];
            }
            const uchar4 mu4 = *reinterpret_cast<const uchar4*>(mult + kc);
            const double mu[4] = {(double)mu4.x, (double)mu4.y, (double)mu4.z, (double)mu4.w};
            double av[2][4], bv[2][4];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const T4 a = *reinterpret_cast<const T4*>(arow[x] + kc);
                const T4 b = *reinterpret_cast<const T4*>(brow[x] + kc);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    av[x][j] = aok[x] && kok ? ((double)a[j] - ma[x][j]) * mu[j] : 0.0;
                    bv[x][j] = bok[x] && kok ? (double)b[j] - mb[x][j] : 0.0;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = Frag<double>::mfma(av[x][j], bv[y][j], acc[x][y]);
        }
        if (wave > 0) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) red[wave - 1][x][y][lane] = acc[x][y];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    V4 v = acc[x][y];
#pragma unroll
                    for (int w = 0; w < 3; ++w) v += red[w][x][y][lane];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int64_t r = 32 * bi + 16 * x + lk + 4 * rr, c = 32 * bj + 16 * y + li;     // f64 C/D fragment: row lk + 4 rr
                        if (r < ns && c <= r) {
                            gram[r * ns + c] = v[rr];
                            gram[c * ns + r] = v[rr];
                        }
                    }
                }
        }
        __syncthreads();
    }
}

}  // namespace rnnwf
