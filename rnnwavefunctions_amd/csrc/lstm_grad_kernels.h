// lstm_grad_kernels.h - back-propagation through time for the LSTM wave function (model LSTM1D_F64), the LSTM counterpart of
// gru_bwd_kernel (grad_kernels.h): grad = sum_s w_s d log P(s) / d theta, float64 on the f64 MFMA, 16 chains per wave.
//
//   lstm_bwd_kernel : walks sites N-1 down to 0.  Site n restores (h_in, c_in) from checkpoint n-1 of the base pass (lstm_kernels.h:
//                     hck, zeros at n = 0), recomputes i, j, f, o, c', tanh c' with LstmCore's arithmetic (the f rows of BINIT carry
//                     the forget bias), and with g = w_s (sigma_n - p1) from the head forms
//                         dh' = dh_carry + g wd              da_o = dh' tanh c' o (1 - o)
//                         dc' = dc_carry + dh' o (1 - tanh^2 c')
//                         da_f = dc' c_in f (1 - f)          da_i = dc' j i (1 - i)          da_j = dc' i (1 - j^2)
//                         dc_carry = dc' f                   dh_carry = sum over the gates of W_h^T da   (MFMA)
//                     One unit group at a time, as LstmCore::step: the group's gate tiles go through the forward MFMA chain, its
//                     da go into the P row and, as B operands, into the backward chain, which accumulates dh_carry over the groups.
//                     h' of site n is h_in of site n + 1, so only the last site runs a whole forward step first.
//                     Rows written per (site, chain):  P = [da_i | da_j | da_f | da_o] in the forward image's tile order,
//                     Q = [h_in in unit-fragment order ; x0, x1, 1 in the spare slots]: the LSTM has one kernel matrix, so its input
//                     rows and its bias come out of the same P^T Q (tn_gemm.h).  Head-row sums go per wave into head_part
//                     (head_reduce_kernel adds them): no atomics, the gradient is bit-reproducible.
//
// Backward operand [NTO][KBG][64] x 16 B (NTO = NFULL + 1 tiles of hidden units that receive dL/dh): k-step 4 kt + gate of output
// tile t holds the weight from pre-activation (gate, unit 4 kt + lane quarter) back to the tile's unit - pack_bwd_side's operand
// (grad.hip) with four gates, the gates of one unit quad adjacent so that a group's da feed the chain as they are formed.
// NFULL 1 and 2 hold it in LDS beside the forward image (35 and 99 KB); at NFULL 3 and 4 (196 and 322 KB) it is read through L2
// with buffer loads one k-group ahead, as GradStream does for the GRU.
#pragma once
#include "grad_kernels.h"
#include "lstm_core.h"

namespace rnnwf {

template <int NFULL>
struct LstmGradLayout {
    using L = LstmLayout<NFULL>;
    static constexpr int KT = L::KT, NT = L::NT;
    static constexpr int NTO = NFULL + 1;                 // 16-row tiles covering the hidden units
    static constexpr int PCOLS = 16 * NT;                 // gate rows in the forward image's tile order
    static constexpr int QCOLS = 16 * NTO;                // [h_in in unit-fragment order ; x0, x1, 1 in the spare slots]
    static constexpr int KB = 4 * KT;                     // k-steps of the backward product: 4 kt + gate
    static constexpr int VW = 2;                          // k-steps per 16-byte vector
    static constexpr int KBG = KB / VW;                   // vector 2 kt: gates (i, j) of unit quad kt; 2 kt + 1: (f, o)
    static constexpr size_t BWD_BYTES = (size_t)NTO * KBG * 64 * 16;
    static constexpr int HEAD_ROW = 4 * KT + 4;           // gradient per unit slot (4 KT) + bias (+ pad)
    static constexpr bool STREAM = L::BYTES + BWD_BYTES > 160 * 1024;     // the backward operand stays in global memory
    static constexpr size_t LDS = L::BYTES + (STREAM ? 0 : BWD_BYTES);
};

struct LstmGradArgs {
    const void* wimg;          // forward image (LstmLayout)
    const void* wbwd;          // backward operand (LstmGradLayout::BWD_BYTES)
    int32_t N;
    int64_t ns, nsb;
    const uint32_t* bits;
    const double* hck;         // [N-1][nsb][2 KT][64]: (h, c) after every site but the last (lstm_kernels.h)
    const double* weights;     // [ns] w_s, or nullptr: w_s = (eloc[s] - mom[0] / mom[2]) * (1 / mom[2]) from the step's moments
    const double* eloc;        // still on the device (GradArgs::mom's arithmetic)
    const double* mom;
    double* P;                 // [N*ns][PCOLS]
    double* Q;                 // [N*ns][QCOLS]
    double* head_grad;         // [HEAD_ROW], written by head_reduce_kernel
    double* head_part;         // [waves of the grid][HEAD_ROW]; SR: [ns][HEAD_ROW], every chain's
};

// SR (sr.hip: the per-sample log-derivatives, docs/sr_lstm.md): unit weights w_s = 1 - weights, eloc and mom are not read - and the
// head row of every chain kept on its own, head_part = [ns][HEAD_ROW] (slot 4 k + q a unit, 4 KT the bias: store_head_part's
// layout), instead of one sum per wave: lane (c, q) holds the units 4 k + q of chain c in hg[0][k], so the row is stored without a
// reduction.  The P and Q rows are the same rows.
template <int NFULL, int WAVES, bool SR = false>
__global__ void __launch_bounds__(WAVES * 64) lstm_bwd_kernel(LstmGradArgs a) {
    using C = LstmCore<NFULL>;
    using L = LstmLayout<NFULL>;
    using G = LstmGradLayout<NFULL>;
    using A = Act<double>;
    using F = Frag<double>;
    using V4 = typename F::V4;
    using VA = typename F::VA;
    constexpr int KT = L::KT, NT = L::NT, NG = L::NG, VW = L::VW, NTO = G::NTO;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const char* img = C::stage(lds, a.wimg);
    if constexpr (!G::STREAM) {
        const uint4* src = reinterpret_cast<const uint4*>(a.wbwd);
        uint4* dst = reinterpret_cast<uint4*>(lds + L::BYTES);
        for (int i = threadIdx.x; i < (int)(G::BWD_BYTES / 16); i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    const char* lbwd = lds + L::BYTES;
    const __amdgpu_buffer_rsrc_t gbwd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wbwd), 0, (int)G::BWD_BYTES, 0x00020000);
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    auto bwd_frag = [&](int t, int kg) -> VA {          // fragment (tile t, vector kg) of the backward operand
        if constexpr (G::STREAM) {
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(gbwd, (threadIdx.x & 63) * 16, (t * G::KBG + kg) * 64 * 16, 0);
            return __builtin_bit_cast(VA, v);
        } else {
            return (reinterpret_cast<const VA*>(lbwd) + (threadIdx.x & 63))[(t * G::KBG + kg) * 64];
        }
    };
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t gw = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t nw = (int64_t)gridDim.x * WAVES;
    const int N = a.N;
    const double* wd = reinterpret_cast<const double*>(img + L::OFF_WD) + q * L::WD_Q;
    const char* avbase = img + L::OFF_AVEC;
    const char* arbase = img + L::OFF_AREM;
    // head-row sums over all chains of this wave
    double hg[1][KT], gb[1] = {0.0};
#pragma unroll
    for (int k = 0; k < KT; ++k) hg[0][k] = 0.0;
    for (int64_t sb = gw; sb < a.nsb; sb += nw) {
        const int64_t s = sb * kChains + c;
        const bool valid = s < a.ns;
        const int64_t sc = valid ? s : a.ns - 1;
        double w = 0.0;
        if constexpr (SR) {
            if (valid) w = 1.0;
            gb[0] = 0.0;
#pragma unroll
            for (int k = 0; k < KT; ++k) hg[0][k] = 0.0;
        } else {
            if (valid) w = a.weights ? a.weights[sc] : (a.eloc[sc] - a.mom[0] / a.mom[2]) * (1.0 / a.mom[2]);
        }
        auto word = [&](int wi) { return a.bits[(int64_t)wi * a.ns + sc]; };
        // the spin words of sites n and n - 1 sit in registers; the word below is fetched 32 sites ahead (gru_bwd_kernel)
        uint32_t wcur = word((N - 1) >> 5), wlow = N > 32 ? word(((N - 1) >> 5) - 1) : 0u;
        auto spin_in = [&](int n) {                       // the spin fed into site n (-1: the zero vector of the first site)
            return n == 0 ? -1 : (n & 31) ? (int)((wcur >> ((n - 1) & 31)) & 1) : (int)(wlow >> 31);
        };
        // (h, c) after site n: checkpoint n; a chain of one site has none (its row 0 is allocated and never read as a value)
        auto state = [&](int n) { return a.hck + (((int64_t)(n > 0 ? n : 0) * a.nsb + sb) * 2 * KT) * 64 + lane; };
        // h' of the last site: the one whole forward step
        double hcur[KT];
        {
            double cs[KT];
            const double* src = state(N - 2);
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const double hv = src[k * 64], cv = src[(KT + k) * 64];
                hcur[k] = N > 1 ? hv : 0.0;
                cs[k] = N > 1 ? cv : 0.0;
            }
            C::step(img, spin_in(N - 1), hcur, cs, lane);
        }
        double dh[KT], dc[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) dh[k] = dc[k] = 0.0;
        for (int n = N - 1; n >= 0; --n) {
            // the input state of this site = checkpoint n - 1, fetched while the head term is formed; c_in follows group by group
            const double* src = state(n - 1);
            const bool first = n == 0;
            double hin[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) hin[k] = src[k * 64];
            const int sig = (int)((wcur >> (n & 31)) & 1);
            const int sig_in = spin_in(n);
            if ((n & 31) == 0 && n > 0) {
                wcur = wlow;
                wlow = n >= 64 ? word((n >> 5) - 2) : 0u;
            }
            // this site's term: d log p(sig) / d(z1 - z0) = sig - p1
            const double z = C::head(img, hcur, lane);
            const double p1 = 1.0 - prob0(z);
            const double g = w * ((double)sig - p1);
            gb[0] += g;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                hg[0][k] += g * hcur[k];
                dh[k] += g * wd[k];                                  // total dL/dh' of this lane's unit
            }
#pragma unroll
            for (int k = 0; k < KT; ++k) hin[k] = first ? 0.0 : hin[k];
            if (valid) {
                double* qrow = a.Q + ((int64_t)n * a.ns + s) * G::QCOLS + 4 * q;
#pragma unroll
                for (int m = 0; m < NFULL; ++m) {
                    V4 v = {hin[4 * m], hin[4 * m + 1], hin[4 * m + 2], hin[4 * m + 3]};
                    *reinterpret_cast<V4*>(qrow + m * 16) = v;
                }
                const double one = q == 0 ? 1.0 : 0.0;
                V4 vq = {hin[KT - 1], one * (sig_in == 0 ? 1.0 : 0.0), one * (sig_in == 1 ? 1.0 : 0.0), one};
                *reinterpret_cast<V4*>(qrow + NFULL * 16) = vq;
            }
            double* prow = a.P + ((int64_t)n * a.ns + s) * G::PCOLS + 4 * q;
            V4 accb[NTO];
#pragma unroll
            for (int t = 0; t < NTO; ++t) accb[t] = V4{0.0, 0.0, 0.0, 0.0};
            const char* binit = img + L::OFF_BINIT + (size_t)(sig_in + 1) * L::SZ_BINIT_VARIANT + (size_t)q * 4 * sizeof(double);
            const VA* av = reinterpret_cast<const VA*>(avbase) + lane;
            const double* ar = reinterpret_cast<const double*>(arbase) + lane;
#pragma unroll
            for (int m = 0; m < NFULL; ++m) {
                constexpr int kMixed = 4;
                const int nt = m == 0 ? 5 : 4;                                     // group 0 carries the mixed tile
                auto tile = [&](int k) { return k < 4 ? k * NFULL + m : NT - 1; };  // k = gate i, j, f, o; 4: mixed
                auto unit_kt = [&](int u) { return u < 4 ? 4 * m + u : KT - 1; };   // unit quad of the group's u-th unit
                asm volatile("" ::: "memory");
                double cin[5];
#pragma unroll
                for (int u = 0; u < 5; ++u)
                    if (u < nt) cin[u] = src[(KT + unit_kt(u)) * 64];
                // ---- the group's pre-activations: LstmCore::step's chain, fragments one k-group ahead ----
                V4 acc[5];
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (k < nt) acc[k] = *reinterpret_cast<const V4*>(binit + (size_t)tile(k) * 16 * sizeof(double));
                __builtin_amdgcn_sched_barrier(0);
                {
                    VA af[2][5];
                    auto fetch = [&](int gk, VA (&dst)[5]) {
#pragma unroll
                        for (int k = 0; k < 5; ++k)
                            if (k < nt) dst[k] = av[(tile(k) * NG + gk) * 64];
                    };
                    fetch(0, af[0]);
#pragma unroll
                    for (int gk = 0; gk < NG; ++gk) {
                        asm volatile("" ::: "memory");
                        if (gk + 1 < NG) fetch(gk + 1, af[(gk + 1) & 1]);
#pragma unroll
                        for (int j = 0; j < VW; ++j)
#pragma unroll
                            for (int k = 0; k < 5; ++k)
                                if (k < nt) acc[k] = F::mfma(af[gk & 1][k][j], hin[gk * VW + j], acc[k]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        if (k < nt) acc[k] = F::mfma(ar[tile(k) * 64], hin[KT - 1], acc[k]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // ---- the first fragments of the backward chain travel while the gates are worked on ----
                const int steps = 2 * nt;                                          // (unit u, gate pair): vector 2 kt(u) + pair
                VA bf[2][NTO];
                auto fetchb = [&](int st, VA (&dst)[NTO]) {
#pragma unroll
                    for (int t = 0; t < NTO; ++t) dst[t] = bwd_frag(t, 2 * unit_kt(st >> 1) + (st & 1));
                };
                fetchb(0, bf[0]);
                // ---- gates and their derivatives, two units per scheduling region ----
                double da[4][5];
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    if (u >= nt) continue;
                    const int kt = unit_kt(u);
                    const double ai = u < 4 ? acc[0][u] : acc[kMixed][0], aj = u < 4 ? acc[1][u] : acc[kMixed][1];
                    const double af_ = u < 4 ? acc[2][u] : acc[kMixed][2], ao = u < 4 ? acc[3][u] : acc[kMixed][3];
                    const double ci = first ? 0.0 : cin[u];
                    double ig, jt, fg, og, tc;
                    {
#pragma clang fp contract(off)
                        ig = A::sigmoid_scaled(ai);
                        jt = A::tanh_scaled(aj);
                        fg = A::sigmoid_scaled(af_);
                        og = A::sigmoid_scaled(ao);
                        tc = A::tanh_scaled(fma_(fg, ci, ig * jt));
                    }
                    const double d = dh[kt];
                    const double dcn = dc[kt] + d * og * (1.0 - tc * tc);
                    da[3][u] = d * tc * og * (1.0 - og);
                    da[2][u] = dcn * ci * fg * (1.0 - fg);
                    da[0][u] = dcn * jt * ig * (1.0 - ig);
                    da[1][u] = dcn * ig * (1.0 - jt * jt);
                    dc[kt] = dcn * fg;
                    if (u & 1) __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (valid) {
#pragma unroll
                    for (int gt = 0; gt < 4; ++gt) {
                        V4 v = {da[gt][0], da[gt][1], da[gt][2], da[gt][3]};
                        *reinterpret_cast<V4*>(prow + (gt * NFULL + m) * 16) = v;
                    }
                    if (m == 0) {
                        V4 vm = {da[0][kMixed], da[1][kMixed], da[2][kMixed], da[3][kMixed]};     // mixed tile: row 4 q + gate
                        *reinterpret_cast<V4*>(prow + (NT - 1) * 16) = vm;
                    }
                }
                // ---- dL/dh_in += W_h^T da of this group's units (A = transposed weights, B = the da as they stand) ----
#pragma unroll
                for (int st = 0; st < 10; ++st) {
                    if (st >= steps) continue;
                    asm volatile("" ::: "memory");
                    if (st + 1 < steps) fetchb(st + 1, bf[(st + 1) & 1]);
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int t = 0; t < NTO; ++t)
                            accb[t] = F::mfma(bf[st & 1][t][e], da[2 * (st & 1) + e][st >> 1], accb[t]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int m = 0; m < NFULL; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) dh[4 * m + r] = accb[m][r];
            dh[KT - 1] = accb[NFULL][0];
#pragma unroll
            for (int k = 0; k < KT; ++k) hcur[k] = hin[k];          // h' of site n - 1
        }
        if constexpr (SR) {
            if (valid) {
                double* row = a.head_part + s * G::HEAD_ROW;
#pragma unroll
                for (int k = 0; k < KT; ++k) row[4 * k + q] = hg[0][k];
                row[4 * KT + q] = q == 0 ? gb[0] : 0.0;
            }
        }
    }
    if constexpr (!SR) store_head_part<double, 1, KT>(a.head_part + (size_t)gw * G::HEAD_ROW, G::HEAD_ROW, hg, gb, c, q);
}

}  // namespace rnnwf
