// lstm_corr.hip - host driver of rnnwf_correlations_lstm (include/rnnwf.h): <sz_i>, <sz_i sz_j>, <sx_i> and <sx_i sx_j> of the LSTM
// wave function over the raster path (LSTM1D_F64, one layer, 1..68 units, float64) for every site and pair at once; the recurrent
// kernels in lstm_corr_kernels.h, from the suffix sums on corr_kernels.h's; the method in docs/correlations_lstm.md.
//
// It is corr.hip's pass with the LSTM's three kernels: per pass of whole 16-chain blocks (the state budget) spins (the caller's, or
// drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass with checkpoints and both outcomes of every site -> trunk pass
// (one flip, states kept) -> branch pass (second flip) -> log-ratios and sums.  The sums of the passes are added on the host in pass
// order.  The launch table, the size of a state row and the refusals are lstm_observable.h's, the pass loop observable.h's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "lstm_corr_kernels.h"
#include "lstm_observable.h"

using namespace rnnwf;

namespace {

constexpr const char* kEntry = "rnnwf_correlations_lstm";

int64_t num_pairs(int N) { return (int64_t)N * (N - 1) / 2; }

// The launch class of a width: the trunk stores (h, c) at every site as the base pass does and takes the base pass's waves per
// workgroup (BWAVES: at 68 units one wave per SIMD), the branch the tails' (profiles/lstm_corr_kernel_resources.txt)
template <int NFULL, int WAVES>
struct LCorr : LPauli<NFULL, WAVES> {
    using P = LPauli<NFULL, WAVES>;
    using L = typename P::L;
    static constexpr int BWAVES = P::BWAVES;
    static int corr_base(rnnwf_handle* h, const CorrArgs& a) {
        return launch_shrinking<BWAVES>(h, kTimerBase, lstm_corr_base_kernel<NFULL, BWAVES>, L::BYTES, a.nsb, a);
    }
    static int trunk(rnnwf_handle* h, const CorrArgs& a) {
        return launch_shrinking<BWAVES>(h, kTimerFlip, lstm_trunk_kernel<NFULL, BWAVES>, L::BYTES, a.ntiles, a);
    }
    static int branch(rnnwf_handle* h, const CorrArgs& a) {
        return launch_shrinking<WAVES>(h, kTimerFlip, lstm_branch_kernel<NFULL, WAVES>, L::BYTES, a.ntiles, a);
    }
};

template <class Fn>
bool with_lcorr(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<LCorr>(LstmKernels(), h, fn); }

// Scratch of one pass of ns chains in h->corr (the trunk states have their own buffer, h->tck): corr.hip's carving
struct Scratch {
    size_t bsel, both, suf, tsel, toth, tail, lr, z, zz, x, xx, bytes;
    Scratch(int N, int64_t ns) {
        Carve c;
        const size_t site = (size_t)N * ns * 8, pair = (size_t)std::max<int64_t>(num_pairs(N), 1) * ns * 8;
        bsel = c.take(site);
        both = c.take(site);
        suf = c.take(site);
        tsel = c.take(pair);
        toth = c.take(pair);
        tail = c.take(pair);
        lr = c.take((size_t)(N + num_pairs(N)) * ns * 8);
        z = c.take((size_t)N * 8);
        zz = c.take((size_t)N * N * 8);
        x = c.take((size_t)N * 2 * 8);
        xx = c.take((size_t)N * N * 5 * 8);
        bytes = c.bytes;
    }
};

// one pass over the ns chains packed in h->bits: the four sums of this pass into `out` (z | zz | x | xx); the log-ratios stay in h->corr
int corr_pass(rnnwf_handle* h, int64_t ns, const Scratch& sc, double* out) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains, NP = num_pairs(N);
    const size_t row = hck_bytes_per_block(h);
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * row)) return rc;
    if (int rc = ensure(h, h->tck, (size_t)std::max<int64_t>(NP, 1) * nsb * row)) return rc;
    if (int rc = ensure(h, h->corr, sc.bytes)) return rc;
    char* buf = (char*)h->corr.p;
    CorrArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.W = (N + 31) / 32;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.tck = h->tck.p;
    a.bsel = (double*)(buf + sc.bsel);
    a.both = (double*)(buf + sc.both);
    a.tsel = (double*)(buf + sc.tsel);
    a.toth = (double*)(buf + sc.toth);
    a.tail = (double*)(buf + sc.tail);
    const double evals = (double)NP + (double)NP * (N - 2) / 3.0;      // N(N-1)/2 trunk + N(N-1)(N-2)/6 branch evaluations per chain
    int rc = 0;
    with_lcorr(h, [&](auto k) {
        using K = decltype(k);
        rc = K::corr_base(h, a);
        if (!rc && N > 1) {
            a.ntiles = (int64_t)(N - 1) * nsb;
            rc = K::trunk(h, a);
        }
        if (!rc && N > 2) {
            a.ntiles = (int64_t)(N - 1) * (N - 2) / 2 * nsb;
            rc = K::branch(h, a);
        }
        if (!rc) h->work[1] += (double)nsb * evals * K::mfma_flops_per_step();
    });
    if (rc) return rc;
    h->work[0] += (double)ns * evals;
    {
        TimedLaunch tl(h, kTimerAssembly);
        const unsigned nblk = (unsigned)((ns + kCorrThreads - 1) / kCorrThreads);
        double* lr = (double*)(buf + sc.lr);
        corr_suffix_kernel<<<nblk, kCorrThreads, 0, h->stream>>>(a.bsel, N, ns, (double*)(buf + sc.suf));
        RNNWF_HIP(h, hipGetLastError());
        corr_assemble_kernel<<<dim3(nblk, (unsigned)N), kCorrThreads, 0, h->stream>>>(a, (const double*)(buf + sc.suf), lr);
        RNNWF_HIP(h, hipGetLastError());
        RNNWF_HIP(h, hipMemsetAsync(buf + sc.xx, 0, (size_t)N * N * 5 * 8, h->stream));      // entries with i >= j stay 0
        corr_sums_kernel<<<(unsigned)(N + NP), kCorrThreads, 0, h->stream>>>(lr, N, ns, (double*)(buf + sc.x), (double*)(buf + sc.xx));
        RNNWF_HIP(h, hipGetLastError());
        corr_diag_kernel<<<dim3((unsigned)N, (unsigned)N), kCorrThreads, 0, h->stream>>>(a.bits, N, ns, (double*)(buf + sc.z),
                                                                                        (double*)(buf + sc.zz));
        RNNWF_HIP(h, hipGetLastError());
    }
    // z | zz | x | xx are contiguous up to their alignment padding: four copies into the packed host vector
    const size_t nz = N, nzz = (size_t)N * N, nx = (size_t)N * 2, nxx = (size_t)N * N * 5;
    RNNWF_HIP(h, hipMemcpyAsync(out, buf + sc.z, nz * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz, buf + sc.zz, nzz * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz + nzz, buf + sc.x, nx * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz + nzz + nx, buf + sc.xx, nxx * 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_correlations_lstm(rnnwf_handle* h, const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step,
                                       int64_t sample_offset, double* z_sums, double* zz_sums, double* x_sums, double* xx_sums,
                                       double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = lstm_pauli_refuse(h, kEntry, LstmEntryKind::Corr)) return rc;
    if (int rc = refuse_uncommitted(h, kEntry, false)) return rc;
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: ns must be >= 1", kEntry);
    if (!z_sums || !zz_sums || !x_sums || !xx_sums)
        return h->fail(RNNWF_ERR_INVALID, "%s: z_sums, zz_sums, x_sums and xx_sums must be non-null", kEntry);
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", kEntry);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N;
    // chains per pass: per block the checkpoints, the trunk states and, beside them, 4 N + 4 N(N-1)/2 rows of 16 doubles
    const int64_t NP = num_pairs(N), rows = N + NP;
    const size_t row = hck_bytes_per_block(h);
    const size_t per_block = (size_t)std::max(N - 1, 1) * row + (size_t)std::max<int64_t>(NP, 1) * row + (size_t)(4 * N + 4 * NP) * kChains * 8;
    const int64_t chunk = kChains * std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on: a batch of
    h->sr_valid = false;                              // rnnwf_lstm_load_batch and its log-derivatives are gone
    const size_t nz = N, nzz = (size_t)N * N, nx = (size_t)N * 2, nxx = (size_t)N * N * 5;
    std::vector<double> total(nz + nzz + nx + nxx, 0.0);
    const ChainSource src{samples, seed, step, sample_offset, out_samples};
    if (int rc = for_each_pass(h, src, ns, chunk, 1, total, [&](int64_t s0, int64_t, int64_t n, double* pass_sums) {
            const Scratch sc(N, n);
            if (int rc = corr_pass(h, n, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + s0, (size_t)ns * 8, (char*)h->corr.p + sc.lr, (size_t)n * 8, (size_t)n * 8,
                                              (size_t)rows, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(z_sums, total.data(), nz * 8);
    memcpy(zz_sums, total.data() + nz, nzz * 8);
    memcpy(x_sums, total.data() + nz + nzz, nx * 8);
    memcpy(xx_sums, total.data() + nz + nzz + nx, nxx * 8);
    return RNNWF_OK;
}
