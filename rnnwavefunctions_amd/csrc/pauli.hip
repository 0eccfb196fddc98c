// pauli.hip - host driver of rnnwf_pauli_step (include/rnnwf.h): expectation values of Pauli strings and the local energy of any
// real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient), for the positive GRU models (GRU1D,
// GRU1D_F64, one layer); kernels in pauli_kernels.h and chain_kernels.h (prnn_masked_tail_kernel, not PAIRED), the
// method in docs/pauli.md; the launch table, refusals, base pass, pass size and pass loop are observable.h's.
//
// Per call: the masks are checked and packed into words, the terms grouped by flip mask (a mask shared by several terms is
// evaluated once) and the distinct masks sorted longest chain first.  Per pass of whole 16-chain blocks (the state budget, as
// renyi_regions.hip): spins (the caller's, or drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass on the one-wave
// kernel with checkpoints -> site terms and flip-mask tails -> log-ratios, per-term sums of v and v^2, E_loc and its moments.  The
// sums of the passes are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, checkpoints, E_loc)
// resident for rnnwf_vmc_gradient.
#include <algorithm>
#include <cstring>
#include <vector>

#include "observable.h"
#include "pauli_kernels.h"
#include "pauli_terms.h"

using namespace rnnwf;

namespace {

using Terms = PauliTerms;

// Scratch of one pass of ns chains in h->renyi; the call's tables lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, sgn, tmask, coeff, terms, logp, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per term
    Scratch(int N, const Terms& g, int64_t ns) {
        Carve c;
        const size_t M = (size_t)std::max(g.M, 1), K = (size_t)g.K;
        nblk = (ns + kPauliThreads - 1) / kPauliThreads;
        mask = c.take(M * g.W * 4);
        order = c.take(M * 4);
        first = c.take(M * 4);
        sgn = c.take(K * g.W * 4);
        tmask = c.take(K * 4);
        coeff = c.take(K * 8);
        terms = c.take((size_t)N * ns * 8);
        logp = c.take((size_t)ns * 8);
        tail = c.take(M * ns * 8);
        lr = c.take(M * ns * 8);
        part = c.take(K * nblk * 16);
        sums = c.take(K * 16);
        bytes = c.bytes;
    }
};

// one pass over the ns chains packed in h->bits: sums_host (K, 2) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
// keep: the pass is the whole call, its checkpoints are left for rnnwf_vmc_gradient (diagonal terms alone need no base pass otherwise)
int pauli_pass(rnnwf_handle* h, int64_t ns, const Terms& g, const Scratch& sc, bool keep, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    double* lr = (double*)(buf + sc.lr);
    if (M > 0 || keep)
        if (int rc = observable_base(h, ns, (double*)(buf + sc.logp))) return rc;
    const ChainArgs c = chain_args(h, ns);
    if (M > 0) {
        SwapArgs t{c};
        t.terms = (double*)(buf + sc.terms);
        MaskArgs a{c};
        a.mask = (const uint32_t*)(buf + sc.mask);
        a.order = (const int32_t*)(buf + sc.order);
        a.first = (const int32_t*)(buf + sc.first);
        a.tail = (double*)(buf + sc.tail);
        a.ntiles = (int64_t)M * a.nsb;
        int rc = 0;
        with_gru1(h, [&](auto k) {
            using L = decltype(k);
            if (g.replay) rc = launch_waves(h, k, kTimerBase, prnn_site_terms_kernel<typename L::T, L::NFULL, L::WAVES>, t.nsb, t);     // N >= 2
            if (!rc) rc = launch_waves(h, k, kTimerFlip, prnn_masked_tail_kernel<typename L::T, L::NFULL, L::WAVES, false>, a.ntiles, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * L::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over masks of N - f cell evaluations per chain
        if (int rc2 = timed_launch(h, kTimerAssembly, pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                   (const double*)a.tail, (const double*)t.terms, (const double*)(buf + sc.logp), a.first, N, ns, lr))
            return rc2;
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
        const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
        pauli_term_kernel<<<(unsigned)(K * sc.nblk), kPauliThreads, 0, h->stream>>>(c.bits, sgn, tmask, lr, g.W, ns, sc.nblk,
                                                                                   (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)K, kPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
        pauli_eloc_kernel<<<(unsigned)sc.nblk, kPauliThreads, 0, h->stream>>>(c.bits, sgn, tmask, (const double*)(buf + sc.coeff), lr, K, g.W,
                                                                             ns, (double*)h->eloc.p);
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)K * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_pauli_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck, h->eloc) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = observable_refuse(h, "rnnwf_pauli_step")) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_pauli_step: nterms must be >= 1");
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_pauli_step: ns must be >= 1");
    if (!flip || !sign || !coeff || !term_sums)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_pauli_step: flip, sign, coeff and term_sums must be non-null");
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_pauli_step: sample_offset must be >= 0");
    Terms g;
    if (int rc = prepare_pauli_terms(h, "rnnwf_pauli_step", flip, sign, nterms, g)) return rc;
    const int N = h->N, K = nterms, M = g.M;
    // chains per pass: per block, beside the checkpoints, the terms (N x 16 x 8 bytes), log P (16 x 8), the tails and log-ratios
    // (2 x M x 16 x 8) and E_loc (16 x 8)
    const int64_t chunk = blocks_per_pass(h, (size_t)(N + 2 + 2 * M) * kChains * 8) * kChains;
    if ((int64_t)K * ((std::min(chunk, ns) + kPauliThreads - 1) / kPauliThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_pauli_step: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", kPauliThreads);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    // the first pass is the largest: one allocation for the call, the tables uploaded once
    const Scratch big(N, g, std::min(chunk, ns));
    if (int rc = ensure(h, h->renyi, big.bytes)) return rc;
    {
        char* buf = (char*)h->renyi.p;
        if (M) {
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.order, g.order.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.first, g.first.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
        }
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.sgn, g.sgn.data(), g.sgn.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.tmask, g.tmask.data(), (size_t)K * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.coeff, coeff, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    std::vector<double> total((size_t)K * 2, 0.0);
    double mom[4] = {0.0, 0.0, 0.0, 0.0};
    const ChainSource src{samples, seed, step, sample_offset, out_samples};
    if (int rc = for_each_pass(h, src, ns, chunk, 1, total, [&](int64_t s0, int64_t, int64_t n, double* pass_sums) {
            const Scratch sc(N, g, n);
            if (int rc = pauli_pass(h, n, g, sc, ns <= chunk, pass_sums)) return rc;
            if (out_log_ratio && M)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + s0, (size_t)ns * 8, (char*)h->renyi.p + sc.lr, (size_t)n * 8, (size_t)n * 8,
                                              (size_t)M, hipMemcpyDeviceToHost, h->stream));
            if (out_eloc) RNNWF_HIP(h, hipMemcpyAsync(out_eloc + s0, h->eloc.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
            if (moments) {                                               // synchronises the stream
                double pm[4];
                if (int rc = run_moments(h, h->eloc.p, n, false, pm)) return rc;
                for (int k = 0; k < 3; ++k) mom[k] += pm[k];
            }
            return 0;
        }))
        return rc;
    memcpy(term_sums, total.data(), total.size() * 8);
    if (moments) memcpy(moments, mom, sizeof mom);
    // one pass: bits, checkpoints and E_loc of the whole batch are on the device, as rnnwf_vmc_step leaves them
    if (ns <= chunk && h->family->gradient) h->last_ns = ns;
    h->sr_valid = false;                              // a new batch: its log-derivatives are not built yet (sr.hip)
    return RNNWF_OK;
}
