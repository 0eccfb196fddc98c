// crnn_pauli.hip - host driver of rnnwf_pauli_step_complex (include/rnnwf.h): expectation values of Pauli strings and the local
// energy of any spin-1/2 Hamiltonian given as terms (flip mask, sign mask, complex coefficient), for the complex RNN with the U(1)
// mask (CRNN_U1, one layer); kernels in crnn_pauli_kernels.h, the method in docs/pauli_complex.md; the scratch carving, the chain
// source and the pass loop are observable.h's.
//
// Per call: the masks are checked and packed into words, the terms grouped by flip mask (a mask shared by several terms is
// evaluated once) and the distinct masks sorted longest chain first.  Per pass of whole 16-chain blocks (the state budget): spins
// (the caller's, or drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints
// -> site terms and flip-mask tails -> complex log-ratios, per-term sums, E_loc (complex64) and its moments.  The sums of the passes
// are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, checkpoints, E_loc) resident for
// rnnwf_vmc_gradient.
#include <algorithm>
#include <cstring>
#include <vector>

#include "crnn_observable.h"
#include "crnn_pauli_kernels.h"
#include "pauli_terms.h"

using namespace rnnwf;

namespace {

const char* const kEntry = "rnnwf_pauli_step_complex";

using Terms = PauliTerms;

// Scratch of one pass of ns chains in h->renyi; the call's tables lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, sgn, tmask, coeff, terms, tot, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per term
    Scratch(int N, const Terms& g, int64_t ns) {
        Carve c;
        const size_t M = (size_t)std::max(g.M, 1), K = (size_t)g.K;
        nblk = (ns + kCPauliThreads - 1) / kCPauliThreads;
        mask = c.take(M * g.W * 4);
        order = c.take(M * 4);
        first = c.take(M * 4);
        sgn = c.take(K * g.W * 4);
        tmask = c.take(K * 4);
        coeff = c.take(K * 16);
        terms = c.take((size_t)N * ns * 16);
        tot = c.take((size_t)ns * 16);
        tail = c.take(M * ns * 16);
        lr = c.take(M * ns * 16);
        part = c.take(K * nblk * 32);
        sums = c.take(K * 32);
        bytes = c.bytes;
    }
};

// one pass over the ns chains packed in h->bits: sums_host (K, 4) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
// keep: the pass is the whole call, its checkpoints are left for rnnwf_vmc_gradient (diagonal terms alone need no base pass otherwise)
int pauli_pass(rnnwf_handle* h, int64_t ns, const Terms& g, const Scratch& sc, bool keep, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->eloc, (size_t)ns * sizeof(float2))) return rc;
    char* buf = (char*)h->renyi.p;
    double2* lr = (double2*)(buf + sc.lr);
    if (M > 0 || keep) {
        if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * crnn_hck_bytes_per_block(h))) return rc;
        CrnnArgs b = crnn_base_args(h, ns);
        b.bits = (uint32_t*)h->bits.p;
        b.hck = h->hck.p;
        b.tot = (double2*)(buf + sc.tot);
        if (int rc = crnn_plain_base(h, b)) return rc;
    }
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    if (M > 0) {
        CPauliArgs a{};
        a.wimg = h->wimg.p;
        a.N = N;
        a.W = g.W;
        a.ns = ns;
        a.nsb = nsb;
        a.bits = bits;
        a.hck = h->hck.p;
        a.terms = (double2*)(buf + sc.terms);
        a.mask = (const uint32_t*)(buf + sc.mask);
        a.order = (const int32_t*)(buf + sc.order);
        a.first = (const int32_t*)(buf + sc.first);
        a.tail = (double2*)(buf + sc.tail);
        a.ntiles = (int64_t)M * nsb;
        int rc = 0;
        with_crnn1(h, [&](auto k) {
            using P = decltype(k);
            using L = typename P::L;
            if (g.replay)
                rc = launch_persistent(h, kTimerBase, crnn_site_terms_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::LDS_BYTES, a.nsb, P::WAVES, a);
            if (!rc)
                rc = launch_persistent(h, kTimerFlip, crnn_masked_tail_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::LDS_BYTES, a.ntiles, P::WAVES, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * P::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over masks of N - f cell evaluations per chain
        if (int rc2 = timed_launch(h, kTimerAssembly, crnn_pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kCPauliThreads, 0,
                                   (const double2*)a.tail, (const double2*)a.terms, (const double2*)(buf + sc.tot), a.first, N, ns, lr))
            return rc2;
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
        const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
        crnn_pauli_term_kernel<<<(unsigned)(K * sc.nblk), kCPauliThreads, 0, h->stream>>>(bits, sgn, tmask, lr, g.W, ns, sc.nblk,
                                                                                         (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        // rows (term, half): half 0 = (sum Re v, sum Im v), half 1 = the sums of their squares
        renyi_sums_kernel<<<(unsigned)(2 * K), kCPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
        crnn_pauli_eloc_kernel<<<(unsigned)sc.nblk, kCPauliThreads, 0, h->stream>>>(bits, sgn, tmask, (const double2*)(buf + sc.coeff), lr, K,
                                                                                   g.W, ns, (float2*)h->eloc.p);
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)K * 32, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_pauli_step_complex(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff_re_im, int32_t nterms,
                                        const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                        double* term_sums, float* out_eloc_re_im, double* moments, double* out_log_ratio,
                                        int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck, h->eloc) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (h->model != RNNWF_MODEL_CRNN_U1)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the complex RNN (CRNN_U1) only, this handle's model is %s; rnnwf_pauli_step serves the "
                       "GRU models, rnnwf_pauli_step_2d the 2D RNN", kEntry, model_name(h->model));
    if (h->NL > 1) return h->fail(RNNWF_ERR_INVALID, "%s: not implemented for stacked layers (one GRU layer only)", kEntry);
    if (!with_crnn1(h, [](auto) {})) return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for NFULL=%d", kEntry, h->NFULL);
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "%s: nterms must be >= 1", kEntry);
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: ns must be >= 1", kEntry);
    if (!flip || !sign || !coeff_re_im || !term_sums)
        return h->fail(RNNWF_ERR_INVALID, "%s: flip, sign, coeff_re_im and term_sums must be non-null", kEntry);
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", kEntry);
    if (h->N < 2) return h->fail(RNNWF_ERR_INVALID, "%s: needs a chain of at least two sites", kEntry);
    if (samples)                                      // the caller's chains must lie in the sector: their own log psi is -inf otherwise
        if (int rc = crnn_check_sector(h, kEntry, samples, ns)) return rc;
    Terms g;
    if (int rc = prepare_pauli_terms(h, kEntry, flip, sign, nterms, g)) return rc;
    const int N = h->N, K = nterms, M = g.M;
    // chains per pass: per block, beside the checkpoints, the terms (N x 16 x 16 bytes), the base pass's totals (16 x 16), the tails
    // and log-ratios (2 x M x 16 x 16) and E_loc (16 x 8)
    const int64_t chunk = crnn_blocks_per_pass(h, (size_t)(N + 1 + 2 * M) * kChains * 16 + kChains * 8) * kChains;
    if ((int64_t)K * ((std::min(chunk, ns) + kCPauliThreads - 1) / kCPauliThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "%s: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", kEntry, kCPauliThreads);
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
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.coeff, coeff_re_im, (size_t)K * 16, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    std::vector<double> total((size_t)K * 4, 0.0);
    double mom[4] = {0.0, 0.0, 0.0, 0.0};
    const ChainSource src{samples, seed, step, sample_offset, out_samples};
    if (int rc = for_each_pass(h, src, ns, chunk, 1, total, [&](int64_t s0, int64_t, int64_t n, double* pass_sums) {
            const Scratch sc(N, g, n);
            if (int rc = pauli_pass(h, n, g, sc, ns <= chunk, pass_sums)) return rc;
            if (out_log_ratio && M)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + 2 * s0, (size_t)ns * 16, (char*)h->renyi.p + sc.lr, (size_t)n * 16, (size_t)n * 16,
                                              (size_t)M, hipMemcpyDeviceToHost, h->stream));
            if (out_eloc_re_im)
                RNNWF_HIP(h, hipMemcpyAsync(out_eloc_re_im + 2 * s0, h->eloc.p, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
            if (moments) {                                               // synchronises the stream
                double pm[4];
                if (int rc = run_moments(h, h->eloc.p, n, true, pm)) return rc;
                for (int k = 0; k < 4; ++k) mom[k] += pm[k];
            }
            return 0;
        }))
        return rc;
    // the device rows are (term, half) x (re, im): {sum Re v, sum Im v, sum (Re v)^2, sum (Im v)^2} per term already
    memcpy(term_sums, total.data(), total.size() * 8);
    if (moments) memcpy(moments, mom, sizeof mom);
    // one pass: bits, checkpoints and complex64 E_loc of the whole batch are on the device, as rnnwf_vmc_step leaves them
    if (ns <= chunk && h->family->gradient) h->last_ns = ns;
    return RNNWF_OK;
}
