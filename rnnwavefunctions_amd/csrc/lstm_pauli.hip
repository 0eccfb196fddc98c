// lstm_pauli.hip - rnnwf_pauli_step_lstm and rnnwf_lstm_pauli_gradient_step (include/rnnwf.h): expectation values of Pauli strings,
// the local energy of any real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient) and the gradient of
// its VMC cost, for the LSTM wave function over the raster path (LSTM1D_F64, one layer, 1..68 units, float64); kernels in
// lstm_pauli_kernels.h and, from the log-ratios on, pauli_kernels.h; the method in docs/pauli_lstm.md.  The driver of
// rnnwf_pauli_step_lstm is pauli_driver.h's, over the policy below; the launch class and the refusals are lstm_observable.h's.
//
// Per pass of whole 16-chain blocks (the state budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) ->
// teacher-forced base pass with checkpoints, log P and site terms (lstm_site_terms_kernel) -> flip-mask tails
// (lstm_masked_tail_kernel) -> log-ratios, per-term sums of v and v^2, E_loc and its moments.  The sums of the passes are added on
// the host in pass order.  The LSTM has no hook in rnnwf_vmc_gradient, so no batch is claimed resident; the fused gradient step runs
// the LSTM's backward pass (lstm_grad.hip) on the checkpoints of its one pass itself.
#include "lstm_observable.h"
#include "pauli_driver.h"
#include "pauli_kernels.h"

using namespace rnnwf;

namespace {

struct LstmPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_step_lstm";
    static constexpr const char* kCoeff = "coeff";
    static constexpr size_t kElem = 8;
    static constexpr bool kComplex = false, kOwnLogP = true, kUncommittedInvalid = false;
    static constexpr int kThreads = kPauliThreads;
    static int refuse(rnnwf_handle* h) { return lstm_pauli_refuse(h, kEntry); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }      // masks by chain position, the column of `samples`
    static int cells(const rnnwf_handle* h) { return h->N; }
    // whole 16-chain blocks within the state budget.  Per block the checkpoints (h, c) of N - 1 sites and, beside them, the terms
    // (N x 16 x 8 bytes), log P (16 x 8), the tails and log-ratios (2 x M x 16 x 8) and E_loc (16 x 8)
    static int64_t chunk(rnnwf_handle* h, int M) {
        const size_t per_block = (size_t)std::max(h->N - 1, 1) * hck_bytes_per_block(h) + (size_t)(h->N + 2 + 2 * M) * kChains * 8;
        return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block)) * kChains;
    }
    static int tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep);
    static int assemble(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_dev);
    static int pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host);
};

// rnnwf_lstm_pauli_train_steps: the model, terms, pass size and kernels of rnnwf_lstm_pauli_gradient_step's pass, the per-term sums
// written into the call's table on the device; the gradient and train.hip's state through the LSTM's own road (pauli_driver.h:
// OwnGradient)
struct LstmPauliTrain : LstmPauli {
    static constexpr const char* kEntry = "rnnwf_lstm_pauli_train_steps";
    static int refuse(rnnwf_handle* h) {
        if (h->model != RNNWF_MODEL_LSTM1D_F64)
            return h->fail(RNNWF_ERR_INVALID, "%s: needs an LSTM1D_F64 handle, this one is %s (its device-resident training on Pauli terms: "
                                              "rnnwf_pauli_train_steps and its siblings)", kEntry, model_name(h->model));
        if (int rc = lstm_pauli_refuse(h, kEntry)) return rc;
        if (h->comm || h->nranks > 1 || h->reduce_in_step)
            return h->fail(RNNWF_ERR_INVALID, "%s: single process only (the weights are centred with this handle's moments), this handle "
                                              "has a communicator", kEntry);
        return 0;
    }
    static int train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row) {
        return assemble(h, ns, g, sc, true, sums_row);
    }
    static int train_prepare(rnnwf_handle* h) { return train_prepare_lstm(h); }
    static int train_gradient(rnnwf_handle* h, int64_t ns) { return lstm_grad_queue(h, kEntry, ns, nullptr, false); }
};

// the front of a pass over the ns chains packed in h->bits: base pass with checkpoints (log P at sc.logp, site terms at sc.terms) and
// the tail of every (mask, chain) (sc.tail).  Diagonal terms alone (M = 0) run no recurrent kernel unless the checkpoints are kept.
int LstmPauli::tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep) {
    const int M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    if (M == 0 && !keep) return 0;
    char* buf = (char*)h->renyi.p;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(h->N - 1, 1) * nsb * hck_bytes_per_block(h))) return rc;
    LstmTermsArgs b{};
    b.wimg = h->wimg.p;
    b.N = h->N;
    b.ns = ns;
    b.nsb = nsb;
    b.bits = (const uint32_t*)h->bits.p;
    b.hck = (double*)h->hck.p;
    b.terms = (double*)(buf + sc.terms);
    b.out_lp = (double*)(buf + sc.logp);
    MaskArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.W = (h->N + 31) / 32;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = b.bits;
    a.hck = h->hck.p;
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)M * nsb;
    int rc = 0;
    with_lpauli(h, [&](auto k) {
        using K = decltype(k);
        rc = K::base(h, b);
        if (!rc && M > 0) rc = K::tails(h, a);
        if (!rc) h->work[1] += (double)nsb * g.steps * K::mfma_flops_per_step();
    });
    if (rc) return rc;
    h->work[0] += (double)ns * g.steps;        // sum over masks of N - f cell evaluations per chain
    return 0;
}

// one pass over the ns chains packed in h->bits: the log-ratios stay in h->renyi, E_loc in h->eloc; sums_dev: where on the device the
// (K, 2) sums of this pass go, or nullptr - then the per-term kernels are not launched.  keep: the checkpoints are wanted whatever the
// terms (the fused gradient step, the training iterations)
int LstmPauli::assemble(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_dev) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = tails(h, ns, g, sc, keep)) return rc;
    char* buf = (char*)h->renyi.p;
    double* lr = (double*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    if (M > 0)
        if (int rc = timed_launch(h, kTimerAssembly, pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                  (const double*)(buf + sc.tail), (const double*)(buf + sc.terms), (const double*)(buf + sc.logp),
                                  (const int32_t*)(buf + sc.first), N, ns, lr))
            return rc;
    {
        TimedLaunch tl(h, kTimerAssembly);
        const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
        const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
        if (sums_dev) {
            pauli_term_kernel<<<(unsigned)(K * sc.nblk), kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, lr, g.W, ns, sc.nblk,
                                                                                       (double*)(buf + sc.part));
            RNNWF_HIP(h, hipGetLastError());
            renyi_sums_kernel<<<(unsigned)K, kPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, sums_dev);
            RNNWF_HIP(h, hipGetLastError());
        }
        pauli_eloc_kernel<<<(unsigned)sc.nblk, kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, (const double*)(buf + sc.coeff), lr, K, g.W,
                                                                             ns, (double*)h->eloc.p);
        RNNWF_HIP(h, hipGetLastError());
    }
    return 0;
}

// the same with the sums copied to the host: sums_host (K, 2) of this pass, or nullptr
int LstmPauli::pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host) {
    char* buf = (char*)h->renyi.p;
    if (int rc = assemble(h, ns, g, sc, keep, sums_host ? (double*)(buf + sc.sums) : nullptr)) return rc;
    if (sums_host) RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)g.K * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_pauli_step_lstm(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                     const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                     double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    // keep = false whatever the batch: no entry reads a resident LSTM batch (lstm_family() has no gradient hook), so a Hamiltonian of
    // diagonal terms alone runs no recurrent kernel
    struct Step : LstmPauli {
        static int pass(rnnwf_handle* h, int64_t n, const PauliTerms& g, const PauliScratch& sc, bool, double* sums_host) {
            return LstmPauli::pass(h, n, g, sc, false, sums_host);
        }
    };
    return pauli_step<Step>(h, flip, sign, coeff, nterms, samples, ns, seed, step, sample_offset, term_sums, out_eloc, moments,
                            out_log_ratio, out_samples);
}

// rnnwf_pauli_step_lstm's one pass on drawn samples with its moments written into the pinned row by the moments kernel, then the
// LSTM's backward pass (lstm_grad.hip: lstm_grad_queue) on the checkpoints the pass just wrote: one host synchronisation behind it all
extern "C" int rnnwf_lstm_pauli_gradient_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff,
                                              int32_t nterms, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                              double* moments, double* term_sums, int32_t* out_samples, double* out_eloc) {
    constexpr const char* kEntry = "rnnwf_lstm_pauli_gradient_step";
    using P = LstmPauli;
    // everything is validated before anything is touched: a refused call leaves an earlier batch, the parameters and the gradient
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = lstm_pauli_refuse(h, kEntry)) return rc;
    if (int rc = refuse_uncommitted(h, kEntry, false)) return rc;
    if (h->comm || h->nranks > 1 || h->reduce_in_step)
        return h->fail(RNNWF_ERR_INVALID, "%s: single process only (the weights are centred with this handle's moments); with a "
                                          "communicator use rnnwf_pauli_step_lstm and rnnwf_lstm_gradient with globally centred weights", kEntry);
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "%s: nterms must be >= 1", kEntry);
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: numsamples must be >= 1", kEntry);
    if (!flip || !sign || !coeff || !moments) return h->fail(RNNWF_ERR_INVALID, "%s: flip, sign, coeff and moments must be non-null", kEntry);
    if (sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", kEntry);
    PauliTerms g;
    if (int rc = prepare_pauli_terms(h, kEntry, flip, sign, nterms, nullptr, P::cells(h), g)) return rc;
    const int N = h->N;
    if (ns > P::chunk(h, g.M))
        return h->fail(RNNWF_ERR_NOMEM, "%s: %lld samples exceed the state budget of one pass; split the batch", kEntry, (long long)ns);
    if ((int64_t)nterms * ((ns + P::kThreads - 1) / P::kThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "%s: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", kEntry, P::kThreads);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const PauliScratch sc(N, g, ns, P::kElem, P::kOwnLogP, P::kThreads);
    if (int rc = ensure(h, h->renyi, sc.bytes)) return rc;
    if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * ns * 4)) return rc;
    char* buf = (char*)h->renyi.p;
    if (g.M) {
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.order, g.order.data(), (size_t)g.M * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.first, g.first.data(), (size_t)g.M * 4, hipMemcpyHostToDevice, h->stream));
    }
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.sgn, g.sgn.data(), g.sgn.size() * 4, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.tmask, g.tmask.data(), (size_t)nterms * 4, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.coeff, coeff, (size_t)nterms * P::kElem, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));           // the set-up's: the tables leave the host's vectors before the step starts
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    const Draw d{seed, step, sample_offset};
    if (int rc = h->family->base(h, ns, &d)) return rc;      // rnnwf_sample's draw
    if (out_samples)
        if (int rc = unpack_and_download(h, h->bits, ns, out_samples, nullptr)) return rc;
    if (int rc = P::pass(h, ns, g, sc, true, term_sums)) return rc;
    if (out_eloc) RNNWF_HIP(h, hipMemcpyAsync(out_eloc, h->eloc.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream));
    h->moments_direct = (double*)h->pinned_dev;       // the moments kernel writes the step's pinned row as well as h->moments
    const int rc_mom = run_moments(h, h->eloc.p, ns, false, nullptr);
    h->moments_direct = nullptr;
    if (rc_mom) return rc_mom;
    if (int rc = lstm_grad_queue(h, kEntry, ns, nullptr)) return rc;
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(moments, h->pinned, 4 * sizeof(double));
    lstm_grad_finish(h);
    return RNNWF_OK;
}

// K whole Adam iterations on the Hamiltonian of the terms with one host synchronisation: rnnwf_pauli_train_steps for the LSTM
// (pauli_driver.h: pauli_train_steps over LstmPauliTrain; docs/lstm.md, "Device-resident training")
extern "C" int rnnwf_lstm_pauli_train_steps(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                            int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                            const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                            double* term_sums, double* out_eloc) {
    return pauli_train_steps<LstmPauliTrain>(h, flip, sign, coeff, nterms, K, numsamples, seed, step0, sample_offset, learning_rates, beta1,
                                             beta2, epsilon, moments, term_sums, out_eloc);
}
