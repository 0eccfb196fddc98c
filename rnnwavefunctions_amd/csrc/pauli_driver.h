// pauli_driver.h - the host driver of the Pauli-step entry points of every family: rnnwf_pauli_step (pauli.hip), rnnwf_pauli_step_2d
// (mdrnn_pauli.hip) and rnnwf_pauli_step_complex (crnn_pauli.hip).  Per call: validation, the terms (pauli_terms.h), the pass size,
// one scratch allocation sized by the largest pass with the tables uploaded once, the pass loop (observable.h) with the per-pass
// copies of log-ratios, E_loc and moments, and the resident-batch rule.  A family's .hip supplies a policy struct P:
//   kEntry, kCoeff             names in the refusals
//   kElem, kComplex, kOwnLogP  bytes of a value (8 real, 16 complex); complex64 E_loc and four moments; a [ns] piece for the log
//                              psi of the pass's own base pass
//   kThreads                   chains per assembly block
//   kUncommittedInvalid        the code of the "not committed" refusal (observable.h: refuse_uncommitted)
//   refuse(h), precheck(h, samples, ns), positions(h), cells(h), chunk(h, M)     the model refusal; further checks of the caller's
//                              arguments; site -> position map (empty: the same) and cell evaluations of a chain flipped from
//                              position 0 on (pauli_terms.h); chains per pass
//   pass(h, ns, g, sc, keep, sums_host)   the kernels of one pass over the chains in h->bits: log-ratios at sc.lr, E_loc in h->eloc
// pauli_train_steps<P> below is the driver of the device-resident Adam iterations on the same terms (rnnwf_pauli_train_steps,
// rnnwf_pauli_train_steps_2d, rnnwf_pauli_train_steps_complex).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "observable.h"
#include "pauli_terms.h"

namespace rnnwf {

// Scratch of one pass of ns chains in h->renyi; the call's tables lead, at offsets that do not depend on ns
struct PauliScratch {
    size_t mask, order, first, sgn, tmask, coeff, terms, logp, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per term
    PauliScratch(int N, const PauliTerms& g, int64_t ns, size_t elem, bool own_logp, int threads) {
        Carve c;
        const size_t M = (size_t)std::max(g.M, 1), K = (size_t)g.K;
        nblk = (ns + threads - 1) / threads;
        mask = c.take(M * g.W * 4);
        order = c.take(M * 4);
        first = c.take(M * 4);
        sgn = c.take(K * g.W * 4);
        tmask = c.take(K * 4);
        coeff = c.take(K * elem);
        terms = c.take((size_t)N * ns * elem);
        logp = c.take(own_logp ? (size_t)ns * elem : 0);
        tail = c.take(M * ns * elem);
        lr = c.take(M * ns * elem);
        part = c.take(K * nblk * 2 * elem);
        sums = c.take(K * 2 * elem);
        bytes = c.bytes;
    }
};

// coeff: [K] values of P::kElem bytes; out_eloc: [ns] float64 or complex64, 8 bytes either way; term_sums: [K] rows of P::kElem / 4 doubles
template <class P>
int pauli_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const void* coeff, int32_t nterms, const int32_t* samples,
               int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset, double* term_sums, void* out_eloc, double* moments,
               double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck, h->eloc) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = P::refuse(h)) return rc;
    if (int rc = refuse_uncommitted(h, P::kEntry, P::kUncommittedInvalid)) return rc;
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "%s: nterms must be >= 1", P::kEntry);
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: ns must be >= 1", P::kEntry);
    if (!flip || !sign || !coeff || !term_sums)
        return h->fail(RNNWF_ERR_INVALID, "%s: flip, sign, %s and term_sums must be non-null", P::kEntry, P::kCoeff);
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", P::kEntry);
    if (int rc = P::precheck(h, samples, ns)) return rc;
    PauliTerms g;
    const std::vector<int32_t> pos = P::positions(h);
    if (int rc = prepare_pauli_terms(h, P::kEntry, flip, sign, nterms, pos.empty() ? nullptr : pos.data(), P::cells(h), g)) return rc;
    const int N = h->N, K = nterms, M = g.M;
    const size_t E = P::kElem;
    const int64_t chunk = P::chunk(h, M);
    if ((int64_t)K * ((std::min(chunk, ns) + P::kThreads - 1) / P::kThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "%s: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", P::kEntry,
                       P::kThreads);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    // the first pass is the largest: one allocation for the call, the tables uploaded once
    const PauliScratch big(N, g, std::min(chunk, ns), E, P::kOwnLogP, P::kThreads);
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
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.coeff, coeff, (size_t)K * E, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    std::vector<double> total((size_t)K * E / 4, 0.0);
    double mom[4] = {0.0, 0.0, 0.0, 0.0};
    const ChainSource src{samples, seed, step, sample_offset, out_samples};
    if (int rc = for_each_pass(h, src, ns, chunk, 1, total, [&](int64_t s0, int64_t, int64_t n, double* pass_sums) {
            const PauliScratch sc(N, g, n, E, P::kOwnLogP, P::kThreads);
            if (int rc = P::pass(h, n, g, sc, ns <= chunk, pass_sums)) return rc;
            if (out_log_ratio && M)
                RNNWF_HIP(h, hipMemcpy2DAsync((char*)out_log_ratio + s0 * E, (size_t)ns * E, (char*)h->renyi.p + sc.lr, (size_t)n * E,
                                              (size_t)n * E, (size_t)M, hipMemcpyDeviceToHost, h->stream));
            if (out_eloc) RNNWF_HIP(h, hipMemcpyAsync((char*)out_eloc + s0 * 8, h->eloc.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
            if (moments) {                                               // synchronises the stream
                double pm[4];
                if (int rc = run_moments(h, h->eloc.p, n, P::kComplex, pm)) return rc;
                for (int k = 0; k < (P::kComplex ? 4 : 3); ++k) mom[k] += pm[k];
            }
            return 0;
        }))
        return rc;
    memcpy(term_sums, total.data(), total.size() * 8);
    if (moments) memcpy(moments, mom, sizeof mom);
    // one pass: bits, states and E_loc of the whole batch are on the device, as rnnwf_vmc_step leaves them
    keep_resident(h, ns <= chunk ? ns : 0);
    return RNNWF_OK;
}

// K whole Adam iterations on the Hamiltonian of the terms with one host synchronisation behind the last (rnnwf_pauli_train_steps,
// rnnwf_pauli_train_steps_2d, rnnwf_pauli_train_steps_complex; docs/pauli_train.md).  The policy adds to pauli_step's
//   train_pass(h, ns, g, sc, sums_row)   the kernels of one iteration's pass over the chains drawn into h->bits: E_loc in h->eloc,
//                                        the checkpoints kept, the per-term sums into sums_row on the device unless it is nullptr
//                                        (the 2D RNN's sampling base pass has kept every state and log P: its pass starts at the tails)
// A family without a hook table in rnnwf_vmc_gradient (the LSTM, lstm_pauli.hip) brings the steps that go through it - detected by
// their presence (OwnGradient):
//   train_prepare(h)                     train.hip's tables and flat parameters for this model, in train_prepare's place
//   train_gradient(h, ns)                the backward pass on the batch of train_pass, the dW image left in h->gradW
// and, on an error inside its loop, has the applied updates counted (train_steps_failed).
// Per call: the refusals, the terms derived and uploaded once, one scratch allocation (the tables, one pass, then the [K][nterms]
// table of per-term sums), train.hip's tables and flat parameters.  Per iteration k, nothing waiting for the host: the family's base
// pass drawing at step index step0 + k, train_pass, the moments into row k of train.hip's pinned table, the gradient reading them on
// the device, Adam with learning_rates[k] and the re-pack of every weight image.  Neither the gradient nor the update touches
// h->renyi, so the tables stay where they were uploaded.  out_eloc: [ns] E_loc of the last iteration's batch, or nullptr.
template <class P, class = void> struct OwnGradient : std::false_type {};
template <class P> struct OwnGradient<P, std::void_t<decltype(&P::train_gradient)>> : std::true_type {};

template <class P>
int pauli_train_steps(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const void* coeff, int32_t nterms, int32_t K, int64_t ns,
                      uint64_t seed, uint64_t step0, int64_t sample_offset, const double* learning_rates, double beta1, double beta2,
                      double epsilon, double* moments, double* term_sums, void* out_eloc) {
    // everything is validated before anything is touched: a refused call leaves the resident batch, the parameters and Adam's state
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = P::refuse(h)) return rc;
    if (int rc = refuse_uncommitted(h, P::kEntry, P::kUncommittedInvalid)) return rc;
    if (h->comm) return h->fail(RNNWF_ERR_INVALID, "%s: runs in one process on one GPU, this handle has a communicator", P::kEntry);
    if constexpr (!OwnGradient<P>::value)
        if (int rc = require_gradient(h, P::kEntry)) return rc;
    if (K < 1 || K > kTrainMaxSteps) return h->fail(RNNWF_ERR_INVALID, "%s: K must be 1..%d", P::kEntry, kTrainMaxSteps);
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "%s: nterms must be >= 1", P::kEntry);
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: numsamples must be >= 1", P::kEntry);
    if (!flip || !sign || !coeff || !learning_rates || !moments)
        return h->fail(RNNWF_ERR_INVALID, "%s: flip, sign, %s, learning_rates and moments must be non-null", P::kEntry, P::kCoeff);
    if (sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", P::kEntry);
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(learning_rates[k])) return h->fail(RNNWF_ERR_INVALID, "%s: learning_rates[%d] must be finite", P::kEntry, k);
    if (int rc = P::precheck(h, nullptr, ns)) return rc;
    PauliTerms g;
    const std::vector<int32_t> pos = P::positions(h);
    if (int rc = prepare_pauli_terms(h, P::kEntry, flip, sign, nterms, pos.empty() ? nullptr : pos.data(), P::cells(h), g)) return rc;
    const int N = h->N;
    const size_t E = P::kElem;
    if (ns > P::chunk(h, g.M))
        return h->fail(RNNWF_ERR_NOMEM, "%s: %lld samples exceed the state budget of one pass; split the batch", P::kEntry, (long long)ns);
    if ((int64_t)nterms * ((ns + P::kThreads - 1) / P::kThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "%s: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", P::kEntry,
                       P::kThreads);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    if constexpr (OwnGradient<P>::value) {
        if (int rc = P::train_prepare(h)) return rc;
    } else {
        if (int rc = train_prepare(h)) return rc;
    }
    const PauliScratch sc(N, g, ns, E, P::kOwnLogP, P::kThreads);
    const size_t row = (size_t)nterms * 2 * E;                // a (nterms, 2) real or (nterms, 4) complex row of per-term sums
    if (int rc = ensure(h, h->renyi, sc.bytes + (term_sums ? (size_t)K * row : 0))) return rc;
    if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * ns * 4)) return rc;
    char* buf = (char*)h->renyi.p;
    if (g.M) {
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.order, g.order.data(), (size_t)g.M * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + sc.first, g.first.data(), (size_t)g.M * 4, hipMemcpyHostToDevice, h->stream));
    }
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.sgn, g.sgn.data(), g.sgn.size() * 4, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.tmask, g.tmask.data(), (size_t)nterms * 4, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(buf + sc.coeff, coeff, (size_t)nterms * E, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));           // the set-up's: the tables leave the host's vectors before the iterations start
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    int rc = 0, applied = 0;
    for (int k = 0; k < K && !rc; ++k) {
        const Draw d{seed, step0 + (uint64_t)k, sample_offset};
        rc = h->family->base(h, ns, &d);
        if (!rc) rc = P::train_pass(h, ns, g, sc, term_sums ? (double*)(buf + sc.bytes + (size_t)k * row) : nullptr);
        if (rc) break;
        h->moments_direct = train_moments_row(h, k);          // as rnnwf_train_steps: the moments kernel writes the pinned row itself
        rc = run_moments(h, h->eloc.p, ns, P::kComplex, nullptr);
        h->moments_direct = nullptr;
        if (rc) break;
        if constexpr (OwnGradient<P>::value) {
            rc = P::train_gradient(h, ns);
        } else {
            keep_resident(h, ns);                             // the batch the gradient reads
            rc = grad_device(h, 0.0, 0.0, 0.0, (const double*)h->moments.p, nullptr);
        }
        if (!rc) rc = train_adam_update(h, k, learning_rates[k], beta1, beta2, epsilon);
        if (!rc) ++applied;
    }
    if (!rc && term_sums && hipMemcpyAsync(term_sums, buf + sc.bytes, (size_t)K * row, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = h->fail(RNNWF_ERR_HIP, "%s: download of the per-term sums failed", P::kEntry);
    if (!rc && out_eloc && hipMemcpyAsync(out_eloc, h->eloc.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = h->fail(RNNWF_ERR_HIP, "%s: download of E_loc failed", P::kEntry);
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = h->fail(RNNWF_ERR_HIP, "%s: stream synchronisation failed", P::kEntry);
    h->last_ns = 0;                       // the resident batch belongs to the weights before the last update
    if (rc) {
        if constexpr (OwnGradient<P>::value) train_steps_failed(h, applied);
        return rc;
    }
    train_steps_done(h, K, moments);
    return RNNWF_OK;
}

}  // namespace rnnwf
