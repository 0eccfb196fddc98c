// crnn_pauli.hip - host driver of rnnwf_pauli_step_complex (include/rnnwf.h): expectation values of Pauli strings and the local
// energy of any spin-1/2 Hamiltonian given as terms (flip mask, sign mask, complex coefficient), for the complex RNN with the U(1)
// mask (CRNN_U1, one layer); kernels in crnn_pauli_kernels.h, the method in docs/pauli_complex.md.  The driver is
// pauli_driver.h's, over the policy below; the launch table, refusal, base pass, pass size and sector check are crnn_observable.h's.
//
// Per call: the masks are checked and packed into words, the terms grouped by flip mask (a mask shared by several terms is
// evaluated once) and the distinct masks sorted longest chain first.  Per pass of whole 16-chain blocks (the state budget): spins
// (the caller's, or drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints
// -> site terms and flip-mask tails -> complex log-ratios, per-term sums, E_loc (complex64) and its moments.  The sums of the passes
// are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, checkpoints, E_loc) resident for
// rnnwf_vmc_gradient.
//
// rnnwf_pauli_train_steps_complex (docs/pauli_train.md) runs K Adam iterations on the same terms through pauli_driver.h's
// pauli_train_steps: the same passes up to the tails (CrnnPauli::tails), then crnn_pauli_train_kernels.h's ratio table and the kernels
// that read it.
#include "crnn_observable.h"
#include "crnn_pauli_kernels.h"
#include "crnn_pauli_train_kernels.h"
#include "pauli_driver.h"

using namespace rnnwf;

namespace {

struct CrnnPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_step_complex";
    static constexpr const char* kCoeff = "coeff_re_im";
    static constexpr size_t kElem = 16;
    static constexpr bool kComplex = true, kOwnLogP = true, kUncommittedInvalid = false;
    static constexpr int kThreads = kCPauliThreads;
    static int refuse(rnnwf_handle* h) { return crnn_refuse(h, kEntry, "rnnwf_pauli_step", "rnnwf_pauli_step_2d"); }
    static int precheck(rnnwf_handle* h, const int32_t* samples, int64_t ns) {
        if (h->N < 2) return h->fail(RNNWF_ERR_INVALID, "%s: needs a chain of at least two sites", kEntry);
        // the caller's chains must lie in the sector: their own log psi is -inf otherwise
        return samples ? crnn_check_sector(h, kEntry, samples, ns) : 0;
    }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // per block, beside the checkpoints, the terms (N x 16 x 16 bytes), the base pass's totals (16 x 16), the tails and log-ratios
    // (2 x M x 16 x 16) and E_loc (16 x 8)
    static int64_t chunk(rnnwf_handle* h, int M) {
        return crnn_blocks_per_pass(h, (size_t)(h->N + 1 + 2 * M) * kChains * 16 + kChains * 8) * kChains;
    }
    static int tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep);
    static int pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host);
};

// rnnwf_pauli_train_steps_complex: the same model, terms, pass size and kernels up to the tails, the table-reading assembly behind them
struct CrnnPauliTrain : CrnnPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_train_steps_complex";
    static int refuse(rnnwf_handle* h) { return crnn_refuse(h, kEntry, "rnnwf_pauli_train_steps", "rnnwf_pauli_step_2d"); }
    static int precheck(rnnwf_handle* h, const int32_t*, int64_t) {
        return h->N < 2 ? h->fail(RNNWF_ERR_INVALID, "%s: needs a chain of at least two sites", kEntry) : 0;
    }
    static int train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row);
};

// the front of a pass over the ns chains packed in h->bits: base pass with checkpoints (log psi at sc.logp), the replayed site terms
// (sc.terms) and the tail of every (mask, chain) (sc.tail)
int CrnnPauli::tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep) {
    const int N = h->N, M = g.M;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->eloc, (size_t)ns * sizeof(float2))) return rc;
    char* buf = (char*)h->renyi.p;
    if (M > 0 || keep)
        if (int rc = crnn_observable_base(h, ns, (double2*)(buf + sc.logp))) return rc;
    if (M == 0) return 0;
    CPauliArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.W = g.W;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
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
    return 0;
}

// one pass over the ns chains packed in h->bits: sums_host (K, 4) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
// keep: the pass is the whole call, its checkpoints are left for rnnwf_vmc_gradient (diagonal terms alone need no base pass otherwise)
int CrnnPauli::pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = tails(h, ns, g, sc, keep)) return rc;
    char* buf = (char*)h->renyi.p;
    double2* lr = (double2*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    if (M > 0)
        if (int rc = timed_launch(h, kTimerAssembly, crnn_pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kCPauliThreads, 0,
                                  (const double2*)(buf + sc.tail), (const double2*)(buf + sc.terms), (const double2*)(buf + sc.logp),
                                  (const int32_t*)(buf + sc.first), N, ns, lr))
            return rc;
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

// one iteration's pass of rnnwf_pauli_train_steps_complex over the ns chains drawn into h->bits: the ratios r[M][ns] in the
// log-ratios' place (sc.lr), E_loc in h->eloc, the checkpoints kept for the gradient; sums_row: the iteration's (K, 4) row of the
// call's table on the device, or nullptr - then the per-term kernels are not launched
int CrnnPauliTrain::train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = tails(h, ns, g, sc, true)) return rc;
    char* buf = (char*)h->renyi.p;
    const double2* ratio = (const double2*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
    const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
    if (M > 0)
        if (int rc = timed_launch(h, kTimerAssembly, crnn_pauli_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kCPauliThreads, 0,
                                  (const double2*)(buf + sc.tail), (const double2*)(buf + sc.terms), (const double2*)(buf + sc.logp),
                                  (const int32_t*)(buf + sc.first), N, ns, (double2*)(buf + sc.lr)))
            return rc;
    if (sums_row) {
        TimedLaunch tl(h, kTimerAssembly);
        crnn_pauli_table_term_kernel<<<(unsigned)(K * sc.nblk), kCPauliThreads, 0, h->stream>>>(bits, sgn, tmask, ratio, g.W, ns, sc.nblk,
                                                                                               (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        // rows (term, half): half 0 = (sum Re v, sum Im v), half 1 = the sums of their squares
        renyi_sums_kernel<<<(unsigned)(2 * K), kCPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, sums_row);
        RNNWF_HIP(h, hipGetLastError());
    }
    return timed_launch(h, kTimerAssembly, crnn_pauli_table_eloc_kernel, (unsigned)sc.nblk, kCPauliThreads, 0, bits, sgn, tmask,
                        (const double2*)(buf + sc.coeff), ratio, K, g.W, ns, (float2*)h->eloc.p);
}

}  // namespace

extern "C" int rnnwf_pauli_train_steps_complex(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff_re_im,
                                               int32_t nterms, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0,
                                               int64_t sample_offset, const double* learning_rates, double beta1, double beta2,
                                               double epsilon, double* moments, double* term_sums, float* out_eloc_re_im) {
    return pauli_train_steps<CrnnPauliTrain>(h, flip, sign, coeff_re_im, nterms, K, numsamples, seed, step0, sample_offset, learning_rates,
                                             beta1, beta2, epsilon, moments, term_sums, out_eloc_re_im);
}

// term_sums: the device rows are (term, half) x (re, im): {sum Re v, sum Im v, sum (Re v)^2, sum (Im v)^2} per term already
extern "C" int rnnwf_pauli_step_complex(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff_re_im, int32_t nterms,
                                        const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                        double* term_sums, float* out_eloc_re_im, double* moments, double* out_log_ratio,
                                        int32_t* out_samples) {
    return pauli_step<CrnnPauli>(h, flip, sign, coeff_re_im, nterms, samples, ns, seed, step, sample_offset, term_sums, out_eloc_re_im,
                                 moments, out_log_ratio, out_samples);
}
