// pauli_stack.hip - rnnwf_pauli_step_stack and rnnwf_pauli_train_steps_stack (include/rnnwf.h): expectation values of Pauli strings,
// the local energy of any real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient) and device-resident
// Adam training on it, for STACKED layers of the positive GRU models (GRU1D float32, GRU1D_F64 float64 on the raster path; 2..4
// layers, every stack rnnwf_create accepts); kernels in stack_chain_kernels.h and, from the log-ratios on, pauli_kernels.h and
// pauli_train_kernels.h; the method in docs/pauli_stack.md.  The drivers are pauli_driver.h's, over the policies below.
//
// Per pass of whole 16-chain blocks (the state budget, at the stack's N checkpoint sites of NL layers each): spins (the caller's, or
// drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass with checkpoints on the one-wave MFMA stack kernel
// (prnn_ml_base_kernel, whatever kernel rnnwf_vmc_step takes for this handle) -> site terms and flip-mask tails -> log-ratios,
// per-term sums of v and v^2, E_loc and its moments.  The sums of the passes are added on the host in pass order.  A call that ran
// in one pass leaves its batch (bits, checkpoints, E_loc) resident for rnnwf_vmc_gradient.
#include "pauli_driver.h"
#include "pauli_kernels.h"
#include "pauli_train_kernels.h"
#include "stack_observable.h"

using namespace rnnwf;

namespace {

struct StackPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_step_stack";
    static constexpr const char* kCoeff = "coeff";
    static constexpr size_t kElem = 8;
    static constexpr bool kComplex = false, kOwnLogP = true, kUncommittedInvalid = false;
    static constexpr int kThreads = kPauliThreads;
    static int refuse(rnnwf_handle* h) { return stack_refuse(h, kEntry, "rnnwf_pauli_step"); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // whole 16-chain blocks within the state budget.  Per block the stack's checkpoints of all N sites and, beside them, the terms
    // (N x 16 x 8 bytes), log P (16 x 8), the tails and log-ratios (2 x M x 16 x 8) and E_loc (16 x 8)
    static int64_t chunk(rnnwf_handle* h, int M) {
        const size_t per_block = (size_t)h->N * stack_hck_bytes_per_block(h) + (size_t)(h->N + 2 + 2 * M) * kChains * 8;
        return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block)) * kChains;
    }
    static int tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep);
    static int pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host);
};

// rnnwf_pauli_train_steps_stack: the same stacks, terms, pass size and kernels up to the tails, the table-reading assembly behind them
struct StackPauliTrain : StackPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_train_steps_stack";
    static int refuse(rnnwf_handle* h) { return stack_refuse(h, kEntry, "rnnwf_pauli_train_steps"); }
    static int train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row);
};

// the front of a pass over the ns chains packed in h->bits: base pass with checkpoints of all N sites (log P at sc.logp), the
// replayed site terms (sc.terms) and the tail of every (mask, chain) (sc.tail)
int StackPauli::tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep) {
    const int M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    if (M > 0 || keep) {
        const int64_t nsb = (ns + kChains - 1) / kChains;
        if (int rc = ensure(h, h->hck, (size_t)h->N * nsb * stack_hck_bytes_per_block(h))) return rc;
        PrnnArgs b = prnn_base_args(h, ns);
        b.bits = (uint32_t*)h->bits.p;
        b.hck = h->hck.p;
        b.out_lp = (double*)(buf + sc.logp);
        if (int rc = prnn_stack_base(h, b)) return rc;
    }
    if (M == 0) return 0;
    const ChainArgs c = chain_args(h, ns);
    SwapArgs t{c};
    t.terms = (double*)(buf + sc.terms);
    MaskArgs a{c};
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)M * a.nsb;
    int rc = 0;
    with_stack(h, [&](auto k) {
        using K = decltype(k);
        using S = typename K::S;
        if (g.replay)
            rc = launch_persistent(h, kTimerBase, prnn_ml_site_terms_kernel<typename K::T, K::NFULL, K::NL, K::WAVES>, K::WAVES * 64,
                                   S::LDS_BYTES, t.nsb, K::WAVES, t);
        if (!rc)
            rc = launch_persistent(h, kTimerFlip, prnn_ml_masked_tail_kernel<typename K::T, K::NFULL, K::NL, K::WAVES>, K::WAVES * 64,
                                   S::LDS_BYTES, a.ntiles, K::WAVES, a);
        if (!rc) h->work[1] += (double)a.nsb * g.steps * K::mfma_flops_per_step();
    });
    if (rc) return rc;
    h->work[0] += (double)ns * g.steps;        // sum over masks of N - f stack steps per chain
    return 0;
}

// one pass over the ns chains packed in h->bits: sums_host (K, 2) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
// keep: the pass is the whole call, its checkpoints are left for rnnwf_vmc_gradient (diagonal terms alone need no base pass otherwise)
int StackPauli::pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host) {
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
        pauli_term_kernel<<<(unsigned)(K * sc.nblk), kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, lr, g.W, ns, sc.nblk,
                                                                                   (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)K, kPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
        pauli_eloc_kernel<<<(unsigned)sc.nblk, kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, (const double*)(buf + sc.coeff), lr, K, g.W,
                                                                             ns, (double*)h->eloc.p);
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)K * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// one iteration's pass of rnnwf_pauli_train_steps_stack over the ns chains drawn into h->bits: the ratios r[M][ns] in the log-ratios'
// place (sc.lr), E_loc in h->eloc, the checkpoints kept for the gradient; sums_row: the iteration's (K, 2) row of the call's table on
// the device, or nullptr - then the per-term kernels are not launched
int StackPauliTrain::train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = tails(h, ns, g, sc, true)) return rc;
    char* buf = (char*)h->renyi.p;
    const double* ratio = (const double*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
    const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
    if (M > 0)
        if (int rc = timed_launch(h, kTimerAssembly, pauli_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                  (const double*)(buf + sc.tail), (const double*)(buf + sc.terms), (const double*)(buf + sc.logp),
                                  (const int32_t*)(buf + sc.first), N, ns, (double*)(buf + sc.lr)))
            return rc;
    if (sums_row) {
        TimedLaunch tl(h, kTimerAssembly);
        pauli_table_term_kernel<<<(unsigned)(K * sc.nblk), kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, ratio, g.W, ns, sc.nblk,
                                                                                         (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)K, kPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, sums_row);
        RNNWF_HIP(h, hipGetLastError());
    }
    return timed_launch(h, kTimerAssembly, pauli_table_eloc_kernel, (unsigned)sc.nblk, kPauliThreads, 0, bits, sgn, tmask,
                        (const double*)(buf + sc.coeff), ratio, K, g.W, ns, (double*)h->eloc.p);
}

}  // namespace

extern "C" int rnnwf_pauli_train_steps_stack(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                             int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                             const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                             double* term_sums, double* out_eloc) {
    return pauli_train_steps<StackPauliTrain>(h, flip, sign, coeff, nterms, K, numsamples, seed, step0, sample_offset, learning_rates, beta1,
                                              beta2, epsilon, moments, term_sums, out_eloc);
}

extern "C" int rnnwf_pauli_step_stack(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                      const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                      double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    return pauli_step<StackPauli>(h, flip, sign, coeff, nterms, samples, ns, seed, step, sample_offset, term_sums, out_eloc, moments,
                                  out_log_ratio, out_samples);
}
