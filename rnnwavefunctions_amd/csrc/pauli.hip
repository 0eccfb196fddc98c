// pauli.hip - host driver of rnnwf_pauli_step (include/rnnwf.h): expectation values of Pauli strings and the local energy of any
// real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient), for the positive GRU models (GRU1D,
// GRU1D_F64, one layer); kernels in pauli_kernels.h and chain_kernels.h (prnn_masked_tail_kernel, not PAIRED), the
// method in docs/pauli.md.  The driver is pauli_driver.h's, over the policy below; the launch table, refusals, base pass and pass size
// are observable.h's.
//
// Per call: the masks are checked and packed into words, the terms grouped by flip mask (a mask shared by several terms is
// evaluated once) and the distinct masks sorted longest chain first.  Per pass of whole 16-chain blocks (the state budget, as
// renyi_regions.hip): spins (the caller's, or drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass on the one-wave
// kernel with checkpoints -> site terms and flip-mask tails -> log-ratios, per-term sums of v and v^2, E_loc and its moments.  The
// sums of the passes are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, checkpoints, E_loc)
// resident for rnnwf_vmc_gradient.
//
// rnnwf_pauli_train_steps (docs/pauli_train.md) runs K Adam iterations on the same terms through pauli_driver.h's pauli_train_steps:
// the same passes up to the tails (GruPauli::tails), then pauli_train_kernels.h's ratio table and the kernels that read it.
#include "pauli_driver.h"
#include "pauli_kernels.h"
#include "pauli_train_kernels.h"

using namespace rnnwf;

namespace {

struct GruPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_step";
    static constexpr const char* kCoeff = "coeff";
    static constexpr size_t kElem = 8;
    static constexpr bool kComplex = false, kOwnLogP = true, kUncommittedInvalid = false;
    static constexpr int kThreads = kPauliThreads;
    static int refuse(rnnwf_handle* h) { return observable_refuse(h, kEntry); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // per block, beside the checkpoints, the terms (N x 16 x 8 bytes), log P (16 x 8), the tails and log-ratios (2 x M x 16 x 8) and
    // E_loc (16 x 8)
    static int64_t chunk(rnnwf_handle* h, int M) { return blocks_per_pass(h, (size_t)(h->N + 2 + 2 * M) * kChains * 8) * kChains; }
    static int tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep);
    static int pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host);
};

// rnnwf_pauli_train_steps: the same model, terms, pass size and kernels up to the tails, the table-reading assembly behind them
struct GruPauliTrain : GruPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_train_steps";
    static int refuse(rnnwf_handle* h) { return observable_refuse(h, kEntry); }
    static int train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row);
};

// the front of a pass over the ns chains packed in h->bits: base pass with checkpoints (log P at sc.logp), the replayed site terms
// (sc.terms) and the tail of every (mask, chain) (sc.tail)
int GruPauli::tails(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep) {
    const int M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    if (M > 0 || keep)
        if (int rc = observable_base(h, ns, (double*)(buf + sc.logp))) return rc;
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
    with_gru1(h, [&](auto k) {
        using L = decltype(k);
        if (g.replay) rc = launch_waves(h, k, kTimerBase, prnn_site_terms_kernel<typename L::T, L::NFULL, L::WAVES>, t.nsb, t);     // N >= 2
        if (!rc) rc = launch_waves(h, k, kTimerFlip, prnn_masked_tail_kernel<typename L::T, L::NFULL, L::WAVES, false>, a.ntiles, a);
        if (!rc) h->work[1] += (double)a.nsb * g.steps * L::mfma_flops_per_step();
    });
    if (rc) return rc;
    h->work[0] += (double)ns * g.steps;        // sum over masks of N - f cell evaluations per chain
    return 0;
}

// one pass over the ns chains packed in h->bits: sums_host (K, 2) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
// keep: the pass is the whole call, its checkpoints are left for rnnwf_vmc_gradient (diagonal terms alone need no base pass otherwise)
int GruPauli::pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = tails(h, ns, g, sc, keep)) return rc;
    char* buf = (char*)h->renyi.p;
    double* lr = (double*)(buf + sc.lr);
    const ChainArgs c = chain_args(h, ns);
    if (M > 0)
        if (int rc = timed_launch(h, kTimerAssembly, pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                  (const double*)(buf + sc.tail), (const double*)(buf + sc.terms), (const double*)(buf + sc.logp),
                                  (const int32_t*)(buf + sc.first), N, ns, lr))
            return rc;
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

// one iteration's pass of rnnwf_pauli_train_steps over the ns chains drawn into h->bits: the ratios r[M][ns] in the log-ratios' place
// (sc.lr), E_loc in h->eloc, the checkpoints kept for the gradient; sums_row: the iteration's (K, 2) row of the call's table on the
// device, or nullptr - then the per-term kernels are not launched
int GruPauliTrain::train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row) {
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

extern "C" int rnnwf_pauli_train_steps(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                       int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                       const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                       double* term_sums, double* out_eloc) {
    return pauli_train_steps<GruPauliTrain>(h, flip, sign, coeff, nterms, K, numsamples, seed, step0, sample_offset, learning_rates, beta1,
                                            beta2, epsilon, moments, term_sums, out_eloc);
}

extern "C" int rnnwf_pauli_step(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    return pauli_step<GruPauli>(h, flip, sign, coeff, nterms, samples, ns, seed, step, sample_offset, term_sums, out_eloc, moments,
                                out_log_ratio, out_samples);
}
