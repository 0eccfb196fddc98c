// mdrnn_pauli.hip - rnnwf_pauli_step_2d (include/rnnwf.h): expectation values of Pauli strings and the local energy of any
// real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient), for the 2D RNN (MDRNN2D, float64);
// kernels in mdrnn_pauli_kernels.h and, from the log-ratios on, pauli_kernels.h; the method in docs/pauli_2d.md.  The driver is
// pauli_driver.h's, over the policy below; the launch table, refusal, lattice -> path map, pass size and the site-term and tail
// launches are mdrnn_observable.h's.
//
// Per call: the masks, given by LATTICE index k = nx Ny + ny, are checked, mapped to visit order and packed into words; the terms
// are grouped by flip mask and the distinct masks sorted longest tail first.  Per pass of whole 16-chain blocks (the state budget):
// spins (the caller's, or drawn exactly as rnnwf_sample draws them) with the family's base pass, which keeps every position's state
// in h->hck and log P in h->out_lp -> site terms -> masked tails -> log-ratios, per-term sums of v and v^2, E_loc and its moments.
// The sums of the passes are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, states, E_loc)
// resident for rnnwf_vmc_gradient.
//
// rnnwf_pauli_train_steps_2d (docs/pauli_train.md) runs K Adam iterations on the same terms through pauli_driver.h's
// pauli_train_steps: the sampling base pass keeps every position's state and log P, so there is no second pass in front of the tails
// (md_terms_and_tails, unchanged), then pauli_train_kernels.h's ratio table and the kernels that read it.
#include "mdrnn_observable.h"
#include "pauli_driver.h"
#include "pauli_kernels.h"
#include "pauli_train_kernels.h"

using namespace rnnwf;

namespace {

struct MdPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_step_2d";
    static constexpr const char* kCoeff = "coeff";
    static constexpr size_t kElem = 8;
    static constexpr bool kComplex = false, kOwnLogP = false, kUncommittedInvalid = true;
    static constexpr int kThreads = kPauliThreads;
    static int refuse(rnnwf_handle* h) { return md_refuse(h, kEntry, "rnnwf_pauli_step"); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle* h) { return md_positions(h); }
    static int cells(const rnnwf_handle* h) { return h->N - 1; }
    // per block, beside the states, the terms (N x 16 x 8 bytes), the tails and log-ratios (2 x M x 16 x 8), log P and E_loc (2 x 16 x 8)
    static int64_t chunk(rnnwf_handle* h, int M) { return md_chains_per_pass(h, (size_t)(h->N + 2 + 2 * M) * kChains * 8); }
    static int pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool keep, double* sums_host);
};

// rnnwf_pauli_train_steps_2d: the same model, terms, lattice -> path map, pass size and kernels up to the tails, the table-reading
// assembly behind them; uncommitted parameters are RNNWF_ERR_STATE as for the other two train entries
struct MdPauliTrain : MdPauli {
    static constexpr const char* kEntry = "rnnwf_pauli_train_steps_2d";
    static constexpr bool kUncommittedInvalid = false;
    static int refuse(rnnwf_handle* h) {
        if (h->model != RNNWF_MODEL_MDRNN2D)
            return h->fail(RNNWF_ERR_INVALID, "%s: serves the 2D RNN (MDRNN2D) only, this handle's model is %s; rnnwf_pauli_train_steps serves "
                           "the GRU models, rnnwf_pauli_train_steps_complex the complex RNN", kEntry, model_name(h->model));
        return md_refuse(h, kEntry, "rnnwf_pauli_train_steps");
    }
    static int train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row);
};

// one pass over the ns chains packed in h->bits, their states in h->hck and log P in h->out_lp (the family's base pass): sums_host
// (K, 2) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
int MdPauli::pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, bool, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    double* lr = (double*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    if (M > 0) {
        MdPauliArgs a = md_args(h, ns, g.W, sc, M);
        if (int rc = md_terms_and_tails<false>(h, a, g.replay, g.steps)) return rc;      // sum over masks of N - 1 - f cell evaluations per chain
        if (int rc = timed_launch(h, kTimerAssembly, pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                  (const double*)a.tail, (const double*)a.terms, (const double*)h->out_lp.p, a.first, N, ns, lr))
            return rc;
    }
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

// one iteration's pass of rnnwf_pauli_train_steps_2d over the ns chains the sampling base pass drew into h->bits, with their states in
// h->hck and log P in h->out_lp: the ratios r[M][ns] in the log-ratios' place (sc.lr), E_loc in h->eloc; sums_row: the iteration's
// (K, 2) row of the call's table on the device, or nullptr - then the per-term kernels are not launched
int MdPauliTrain::train_pass(rnnwf_handle* h, int64_t ns, const PauliTerms& g, const PauliScratch& sc, double* sums_row) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    const double* ratio = (const double*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
    const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
    if (M > 0) {
        MdPauliArgs a = md_args(h, ns, g.W, sc, M);
        if (int rc = md_terms_and_tails<false>(h, a, g.replay, g.steps)) return rc;
        if (int rc = timed_launch(h, kTimerAssembly, pauli_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                  (const double*)a.tail, (const double*)a.terms, (const double*)h->out_lp.p, a.first, N, ns,
                                  (double*)(buf + sc.lr)))
            return rc;
    }
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

extern "C" int rnnwf_pauli_train_steps_2d(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                          int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                          const double* learning_rates, double beta1, double beta2, double epsilon, double* moments,
                                          double* term_sums, double* out_eloc) {
    return pauli_train_steps<MdPauliTrain>(h, flip, sign, coeff, nterms, K, numsamples, seed, step0, sample_offset, learning_rates, beta1,
                                           beta2, epsilon, moments, term_sums, out_eloc);
}

extern "C" int rnnwf_pauli_step_2d(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                   const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                   double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    return pauli_step<MdPauli>(h, flip, sign, coeff, nterms, samples, ns, seed, step, sample_offset, term_sums, out_eloc, moments,
                               out_log_ratio, out_samples);
}
