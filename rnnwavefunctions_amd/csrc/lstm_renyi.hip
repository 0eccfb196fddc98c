// lstm_renyi.hip - rnnwf_renyi2_regions_lstm (include/rnnwf.h): the second Renyi entropy of arbitrary regions, given as site masks,
// by the replica swap trick for the LSTM wave function over the raster path (LSTM1D_F64, one layer, 1..68 units, float64); kernels
// in lstm_pauli_kernels.h (lstm_site_terms_kernel, lstm_masked_tail_kernel PAIRED) and, from the tails on, renyi_region_kernels.h;
// the method in docs/renyi_lstm.md.  The driver is region_driver.h's, over the policy below; the launch class and the refusals are
// lstm_observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed chain
// first.  Per pass of whole 16-chain blocks (the state budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) ->
// teacher-forced base pass with checkpoints (h, c) and site terms (lstm_site_terms_kernel) -> region tails of the mixed chains ->
// log-ratios and per-region sums of r and r^2.  The sums of the passes are added on the host in pass order.  No batch is resident
// after a call.
#include "lstm_observable.h"
#include "region_driver.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

struct LstmRegions {
    static constexpr const char* kEntry = "rnnwf_renyi2_regions_lstm";
    static constexpr size_t kElem = 8;
    static constexpr int kSumsRow = 2, kThreads = kRenyiThreads;
    static constexpr bool kSurvivors = false, kUncommittedInvalid = false;
    static int refuse(rnnwf_handle* h) { return lstm_pauli_refuse(h, kEntry, LstmEntryKind::Renyi); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }      // masks by chain position, the raster index ny Nx + nx
    static int cells(const rnnwf_handle* h) { return h->N; }
    // pairs: whole 16-chain blocks within the state budget.  Per block the checkpoints (h, c) of N - 1 sites and, beside them, the
    // terms (N x 16 x 8 bytes), log P (16 x 8), the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
    static int64_t chunk(rnnwf_handle* h, const Regions& g) {
        const size_t per_block = (size_t)std::max(h->N - 1, 1) * hck_bytes_per_block(h) + (size_t)(h->N + 1) * kChains * 8 +
                                 (size_t)g.R * kChains * 8 + (size_t)g.R * (kChains / 2) * 8;
        return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block)) * kChains / 2;
    }
    static int pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host);
    static void finish(rnnwf_handle*, const Regions&, const std::vector<double>&, int64_t, int64_t*) {}
};

// one pass over the ns chains packed in h->bits: sums_host (R, 2) of this pass; the log-ratios stay in h->renyi
int LstmRegions::pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    char* buf = (char*)h->renyi.p;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    double* terms = (double*)(buf + sc.terms);
    double* tail = (double*)(buf + sc.tail);
    const int32_t* first = (const int32_t*)(buf + sc.first);
    if (g.nact > 0) {                              // N >= 2; regions that are all empty need neither states nor tails
        if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * hck_bytes_per_block(h))) return rc;
        if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;      // the base pass's log P: written, not read by this pass
        LstmTermsArgs b{};
        b.wimg = h->wimg.p;
        b.N = N;
        b.ns = ns;
        b.nsb = nsb;
        b.bits = (const uint32_t*)h->bits.p;
        b.hck = (double*)h->hck.p;
        b.terms = terms;
        b.out_lp = (double*)h->eloc.p;
        MaskArgs a{};
        a.wimg = h->wimg.p;
        a.N = N;
        a.W = g.W;
        a.ns = ns;
        a.nsb = nsb;
        a.bits = b.bits;
        a.hck = h->hck.p;
        a.mask = (const uint32_t*)(buf + sc.mask);
        a.order = (const int32_t*)(buf + sc.order);
        a.first = first;
        a.tail = tail;
        a.ntiles = (int64_t)g.nact * nsb;
        int rc = 0;
        with_lpauli(h, [&](auto k) {
            using K = decltype(k);
            rc = K::base(h, b);
            if (!rc) rc = K::paired_tails(h, a);
            if (!rc) h->work[1] += (double)nsb * g.steps * K::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over regions of N - f cell evaluations per chain
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        renyi_region_assemble_kernel<<<dim3((unsigned)sc.nblk, (unsigned)R), kRenyiThreads, 0, h->stream>>>(
            tail, terms, first, N, ns, (double*)(buf + sc.lr), (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)R, kRenyiThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)R * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_renyi2_regions_lstm(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                         uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                         int32_t* out_samples) {
    return renyi2_regions<LstmRegions>(h, regions, nregions, samples, npairs, seed, step, pair_offset, sums, out_log_ratio, nullptr,
                                       out_samples);
}
