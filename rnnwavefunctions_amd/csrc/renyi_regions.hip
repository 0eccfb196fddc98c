// renyi_regions.hip - host driver of rnnwf_renyi2_regions (include/rnnwf.h): the second Renyi entropy of the positive GRU models
// (GRU1D, GRU1D_F64, one layer) for any list of regions given as site masks, by the replica swap trick; kernels in
// renyi_region_kernels.h and chain_kernels.h (prnn_masked_tail_kernel, PAIRED), the method in docs/renyi_regions.md.  The driver is
// region_driver.h's, over the policy below; the launch table, refusals, base pass and pass size are observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed
// chain first.  Per pass of whole 16-chain blocks (the state budget, as renyi.hip): spins (the caller's, or drawn exactly as
// rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> site terms and region tails ->
// log-ratios and per-region sums of r and r^2.  The sums of the passes are added on the host in pass order.
#include "region_driver.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

struct GruRegions {
    static constexpr const char* kEntry = "rnnwf_renyi2_regions";
    static constexpr size_t kElem = 8;
    static constexpr int kSumsRow = 2, kThreads = kRenyiThreads;
    static constexpr bool kSurvivors = false, kUncommittedInvalid = false;
    static int refuse(rnnwf_handle* h) { return observable_refuse(h, kEntry); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // pairs: per block, beside the checkpoints, the terms (N x 16 x 8 bytes), the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
    static int64_t chunk(rnnwf_handle* h, const Regions& g) {
        return blocks_per_pass(h, (size_t)h->N * kChains * 8 + (size_t)g.R * kChains * 8 + (size_t)g.R * (kChains / 2) * 8) * kChains / 2;
    }
    static int pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host);
    static void finish(rnnwf_handle*, const Regions&, const std::vector<double>&, int64_t, int64_t*) {}
};

// one pass over the ns chains packed in h->bits: sums_host (R, 2) of this pass; the log-ratios stay in h->renyi
int GruRegions::pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    if (int rc = observable_base(h, ns, nullptr)) return rc;
    char* buf = (char*)h->renyi.p;
    const ChainArgs c = chain_args(h, ns);
    SwapArgs t{c};
    t.terms = (double*)(buf + sc.terms);
    MaskArgs a{c};
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)g.nact * a.nsb;
    if (g.nact > 0) {                              // N >= 2
        int rc = 0;
        with_gru1(h, [&](auto k) {
            using K = decltype(k);
            rc = launch_waves(h, k, kTimerBase, prnn_site_terms_kernel<typename K::T, K::NFULL, K::WAVES>, t.nsb, t);
            if (!rc) rc = launch_waves(h, k, kTimerFlip, prnn_masked_tail_kernel<typename K::T, K::NFULL, K::WAVES, true>, a.ntiles, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * K::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over regions of N - f cell evaluations per chain
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        renyi_region_assemble_kernel<<<dim3((unsigned)sc.nblk, (unsigned)R), kRenyiThreads, 0, h->stream>>>(
            a.tail, t.terms, a.first, N, ns, (double*)(buf + sc.lr), (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)R, kRenyiThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)R * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_renyi2_regions(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                    uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                    int32_t* out_samples) {
    return renyi2_regions<GruRegions>(h, regions, nregions, samples, npairs, seed, step, pair_offset, sums, out_log_ratio, nullptr, out_samples);
}
