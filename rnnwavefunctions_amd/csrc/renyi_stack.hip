// renyi_stack.hip - rnnwf_renyi2_regions_stack (include/rnnwf.h): the second Renyi entropy of arbitrary regions, given as site masks,
// by the replica swap trick for STACKED layers of the positive GRU models (GRU1D float32, GRU1D_F64 float64 on the raster path; 2..4
// layers, every stack rnnwf_create accepts); kernels in stack_chain_kernels.h (prnn_ml_masked_tail_kernel, PAIRED) and, from the
// tails on, renyi_region_kernels.h; the method in docs/renyi_stack.md.  The driver is region_driver.h's, over the policy below; the
// launch classes and the refusals are stack_observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed chain
// first.  Per pass of whole 16-chain blocks (the state budget, at the stack's N checkpoint sites of NL layers each): spins (the
// caller's, or drawn exactly as rnnwf_sample draws them) -> teacher-forced base pass with checkpoints on the one-wave MFMA stack
// kernel (prnn_ml_base_kernel, whatever kernel rnnwf_vmc_step takes for this handle) -> site terms and region tails -> log-ratios
// and per-region sums of r and r^2.  The sums of the passes are added on the host in pass order.  No batch is resident after a call.
#include "region_driver.h"
#include "renyi_region_kernels.h"
#include "stack_observable.h"

using namespace rnnwf;

namespace {

struct StackRegions {
    static constexpr const char* kEntry = "rnnwf_renyi2_regions_stack";
    static constexpr size_t kElem = 8;
    static constexpr int kSumsRow = 2, kThreads = kRenyiThreads;
    static constexpr bool kSurvivors = false, kUncommittedInvalid = false;
    static int refuse(rnnwf_handle* h) { return stack_refuse(h, kEntry, "rnnwf_renyi2_regions"); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // pairs: whole 16-chain blocks within the state budget.  Per block the stack's checkpoints of all N sites and, beside them, the
    // terms (N x 16 x 8 bytes), the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
    static int64_t chunk(rnnwf_handle* h, const Regions& g) {
        const size_t per_block = (size_t)h->N * stack_hck_bytes_per_block(h) + (size_t)h->N * kChains * 8 + (size_t)g.R * kChains * 8 +
                                 (size_t)g.R * (kChains / 2) * 8;
        return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block)) * kChains / 2;
    }
    static int pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host);
    static void finish(rnnwf_handle*, const Regions&, const std::vector<double>&, int64_t, int64_t*) {}
};

// one pass over the ns chains packed in h->bits: sums_host (R, 2) of this pass; the log-ratios stay in h->renyi
int StackRegions::pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    char* buf = (char*)h->renyi.p;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (g.nact > 0) {                              // N >= 2; regions that are all empty need neither states nor tails
        if (int rc = ensure(h, h->hck, (size_t)N * nsb * stack_hck_bytes_per_block(h))) return rc;
        PrnnArgs b = prnn_base_args(h, ns);
        b.bits = (uint32_t*)h->bits.p;
        b.hck = h->hck.p;
        b.out_lp = nullptr;
        if (int rc = prnn_stack_base(h, b)) return rc;
    }
    const ChainArgs c = chain_args(h, ns);
    SwapArgs t{c};
    t.terms = (double*)(buf + sc.terms);
    MaskArgs a{c};
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)g.nact * a.nsb;
    if (g.nact > 0) {
        int rc = 0;
        with_stack(h, [&](auto k) {
            using K = decltype(k);
            using S = typename K::S;
            rc = launch_persistent(h, kTimerBase, prnn_ml_site_terms_kernel<typename K::T, K::NFULL, K::NL, K::WAVES>, K::WAVES * 64,
                                   S::LDS_BYTES, t.nsb, K::WAVES, t);
            if (!rc)
                rc = launch_persistent(h, kTimerFlip, prnn_ml_masked_tail_kernel<typename K::T, K::NFULL, K::NL, K::WAVES, true>,
                                       K::WAVES * 64, S::LDS_BYTES, a.ntiles, K::WAVES, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * K::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over regions of N - f stack steps per chain
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

extern "C" int rnnwf_renyi2_regions_stack(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                          uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                          int32_t* out_samples) {
    return renyi2_regions<StackRegions>(h, regions, nregions, samples, npairs, seed, step, pair_offset, sums, out_log_ratio, nullptr,
                                        out_samples);
}
