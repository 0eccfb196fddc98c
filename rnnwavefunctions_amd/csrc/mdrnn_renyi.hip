// mdrnn_renyi.hip - rnnwf_renyi2_regions_2d (include/rnnwf.h): the second Renyi entropy of arbitrary lattice regions for the 2D RNN
// (MDRNN2D, float64) by the replica swap trick; kernels in mdrnn_pauli_kernels.h (mdrnn_site_terms_kernel and
// mdrnn_masked_tail_kernel<..., PAIRED = true>) and, from the tails on, renyi_region_kernels.h; the method in docs/renyi_2d.md.  The
// driver is region_driver.h's, over the policy below; the launch table, refusal, lattice -> path map, pass size and the site-term
// and tail launches are mdrnn_observable.h's.
//
// Per call: the masks, given by LATTICE index k = nx Ny + ny, are checked, mapped to visit order, normalised (position 0 of the path
// not in A: r_A = r_complement), packed into words and sorted longest mixed chain first.  Per pass of whole 16-chain blocks (the state
// budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) with the family's base pass, which keeps every position's
// state in h->hck -> site terms -> paired masked tails -> log-ratios and per-region sums of r and r^2.  The sums of the passes are
// added on the host in pass order.
#include "mdrnn_observable.h"
#include "region_driver.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

struct MdRegions {
    static constexpr const char* kEntry = "rnnwf_renyi2_regions_2d";
    static constexpr size_t kElem = 8;
    static constexpr int kSumsRow = 2, kThreads = kRenyiThreads;
    static constexpr bool kSurvivors = false, kUncommittedInvalid = true;
    static int refuse(rnnwf_handle* h) { return md_refuse(h, kEntry, "rnnwf_renyi2_regions"); }
    static int precheck(rnnwf_handle*, const int32_t*, int64_t) { return 0; }
    static std::vector<int32_t> positions(const rnnwf_handle* h) { return md_positions(h); }
    static int cells(const rnnwf_handle* h) { return h->N - 1; }
    // pairs: per block, beside the states, the terms (N x 16 x 8 bytes), the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
    static int64_t chunk(rnnwf_handle* h, const Regions& g) {
        return md_chains_per_pass(h, (size_t)h->N * kChains * 8 + (size_t)g.R * kChains * 8 + (size_t)g.R * (kChains / 2) * 8) / 2;
    }
    static int pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host);
    static void finish(rnnwf_handle*, const Regions&, const std::vector<double>&, int64_t, int64_t*) {}
};

// one pass over the ns chains packed in h->bits, their states in h->hck (the family's base pass): sums_host (R, 2) of this pass; the
// log-ratios stay in h->renyi
int MdRegions::pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    char* buf = (char*)h->renyi.p;
    MdPauliArgs a = md_args(h, ns, g.W, sc, g.nact);
    if (g.nact > 0)                                // N >= 2; sum over non-empty regions of N - 1 - f cell evaluations per chain
        if (int rc = md_terms_and_tails<true>(h, a, true, g.steps)) return rc;
    {
        TimedLaunch tl(h, kTimerAssembly);
        renyi_region_assemble_kernel<<<dim3((unsigned)sc.nblk, (unsigned)R), kRenyiThreads, 0, h->stream>>>(
            a.tail, a.terms, a.first, N, ns, (double*)(buf + sc.lr), (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)R, kRenyiThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)R * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_renyi2_regions_2d(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                       uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                       int32_t* out_samples) {
    return renyi2_regions<MdRegions>(h, regions, nregions, samples, npairs, seed, step, pair_offset, sums, out_log_ratio, nullptr, out_samples);
}
