// crnn_renyi.hip - host driver of rnnwf_renyi2_regions_complex (include/rnnwf.h): the second Renyi entropy of the complex RNN with
// the U(1) mask (CRNN_U1, one layer) for any list of regions given as site masks, by the replica swap trick; kernels in
// crnn_renyi_kernels.h, the method in docs/renyi_complex.md.  The driver is region_driver.h's, over the policy below; the launch
// table, refusal, base pass, pass size and sector check are crnn_observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed
// chain first.  Per pass of whole pairs (the state budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) ->
// teacher-forced base pass on the one-wave kernel with checkpoints -> site terms -> per region the list of the pairs whose mixed
// chains stay in the zero-magnetisation sector and the tile offsets (on the device: no synchronisation in front of the tails) ->
// tails of the survivors, 16 to a tile -> complex log-ratios, per-region sums of Re r, Im r and their squares.  The sums and the
// survivor counts of the passes are added on the host in pass order.
#include "crnn_observable.h"
#include "crnn_renyi_kernels.h"
#include "region_driver.h"

using namespace rnnwf;

namespace {

struct CrnnRegions {
    static constexpr const char* kEntry = "rnnwf_renyi2_regions_complex";
    static constexpr size_t kElem = 16;
    static constexpr int kSumsRow = 6, kThreads = kCRenyiThreads;      // (R, 4) sums, then (R) surviving pairs and (R) tiles: one copy
    static constexpr bool kSurvivors = true, kUncommittedInvalid = false;
    static int refuse(rnnwf_handle* h) { return crnn_refuse(h, kEntry, "rnnwf_renyi2_regions", "rnnwf_renyi2_regions_2d"); }
    // the caller's chains must lie in the sector: the survivor rule rests on it
    static int precheck(rnnwf_handle* h, const int32_t* samples, int64_t ns) { return samples ? crnn_check_sector(h, kEntry, samples, ns) : 0; }
    static std::vector<int32_t> positions(const rnnwf_handle*) { return {}; }
    static int cells(const rnnwf_handle* h) { return h->N; }
    // pairs: per block, beside the checkpoints, the terms (N x 16 x 16 bytes), the tails (R x 16 x 16), the log-ratios (R x 8 x 16) and
    // the survivor lists (R x 16 x 4)
    static int64_t chunk(rnnwf_handle* h, const Regions& g) {
        const size_t R = (size_t)g.R;
        int64_t chunk = crnn_blocks_per_pass(h, (size_t)h->N * kChains * 16 + R * (kChains * 16 + (kChains / 2) * 16 + kChains * 4)) * kChains / 2;
        // the tile index is an int
        chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, 0x7fffffffLL / std::max(g.nact, 1) - 1) * (kChains / 2));
        // and so is the tail kernel's offset of a chain's block within one checkpoint row
        return std::min<int64_t>(chunk, std::max<int64_t>(1, 0x7fffffffLL / (int64_t)(crnn_hck_bytes_per_block(h) / 4) - 1) * (kChains / 2));
    }
    static int pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host);
    // the work of the tail pass is known now that the counts are back: evaluated cell steps, and the MFMA flops of the tiles run
    static void finish(rnnwf_handle* h, const Regions& g, const std::vector<double>& total, int64_t npairs, int64_t* out_in_sector) {
        const int N = h->N, R = g.R;
        double flops_per_step = 0.0;
        with_crnn1(h, [&](auto k) { flops_per_step = decltype(k)::mfma_flops_per_step(); });
        for (int r = 0; r < R; ++r) {
            const double pairs = total[(size_t)R * 4 + r], tiles = total[(size_t)R * 5 + r];
            if (out_in_sector) out_in_sector[r] = g.first[r] ? (int64_t)pairs : npairs;
            h->work[0] += (double)(N - g.first[r]) * 2.0 * pairs;
            h->work[1] += (double)(N - g.first[r]) * tiles * flops_per_step;
        }
    }
};

// one pass over the ns chains packed in h->bits: sums_host (R, 4) sums then (2, R) counts of this pass; the log-ratios stay in h->renyi
int CrnnRegions::pass(rnnwf_handle* h, int64_t ns, const Regions& g, const RegionScratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    char* buf = (char*)h->renyi.p;
    CRenyiArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.W = g.W;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.nact = g.nact;
    a.surv = (int32_t*)(buf + sc.surv);
    a.cnt = (int32_t*)(buf + sc.cnt);
    a.tile_begin = (int32_t*)(buf + sc.tile_begin);
    a.tail = (double2*)(buf + sc.tail);
    double2* terms = (double2*)(buf + sc.terms);
    double* sums = (double*)(buf + sc.sums);
    if (g.nact > 0) {                              // N >= 2
        if (int rc = crnn_observable_base(h, ns, nullptr)) return rc;
        a.hck = h->hck.p;
        CPauliArgs t{};
        static_cast<ChainArgs&>(t) = a;
        t.terms = terms;
        int rc = 0;
        with_crnn1(h, [&](auto k) {
            using P = decltype(k);
            using L = typename P::L;
            rc = launch_persistent(h, kTimerBase, crnn_site_terms_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::LDS_BYTES, nsb, P::WAVES, t);
            if (rc) return;
            {
                TimedLaunch tl(h, kTimerFlip);
                if ((rc = plain_launch(h, crnn_survivor_list_kernel, dim3((unsigned)g.nact), kCRenyiThreads, 0, a))) return;
                if ((rc = plain_launch(h, crnn_tile_scan_kernel, dim3(1), kCRenyiThreads, 0, a, R, sums + 4 * (size_t)R))) return;
                // the tile count lives on the device: the persistent grid is bounded by the worst case, every pair surviving
                unsigned grid = 0;
                if ((rc = persistent_grid(h, crnn_paired_tail_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::LDS_BYTES, (int64_t)g.nact * nsb,
                                          P::WAVES, &grid)))
                    return;
                rc = plain_launch(h, crnn_paired_tail_kernel<P::NFULL, P::WAVES>, dim3(grid), P::WAVES * 64, L::LDS_BYTES, a);
            }
        });
        if (rc) return rc;
    } else {
        RNNWF_HIP(h, hipMemsetAsync(sums + 4 * (size_t)R, 0, (size_t)R * 16, h->stream));
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        double2* lr = (double2*)(buf + sc.lr);
        if (int rc = plain_launch(h, crnn_renyi_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)R), kCRenyiThreads, 0, a,
                                  (const double2*)terms, lr))
            return rc;
        if (int rc = plain_launch(h, crnn_renyi_value_kernel, dim3((unsigned)sc.nblk, (unsigned)R), kCRenyiThreads, 0, (const double2*)lr,
                                  ns / 2, (double*)(buf + sc.part)))
            return rc;
        // rows (region, half): half 0 = (sum Re r, sum Im r), half 1 = the sums of their squares
        if (int rc = plain_launch(h, renyi_sums_kernel, dim3((unsigned)(2 * R)), kCRenyiThreads, 0, (const double*)(buf + sc.part), sc.nblk, sums))
            return rc;
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, sums, (size_t)R * 48, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_renyi2_regions_complex(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                            uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                            int64_t* out_in_sector, int32_t* out_samples) {
    return renyi2_regions<CrnnRegions>(h, regions, nregions, samples, npairs, seed, step, pair_offset, sums, out_log_ratio, out_in_sector,
                                       out_samples);
}
