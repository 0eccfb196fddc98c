// crnn_renyi.hip - host driver of rnnwf_renyi2_regions_complex (include/rnnwf.h): the second Renyi entropy of the complex RNN with
// the U(1) mask (CRNN_U1, one layer) for any list of regions given as site masks, by the replica swap trick; kernels in
// crnn_renyi_kernels.h, the method in docs/renyi_complex.md; the launch table, the pass size and the sector check are
// crnn_observable.h's, the scratch carving, the chain source and the pass loop observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed
// chain first.  Per pass of whole pairs (the state budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) ->
// teacher-forced base pass on the one-wave kernel with checkpoints -> site terms -> per region the list of the pairs whose mixed
// chains stay in the zero-magnetisation sector and the tile offsets (on the device: no synchronisation in front of the tails) ->
// tails of the survivors, 16 to a tile -> complex log-ratios, per-region sums of Re r, Im r and their squares.  The sums and the
// survivor counts of the passes are added on the host in pass order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "crnn_observable.h"
#include "crnn_renyi_kernels.h"

using namespace rnnwf;

namespace {

const char* const kEntry = "rnnwf_renyi2_regions_complex";
constexpr int kMaxRegions = 65535;       // blockIdx.y of the assembly

// The regions of one call as the kernels read them
struct Regions {
    int R = 0, W = 0, nact = 0;
    std::vector<uint32_t> mask;          // [R][W], normalised
    std::vector<int32_t> first, order;   // [R]: f, 0 = empty; [nact]: non-empty regions, f ascending, ties by index
};

// Scratch of one pass of ns chains in h->renyi; the call's tables lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, cnt, tile_begin, surv, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per region
    Scratch(int N, int R, int W, int64_t ns) {
        Carve c;
        nblk = (ns / 2 + kCRenyiThreads - 1) / kCRenyiThreads;
        mask = c.take((size_t)R * W * 4);
        order = c.take((size_t)R * 4);
        first = c.take((size_t)R * 4);
        cnt = c.take((size_t)R * 4);
        tile_begin = c.take((size_t)(R + 1) * 4);
        surv = c.take((size_t)R * ns * 4);
        terms = c.take((size_t)N * ns * 16);
        tail = c.take((size_t)R * ns * 16);
        lr = c.take((size_t)R * (ns / 2) * 16);
        part = c.take((size_t)R * nblk * 32);
        sums = c.take((size_t)R * 48);             // [R][4] sums, then [2][R] surviving pairs and tiles: one copy to the host
        bytes = c.bytes;
    }
};

// check, normalise, pack and sort the (R, N) masks
int prepare(rnnwf_handle* h, const int32_t* regions, int R, Regions& g) {
    const int N = h->N;
    g.R = R;
    g.W = (N + 31) / 32;
    g.mask.assign((size_t)R * g.W, 0u);
    g.first.assign(R, 0);
    for (int r = 0; r < R; ++r) {
        const int32_t* m = regions + (size_t)r * N;
        for (int n = 0; n < N; ++n)
            if (m[n] != 0 && m[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: regions[%d][%d] = %d, a mask entry must be 0 or 1", kEntry, r, n, (int)m[n]);
        const int32_t flip = m[0];                 // site 0 in A: take the complement
        for (int n = 0; n < N; ++n)
            if (m[n] ^ flip) {
                g.mask[(size_t)r * g.W + (n >> 5)] |= 1u << (n & 31);
                if (!g.first[r]) g.first[r] = n;
            }
        if (g.first[r]) g.order.push_back(r);
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    g.nact = (int)g.order.size();
    return 0;
}

// one pass over the ns chains packed in h->bits: sums_host (R, 4) sums then (2, R) counts of this pass; the log-ratios stay in h->renyi
int region_pass(rnnwf_handle* h, int64_t ns, const Regions& g, const Scratch& sc, double* sums_host) {
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
        if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * crnn_hck_bytes_per_block(h))) return rc;
        a.hck = h->hck.p;
        CrnnArgs b = crnn_base_args(h, ns);
        b.bits = (uint32_t*)h->bits.p;
        b.hck = h->hck.p;
        if (int rc = crnn_plain_base(h, b)) return rc;
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
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (h->model != RNNWF_MODEL_CRNN_U1)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the complex RNN (CRNN_U1) only, this handle's model is %s; rnnwf_renyi2_regions serves "
                       "the GRU models, rnnwf_renyi2_regions_2d the 2D RNN", kEntry, model_name(h->model));
    if (h->NL > 1) return h->fail(RNNWF_ERR_INVALID, "%s: not implemented for stacked layers (one GRU layer only)", kEntry);
    if (!with_crnn1(h, [](auto) {})) return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for NFULL=%d", kEntry, h->NFULL);
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (nregions < 1 || nregions > kMaxRegions) return h->fail(RNNWF_ERR_INVALID, "%s: nregions must be in 1..%d", kEntry, kMaxRegions);
    if (npairs < 1) return h->fail(RNNWF_ERR_INVALID, "%s: npairs must be >= 1", kEntry);
    if (!regions || !sums) return h->fail(RNNWF_ERR_INVALID, "%s: regions and sums must be non-null", kEntry);
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: pair_offset must be >= 0", kEntry);
    if (samples)                                      // the caller's chains must lie in the sector: the survivor rule rests on it
        if (int rc = crnn_check_sector(h, kEntry, samples, 2 * npairs)) return rc;
    Regions g;
    if (int rc = prepare(h, regions, nregions, g)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N, R = nregions;
    // pairs per pass: per block, beside the checkpoints, the terms (N x 16 x 16 bytes), the tails (R x 16 x 16), the log-ratios
    // (R x 8 x 16) and the survivor lists (R x 16 x 4); the tile index is an int
    int64_t chunk = crnn_blocks_per_pass(h, (size_t)N * kChains * 16 + (size_t)R * (kChains * 16 + (kChains / 2) * 16 + kChains * 4)) * kChains / 2;
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, 0x7fffffffLL / std::max(g.nact, 1) - 1) * (kChains / 2));
    // and so is the tail kernel's offset of a chain's block within one checkpoint row
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, 0x7fffffffLL / (int64_t)(crnn_hck_bytes_per_block(h) / 4) - 1) * (kChains / 2));
    // the first pass is the largest: one allocation for the call, the masks uploaded once
    const Scratch big(N, R, g.W, 2 * std::min(chunk, npairs));
    if (int rc = ensure(h, h->renyi, big.bytes)) return rc;
    {
        char* buf = (char*)h->renyi.p;
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.first, g.first.data(), (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
        if (g.nact) RNNWF_HIP(h, hipMemcpyAsync(buf + big.order, g.order.data(), (size_t)g.nact * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    std::vector<double> total((size_t)R * 6, 0.0);    // (R, 4) sums, (R) surviving pairs, (R) tiles
    const ChainSource src{samples, seed, step, pair_offset, out_samples};
    if (int rc = for_each_pass(h, src, npairs, chunk, 2, total, [&](int64_t p0, int64_t np, int64_t ns, double* pass_sums) {
            const Scratch sc(N, R, g.W, ns);
            if (int rc = region_pass(h, ns, g, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + 2 * p0, (size_t)npairs * 16, (char*)h->renyi.p + sc.lr, (size_t)np * 16,
                                              (size_t)np * 16, (size_t)R, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(sums, total.data(), (size_t)R * 32);
    // the work of the tail pass is known now that the counts are back: evaluated cell steps, and the MFMA flops of the tiles run
    double flops_per_step = 0.0;
    with_crnn1(h, [&](auto k) { flops_per_step = decltype(k)::mfma_flops_per_step(); });
    for (int r = 0; r < R; ++r) {
        const double pairs = total[(size_t)R * 4 + r], tiles = total[(size_t)R * 5 + r];
        if (out_in_sector) out_in_sector[r] = g.first[r] ? (int64_t)pairs : npairs;
        h->work[0] += (double)(N - g.first[r]) * 2.0 * pairs;
        h->work[1] += (double)(N - g.first[r]) * tiles * flops_per_step;
    }
    return RNNWF_OK;
}
