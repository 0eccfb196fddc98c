// region_driver.h - the host driver of the region-Renyi entry points of every family: rnnwf_renyi2_regions (renyi_regions.hip),
// rnnwf_renyi2_regions_2d (mdrnn_renyi.hip) and rnnwf_renyi2_regions_complex (crnn_renyi.hip).  Per call: validation, the regions
// (pauli_terms.h), the pass size, one scratch allocation sized by the largest pass with the masks uploaded once, and the pass loop
// (observable.h) with the per-pass copy of the log-ratios.  A family's .hip supplies a policy struct P:
//   kEntry                     its name in the refusals
//   kElem, kSumsRow, kSurvivors   bytes of a value (8 real, 16 complex); doubles per region that a pass returns, the first kElem / 4
//                              of them the caller's sums; pieces for the complex RNN's survivor lists
//   kThreads                   pairs per assembly block
//   kUncommittedInvalid        the code of the "not committed" refusal (observable.h: refuse_uncommitted)
//   refuse(h), precheck(h, samples, ns), positions(h), cells(h), chunk(h, g)     as pauli_driver.h; chunk in pairs
//   pass(h, ns, g, sc, sums_host)   the kernels of one pass over the chains in h->bits: log-ratios at sc.lr
//   finish(h, g, total, npairs, out_in_sector)   what follows the loop (the complex RNN: survivor counts -> out_in_sector and work)
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "observable.h"
#include "pauli_terms.h"

namespace rnnwf {

// Scratch of one pass of ns chains in h->renyi; the call's masks, order and first positions lead, at offsets that do not depend on ns
struct RegionScratch {
    size_t mask, order, first, cnt, tile_begin, surv, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per region
    RegionScratch(int N, const Regions& g, int64_t ns, size_t elem, int sums_row, bool survivors, int threads) {
        Carve c;
        const size_t R = (size_t)g.R;
        nblk = (ns / 2 + threads - 1) / threads;
        mask = c.take(R * g.W * 4);
        order = c.take(R * 4);
        first = c.take(R * 4);
        cnt = c.take(survivors ? R * 4 : 0);
        tile_begin = c.take(survivors ? (R + 1) * 4 : 0);
        surv = c.take(survivors ? R * ns * 4 : 0);
        terms = c.take((size_t)N * ns * elem);
        tail = c.take(R * ns * elem);
        lr = c.take(R * (ns / 2) * elem);
        part = c.take(R * nblk * 2 * elem);
        sums = c.take(R * sums_row * 8);
        bytes = c.bytes;
    }
};

// sums: [R] rows of P::kElem / 4 doubles; out_log_ratio: [R][npairs] values of P::kElem bytes
template <class P>
int renyi2_regions(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs, uint64_t seed,
                   uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio, int64_t* out_in_sector, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = P::refuse(h)) return rc;
    if (int rc = refuse_uncommitted(h, P::kEntry, P::kUncommittedInvalid)) return rc;
    if (nregions < 1 || nregions > kMaxRegions) return h->fail(RNNWF_ERR_INVALID, "%s: nregions must be in 1..%d", P::kEntry, kMaxRegions);
    if (npairs < 1) return h->fail(RNNWF_ERR_INVALID, "%s: npairs must be >= 1", P::kEntry);
    if (!regions || !sums) return h->fail(RNNWF_ERR_INVALID, "%s: regions and sums must be non-null", P::kEntry);
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: pair_offset must be >= 0", P::kEntry);
    if (int rc = P::precheck(h, samples, 2 * npairs)) return rc;
    Regions g;
    const std::vector<int32_t> pos = P::positions(h);
    if (int rc = prepare_regions(h, P::kEntry, regions, nregions, pos.empty() ? nullptr : pos.data(), P::cells(h), g)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N, R = nregions;
    const size_t E = P::kElem;
    const int64_t chunk = P::chunk(h, g);
    // the first pass is the largest: one allocation for the call, the masks uploaded once
    const RegionScratch big(N, g, 2 * std::min(chunk, npairs), E, P::kSumsRow, P::kSurvivors, P::kThreads);
    if (int rc = ensure(h, h->renyi, big.bytes)) return rc;
    {
        char* buf = (char*)h->renyi.p;
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.first, g.first.data(), (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
        if (g.nact) RNNWF_HIP(h, hipMemcpyAsync(buf + big.order, g.order.data(), (size_t)g.nact * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    h->call_ns = 2 * npairs;
    std::vector<double> total((size_t)R * P::kSumsRow, 0.0);
    const ChainSource src{samples, seed, step, pair_offset, out_samples};
    if (int rc = for_each_pass(h, src, npairs, chunk, 2, total, [&](int64_t p0, int64_t np, int64_t ns, double* pass_sums) {
            const RegionScratch sc(N, g, ns, E, P::kSumsRow, P::kSurvivors, P::kThreads);
            if (int rc = P::pass(h, ns, g, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync((char*)out_log_ratio + p0 * E, (size_t)npairs * E, (char*)h->renyi.p + sc.lr, (size_t)np * E,
                                              (size_t)np * E, (size_t)R, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(sums, total.data(), (size_t)R * E / 4 * 8);
    P::finish(h, g, total, npairs, out_in_sector);
    return RNNWF_OK;
}

}  // namespace rnnwf
