// renyi_regions.hip - host driver of rnnwf_renyi2_regions (include/rnnwf.h): the second Renyi entropy of the positive GRU models
// (GRU1D, GRU1D_F64, one layer) for any list of regions given as site masks, by the replica swap trick; kernels in
// renyi_region_kernels.h and chain_kernels.h (prnn_masked_tail_kernel, PAIRED), the method in docs/renyi_regions.md; the launch table,
// refusals, base pass, pass size and pass loop are observable.h's.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed
// chain first.  Per pass of whole 16-chain blocks (the state budget, as renyi.hip): spins (the caller's, or drawn exactly as
// rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> site terms and region tails ->
// log-ratios and per-region sums of r and r^2.  The sums of the passes are added on the host in pass order.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "observable.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

constexpr int kMaxRegions = 65535;       // blockIdx.y of the assembly

// The regions of one call as the kernels read them
struct Regions {
    int R = 0, W = 0, nact = 0;
    std::vector<uint32_t> mask;          // [R][W], normalised
    std::vector<int32_t> first, order;   // [R]: f, 0 = empty; [nact]: non-empty regions, f ascending, ties by index
    double steps = 0.0;                  // sum over regions of N - f: cell evaluations per chain
};

// Scratch of one pass of ns chains in h->renyi; the call's masks, order and first sites lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per region
    Scratch(int N, int R, int W, int64_t ns) {
        Carve c;
        nblk = (ns / 2 + kRenyiThreads - 1) / kRenyiThreads;
        mask = c.take((size_t)R * W * 4);
        order = c.take((size_t)R * 4);
        first = c.take((size_t)R * 4);
        terms = c.take((size_t)N * ns * 8);
        tail = c.take((size_t)R * ns * 8);
        lr = c.take((size_t)R * (ns / 2) * 8);
        part = c.take((size_t)R * nblk * 16);
        sums = c.take((size_t)R * 16);
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
                return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: regions[%d][%d] = %d, a mask entry must be 0 or 1", r, n, (int)m[n]);
        const int32_t flip = m[0];                 // site 0 in A: take the complement
        for (int n = 0; n < N; ++n)
            if (m[n] ^ flip) {
                g.mask[(size_t)r * g.W + (n >> 5)] |= 1u << (n & 31);
                if (!g.first[r]) g.first[r] = n;
            }
        if (g.first[r]) {
            g.order.push_back(r);
            g.steps += (double)(N - g.first[r]);
        }
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    g.nact = (int)g.order.size();
    return 0;
}

// one pass over the ns chains packed in h->bits: sums_host (R, 2) of this pass; the log-ratios stay in h->renyi
int region_pass(rnnwf_handle* h, int64_t ns, const Regions& g, const Scratch& sc, double* sums_host) {
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
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = observable_refuse(h, "rnnwf_renyi2_regions")) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (nregions < 1 || nregions > kMaxRegions)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: nregions must be in 1..%d", kMaxRegions);
    if (npairs < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: npairs must be >= 1");
    if (!regions || !sums) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: regions and sums must be non-null");
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: pair_offset must be >= 0");
    Regions g;
    if (int rc = prepare(h, regions, nregions, g)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N, R = nregions;
    // pairs per pass: per block, beside the checkpoints, the terms (N x 16 x 8 bytes), the tails (R x 16 x 8) and the log-ratios
    // (R x 8 x 8)
    const int64_t chunk = blocks_per_pass(h, (size_t)N * kChains * 8 + (size_t)R * kChains * 8 + (size_t)R * (kChains / 2) * 8) * kChains / 2;
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
    std::vector<double> total((size_t)R * 2, 0.0);
    const ChainSource src{samples, seed, step, pair_offset, out_samples};
    if (int rc = for_each_pass(h, src, npairs, chunk, 2, total, [&](int64_t p0, int64_t np, int64_t ns, double* pass_sums) {
            const Scratch sc(N, R, g.W, ns);
            if (int rc = region_pass(h, ns, g, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + p0, (size_t)npairs * 8, (char*)h->renyi.p + sc.lr, (size_t)np * 8,
                                              (size_t)np * 8, (size_t)R, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(sums, total.data(), total.size() * 8);
    return RNNWF_OK;
}
