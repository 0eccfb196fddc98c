// renyi_regions.hip - host driver of rnnwf_renyi2_regions (include/rnnwf.h): the second Renyi entropy of the positive GRU models
// (GRU1D, GRU1D_F64, one layer) for any list of regions given as site masks, by the replica swap trick; kernels in
// renyi_region_kernels.h, the method in docs/renyi_regions.md.
//
// Per call: the masks are checked, normalised (site 0 not in A: r_A = r_complement), packed into words and sorted longest mixed
// chain first.  Per pass of whole 16-chain blocks (the state budget, as renyi.hip): spins (the caller's, or drawn exactly as
// rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> site terms and region tails ->
// log-ratios and per-region sums of r and r^2.  The sums of the passes are added on the host in pass order.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "gru_kernels.h"
#include "models.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

constexpr int kMaxRegions = 65535;       // blockIdx.y of the assembly

template <typename T, int NFULL, int WAVES>
struct RegionLaunch {
    using L = GruLayout<T, NFULL, 1>;
    static int terms(rnnwf_handle* h, const SwapArgs& a) {
        return launch_persistent(h, kTimerBase, prnn_site_terms_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.nsb, WAVES, a);
    }
    static int region(rnnwf_handle* h, const RegionArgs& a) {
        return launch_persistent(h, kTimerFlip, prnn_region_swap_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.ntiles, WAVES, a);
    }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for a width without kernels: the rows and waves per workgroup of
// the swap pass (renyi.hip: with_swap), f64 at 53..68 units on 4 waves included; no instantiation uses scratch at these
// (profiles/renyi_regions_kernel_resources.txt)
template <class Fn>
bool with_region(const rnnwf_handle* h, Fn&& fn) {
    if (!h->f64) {
        switch (h->NFULL) {
            case 1: fn(RegionLaunch<float, 1, 4>()); return true;
            case 2: fn(RegionLaunch<float, 2, 4>()); return true;
            case 3: fn(RegionLaunch<float, 3, 4>()); return true;
            case 4: fn(RegionLaunch<float, 4, 4>()); return true;
            case 6: fn(RegionLaunch<float, 6, 8>()); return true;
            case 8: fn(RegionLaunch<float, 8, 4>()); return true;
            case 12: fn(RegionLaunch<float, 12, 4>()); return true;
            case 16: fn(RegionLaunch<float, 16, 4>()); return true;
        }
        return false;
    }
    switch (h->NFULL) {
        case 1: fn(RegionLaunch<double, 1, 4>()); return true;
        case 2: fn(RegionLaunch<double, 2, 4>()); return true;
        case 3: fn(RegionLaunch<double, 3, 4>()); return true;
        case 4: fn(RegionLaunch<double, 4, 4>()); return true;
        case 6: fn(RegionLaunch<double, 6, 4>()); return true;
    }
    return false;
}

bool has_kernel(const rnnwf_handle* h) { return with_region(h, [](auto) {}); }

// The regions of one call as the kernels read them
struct Regions {
    int R = 0, W = 0, nact = 0;
    std::vector<uint32_t> mask;          // [R][W], normalised
    std::vector<int32_t> first, order;   // [R]: f, 0 = empty; [nact]: non-empty regions, f ascending, ties by index
    double steps = 0.0;                  // sum over regions of N - f: cell evaluations per chain
};

// Scratch of one pass of ns chains in h->renyi, 256-byte aligned pieces; the call's masks, order and first sites lead, at offsets
// that do not depend on ns
struct Scratch {
    size_t mask, order, first, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per region
    Scratch(int N, int R, int W, int64_t ns) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        nblk = (ns / 2 + kRenyiThreads - 1) / kRenyiThreads;
        mask = 0;
        order = mask + al((size_t)R * W * 4);
        first = order + al((size_t)R * 4);
        terms = first + al((size_t)R * 4);
        tail = terms + al((size_t)N * ns * 8);
        lr = tail + al((size_t)R * ns * 8);
        part = lr + al((size_t)R * (ns / 2) * 8);
        sums = part + al((size_t)R * nblk * 16);
        bytes = sums + al((size_t)R * 16);
    }
};

// pairs per pass: whole 16-chain blocks of checkpoints and scratch within the state budget; per block the checkpoints, the terms
// (N x 16 x 8 bytes), the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
int64_t pairs_per_pass(rnnwf_handle* h, int R) {
    const int N = h->N;
    const size_t per_block = (size_t)std::max(N - 1, 1) * prnn_hck_bytes_per_block(h) + (size_t)N * kChains * 8
                             + (size_t)R * kChains * 8 + (size_t)R * (kChains / 2) * 8;
    const int64_t blocks = std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
    return blocks * kChains / 2;
}

int refuse(rnnwf_handle* h) {
    const char* why = nullptr;
    switch (h->model) {
        case RNNWF_MODEL_GRU1D_PARITY: why = "the parity model's symmetrised P is not autoregressive"; break;
        case RNNWF_MODEL_CRNN_U1: why = "not implemented for the complex RNN"; break;
        case RNNWF_MODEL_MDRNN2D: why = "not implemented for the 2D RNN (MDRNN)"; break;
        case RNNWF_MODEL_LSTM1D_F64: why = "not implemented for the LSTM cell"; break;
        default: if (h->NL > 1) why = "not implemented for stacked layers (one GRU layer only)";
    }
    return why ? h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: %s", why) : 0;
}

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
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * prnn_hck_bytes_per_block(h))) return rc;
    char* buf = (char*)h->renyi.p;
    PrnnArgs b = prnn_base_args(h, ns);
    b.bits = (uint32_t*)h->bits.p;
    b.hck = h->hck.p;
    if (int rc = prnn_plain_base(h, b)) return rc;
    SwapArgs t{};
    t.wimg = h->wimg.p;
    t.N = N;
    t.ns = ns;
    t.nsb = nsb;
    t.bits = (const uint32_t*)h->bits.p;
    t.hck = h->hck.p;
    t.terms = (double*)(buf + sc.terms);
    RegionArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.W = g.W;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = t.bits;
    a.hck = h->hck.p;
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)g.nact * nsb;
    if (g.nact > 0) {                              // N >= 2
        int rc = 0;
        with_region(h, [&](auto k) {
            using K = decltype(k);
            rc = K::terms(h, t);
            if (!rc) rc = K::region(h, a);
            if (!rc) h->work[1] += (double)nsb * g.steps * K::mfma_flops_per_step();
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
    if (int rc = refuse(h)) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (nregions < 1 || nregions > kMaxRegions)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: nregions must be in 1..%d", kMaxRegions);
    if (npairs < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: npairs must be >= 1");
    if (!regions || !sums) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: regions and sums must be non-null");
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: pair_offset must be >= 0");
    if (!has_kernel(h)) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_regions: no region kernel for NFULL=%d f64=%d", h->NFULL, (int)h->f64);
    Regions g;
    if (int rc = prepare(h, regions, nregions, g)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N, R = nregions;
    const int64_t chunk = pairs_per_pass(h, R);
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
    std::vector<double> total((size_t)R * 2, 0.0), pass((size_t)R * 2);
    for (int64_t p0 = 0; p0 < npairs; p0 += chunk) {
        const int64_t np = std::min(chunk, npairs - p0), ns = 2 * np;
        const Scratch sc(N, R, g.W, ns);
        if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * ns * 4)) return rc;
        if (samples) {
            if (int rc = upload_and_pack(h, samples + 2 * p0 * N, ns, h->bits, 0, nullptr)) return rc;
        } else {
            const Draw d{seed, step, 2 * (pair_offset + p0)};        // rnnwf_sample's draw (its own base-pass kernel)
            if (int rc = h->family->base(h, ns, &d)) return rc;
            if (out_samples)
                if (int rc = unpack_and_download(h, h->bits, ns, out_samples + 2 * p0 * N, nullptr)) return rc;
        }
        if (int rc = region_pass(h, ns, g, sc, pass.data())) return rc;
        if (out_log_ratio)
            RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + p0, (size_t)npairs * 8, (char*)h->renyi.p + sc.lr, (size_t)np * 8,
                                          (size_t)np * 8, (size_t)R, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass[k];
    }
    memcpy(sums, total.data(), total.size() * 8);
    return RNNWF_OK;
}
