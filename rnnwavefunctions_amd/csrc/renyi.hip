// renyi.hip - host driver of rnnwf_renyi2_swap (include/rnnwf.h): the second Renyi entropy of the positive GRU models (GRU1D,
// GRU1D_F64, one layer) for every cut at once by the replica swap trick; kernels in renyi_kernels.h, the method in docs/renyi.md.
//
// The launch table, refusals, base pass, pass size and pass loop are observable.h's, shared with corr.hip, renyi_regions.hip and
// pauli.hip.  Per pass of whole 16-chain blocks (the state budget, as tfim_eloc): spins (the caller's, or drawn exactly as rnnwf_sample
// draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> site terms and swap tails -> log-ratios and
// per-cut sums of r and r^2.  The sums of the passes are added on the host in pass order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "observable.h"
#include "renyi_kernels.h"

using namespace rnnwf;

namespace {

// Scratch of one pass of ns chains in h->renyi
struct Scratch {
    size_t terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per cut
    Scratch(int N, int64_t ns) {
        Carve c;
        nblk = (ns / 2 + kRenyiThreads - 1) / kRenyiThreads;
        terms = c.take((size_t)N * ns * 8);
        tail = c.take((size_t)std::max(N - 1, 1) * ns * 8);
        lr = c.take((size_t)(N + 1) * (ns / 2) * 8);
        part = c.take((size_t)(N + 1) * nblk * 16);
        sums = c.take((size_t)(N + 1) * 16);
        bytes = c.bytes;
    }
};

// one pass over the ns chains packed in h->bits: sums_host (N+1, 2) of this pass; the log-ratios stay in h->renyi
int swap_pass(rnnwf_handle* h, int64_t ns, const Scratch& sc, double* sums_host) {
    const int N = h->N;
    if (int rc = observable_base(h, ns, nullptr)) return rc;
    if (int rc = ensure(h, h->renyi, sc.bytes)) return rc;
    char* buf = (char*)h->renyi.p;
    SwapArgs a{chain_args(h, ns)};
    a.tail = (double*)(buf + sc.tail);
    a.terms = (double*)(buf + sc.terms);
    a.ntiles = (int64_t)(N - 1) * a.nsb;
    if (N > 1) {
        int rc = 0;
        with_gru1(h, [&](auto k) {
            using K = decltype(k);
            rc = launch_waves(h, k, kTimerBase, prnn_site_terms_kernel<typename K::T, K::NFULL, K::WAVES>, a.nsb, a);
            if (!rc) rc = launch_waves(h, k, kTimerFlip, prnn_swap_kernel<typename K::T, K::NFULL, K::WAVES>, a.ntiles, a);
            if (!rc) h->work[1] += (double)a.nsb * N * (N - 1) / 2.0 * K::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * N * (N - 1) / 2.0;          // N (N - 1) cell evaluations per pair
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        renyi_assemble_kernel<<<dim3((unsigned)sc.nblk, (unsigned)(N + 1)), kRenyiThreads, 0, h->stream>>>(
            a.tail, a.terms, N, ns, (double*)(buf + sc.lr), (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)(N + 1), kRenyiThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk,
                                                                             (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)(N + 1) * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_renyi2_swap(rnnwf_handle* h, const int32_t* samples, int64_t npairs, uint64_t seed, uint64_t step,
                                 int64_t pair_offset, double* sums, double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = observable_refuse(h, "rnnwf_renyi2_swap")) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (npairs < 1 || !sums) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: npairs must be >= 1 and sums non-null");
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: pair_offset must be >= 0");
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N;
    const int64_t chunk = blocks_per_pass(h, Scratch(N, kChains).bytes) * kChains / 2;      // pairs per pass
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    std::vector<double> total((size_t)(N + 1) * 2, 0.0);
    const ChainSource src{samples, seed, step, pair_offset, out_samples};
    if (int rc = for_each_pass(h, src, npairs, chunk, 2, total, [&](int64_t p0, int64_t np, int64_t ns, double* pass_sums) {
            const Scratch sc(N, ns);
            if (int rc = swap_pass(h, ns, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + p0, (size_t)npairs * 8, (char*)h->renyi.p + sc.lr, (size_t)np * 8,
                                              (size_t)np * 8, (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(sums, total.data(), total.size() * 8);
    return RNNWF_OK;
}
