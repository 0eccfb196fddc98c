// corr.hip - host driver of rnnwf_correlations (include/rnnwf.h): <sz_i>, <sz_i sz_j>, <sx_i> and <sx_i sx_j> of the positive GRU
// models (GRU1D, GRU1D_F64, one layer) for every site and pair at once; kernels in corr_kernels.h, the method in docs/correlations.md.
//
// The launch table, refusals, base pass, pass size and pass loop are observable.h's.  Per pass of whole 16-chain blocks (the state
// budget, as tfim_eloc and the swap pass): spins (the caller's, or drawn exactly as
// rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> both outcomes of every site ->
// trunk pass (one flip, states kept) -> branch pass (second flip) -> log-ratios and sums.  The sums of the passes are added on the
// host in pass order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "corr_kernels.h"
#include "observable.h"

using namespace rnnwf;

namespace {

int64_t num_pairs(int N) { return (int64_t)N * (N - 1) / 2; }

// Scratch of one pass of ns chains in h->corr (the trunk states have their own buffer, h->tck)
struct Scratch {
    size_t bsel, both, suf, tsel, toth, tail, lr, z, zz, x, xx, bytes;
    Scratch(int N, int64_t ns) {
        Carve c;
        const size_t site = (size_t)N * ns * 8, pair = (size_t)std::max<int64_t>(num_pairs(N), 1) * ns * 8;
        bsel = c.take(site);
        both = c.take(site);
        suf = c.take(site);
        tsel = c.take(pair);
        toth = c.take(pair);
        tail = c.take(pair);
        lr = c.take((size_t)(N + num_pairs(N)) * ns * 8);
        z = c.take((size_t)N * 8);
        zz = c.take((size_t)N * N * 8);
        x = c.take((size_t)N * 2 * 8);
        xx = c.take((size_t)N * N * 5 * 8);
        bytes = c.bytes;
    }
};

// one pass over the ns chains packed in h->bits: the four sums of this pass into `out` (z | zz | x | xx); the log-ratios stay in h->corr
int corr_pass(rnnwf_handle* h, int64_t ns, const Scratch& sc, double* out) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains, NP = num_pairs(N);
    if (int rc = observable_base(h, ns, nullptr)) return rc;
    if (int rc = ensure(h, h->tck, (size_t)std::max<int64_t>(NP, 1) * nsb * prnn_hck_bytes_per_block(h))) return rc;
    if (int rc = ensure(h, h->corr, sc.bytes)) return rc;
    char* buf = (char*)h->corr.p;
    CorrArgs a{chain_args(h, ns)};
    a.tck = h->tck.p;
    a.bsel = (double*)(buf + sc.bsel);
    a.both = (double*)(buf + sc.both);
    a.tsel = (double*)(buf + sc.tsel);
    a.toth = (double*)(buf + sc.toth);
    a.tail = (double*)(buf + sc.tail);
    int rc = 0;
    with_gru1(h, [&](auto k) {
        using K = decltype(k);
        rc = launch_waves(h, k, kTimerBase, prnn_site_both_kernel<typename K::T, K::NFULL, K::WAVES>, nsb, a);
        if (!rc && N > 1) {
            a.ntiles = (int64_t)(N - 1) * nsb;
            rc = launch_waves(h, k, kTimerFlip, prnn_trunk_kernel<typename K::T, K::NFULL, K::WAVES>, a.ntiles, a);
        }
        if (!rc && N > 2) {
            a.ntiles = (int64_t)(N - 1) * (N - 2) / 2 * nsb;
            rc = launch_waves(h, k, kTimerFlip, prnn_branch_kernel<typename K::T, K::NFULL, K::WAVES>, a.ntiles, a);
        }
        if (!rc) h->work[1] += (double)nsb * ((double)NP + (double)NP * (N - 2) / 3.0) * K::mfma_flops_per_step();
    });
    if (rc) return rc;
    h->work[0] += (double)ns * ((double)NP + (double)NP * (N - 2) / 3.0);     // N(N-1)/2 trunk + N(N-1)(N-2)/6 branch evaluations
    {
        TimedLaunch tl(h, kTimerAssembly);
        const unsigned nblk = (unsigned)((ns + kCorrThreads - 1) / kCorrThreads);
        double* lr = (double*)(buf + sc.lr);
        corr_suffix_kernel<<<nblk, kCorrThreads, 0, h->stream>>>(a.bsel, N, ns, (double*)(buf + sc.suf));
        RNNWF_HIP(h, hipGetLastError());
        corr_assemble_kernel<<<dim3(nblk, (unsigned)N), kCorrThreads, 0, h->stream>>>(a, (const double*)(buf + sc.suf), lr);
        RNNWF_HIP(h, hipGetLastError());
        RNNWF_HIP(h, hipMemsetAsync(buf + sc.xx, 0, (size_t)N * N * 5 * 8, h->stream));      // entries with i >= j stay 0
        corr_sums_kernel<<<(unsigned)(N + NP), kCorrThreads, 0, h->stream>>>(lr, N, ns, (double*)(buf + sc.x), (double*)(buf + sc.xx));
        RNNWF_HIP(h, hipGetLastError());
        corr_diag_kernel<<<dim3((unsigned)N, (unsigned)N), kCorrThreads, 0, h->stream>>>(a.bits, N, ns, (double*)(buf + sc.z),
                                                                                        (double*)(buf + sc.zz));
        RNNWF_HIP(h, hipGetLastError());
    }
    // z | zz | x | xx are contiguous up to their alignment padding: four copies into the packed host vector
    const size_t nz = N, nzz = (size_t)N * N, nx = (size_t)N * 2, nxx = (size_t)N * N * 5;
    RNNWF_HIP(h, hipMemcpyAsync(out, buf + sc.z, nz * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz, buf + sc.zz, nzz * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz + nzz, buf + sc.x, nx * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(out + nz + nzz + nx, buf + sc.xx, nxx * 8, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

}  // namespace

extern "C" int rnnwf_correlations(rnnwf_handle* h, const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step,
                                  int64_t sample_offset, double* z_sums, double* zz_sums, double* x_sums, double* xx_sums,
                                  double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = observable_refuse(h, "rnnwf_correlations")) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: ns must be >= 1");
    if (!z_sums || !zz_sums || !x_sums || !xx_sums)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: z_sums, zz_sums, x_sums and xx_sums must be non-null");
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: sample_offset must be >= 0");
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N;
    // chains per pass: per block the trunk states and, beside them and the checkpoints, 4 N + 4 N(N-1)/2 rows of 16 doubles
    const int64_t NP = num_pairs(N), rows = N + NP;
    const int64_t chunk = kChains * blocks_per_pass(h, (size_t)std::max<int64_t>(NP, 1) * prnn_hck_bytes_per_block(h)
                                                           + (size_t)(4 * N + 4 * NP) * kChains * 8);
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    const size_t nz = N, nzz = (size_t)N * N, nx = (size_t)N * 2, nxx = (size_t)N * N * 5;
    std::vector<double> total(nz + nzz + nx + nxx, 0.0);
    const ChainSource src{samples, seed, step, sample_offset, out_samples};
    if (int rc = for_each_pass(h, src, ns, chunk, 1, total, [&](int64_t s0, int64_t, int64_t n, double* pass_sums) {
            const Scratch sc(N, n);
            if (int rc = corr_pass(h, n, sc, pass_sums)) return rc;
            if (out_log_ratio)
                RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + s0, (size_t)ns * 8, (char*)h->corr.p + sc.lr, (size_t)n * 8, (size_t)n * 8,
                                              (size_t)rows, hipMemcpyDeviceToHost, h->stream));
            return 0;
        }))
        return rc;
    memcpy(z_sums, total.data(), nz * 8);
    memcpy(zz_sums, total.data() + nz, nzz * 8);
    memcpy(x_sums, total.data() + nz + nzz, nx * 8);
    memcpy(xx_sums, total.data() + nz + nzz + nx, nxx * 8);
    return RNNWF_OK;
}
