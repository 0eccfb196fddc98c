// corr.hip - host driver of rnnwf_correlations (include/rnnwf.h): <sz_i>, <sz_i sz_j>, <sx_i> and <sx_i sx_j> of the positive GRU
// models (GRU1D, GRU1D_F64, one layer) for every site and pair at once; kernels in corr_kernels.h, the method in docs/correlations.md.
//
// Per pass of whole 16-chain blocks (the state budget, as tfim_eloc and the swap pass): spins (the caller's, or drawn exactly as
// rnnwf_sample draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> both outcomes of every site ->
// trunk pass (one flip, states kept) -> branch pass (second flip) -> log-ratios and sums.  The sums of the passes are added on the
// host in pass order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "corr_kernels.h"
#include "gru_kernels.h"
#include "models.h"

using namespace rnnwf;

namespace {

template <typename T, int NFULL, int WAVES>
struct CorrLaunch {
    using L = GruLayout<T, NFULL, 1>;
    static int both(rnnwf_handle* h, const CorrArgs& a) {
        return launch_persistent(h, kTimerBase, prnn_site_both_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.nsb, WAVES, a);
    }
    static int trunk(rnnwf_handle* h, const CorrArgs& a) {
        return launch_persistent(h, kTimerFlip, prnn_trunk_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.ntiles, WAVES, a);
    }
    static int branch(rnnwf_handle* h, const CorrArgs& a) {
        return launch_persistent(h, kTimerFlip, prnn_branch_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.ntiles, WAVES, a);
    }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for a width without kernels: the rows and waves per workgroup of
// the swap pass (renyi.hip: with_swap), f64 at 53..68 units on 4 waves included
template <class Fn>
bool with_corr(const rnnwf_handle* h, Fn&& fn) {
    if (!h->f64) {
        switch (h->NFULL) {
            case 1: fn(CorrLaunch<float, 1, 4>()); return true;
            case 2: fn(CorrLaunch<float, 2, 4>()); return true;
            case 3: fn(CorrLaunch<float, 3, 4>()); return true;
            case 4: fn(CorrLaunch<float, 4, 4>()); return true;
            case 6: fn(CorrLaunch<float, 6, 8>()); return true;
            case 8: fn(CorrLaunch<float, 8, 4>()); return true;
            case 12: fn(CorrLaunch<float, 12, 4>()); return true;
            case 16: fn(CorrLaunch<float, 16, 4>()); return true;
        }
        return false;
    }
    switch (h->NFULL) {
        case 1: fn(CorrLaunch<double, 1, 4>()); return true;
        case 2: fn(CorrLaunch<double, 2, 4>()); return true;
        case 3: fn(CorrLaunch<double, 3, 4>()); return true;
        case 4: fn(CorrLaunch<double, 4, 4>()); return true;
        case 6: fn(CorrLaunch<double, 6, 4>()); return true;
    }
    return false;
}

int64_t num_pairs(int N) { return (int64_t)N * (N - 1) / 2; }

// Scratch of one pass of ns chains in h->corr, 256-byte aligned pieces (the trunk states have their own buffer, h->tck)
struct Scratch {
    size_t bsel, both, suf, tsel, toth, tail, lr, z, zz, x, xx, bytes;
    Scratch(int N, int64_t ns) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t site = al((size_t)N * ns * 8), pair = al((size_t)std::max<int64_t>(num_pairs(N), 1) * ns * 8);
        bsel = 0;
        both = bsel + site;
        suf = both + site;
        tsel = suf + site;
        toth = tsel + pair;
        tail = toth + pair;
        lr = tail + pair;
        z = lr + al((size_t)(N + num_pairs(N)) * ns * 8);
        zz = z + al((size_t)N * 8);
        x = zz + al((size_t)N * N * 8);
        xx = x + al((size_t)N * 2 * 8);
        bytes = xx + al((size_t)N * N * 5 * 8);
    }
};

// chains per pass: whole 16-chain blocks of checkpoints, trunk states and scratch within the state budget
int64_t chains_per_pass(rnnwf_handle* h) {
    const int N = h->N;
    const size_t state = prnn_hck_bytes_per_block(h);
    const size_t per_block = (size_t)(std::max(N - 1, 1) + std::max<int64_t>(num_pairs(N), 1)) * state
                             + (size_t)(4 * N + 4 * num_pairs(N)) * kChains * 8;
    const int64_t blocks = std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
    return blocks * kChains;
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
    return why ? h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: %s", why) : 0;
}

// one pass over the ns chains packed in h->bits: the four sums of this pass into `out` (z | zz | x | xx); the log-ratios stay in h->corr
int corr_pass(rnnwf_handle* h, int64_t ns, const Scratch& sc, double* out) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains, NP = num_pairs(N);
    const size_t state = prnn_hck_bytes_per_block(h);
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * state)) return rc;
    if (int rc = ensure(h, h->tck, (size_t)std::max<int64_t>(NP, 1) * nsb * state)) return rc;
    if (int rc = ensure(h, h->corr, sc.bytes)) return rc;
    char* buf = (char*)h->corr.p;
    PrnnArgs b = prnn_base_args(h, ns);
    b.bits = (uint32_t*)h->bits.p;
    b.hck = h->hck.p;
    if (int rc = prnn_plain_base(h, b)) return rc;
    CorrArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.tck = h->tck.p;
    a.bsel = (double*)(buf + sc.bsel);
    a.both = (double*)(buf + sc.both);
    a.tsel = (double*)(buf + sc.tsel);
    a.toth = (double*)(buf + sc.toth);
    a.tail = (double*)(buf + sc.tail);
    int rc = 0;
    const bool found = with_corr(h, [&](auto k) {
        using K = decltype(k);
        rc = K::both(h, a);
        if (!rc && N > 1) {
            a.ntiles = (int64_t)(N - 1) * nsb;
            rc = K::trunk(h, a);
        }
        if (!rc && N > 2) {
            a.ntiles = (int64_t)(N - 1) * (N - 2) / 2 * nsb;
            rc = K::branch(h, a);
        }
        if (!rc) h->work[1] += (double)nsb * ((double)NP + (double)NP * (N - 2) / 3.0) * K::mfma_flops_per_step();
    });
    if (!found) return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: no kernel for NFULL=%d f64=%d", h->NFULL, (int)h->f64);
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
    if (int rc = refuse(h)) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: ns must be >= 1");
    if (!z_sums || !zz_sums || !x_sums || !xx_sums)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: z_sums, zz_sums, x_sums and xx_sums must be non-null");
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_correlations: sample_offset must be >= 0");
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N;
    const int64_t chunk = chains_per_pass(h), rows = N + num_pairs(N);
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    const size_t nz = N, nzz = (size_t)N * N, nx = (size_t)N * 2, nxx = (size_t)N * N * 5;
    std::vector<double> total(nz + nzz + nx + nxx, 0.0), pass(total.size());
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t n = std::min(chunk, ns - s0);
        const Scratch sc(N, n);
        if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * n * 4)) return rc;
        if (samples) {
            if (int rc = upload_and_pack(h, samples + s0 * N, n, h->bits, 0, nullptr)) return rc;
        } else {
            const Draw d{seed, step, sample_offset + s0};            // rnnwf_sample's draw (its own base-pass kernel)
            if (int rc = h->family->base(h, n, &d)) return rc;
            if (out_samples)
                if (int rc = unpack_and_download(h, h->bits, n, out_samples + s0 * N, nullptr)) return rc;
        }
        if (int rc = corr_pass(h, n, sc, pass.data())) return rc;
        if (out_log_ratio)
            RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + s0, (size_t)ns * 8, (char*)h->corr.p + sc.lr, (size_t)n * 8, (size_t)n * 8,
                                          (size_t)rows, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass[k];
    }
    memcpy(z_sums, total.data(), nz * 8);
    memcpy(zz_sums, total.data() + nz, nzz * 8);
    memcpy(x_sums, total.data() + nz + nzz, nx * 8);
    memcpy(xx_sums, total.data() + nz + nzz + nx, nxx * 8);
    return RNNWF_OK;
}
