// renyi.hip - host driver of rnnwf_renyi2_swap (include/rnnwf.h): the second Renyi entropy of the positive GRU models (GRU1D,
// GRU1D_F64, one layer) for every cut at once by the replica swap trick; kernels in renyi_kernels.h, the method in docs/renyi.md.
//
// Per pass of whole 16-chain blocks (the state budget, as tfim_eloc): spins (the caller's, or drawn exactly as rnnwf_sample
// draws them) -> teacher-forced base pass on the one-wave kernel with checkpoints -> site terms and swap tails -> log-ratios and
// per-cut sums of r and r^2.  The sums of the passes are added on the host in pass order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "gru_kernels.h"
#include "models.h"
#include "renyi_kernels.h"

using namespace rnnwf;

namespace {

template <typename T, int NFULL, int WAVES>
struct SwapLaunch {
    using L = GruLayout<T, NFULL, 1>;
    static int terms(rnnwf_handle* h, const SwapArgs& a) {
        return launch_persistent(h, kTimerBase, prnn_site_terms_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.nsb, WAVES, a);
    }
    static int swap(rnnwf_handle* h, const SwapArgs& a) {
        return launch_persistent(h, kTimerFlip, prnn_swap_kernel<T, NFULL, WAVES>, WAVES * 64, L::LDS_BYTES, a.ntiles, WAVES, a);
    }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for a width without kernels: the one-layer rows of prnn.hip's
// table, with its flip pass's waves per workgroup - except f64 at 53..68 units: 4, not 8 (at 8 the swap kernel spills 20 bytes per
// lane to scratch; profiles/renyi_kernel_resources.txt)
template <class Fn>
bool with_swap(const rnnwf_handle* h, Fn&& fn) {
    if (!h->f64) {
        switch (h->NFULL) {
            case 1: fn(SwapLaunch<float, 1, 4>()); return true;
            case 2: fn(SwapLaunch<float, 2, 4>()); return true;
            case 3: fn(SwapLaunch<float, 3, 4>()); return true;
            case 4: fn(SwapLaunch<float, 4, 4>()); return true;
            case 6: fn(SwapLaunch<float, 6, 8>()); return true;
            case 8: fn(SwapLaunch<float, 8, 4>()); return true;
            case 12: fn(SwapLaunch<float, 12, 4>()); return true;
            case 16: fn(SwapLaunch<float, 16, 4>()); return true;
        }
        return false;
    }
    switch (h->NFULL) {
        case 1: fn(SwapLaunch<double, 1, 4>()); return true;
        case 2: fn(SwapLaunch<double, 2, 4>()); return true;
        case 3: fn(SwapLaunch<double, 3, 4>()); return true;
        case 4: fn(SwapLaunch<double, 4, 4>()); return true;
        case 6: fn(SwapLaunch<double, 6, 4>()); return true;
    }
    return false;
}

// Scratch of one pass of ns chains in h->renyi, 256-byte aligned pieces
struct Scratch {
    size_t terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per cut
    Scratch(int N, int64_t ns) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        nblk = (ns / 2 + kRenyiThreads - 1) / kRenyiThreads;
        terms = 0;
        tail = terms + al((size_t)N * ns * 8);
        lr = tail + al((size_t)std::max(N - 1, 1) * ns * 8);
        part = lr + al((size_t)(N + 1) * (ns / 2) * 8);
        sums = part + al((size_t)(N + 1) * nblk * 16);
        bytes = sums + al((size_t)(N + 1) * 16);
    }
};

// pairs per pass: whole 16-chain blocks of checkpoints and scratch within the state budget
int64_t pairs_per_pass(rnnwf_handle* h) {
    const int N = h->N;
    const size_t per_block = (size_t)std::max(N - 1, 1) * prnn_hck_bytes_per_block(h) + Scratch(N, kChains).bytes;
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
    return why ? h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: %s", why) : 0;
}

// one pass over the ns chains packed in h->bits: sums_host (N+1, 2) of this pass; the log-ratios stay in h->renyi
int swap_pass(rnnwf_handle* h, int64_t ns, const Scratch& sc, double* sums_host) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * prnn_hck_bytes_per_block(h))) return rc;
    if (int rc = ensure(h, h->renyi, sc.bytes)) return rc;
    char* buf = (char*)h->renyi.p;
    PrnnArgs b = prnn_base_args(h, ns);
    b.bits = (uint32_t*)h->bits.p;
    b.hck = h->hck.p;
    if (int rc = prnn_plain_base(h, b)) return rc;
    SwapArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.ns = ns;
    a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.tail = (double*)(buf + sc.tail);
    a.terms = (double*)(buf + sc.terms);
    a.ntiles = (int64_t)(N - 1) * nsb;
    if (N > 1) {
        int rc = 0;
        const bool found = with_swap(h, [&](auto k) {
            using K = decltype(k);
            rc = K::terms(h, a);
            if (!rc) rc = K::swap(h, a);
            if (!rc) h->work[1] += (double)nsb * N * (N - 1) / 2.0 * K::mfma_flops_per_step();
        });
        if (!found) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: no swap kernel for NFULL=%d f64=%d", h->NFULL, (int)h->f64);
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
    if (int rc = refuse(h)) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
    if (npairs < 1 || !sums) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: npairs must be >= 1 and sums non-null");
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "rnnwf_renyi2_swap: pair_offset must be >= 0");
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int N = h->N;
    const int64_t chunk = pairs_per_pass(h);
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    std::vector<double> total((size_t)(N + 1) * 2, 0.0), pass((size_t)(N + 1) * 2);
    for (int64_t p0 = 0; p0 < npairs; p0 += chunk) {
        const int64_t np = std::min(chunk, npairs - p0), ns = 2 * np;
        const Scratch sc(N, ns);
        if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * ns * 4)) return rc;
        if (samples) {
            if (int rc = upload_and_pack(h, samples + 2 * p0 * N, ns, h->bits, 0, nullptr)) return rc;
        } else {
            const Draw d{seed, step, 2 * (pair_offset + p0)};        // rnnwf_sample's draw (its own base-pass kernel)
            if (int rc = h->family->base(h, ns, &d)) return rc;
            if (out_samples)
                if (int rc = unpack_and_download(h, h->bits, ns, out_samples + 2 * p0 * N, nullptr)) return rc;
        }
        if (int rc = swap_pass(h, ns, sc, pass.data())) return rc;
        if (out_log_ratio)
            RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + p0, (size_t)npairs * 8, (char*)h->renyi.p + sc.lr, (size_t)np * 8,
                                          (size_t)np * 8, (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass[k];
    }
    memcpy(sums, total.data(), total.size() * 8);
    return RNNWF_OK;
}
