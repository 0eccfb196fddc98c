// observable.h - what the host drivers of the observable passes share.  The launch table, the refusals, the common kernel arguments,
// the base pass and the pass size serve the positive GRU models with one layer (GRU1D, GRU1D_F64): rnnwf_renyi2_swap (renyi.hip),
// rnnwf_correlations (corr.hip), rnnwf_renyi2_regions (renyi_regions.hip) and rnnwf_pauli_step (pauli.hip).  The scratch carving, the
// chain source and the pass loop serve every family: the complex RNN's pieces are in crnn_observable.h, the 2D RNN's in
// mdrnn_observable.h, the drivers of the Pauli and region-Renyi entry points of all three in pauli_driver.h and region_driver.h.
// Per pass of whole 16-chain blocks within the state budget: spins (the caller's, or drawn exactly as rnnwf_sample draws them) ->
// base pass that keeps the states -> the entry's own kernels on chains restarted from them -> log-ratios and sums.  The sums of the
// passes are added on the host in pass order.  Each .hip instantiates its own kernels, under its own flags.
#pragma once
#include <algorithm>
#include <vector>

#include "chain_kernels.h"
#include "gru_kernels.h"
#include "models.h"
#include "shapes.h"

namespace rnnwf {

template <typename T_, int NFULL_, int WAVES_>
struct Gru1Launch {
    using T = T_;
    using L = GruLayout<T_, NFULL_, 1>;
    static constexpr int NFULL = NFULL_, WAVES = WAVES_;
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for a width without kernels: the one-layer rows of the positive
// GRU's table at the waves per workgroup shapes.h gives these passes (kGru1Waves).  The rows are every width rnnwf_create accepts
// for these models.
template <typename T, int NFULL, int WAVES> using Gru1Row = Gru1Launch<T, NFULL, kGru1Waves<T, NFULL, WAVES>>;
template <class Fn>
bool with_gru1(const rnnwf_handle* h, Fn&& fn) { return with_layer_kernels<Gru1Row>(GruKernels(), h, fn); }

inline bool has_kernel(const rnnwf_handle* h) { return with_gru1(h, [](auto) {}); }

// kern (an instantiation for launch class K) as a persistent kernel, one item (16-chain block or tile) per wave at a time
template <class K, typename Kern, typename Args>
int launch_waves(rnnwf_handle* h, K, TimerId id, Kern kern, int64_t items, const Args& a) {
    return launch_persistent(h, id, kern, K::WAVES * 64, K::L::LDS_BYTES, items, K::WAVES, a);
}

// 0, or RNNWF_ERR_INVALID with "<entry>: <why>" for a model the observable passes do not serve.  Called before anything is touched:
// a refused call leaves the resident batch usable.
inline int observable_refuse(rnnwf_handle* h, const char* entry) {
    const char* why = nullptr;
    switch (h->model) {
        case RNNWF_MODEL_GRU1D_PARITY: why = "the parity model's symmetrised P is not autoregressive"; break;
        case RNNWF_MODEL_CRNN_U1: why = "not implemented for the complex RNN"; break;
        case RNNWF_MODEL_MDRNN2D: why = "not implemented for the 2D RNN (MDRNN)"; break;
        case RNNWF_MODEL_LSTM1D_F64: why = "not implemented for the LSTM cell"; break;
        default: if (h->NL > 1) why = "not implemented for stacked layers (one GRU layer only)";
    }
    if (why) return h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why);
    if (!has_kernel(h)) return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for NFULL=%d f64=%d", entry, h->NFULL, (int)h->f64);
    return 0;
}

// the arguments of a pass over the ns chains packed in h->bits, checkpoints in h->hck
inline ChainArgs chain_args(rnnwf_handle* h, int64_t ns) {
    ChainArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.W = (h->N + 31) / 32;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    return a;
}

// the teacher-forced base pass over the ns chains in h->bits on the one-wave kernel, checkpoints into h->hck; out_lp: [ns] log P on
// the device, or nullptr
inline int observable_base(rnnwf_handle* h, int64_t ns, double* out_lp) {
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(h->N - 1, 1) * nsb * prnn_hck_bytes_per_block(h))) return rc;
    PrnnArgs b = prnn_base_args(h, ns);
    b.bits = (uint32_t*)h->bits.p;
    b.hck = h->hck.p;
    b.out_lp = out_lp;
    return prnn_plain_base(h, b);
}

// whole 16-chain blocks per pass within the state budget: per block the checkpoints and the pass's `bytes_per_block` beside them
inline int64_t blocks_per_pass(rnnwf_handle* h, size_t bytes_per_block) {
    const size_t per_block = (size_t)std::max(h->N - 1, 1) * prnn_hck_bytes_per_block(h) + bytes_per_block;
    return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
}

// Scratch of one pass carved into 256-byte aligned pieces: take(bytes) is the next piece's offset, `bytes` the total so far.  A
// piece's offset depends on the sizes of the pieces before it alone.
struct Carve {
    size_t bytes = 0;
    size_t take(size_t b) {
        const size_t at = bytes;
        bytes += (b + 255) & ~(size_t)255;
        return at;
    }
};

// Where the chains come from: the caller's samples, or drawn as rnnwf_sample draws them at (seed, step, offset + chain) and, if
// out_samples, copied back
struct ChainSource {
    const int32_t* samples;
    uint64_t seed, step;
    int64_t offset;              // in units (chains or pairs)
    int32_t* out_samples;
};

// The pass loop of every family: `count` units (chains_per_unit = 1: chains, 2: pairs) in passes of `chunk`.  Per pass: the spins into
// h->bits in the family's site order (Family::site_maps) - after the caller's samples the family's base pass, where that is what
// keeps the states (Family::base_keeps_states) - then pass(u0, n_units, ns, pass_sums) launches and queues its own copies to the host
// (this pass's sums into pass_sums, total.size() doubles); after the synchronisation pass_sums is added to `total`, in pass order.
template <class Pass>
int for_each_pass(rnnwf_handle* h, const ChainSource& src, int64_t count, int64_t chunk, int chains_per_unit, std::vector<double>& total,
                  Pass&& pass) {
    const int N = h->N;
    const Family& f = *h->family;
    const int32_t *col_of_pos = nullptr, *pos_of_site = nullptr;
    if (f.site_maps)
        if (int rc = f.site_maps(h, &col_of_pos, &pos_of_site)) return rc;
    std::vector<double> pass_sums(total.size());
    for (int64_t u0 = 0; u0 < count; u0 += chunk) {
        const int64_t nu = std::min(chunk, count - u0), ns = chains_per_unit * nu, s0 = chains_per_unit * u0;
        if (int rc = ensure(h, h->bits, (size_t)(N + 31) / 32 * ns * 4)) return rc;
        if (src.samples) {
            if (int rc = upload_and_pack(h, src.samples + s0 * N, ns, h->bits, 0, col_of_pos)) return rc;
            if (f.base_keeps_states)
                if (int rc = f.base(h, ns, nullptr)) return rc;
        } else {
            const Draw d{src.seed, src.step, chains_per_unit * src.offset + s0};      // rnnwf_sample's draw (its own base-pass kernel)
            if (int rc = f.base(h, ns, &d)) return rc;
            if (src.out_samples)
                if (int rc = unpack_and_download(h, h->bits, ns, src.out_samples + s0 * N, pos_of_site)) return rc;
        }
        if (int rc = pass(u0, nu, ns, pass_sums.data())) return rc;
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass_sums[k];
    }
    return 0;
}

// the refusal of a handle whose parameters are not committed: RNNWF_ERR_STATE, or (the 2D entries) RNNWF_ERR_INVALID with the entry
inline int refuse_uncommitted(rnnwf_handle* h, const char* entry, bool invalid_with_entry) {
    if (h->committed) return 0;
    if (invalid_with_entry) return h->fail(RNNWF_ERR_INVALID, "%s: parameters not committed (call rnnwf_commit_params)", entry);
    return h->fail(RNNWF_ERR_STATE, "parameters not committed (call rnnwf_commit_params)");
}

}  // namespace rnnwf
