// crnn_observable.h - what the complex RNN's policies of the Pauli and region-Renyi drivers share: rnnwf_pauli_step_complex
// (crnn_pauli.hip, pauli_driver.h) and rnnwf_renyi2_regions_complex (crnn_renyi.hip, region_driver.h).  Both serve CRNN_U1 with one
// GRU layer and run, per pass of whole 16-chain blocks within the state budget: spins -> teacher-forced base pass on the one-wave f32
// kernel with checkpoints -> their own kernels on chains restarted from the checkpoints.  Here are the launch table, the model
// refusal, the base pass, the pass size and the sector check of the caller's samples.
#pragma once
#include <algorithm>

#include "crnn_kernels.h"
#include "observable.h"

namespace rnnwf {

template <int NFULL_, int WAVES_>
struct CPauliLaunch {
    using L = GruLayout<float, NFULL_, 3>;
    static constexpr int NFULL = NFULL_, WAVES = WAVES_;
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// the one-layer rows of the complex RNN's table (shapes.h), with its waves per workgroup
template <class Fn>
bool with_crnn1(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<CPauliLaunch>(CrnnKernels(), h, fn); }

// whole 16-chain blocks per pass within the state budget: per block the checkpoints and the pass's `bytes_per_block` beside them
inline int64_t crnn_blocks_per_pass(rnnwf_handle* h, size_t bytes_per_block) {
    const size_t per_block = (size_t)std::max(h->N - 1, 1) * crnn_hck_bytes_per_block(h) + bytes_per_block;
    return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
}

// 0, or RNNWF_ERR_INVALID for another model, stacked layers or a width without kernels; gru_entry, md_entry: the entry points that
// serve the GRU models and the 2D RNN
inline int crnn_refuse(rnnwf_handle* h, const char* entry, const char* gru_entry, const char* md_entry) {
    if (h->model != RNNWF_MODEL_CRNN_U1)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the complex RNN (CRNN_U1) only, this handle's model is %s; %s serves the GRU models, %s "
                       "the 2D RNN", entry, model_name(h->model), gru_entry, md_entry);
    if (h->NL > 1) return h->fail(RNNWF_ERR_INVALID, "%s: not implemented for stacked layers (one GRU layer only)", entry);
    if (!with_crnn1(h, [](auto) {})) return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for NFULL=%d", entry, h->NFULL);
    return 0;
}

// the teacher-forced base pass over the ns chains in h->bits on the one-wave kernel, checkpoints into h->hck; tot: [ns] log psi on the
// device, or nullptr
inline int crnn_observable_base(rnnwf_handle* h, int64_t ns, double2* tot) {
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(h->N - 1, 1) * nsb * crnn_hck_bytes_per_block(h))) return rc;
    CrnnArgs b = crnn_base_args(h, ns);
    b.bits = (uint32_t*)h->bits.p;
    b.hck = h->hck.p;
    b.tot = tot;
    return crnn_plain_base(h, b);
}

// 0, or RNNWF_ERR_INVALID naming the first of the caller's ns chains outside the zero-magnetisation sector: its own log psi is -inf
// and every ratio against it +inf or NaN
inline int crnn_check_sector(rnnwf_handle* h, const char* entry, const int32_t* samples, int64_t ns) {
    for (int64_t s = 0; s < ns; ++s) {
        int up = 0;
        for (int n = 0; n < h->N; ++n) up += samples[s * h->N + n] != 0;
        if (up != h->N / 2)
            return h->fail(RNNWF_ERR_INVALID, "%s: samples[%lld] has %d up spins, the zero-magnetisation sector has %d", entry, (long long)s,
                           up, h->N / 2);
    }
    return 0;
}

}  // namespace rnnwf
