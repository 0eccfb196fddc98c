// crnn_observable.h - what the host drivers of the complex RNN's observable passes share: rnnwf_pauli_step_complex (crnn_pauli.hip)
// and rnnwf_renyi2_regions_complex (crnn_renyi.hip).  Both serve CRNN_U1 with one GRU layer and run, per pass of whole 16-chain
// blocks within the state budget: spins -> teacher-forced base pass on the one-wave f32 kernel with checkpoints (crnn_plain_base) ->
// their own kernels on chains restarted from the checkpoints.  Here are the launch table, the pass size, the sector check of the
// caller's samples and the model names of the refusals; the scratch carving, the chain source and the pass loop are observable.h's.
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

// the one-layer rows of crnn.hip's with_launch, with its waves per workgroup
template <class Fn>
bool with_crnn1(const rnnwf_handle* h, Fn&& fn) {
    switch (h->NFULL) {
        case 1: fn(CPauliLaunch<1, 4>()); return true;
        case 2: fn(CPauliLaunch<2, 4>()); return true;
        case 3: fn(CPauliLaunch<3, 4>()); return true;
        case 4: fn(CPauliLaunch<4, 4>()); return true;
        case 6: fn(CPauliLaunch<6, 8>()); return true;
        case 8: fn(CPauliLaunch<8, 4>()); return true;
        case 12: fn(CPauliLaunch<12, 4>()); return true;
        case 16: fn(CPauliLaunch<16, 4>()); return true;
    }
    return false;
}

// whole 16-chain blocks per pass within the state budget: per block the checkpoints and the pass's `bytes_per_block` beside them
inline int64_t crnn_blocks_per_pass(rnnwf_handle* h, size_t bytes_per_block) {
    const size_t per_block = (size_t)std::max(h->N - 1, 1) * crnn_hck_bytes_per_block(h) + bytes_per_block;
    return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
}

inline const char* model_name(int model) {
    static const char* const names[] = {"GRU1D", "GRU1D_PARITY", "CRNN_U1", "GRU1D_F64", "MDRNN2D", "LSTM1D_F64"};
    return model >= 0 && model < (int)(sizeof names / sizeof *names) ? names[model] : "unknown";
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
