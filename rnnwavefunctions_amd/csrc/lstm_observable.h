// lstm_observable.h - what the host drivers of the observable passes of the LSTM wave function share: rnnwf_pauli_step_lstm and
// rnnwf_lstm_pauli_gradient_step (lstm_pauli.hip), rnnwf_renyi2_regions_lstm (lstm_renyi.hip), rnnwf_correlations_lstm (lstm_corr.hip,
// which derives its own launch class from this one).  The launch class of a width, the walk
// over the LSTM's table, the size of a checkpoint row and the refusals.  All serve LSTM1D_F64 (one layer, 1..68 units, float64, raster
// path); kernels in lstm_pauli_kernels.h.  Each .hip instantiates its own kernels, under its own flags.
#pragma once
#include "lstm_pauli_kernels.h"
#include "models.h"
#include "observable.h"
#include "shapes.h"

namespace rnnwf {

// WAVES: waves per workgroup of the LSTM's flip pass (shapes.h), taken by the tails; BWAVES: of the base pass - at 68 units one
// wave per SIMD, as lstm.hip's base pass: its checkpoint stores beside h, c and h' need more than the 256 registers of two waves per
// SIMD.  PWAVES: of the PAIRED tails (lstm_renyi.hip) - the !PAIRED row's at every NFULL (profiles/lstm_renyi_kernel_resources.txt).
// All shrink their workgroups for small batches (handle.h: launch_shrinking).  profiles/lstm_pauli_kernel_resources.txt
template <int NFULL, int WAVES>
struct LPauli {
    using L = LstmLayout<NFULL>;
    static constexpr int BWAVES = NFULL == 4 ? 4 : WAVES;
    static constexpr int PWAVES = WAVES;
    static int base(rnnwf_handle* h, const LstmTermsArgs& a) {
        return launch_shrinking<BWAVES>(h, kTimerBase, lstm_site_terms_kernel<NFULL, BWAVES>, L::BYTES, a.nsb, a);
    }
    static int tails(rnnwf_handle* h, const MaskArgs& a) {
        return launch_shrinking<WAVES>(h, kTimerFlip, lstm_masked_tail_kernel<NFULL, WAVES>, L::BYTES, a.ntiles, a);
    }
    // the tails of the mixed chains of replica pairs (2p, 2p + 1): a.mask the normalised region masks, no tile with f = 0
    static int paired_tails(rnnwf_handle* h, const MaskArgs& a) {
        return launch_shrinking<PWAVES>(h, kTimerFlip, lstm_masked_tail_kernel<NFULL, PWAVES, true>, L::BYTES, a.ntiles, a);
    }
    static size_t hck_bytes_per_block() { return (size_t)2 * L::KT * 64 * sizeof(double); }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

template <class Fn>
bool with_lpauli(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<LPauli>(LstmKernels(), h, fn); }

inline size_t hck_bytes_per_block(const rnnwf_handle* h) {
    size_t b = 0;
    with_lpauli(h, [&](auto k) { b = decltype(k)::hck_bytes_per_block(); });
    return b;
}

// which entries a refusal names to a handle of another model
enum class LstmEntryKind { Pauli, Renyi, Corr };

// 0, or RNNWF_ERR_INVALID "<entry>: ..." for a handle these entries do not serve, naming the entry that does.  Called before
// anything is touched.
inline int lstm_pauli_refuse(rnnwf_handle* h, const char* entry, LstmEntryKind kind = LstmEntryKind::Pauli) {
    const bool renyi = kind == LstmEntryKind::Renyi;
    if (h->model != RNNWF_MODEL_LSTM1D_F64 && kind == LstmEntryKind::Corr) {
        // rnnwf_correlations is the one other all-pair pass: it serves the positive GRU models with one layer
        const bool gru = h->model == RNNWF_MODEL_GRU1D || h->model == RNNWF_MODEL_GRU1D_F64;
        const char* other = gru ? (h->NL > 1 ? "no all-pair correlation pass serves stacked GRU layers (rnnwf_correlations: one GRU layer)"
                                             : "rnnwf_correlations serves the one-layer GRU models")
                                : "no all-pair correlation pass serves this model (rnnwf_correlations: the one-layer GRU models)";
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the LSTM cell (LSTM1D_F64) only, this handle's model is %s; %s", entry,
                       model_name(h->model), other);
    }
    if (h->model != RNNWF_MODEL_LSTM1D_F64) {
        const char* other = renyi ? "no region-Renyi pass serves the parity model" : "no Pauli pass serves the parity model";
        switch (h->model) {
            case RNNWF_MODEL_GRU1D:
            case RNNWF_MODEL_GRU1D_F64:
                if (renyi)
                    other = h->NL > 1 ? "rnnwf_renyi2_regions_stack serves stacked GRU layers" : "rnnwf_renyi2_regions serves the GRU models";
                else
                    other = h->NL > 1 ? "rnnwf_pauli_step_stack serves stacked GRU layers" : "rnnwf_pauli_step serves the GRU models";
                break;
            case RNNWF_MODEL_MDRNN2D: other = renyi ? "rnnwf_renyi2_regions_2d serves the 2D RNN" : "rnnwf_pauli_step_2d serves the 2D RNN"; break;
            case RNNWF_MODEL_CRNN_U1:
                other = renyi ? "rnnwf_renyi2_regions_complex serves the complex RNN" : "rnnwf_pauli_step_complex serves the complex RNN";
                break;
            default: break;
        }
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the LSTM cell (LSTM1D_F64) only, this handle's model is %s; %s", entry,
                       model_name(h->model), other);
    }
    if (!with_lpauli(h, [](auto) {}))
        return h->fail(RNNWF_ERR_INVALID, "%s: no LSTM kernel for NFULL=%d (one layer, <= 68 units)", entry, h->NFULL);
    return 0;
}

}  // namespace rnnwf
