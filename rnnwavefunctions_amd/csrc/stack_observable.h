// stack_observable.h - what the host drivers of the observable passes of STACKED GRU layers share: rnnwf_pauli_step_stack and
// rnnwf_pauli_train_steps_stack (pauli_stack.hip), rnnwf_renyi2_regions_stack (renyi_stack.hip).  The launch class of a stack, the
// walk over the stack rows of the positive GRU's table, the refusals and the size of a checkpoint row.  Both serve the positive
// models GRU1D (float32) and GRU1D_F64 (float64, raster path) with 2..4 layers, every stack rnnwf_create accepts; kernels in
// stack_chain_kernels.h.  Each .hip instantiates its own kernels, under its own flags.
#pragma once
#include "observable.h"
#include "stack_chain_kernels.h"

namespace rnnwf {

template <typename T_, int NFULL_, int NL_, int WAVES_>
struct StackLaunch {
    using T = T_;
    using S = GruStack<T_, NFULL_, NL_, 1>;
    using L = GruLayout<T_, NFULL_, 1>;
    static constexpr int NFULL = NFULL_, NL = NL_, WAVES = WAVES_;
    static size_t hck_bytes_per_block() { return (size_t)S::ROW * 64 * sizeof(T); }
    static double mfma_flops_per_step() { return ((double)L::NT + 2.0 * (NL - 1) * UpperLayout<NFULL, T>::NT) * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for one layer or a stack without kernels: the stack rows of the
// positive GRU's table (shapes.h) at the row's waves per workgroup, as prnn_ml_flip_kernel runs
template <class R> struct Stacked : std::bool_constant<(R::NL > 1)> {};
template <class Fn>
bool with_stack(const rnnwf_handle* h, Fn&& fn) {
    return with_row<Stacked>(GruKernels(), h, [&](auto r) {
        using R = decltype(r);
        fn(StackLaunch<typename R::T, R::NFULL, R::NL, R::WAVES>());
    });
}

// 0, or RNNWF_ERR_INVALID "<entry>: <why>".  Called before anything is touched: a refused call leaves the resident batch usable.
inline int stack_refuse(rnnwf_handle* h, const char* entry, const char* one_layer_entry) {
    if (h->model != RNNWF_MODEL_GRU1D && h->model != RNNWF_MODEL_GRU1D_F64) return observable_refuse(h, entry);
    if (h->NL == 1)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves stacked layers (2..%d GRU layers), this handle has one layer; %s serves it", entry,
                       RNNWF_MAX_LAYERS, one_layer_entry);
    if (!with_stack(h, [](auto) {}))
        return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for NFULL=%d f64=%d layers=%d", entry, h->NFULL, (int)h->f64, h->NL);
    return 0;
}

inline size_t stack_hck_bytes_per_block(rnnwf_handle* h) {
    size_t b = 0;
    with_stack(h, [&](auto k) { b = decltype(k)::hck_bytes_per_block(); });
    return b;
}

}  // namespace rnnwf
