// mdrnn_observable.h - what the 2D RNN's policies of the Pauli and region-Renyi drivers share: rnnwf_pauli_step_2d (mdrnn_pauli.hip,
// pauli_driver.h) and rnnwf_renyi2_regions_2d (mdrnn_renyi.hip, region_driver.h).  Both serve MDRNN2D (float64) and run, per pass of
// whole 16-chain blocks within the state budget, on the family's base pass, which keeps every position's state in h->hck: site
// terms -> masked tails (mdrnn_pauli_kernels.h).  Here are the launch table, the model refusal, the lattice -> path map, the pass
// size, the kernels' arguments and the two launches, which each .hip instantiates for itself (PAIRED or not).
#pragma once
#include <algorithm>
#include <vector>

#include "mdrnn_pauli_kernels.h"
#include "observable.h"

namespace rnnwf {

template <int NFULL_, int WAVES_>
struct MdLaunch {
    using L = MdLayout<NFULL_>;
    static constexpr int NFULL = NFULL_, WAVES = WAVES_;
    static constexpr size_t TAIL_LDS = L::BYTES + (size_t)WAVES * L::WORDS_BYTES;     // image + the waves' spin words
    static constexpr size_t HS_BYTES_PER_BLOCK = (size_t)((L::KT + 1) / 2) * 64 * 16;
    static double mfma_flops_per_step() { return (double)NFULL * 2 * L::KT * 2048.0; }
};

// the rows of the 2D RNN's table (shapes.h), as mdrnn.hip's with_width
template <class Fn>
bool with_md_width(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<MdLaunch>(MdKernels(), h, fn); }

// 0, or RNNWF_ERR_INVALID for another model or a width without kernels; gru_entry: the entry point that serves the GRU models
inline int md_refuse(rnnwf_handle* h, const char* entry, const char* gru_entry) {
    if (h->model != RNNWF_MODEL_MDRNN2D)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the 2D RNN (MDRNN2D) only, this handle's model is %s; %s serves the GRU models", entry,
                       model_name(h->model), gru_entry);
    if (!with_md_width(h, [](auto) {}))
        return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for num_units = %d (the 2D RNN's kernels serve 1..84)", entry, h->H);
    return 0;
}

// visit position of lattice site k = nx Ny + ny (mdrnn.hip: get_maps)
inline int pos_of_site(const rnnwf_handle* h, int k) {
    const int nx = k / h->Ny, ny = k % h->Ny;
    return ny * h->Nx + (ny % 2 == 0 ? nx : h->Nx - 1 - nx);
}

inline std::vector<int32_t> md_positions(const rnnwf_handle* h) {
    std::vector<int32_t> pos(h->N);
    for (int k = 0; k < h->N; ++k) pos[k] = pos_of_site(h, k);
    return pos;
}

// chains per pass: the family's pass holds N states per block in its budget; beside them, per block, the entry's `bytes_per_block`
inline int64_t md_chains_per_pass(rnnwf_handle* h, size_t bytes_per_block) {
    size_t hs_bytes = 0;
    with_md_width(h, [&](auto k) { hs_bytes = decltype(k)::HS_BYTES_PER_BLOCK; });
    const size_t budget = (size_t)(h->family->max_chains_per_pass(h) / kChains) * h->N * hs_bytes;
    return std::max<int64_t>(1, (int64_t)(budget / ((size_t)h->N * hs_bytes + bytes_per_block))) * kChains;
}

// the arguments of a pass over the ns chains packed in h->bits, their states in h->hck; sc: the pass's PauliScratch or RegionScratch;
// nmasks: masks with a tail
template <class Scratch>
MdPauliArgs md_args(rnnwf_handle* h, int64_t ns, int W, const Scratch& sc, int nmasks) {
    char* buf = (char*)h->renyi.p;
    MdPauliArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.Nx = h->Nx;
    a.rem = h->H - 16 * h->NFULL;
    a.W = W;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.bits = (const uint32_t*)h->bits.p;
    a.hs = (const double*)h->hck.p;
    a.terms = (double*)(buf + sc.terms);
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)nmasks * a.nsb;
    return a;
}

// the site terms (if `replay`) and the masked tails of a.ntiles tiles, with the work counters; steps: cell evaluations per chain
template <bool PAIRED>
int md_terms_and_tails(rnnwf_handle* h, MdPauliArgs& a, bool replay, double steps) {
    int rc = 0;
    with_md_width(h, [&](auto k) {
        using P = decltype(k);
        using L = typename P::L;
        if (replay) rc = launch_persistent(h, kTimerBase, mdrnn_site_terms_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::BYTES, a.nsb, P::WAVES, a);
        if (rc) return;
        const auto kern = mdrnn_masked_tail_kernel<P::NFULL, P::WAVES, PAIRED>;
        unsigned grid = 0;
        if ((rc = persistent_grid(h, kern, P::WAVES * 64, P::TAIL_LDS, a.ntiles, P::WAVES, &grid))) return;
        if ((rc = ensure(h, h->rowbuf, (size_t)grid * P::WAVES * a.Nx * P::HS_BYTES_PER_BLOCK))) return;      // one slot per lattice column
        a.ring = (double*)h->rowbuf.p;
        rc = timed_launch(h, kTimerFlip, kern, grid, P::WAVES * 64, P::TAIL_LDS, a);
        if (!rc) h->work[1] += (double)a.nsb * steps * P::mfma_flops_per_step();
    });
    if (!rc) h->work[0] += (double)a.ns * steps;
    return rc;
}

}  // namespace rnnwf
