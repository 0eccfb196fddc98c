// prnn.hip - host side of the positive GRU RNN wave function (models GRU1D, GRU1D_PARITY, GRU1D_F64): weight image, base pass,
// fused TFIM local energies (the driver of the entry points is rnnwf_api.hip's, through gru_family).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "gru_kernels.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

// The kernels of one shape: NL == 1 one GRU layer, NL > 1 stacked layers.
template <typename T, int NFULL, int NL, int WAVES>
struct Launch {
    using S = GruStack<T, NFULL, NL, 1>;
    using L = GruLayout<T, NFULL, 1>;
    static constexpr bool F32 = std::is_same<T, float>::value;
    static int base(rnnwf_handle* h, const PrnnArgs& a) {
        if constexpr (NL > 1) {
            // all layers' images resident in LDS (f32, up to 52 units): the gate tiles of every layer spread over NFULL + 1 waves per block
            // of 16 chains (ml_coop.h) - for every batch size, its accumulation order is not the one-wave kernel's; RNNWF_NO_COOP=1 keeps that one
            if constexpr (F32 && MlCoopLayout<NFULL, NL, 1>::FITS && S::SPILL == 0) {
                if (!h->knobs.no_coop) {
                    using ML = MlCoopLayout<NFULL, NL, 1>;
                    return launch_persistent(h, kTimerBase, prnn_base_coop_kernel<NFULL, false, NL>, ML::THREADS, ML::LDS, a.nsb, ML::NB, a);
                }
            }
            return launch_shrinking<WAVES>(h, kTimerBase, prnn_ml_base_kernel<T, NFULL, NL, WAVES>, S::LDS_BYTES, a.nsb, a);
        } else {
            // f32 models of 37..52 units: the cooperative kernel on the bf16 matrix core, for every batch size (a batch and its
            // shards always take the same kernel); RNNWF_BASE=f32 / RNNWF_NO_COOP=1 keep the f32-input-MFMA kernels
            if (F32 && NFULL <= 3 && base_bf_available(h)) return prnn_base_coop_bf(h, a);
            // fewer 16-chain blocks than SIMDs: the cooperative kernel (NFULL + 1 waves per block) cuts the per-site latency
            if constexpr (F32 && NFULL <= 4) {
                if (a.nsb <= (int64_t)4 * h->cu_count && !h->knobs.no_coop) {
                    const size_t lds = L::BYTES + (size_t)2 * L::KT * 64 * 4 + 2 * 64 * 4;
                    return launch_persistent(h, kTimerBase, prnn_base_coop_kernel<NFULL>, (NFULL + 1) * 64, lds, a.nsb, 1, a);
                }
            }
            return plain(h, a);
        }
    }
    // the one-wave-per-block kernel whatever the batch size
    static int plain(rnnwf_handle* h, const PrnnArgs& a) {
        if constexpr (NL > 1) return h->fail(RNNWF_ERR_INVALID, "stacked layers: no one-wave base pass");
        else return launch_persistent(h, kTimerBase, prnn_base_kernel<T, NFULL, WAVES>, WAVES * 64, S::LDS_BYTES, a.nsb, WAVES, a);
    }
    // stacked layers: the one-wave MFMA kernel whatever the batch size and whatever `base` would take
    static int stack_plain(rnnwf_handle* h, const PrnnArgs& a) {
        if constexpr (NL > 1) return launch_shrinking<WAVES>(h, kTimerBase, prnn_ml_base_kernel<T, NFULL, NL, WAVES>, S::LDS_BYTES, a.nsb, a);
        else return h->fail(RNNWF_ERR_INVALID, "one layer: its one-wave base pass is prnn_plain_base");
    }
    static int flip(rnnwf_handle* h, const PrnnArgs& a) {
        if constexpr (NL > 1) return launch_persistent(h, kTimerFlip, prnn_ml_flip_kernel<T, NFULL, NL, WAVES>, WAVES * 64, S::LDS_BYTES, a.ntiles, WAVES, a);
        else return launch_persistent(h, kTimerFlip, prnn_flip_kernel<T, NFULL, WAVES>, WAVES * 64, S::LDS_BYTES, a.ntiles, WAVES, a);
    }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_gru_stack<T, NFULL, NL, 1>(h); }
    static void pack_table(const rnnwf_handle* h) { pack_gru_stack<T, NFULL, NL, 1, Lin>(h); }
    static size_t hck_bytes_per_block() { return (size_t)S::ROW * 64 * sizeof(T); }
    static double mfma_flops_per_step() { return ((double)L::NT + 2.0 * (NL - 1) * UpperLayout<NFULL, T>::NT) * L::KT * 2048.0; }
};

// every shape with kernels: shapes.h
template <class Fn>
bool with_launch(const rnnwf_handle* h, Fn&& fn) { return with_kernels<Launch>(GruKernels(), h, fn); }

int no_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no pRNN kernel for NFULL=%d f64=%d", h->NFULL, (int)h->f64); }
int launch_base(rnnwf_handle* h, const PrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::base(h, a); }) ? rc : no_kernel(h);
}
int launch_flip(rnnwf_handle* h, const PrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::flip(h, a); }) ? rc : no_kernel(h);
}
size_t hck_bytes_per_block(rnnwf_handle* h) {
    size_t b = 0;
    with_launch(h, [&](auto k) { b = decltype(k)::hck_bytes_per_block(); });
    return b;
}
double mfma_flops_per_step(rnnwf_handle* h) {
    double f = 0;
    with_launch(h, [&](auto k) { f = decltype(k)::mfma_flops_per_step(); });
    return f;
}

PrnnArgs base_args(rnnwf_handle* h, int64_t ns) {
    PrnnArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.ablate = h->knobs.ablate_base & (8 | 16 | 32);   // 0 unless a -DRNNWF_DIAGNOSTICS build read RNNWF_ABLATE_BASE
    return a;
}

// row_of_pos map for the reversed pass of the parity-symmetric model: position n of the reversed chain
// is site N-1-n, so its flip lands in lpq row (N-1-n)+1.
int ensure_reverse_map(rnnwf_handle* h) {
    const int N = h->N;
    if (h->maps.p) return 0;
    std::vector<int32_t> m(N);
    for (int n = 0; n < N; ++n) m[n] = N - n;
    if (int rc = ensure(h, h->maps, (size_t)N * 4)) return rc;
    RNNWF_HIP(h, hipMemcpy(h->maps.p, m.data(), (size_t)N * 4, hipMemcpyHostToDevice));
    return 0;
}

// bf16x3 or f32-input MFMA for this flip pass?  The bf16x3 kernel works on 32-chain tiles; when there are not enough
// of them for two waves per SIMD (config 1: 304 tiles for 1 024 SIMDs) the 16-chain f32 kernel fills the chip better
// (measured 0.0198 vs 0.0223 ms at config 1).  RNNWF_ENGINE=bf16x3 pins the bf16x3 engine.
bool use_split(rnnwf_handle* h, int64_t ns_pass) {
    const int64_t ns = std::max<int64_t>(h->call_ns, ns_pass);     // the whole call decides, not the pass
    const int64_t tiles32 = (int64_t)(h->N - 1) * ((ns + 31) / 32);
    const bool split = h->engine_split && (h->engine_forced || tiles32 >= (int64_t)8 * h->cu_count);
    h->last_flip_engine = split ? 1 : 0;
    return split;
}

// The flip pass of one direction on the engine the call chose, with its work counters (cell evaluations, MFMA flops issued).
int flip_pass(rnnwf_handle* h, const PrnnArgs& a, int64_t ns) {
    const int N = h->N;
    const double wave_steps32 = (double)((ns + 31) / 32) * N * (N - 1) / 2.0;
    if (use_split(h, ns)) {
        if (h->NL > 1) {
            if (int rc = prnn_stack_flip(h, a)) return rc;
            h->work[1] += wave_steps32 * stack_split_flops_per_step(h);
        } else {
            if (int rc = prnn_split_flip(h, a)) return rc;
            h->work[1] += wave_steps32 * prnn_split_flops_per_step(h);
        }
    } else {
        if (int rc = launch_flip(h, a)) return rc;
        h->work[1] += (double)a.nsb * N * (N - 1) / 2.0 * mfma_flops_per_step(h);
    }
    h->work[0] += (double)ns * N * (N - 1) / 2.0;
    return 0;
}

// Fused local energies of ns chains whose packed spins are in h->bits (drawn into it when `d`): base pass with checkpoints ->
// flip pass -> assembly.  Leaves E_loc in h->eloc and the log-prob queue in h->lpq.  The parity model also runs the reversed chains,
// packed into h->bits2 from h->samples_i32 (the caller's upload, or the drawn spins unpacked there).
int eloc_on_device(rnnwf_handle* h, int64_t ns, const Draw* d, const double* couplings) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    const bool parity = h->model == RNNWF_MODEL_GRU1D_PARITY;
    const bool raster = h->model == RNNWF_MODEL_GRU1D_F64;     // the 1D models' handles hold (Nx, Ny) = (N, 1); the assembly takes (1, N)
    const double Bx = couplings[N];
    const size_t hck_bytes = (size_t)(h->NL > 1 ? N : std::max(N - 1, 1)) * nsb * hck_bytes_per_block(h);
    if (int rc = ensure(h, h->lpq, (size_t)(N + 1) * ns * 8)) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    if (int rc = ensure(h, h->hck, hck_bytes)) return rc;    // always: the gradient pass reuses the states

    PrnnArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.lpq = (double*)h->lpq.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    if (int rc = launch_base(h, a)) return rc;
    if (Bx != 0.0 && N > 1) {
        a.ntiles = (int64_t)(N - 1) * nsb;
        a.sampling = 0;
        a.ablate |= h->knobs.ablate & 15;   // 0 unless a -DRNNWF_DIAGNOSTICS build read RNNWF_ABLATE
        if (int rc = flip_pass(h, a, ns)) return rc;
    }
    if (parity) {
        // second direction on the reversed chains, then log(0.5 (e^a + e^b)) row by row
        if (d)
            if (int rc = unpack_device(h, h->bits, ns, nullptr)) return rc;
        if (int rc = pack_device(h, ns, h->bits2, 1, nullptr)) return rc;
        if (int rc = ensure_reverse_map(h)) return rc;
        if (int rc = ensure(h, h->lpq2, (size_t)(N + 1) * ns * 8)) return rc;
        PrnnArgs b = base_args(h, ns);
        b.bits = (uint32_t*)h->bits2.p;
        b.hck = a.hck;
        b.lpq = (double*)h->lpq2.p;
        b.row_of_pos = (const int32_t*)h->maps.p;
        if (int rc = launch_base(h, b)) return rc;
        if (Bx != 0.0 && N > 1) {
            b.ntiles = (int64_t)(N - 1) * nsb;
            if (int rc = flip_pass(h, b, ns)) return rc;
        }
        if (int rc = run_parity_combine(h, (const double*)h->lpq.p, (const double*)h->lpq2.p, (int64_t)(N + 1) * ns,
                                        (double*)h->lpq.p)) return rc;
    }
    return run_tfim_eloc(h, (const uint32_t*)h->bits.p, (const double*)h->lpq.p, ns, raster ? h->Nx : 1, raster ? h->Ny : N,
                         nullptr, (const double*)h->coupl.p, Bx, (double*)h->eloc.p);
}

// base pass alone: log P of every chain -> h->out_lp (the spins drawn into h->bits when `d`)
int log_prob_pass(rnnwf_handle* h, int64_t ns, const Draw* d) {
    if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
    PrnnArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.out_lp = (double*)h->out_lp.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    return launch_base(h, a);
}

// parity model: log P of the reversed chains of the spins in h->samples_i32, combined with h->out_lp into the symmetrised one
int symmetrise(rnnwf_handle* h, int64_t ns) {
    if (h->model != RNNWF_MODEL_GRU1D_PARITY) return 0;
    if (int rc = pack_device(h, ns, h->bits2, 1, nullptr)) return rc;
    if (int rc = ensure(h, h->out_lp2, (size_t)ns * 8)) return rc;
    PrnnArgs b = base_args(h, ns);
    b.bits = (uint32_t*)h->bits2.p;
    b.out_lp = (double*)h->out_lp2.p;
    if (int rc = launch_base(h, b)) return rc;
    return run_parity_combine(h, (const double*)h->out_lp.p, (const double*)h->out_lp2.p, ns, (double*)h->out_lp.p);
}

int64_t max_chains_per_pass(rnnwf_handle* h) {
    size_t per_block = (size_t)(h->NL > 1 ? h->N : std::max(h->N - 1, 1)) * hck_bytes_per_block(h);
    if (h->NL > 1 && h->engine_split)                         // per 16 chains: half a 32-chain tile column of the layer pipeline's records
        per_block += stack_record_bytes_per_32_chains(h, (int64_t)h->N * (h->N - 1) / 2) / 2;
    const int64_t blocks = std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
    return blocks * kChains;
}

int pack_image(rnnwf_handle* h, std::vector<char>& img) {
    // flip-pass engine: bf16x3 on the matrix core for the f32 models (RNNWF_ENGINE=f32 keeps the f32-input MFMA
    // everywhere; above 68 units the w3 fragments of the image are read through L2, split_stream.hip); the base pass, sampling and log_probability always run the f32-MFMA kernels
    // stacked layers: 37..50 units run as a pipeline of bf16x3 kernels, one per layer (split.hip: prnn_stack_flip); other widths
    // keep the f32-input MFMA
    h->engine_split = !h->f64 && h->knobs.engine != 1 && (h->NL == 1 ? h->NFULL <= 6 : stack_split_available(h));     // above 100 units: f32-input MFMA, image through L2
    h->engine_forced = h->knobs.engine >= 2;
    if (h->engine_split && h->NL > 1) {
        if (int rc = stack_pack<1>(h)) return rc;
    } else if (h->engine_split) {
        std::vector<char> simg, simg_g;
        if (int rc = prnn_split_pack(h, simg, simg_g)) return rc;
        if (int rc = ensure(h, h->wsplit, simg.size())) return rc;
        if (int rc = upload(h, h->wsplit.p, simg.data(), simg.size())) return rc;
        if (!simg_g.empty()) {                                // 37..50 units: the ping-pong kernel's g-state form runs on its own image
            if (int rc = ensure(h, h->wsplit_g, simg_g.size())) return rc;
            if (int rc = upload(h, h->wsplit_g.p, simg_g.data(), simg_g.size())) return rc;
        }
    }
    if (int rc = base_bf_pack(h)) return rc;
    return with_launch(h, [&](auto k) { img = decltype(k)::pack(h); }) ? 0 : no_kernel(h);
}

// device-resident training (train.hip): the table of the image pack_image returns
int pack_table(rnnwf_handle* h) {
    return with_launch(h, [&](auto k) { decltype(k)::pack_table(h); }) ? 0 : no_kernel(h);
}

}  // namespace

// Teacher-forced base pass with checkpoints over the resident spins (h->bits, or the reversed ones in h->bits2), log P of every
// chain to out_lp: what a backward pass of the parity-symmetric model needs per direction (grad.hip).
int rnnwf::prnn_teacher_base(rnnwf_handle* h, int64_t ns, bool reversed, double* out_lp) {
    PrnnArgs a = base_args(h, ns);
    a.bits = (uint32_t*)(reversed ? h->bits2.p : h->bits.p);
    a.hck = h->hck.p;
    a.out_lp = out_lp;
    return launch_base(h, a);
}

// The base pass on the one-wave-per-block kernel for every batch size (never the cooperative or bf16x3 kernels): the swap pass of
// renyi.hip restarts from its checkpoints and must repeat its arithmetic step for step.
int rnnwf::prnn_plain_base(rnnwf_handle* h, const PrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::plain(h, a); }) ? rc : no_kernel(h);
}
// The same for stacked layers (pauli_stack.hip): the base pass on prnn_ml_base_kernel for every batch size, never the cooperative
// kernel, whose accumulation order is its own - the stack's masked tails restart from these checkpoints and repeat this arithmetic.
int rnnwf::prnn_stack_base(rnnwf_handle* h, const PrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::stack_plain(h, a); }) ? rc : no_kernel(h);
}
PrnnArgs rnnwf::prnn_base_args(rnnwf_handle* h, int64_t ns) { return base_args(h, ns); }
size_t rnnwf::prnn_hck_bytes_per_block(rnnwf_handle* h) { return hck_bytes_per_block(h); }

const Family* rnnwf::gru_family() {
    static const Family f = {
        "GRU cell", pack_image, pack_table, log_prob_pass, symmetrise, eloc_on_device, max_chains_per_pass, nullptr, nullptr,
        1, 1,                // Jz per site; Bx
        false, false, gru_gradient(),   // float64 E_loc; the base pass alone keeps no states
    };
    return &f;
}
