// crnn.hip - host side of the complex GRU RNN wave function with the U(1) mask (model CRNN_U1): weight image, base pass,
// log_amplitude, fused J1-J2 local energies (the VMC step and sampling are rnnwf_api.hip's driver, through crnn_family).
#include <algorithm>

#include <cstdlib>

#include "crnn_kernels.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

constexpr int64_t kChunk = (int64_t)1 << 20;

// The kernels of one shape: NL == 1 one GRU layer, NL > 1 stacked layers (T: float, the one element type of this family).
template <typename T, int NFULL, int NL, int WAVES>
struct CLaunch {
    using S = GruStack<T, NFULL, NL, 3>;
    using L = GruLayout<T, NFULL, 3>;
    static int base(rnnwf_handle* h, const CrnnArgs& a) {
        if constexpr (NL > 1) {
            // all layers' images resident in LDS (up to 52 units): the gate tiles of every layer spread over NFULL + 1 waves per block of
            // 16 chains (ml_coop.h) - for every batch size, its accumulation order is not the one-wave kernel's; RNNWF_NO_COOP=1 keeps that one
            if constexpr (MlCoopLayout<NFULL, NL, 3>::FITS && S::SPILL == 0) {
                if (!h->knobs.no_coop) {
                    using ML = MlCoopLayout<NFULL, NL, 3>;
                    return launch_persistent(h, kTimerBase, crnn_base_coop_kernel<NFULL, false, NL>, ML::THREADS, ML::LDS, a.nsb, ML::NB, a);
                }
            }
            return launch_shrinking<WAVES>(h, kTimerBase, crnn_ml_base_kernel<NFULL, NL, WAVES>, S::LDS_BYTES, a.nsb, a);
        } else {
            if (NFULL <= 3 && base_bf_available(h)) return crnn_base_coop_bf(h, a);      // bf16 cooperative kernel, every batch size (prnn.hip)
            // fewer 16-chain blocks than SIMDs: the cooperative kernel (NFULL + 1 waves per block, bit-identical)
            if constexpr (NFULL <= 4) {
                if (a.nsb <= (int64_t)4 * h->cu_count && !h->knobs.no_coop) {
                    const size_t lds = L::BYTES + (size_t)2 * L::KT * 64 * 4 + 2 * 64 * 4;
                    return launch_persistent(h, kTimerBase, crnn_base_coop_kernel<NFULL>, (NFULL + 1) * 64, lds, a.nsb, 1, a);
                }
            }
            return plain(h, a);
        }
    }
    // the one-wave kernel for every batch size (crnn_plain_base)
    static int plain(rnnwf_handle* h, const CrnnArgs& a) {
        if constexpr (NL > 1) return h->fail(RNNWF_ERR_INVALID, "crnn_plain_base: one GRU layer only");
        else return launch_persistent(h, kTimerBase, crnn_base_kernel<NFULL, WAVES>, WAVES * 64, S::LDS_BYTES, a.nsb, WAVES, a);
    }
    // the tile count lives on the device: the persistent grid is bounded by the worst case
    static int swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles) {
        if constexpr (NL > 1) return launch_persistent(h, kTimerFlip, crnn_ml_swap_kernel<NFULL, NL, WAVES>, WAVES * 64, S::LDS_BYTES, max_tiles, WAVES, a);
        else return launch_persistent(h, kTimerFlip, crnn_swap_kernel<NFULL, WAVES>, WAVES * 64, S::LDS_BYTES, max_tiles, WAVES, a);
    }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_gru_stack<T, NFULL, NL, 3>(h); }
    static void pack_table(const rnnwf_handle* h) { pack_gru_stack<T, NFULL, NL, 3, Lin>(h); }
    static size_t hck_bytes_per_block() { return (size_t)S::ROW * 64 * sizeof(T); }
};

// every shape with kernels: shapes.h
template <class Fn>
bool with_launch(const rnnwf_handle* h, Fn&& fn) { return with_kernels<CLaunch>(CrnnKernels(), h, fn); }

int no_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no cRNN kernel for NFULL=%d", h->NFULL); }
int launch_base(rnnwf_handle* h, const CrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::base(h, a); }) ? rc : no_kernel(h);
}
int launch_swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::swap(h, a, max_tiles); }) ? rc : no_kernel(h);
}
size_t hck_bytes_per_block(rnnwf_handle* h) {
    size_t b = 0;
    with_launch(h, [&](auto k) { b = decltype(k)::hck_bytes_per_block(); });
    return b;
}

// sites with a stored state: a stack keeps all N (the layer-wise gradient reads the lower layers' last site too)
int hck_sites(const rnnwf_handle* h) { return h->NL > 1 ? h->N : std::max(h->N - 1, 1); }

CrnnArgs base_args(rnnwf_handle* h, int64_t ns) {
    CrnnArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    return a;
}

int64_t max_chains_per_pass(rnnwf_handle* h) {
    size_t per_block = (size_t)hck_sites(h) * hck_bytes_per_block(h);
    if (h->NL > 1 && h->engine_split)                         // the layer pipeline's records: ~2 items per sample and site, per 16 chains
        per_block += stack_record_bytes_per_32_chains(h, (int64_t)h->N * (h->N - 1) / 2) + stack_record_bytes_per_32_chains(h, 4 * (int64_t)h->N);
    return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block)) * kChains;
}

// Upper bound of the wave-steps (32-item tiles x chain length) of one swap pass: first-changed site lo owns the bonds (lo, lo + 1) and
// (lo, lo + 2), with periodic couplings also (N - 1, 0), (N - 2, 0) at lo = 0 and (N - 1, 1) at lo = 1 (j1j2_enumerate_kernel) - at most
// 4, 3, 2, 2, ... items per sample.
int64_t stack_max_records(int N, int64_t ns) {
    int64_t r = 0;
    for (int lo = 0; lo < N - 1; ++lo) r += ((int64_t)(lo == 0 ? 4 : lo == 1 ? 3 : 2) * ns + 31) / 32 * (N - 1 - lo);
    return std::max<int64_t>(r, 1);
}

// J1-J2 local energies of the ns chains whose packed spins are in h->bits (drawn here when `sampling`).
// couplings_dev: J1 (N), J2 (N), Bz (N).  Leaves complex64 E_loc in h->eloc; *ncon_host (optional) receives
// the number of scored configurations after a stream sync.
int j1j2_on_device(rnnwf_handle* h, int64_t ns, bool sampling, uint64_t seed, uint64_t step, int64_t offset,
                   const double* couplings_dev, int periodic, int marshall) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    const int64_t cap = 4 * ns;
    if (int rc = ensure(h, h->hck, (size_t)hck_sites(h) * nsb * hck_bytes_per_block(h))) return rc;
    if (int rc = ensure(h, h->cbase, (size_t)N * ns * sizeof(double2))) return rc;
    if (int rc = ensure(h, h->cout, (size_t)ns * (sizeof(double2) + sizeof(double)))) return rc;
    if (int rc = ensure(h, h->tile_count, (size_t)(2 * N + 8) * 4 + 64 + (size_t)N * 8)) return rc;
    if (int rc = ensure(h, h->tiles, (size_t)N * cap * sizeof(SwapItem))) return rc;
    if (int rc = ensure(h, h->lpq, (size_t)ns * 2 * N * sizeof(double2))) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * sizeof(float2))) return rc;

    double2* tot = (double2*)h->cout.p;
    double* diag = (double*)((char*)h->cout.p + (size_t)ns * sizeof(double2));
    int32_t* cnt = (int32_t*)h->tile_count.p;
    int32_t* tile_start = cnt + N;
    int64_t* total_items = (int64_t*)((char*)h->tile_count.p + (((size_t)(2 * N + 1) * 4 + 15) / 16) * 16);
    const bool stack = h->engine_split && h->NL > 1;
    int64_t* rec_start = stack ? total_items + 4 : nullptr;     // [N] first record of each site's tiles (layer pipeline)

    CrnnArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.cb = (double2*)h->cbase.p;
    a.tot = tot;
    a.sampling = sampling ? 1 : 0;
    a.seed = seed; a.step = step; a.sample_offset = offset;
    if (int rc = launch_base(h, a)) return rc;

    // the item counters are zeroed by the previous step's assembly kernel (j1j2_eloc_kernel); a memset only when that did not happen
    if (!h->j1j2_cnt_clean) RNNWF_HIP(h, hipMemsetAsync(cnt, 0, (size_t)N * 4, h->stream));
    h->j1j2_cnt_clean = false;
    J1J2Args e{};
    e.bits = (const uint32_t*)h->bits.p;
    e.ns = ns; e.N = N;
    e.J1 = couplings_dev; e.J2 = couplings_dev + N; e.Bz = couplings_dev + 2 * N;
    e.periodic = periodic; e.marshall = marshall;
    e.cnt = cnt; e.items = (SwapItem*)h->tiles.p; e.cap = cap;
    e.contrib = (double2*)h->lpq.p; e.diag = diag;
    {
        TimedLaunch tl(h, kTimerAssembly);
        dim3 grid((unsigned)((ns + 255) / 256), (unsigned)(2 * N));
        j1j2_enumerate_kernel<<<grid, 256, 0, h->stream>>>(e);
        RNNWF_HIP(h, hipGetLastError());
        // the three totals land in pinned[64..88) - written by the kernel itself - and are read at the caller's next stream sync
        // (collect_totals)
        j1j2_tile_scan_kernel<<<1, 64, 0, h->stream>>>(cnt, N, tile_start, total_items, (int64_t*)((char*)h->pinned_dev + 64),
                                                       h->engine_split ? 32 : kChains, rec_start);
        RNNWF_HIP(h, hipGetLastError());
    }
    a.sampling = 0;
    a.tile_start = tile_start;
    a.cnt = cnt;
    a.items = (const SwapItem*)h->tiles.p;
    a.cap = cap;
    a.contrib = (double2*)h->lpq.p;
    const int64_t max_tiles = (int64_t)N * ((2 * ns + kChains - 1) / kChains + 2);
    if (stack) {
        a.rec_start = rec_start;
        if (int rc = crnn_stack_swap(h, a, max_tiles, stack_max_records(N, ns))) return rc;
    } else if (h->engine_split) {
        if (int rc = crnn_split_swap(h, a, max_tiles)) return rc;
    } else {
        if (int rc = launch_swap(h, a, max_tiles)) return rc;
    }
    if (int rc = timed_launch(h, kTimerAssembly, j1j2_eloc_kernel, (unsigned)((ns + 255) / 256), 256, 0, (const double2*)h->lpq.p, diag,
                              ns, N, (float2*)h->eloc.p, N <= 256 ? cnt : nullptr)) return rc;
    h->j1j2_cnt_clean = N <= 256;
    return 0;
}

// after a stream sync: number of scored configurations (the reference's len_sigmas) and work counters
int64_t collect_totals(rnnwf_handle* h, int64_t ns) {
    const int64_t* t = (const int64_t*)((char*)h->pinned + 64);
    h->work[0] += (double)t[1];
    h->work[1] += (double)t[2] * (h->engine_split ? (h->NL > 1 ? stack_split_flops_per_step(h) : crnn_split_flops_per_step(h))
                                                  : (double)(3 * h->NFULL + 1) * (4 * h->NFULL + 1) * 2048.0);
    return t[0] + ns;   // + one diagonal configuration per sample
}

// base pass alone: 2 Re log psi of every chain -> h->out_lp (the spins drawn into h->bits when `d`)
int log_prob_pass(rnnwf_handle* h, int64_t ns, const Draw* d) {
    if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
    CrnnArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.out_logp = (double*)h->out_lp.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    return launch_base(h, a);
}

// couplings: J1, J2, Bz (N each, on the device in h->coupl), then the periodic and Marshall flags
int energy(rnnwf_handle* h, int64_t ns, const Draw* d, const double* couplings) {
    const int N = h->N;
    return j1j2_on_device(h, ns, d != nullptr, d ? d->seed : 0, d ? d->step : 0, d ? d->offset : 0, (const double*)h->coupl.p,
                          couplings[3 * N] != 0.0, couplings[3 * N + 1] != 0.0);
}

void count_work(rnnwf_handle* h, int64_t ns) { collect_totals(h, ns); }

int pack_image(rnnwf_handle* h, std::vector<char>& img) {
    // swap-pass engine: bf16x3 on the matrix core (RNNWF_ENGINE=f32: f32-input MFMA everywhere; above 68 units the w3
    // fragments are read through L2, split_stream.hip)
    // stacked layers of 37..50 units: a pipeline of bf16x3 kernels, one per layer (split.hip: crnn_stack_swap); other stacks and
    // > 100 units: f32-input MFMA
    h->engine_split = h->knobs.engine != 1 && (h->NL == 1 ? h->NFULL <= 6 : stack_split_available(h));
    if (h->engine_split && h->NL > 1) {
        if (int rc = stack_pack<3>(h)) return rc;
    } else if (h->engine_split) {
        std::vector<char> simg;
        if (int rc = crnn_split_pack(h, simg)) return rc;
        if (int rc = ensure(h, h->wsplit, simg.size())) return rc;
        if (int rc = upload(h, h->wsplit.p, simg.data(), simg.size())) return rc;
    }
    if (int rc = base_bf_pack(h)) return rc;
    return with_launch(h, [&](auto k) { img = decltype(k)::pack(h); }) ? 0 : no_kernel(h);
}

// device-resident training (train.hip): the table of the image pack_image returns
int pack_table(rnnwf_handle* h) {
    return with_launch(h, [&](auto k) { decltype(k)::pack_table(h); }) ? 0 : no_kernel(h);
}

}  // namespace

int rnnwf::crnn_log_amp(rnnwf_handle* h, const int32_t* samples, int64_t B, float* out_re_im, double* out_logp) {
    const int N = h->N;
    h->last_ns = 0;
    for (int64_t off = 0; off < B; off += kChunk) {
        const int64_t nb = std::min(kChunk, B - off);
        if (int rc = upload_and_pack(h, samples + off * N, nb, h->bits, 0, nullptr)) return rc;
        if (int rc = ensure(h, h->camp, (size_t)nb * sizeof(float2))) return rc;
        if (int rc = ensure(h, h->out_lp, (size_t)nb * 8)) return rc;
        CrnnArgs a = base_args(h, nb);
        a.bits = (uint32_t*)h->bits.p;
        a.out_amp = (float2*)h->camp.p;
        a.out_logp = (double*)h->out_lp.p;
        if (int rc = launch_base(h, a)) return rc;
        if (out_re_im)
            RNNWF_HIP(h, hipMemcpyAsync(out_re_im + 2 * off, h->camp.p, (size_t)nb * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
        if (out_logp)
            RNNWF_HIP(h, hipMemcpyAsync(out_logp + off, h->out_lp.p, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    return RNNWF_OK;
}

int rnnwf::crnn_j1j2_eloc(rnnwf_handle* h, const int32_t* samples, int64_t ns, const double* J1, const double* J2,
                          const double* Bz, int periodic, int marshall, float* eloc, int64_t* ncon) {
    const int N = h->N;
    h->last_ns = 0;
    {
        std::vector<double> c((size_t)3 * N);
        std::copy(J1, J1 + N, c.begin());
        std::copy(J2, J2 + N, c.begin() + N);
        std::copy(Bz, Bz + N, c.begin() + 2 * N);
        if (int rc = upload_couplings(h, c.data(), c.size())) return rc;
    }
    const int64_t chunk = max_chains_per_pass(h);
    int64_t total = 0;
    for (int64_t off = 0; off < ns; off += chunk) {
        const int64_t nb = std::min(chunk, ns - off);
        if (int rc = upload_and_pack(h, samples + off * N, nb, h->bits, 0, nullptr)) return rc;
        if (int rc = j1j2_on_device(h, nb, false, 0, 0, 0, (const double*)h->coupl.p, periodic, marshall)) return rc;
        RNNWF_HIP(h, hipMemcpyAsync(eloc + 2 * off, h->eloc.p, (size_t)nb * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        total += collect_totals(h, nb);
    }
    if (ncon) *ncon = total;
    return RNNWF_OK;
}

// The base pass on the one-wave-per-block kernel for every batch size (never the cooperative or bf16 kernels): the masked-tail pass
// of crnn_pauli.hip restarts from its checkpoints and must repeat its arithmetic step for step.  One layer only.
int rnnwf::crnn_plain_base(rnnwf_handle* h, const CrnnArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::plain(h, a); }) ? rc : no_kernel(h);
}
CrnnArgs rnnwf::crnn_base_args(rnnwf_handle* h, int64_t ns) { return base_args(h, ns); }
size_t rnnwf::crnn_hck_bytes_per_block(rnnwf_handle* h) { return hck_bytes_per_block(h); }

const Family* rnnwf::crnn_family() {
    static const Family f = {
        "complex RNN", pack_image, pack_table, log_prob_pass, nullptr, energy, max_chains_per_pass, nullptr, count_work,
        3, 2,               // J1, J2, Bz per site; periodic, marshall
        true, false, gru_gradient(),    // complex64 E_loc; the base pass alone keeps no states
    };
    return &f;
}
