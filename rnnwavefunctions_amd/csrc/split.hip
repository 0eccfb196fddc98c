// split.hip - host side of the bf16x3 engine (split_core.h): the flip pass of the positive RNN and the swap pass of the
// complex RNN on the bf16 matrix core, incl. their ping-pong kernels.  A translation unit of its own because it is
// compiled with -fno-slp-vectorize (build.py): packed-f32 instructions stall behind bf16 MFMAs - their own wave's and the
// SIMD partner's - whereas the f32-input-MFMA kernels of prnn.hip / crnn.hip WANT the packed forms (their MFMA and VALU
// serialise anyway, so half the VALU instructions is a straight gain: config 5 0.79 -> 0.86 of the f32 pipe).
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "crnn_split_kernels.h"
#include "models.h"
#include "pack.h"
#include "pack_split.h"
#include "shapes.h"
#include "split_kernels.h"

using namespace rnnwf;

namespace {

#ifdef RNNWF_DIAGNOSTICS
// In-kernel cycle stamps (tools/stamps.py, tools/stamps_base.py): launch(buffer) runs the kernel with a zeroed buffer of `words` counters
// for each of `waves` waves, outside the timers; st <- the buffer.
template <class Launch>
int read_stamps(rnnwf_handle* h, Launch&& launch, size_t waves, int words, std::vector<unsigned long long>& st) {
    unsigned long long* dev = nullptr;
    const size_t bytes = waves * words * sizeof(unsigned long long);
    RNNWF_HIP(h, hipMalloc((void**)&dev, bytes));
    RNNWF_HIP(h, hipMemsetAsync(dev, 0, bytes, h->stream));
    launch(dev);
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    st.resize(waves * words);
    RNNWF_HIP(h, hipMemcpy(st.data(), dev, bytes, hipMemcpyDeviceToHost));
    RNNWF_HIP(h, hipFree(dev));
    return 0;
}
// the same, then one stderr line: counter k's median, minimum and maximum over the waves under names[k]
template <class Launch>
int read_stamps(rnnwf_handle* h, Launch&& launch, size_t waves, int words, const char* label, unsigned grid, std::initializer_list<const char*> names) {
    std::vector<unsigned long long> st;
    if (int rc = read_stamps(h, launch, waves, words, st)) return rc;
    fprintf(stderr, "%s grid=%u waves=%zu:", label, grid, waves);
    int k = 0;
    for (const char* name : names) {
        std::vector<unsigned long long> v(waves);
        for (size_t w = 0; w < waves; ++w) v[w] = st[w * words + k];
        std::sort(v.begin(), v.end());
        fprintf(stderr, " %s med %llu min %llu max %llu;", name, v[waves / 2], v[0], v[waves - 1]);
        ++k;
    }
    fprintf(stderr, "\n");
    return 0;
}
#endif

// ---- bf16x3 engine for the flip pass (f32 models; above 52 units: split_stream.hip) ----------------------
template <int NF32, int RJ, int WAVES, int MODE>
struct SLaunch {
    using L = SplitLayout<NF32, RJ, 1, MODE>;
    static int flip(rnnwf_handle* h, const PrnnArgs& a, int kt16) {
        if (L::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", L::HP, 4 * kt16);
        const int64_t ntiles = (int64_t)(a.N - 1) * ((a.ns + 31) / 32);
        return launch_persistent(h, kTimerFlip, prnn_flip_split_kernel<NF32, RJ, WAVES, MODE>, WAVES * 64, L::LDS_BYTES, ntiles, WAVES, a,
                                 h->wsplit.p, kt16);
    }
    // ping-pong form (8 waves per workgroup, two per SIMD, alternating MFMA / VALU segments): K-packed layouts only.  One layer runs
    // the g-state form of the step on the g-state form of the image (h->wsplit_g; pack_split.h)
    static int flip_pp(rnnwf_handle* h, const PrnnArgs& a, int kt16) {
        if constexpr (MODE == 2) {
            const auto kern = prnn_flip_pp_kernel<NF32, RJ, false, true>;
            const void* img = h->wsplit_g.p;
            if (L::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", L::HP, 4 * kt16);
            const int64_t ntiles = (int64_t)(a.N - 1) * ((a.ns + 31) / 32);
            unsigned grid = 0;
            if (int rc = persistent_grid(h, kern, 512, L::BYTES, ntiles, 8, &grid)) return rc;
#ifdef RNNWF_DIAGNOSTICS
            if (getenv("RNNWF_STAMPS")) {
                return read_stamps(h, [&](unsigned long long* buf) { PrnnArgs b = a; b.stamps = buf; kern<<<grid, 512, L::BYTES, h->stream>>>(b, img, kt16, StackArgs{}); },
                                   (size_t)grid * 8, 16, "RNNWF_STAMPS", grid,
                                   {"mfma_seg", "barrier_after_mfma", "valu_seg_split_part", "barrier_after_valu", "tile_switch", "total_cycles",
                                    "realtime_ticks_100MHz", "iterations", "valu_seg_gates", "valu_seg_head_logsoftmax"});
            }
#endif
            return timed_launch(h, kTimerFlip, kern, grid, 512, L::BYTES, a, img, kt16, StackArgs{});
        } else {
            return flip(h, a, kt16);
        }
    }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_split_image<NF32, RJ, 1, MODE>(h); }
    // the layout's g-state form (pack_split.h): false for a layout whose kernels have none
    static bool gstate(GstateLayout* g) {
        if constexpr (MODE == 2) { *g = gstate_layout<L>(); return true; }
        else return false;
    }
    static double mfma_flops_per_step() { return (double)L::NT * L::KS * 32768.0; }   // per 32-chain wave-step
};

// ---- bf16x3 engine for the swap pass (num_units <= 52) ---------------------------------------------------
template <int NF32, int RJ, int WAVES, int MODE>
struct CSLaunch {
    using L = SplitLayout<NF32, RJ, 3, MODE>;
    static int swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int kt16) {
        return launch_persistent(h, kTimerFlip, crnn_swap_split_kernel<NF32, RJ, WAVES, MODE>, WAVES * 64, L::BYTES, max_tiles, WAVES, a,
                                 h->wsplit.p, kt16);
    }
    // ping-pong form (8 waves per workgroup, alternating MFMA / VALU segments): K-packed layout MODE 2 only
    static int swap_pp(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int kt16) {
        if constexpr (MODE == 2) {
            if (L::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", L::HP, 4 * kt16);
            return launch_persistent(h, kTimerFlip, crnn_swap_pp_kernel<NF32, RJ>, 512, SplitPP<NF32, RJ, 3>::LDS_WITH_SLOTS, max_tiles, 8, a,
                                     h->wsplit.p, kt16, StackArgs{});
        } else {
            return swap(h, a, max_tiles, kt16);
        }
    }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_split_image<NF32, RJ, 3, MODE>(h); }
    static double mfma_flops_per_step() { return (double)L::NT * L::KS * 32768.0; }
};

// fn(K<NF32, RJ, WAVES, MODE>()) for the handle's row of the bf16x3 table (shapes.h) among those of this translation unit (MODE 0..2),
// false (fn not called) for a width without kernels here: K = SLaunch (positive RNN) or CSLaunch (complex RNN), which share the
// bf16x3 layouts of each width
template <template <int, int, int, int> class K, class Fn>
bool with_layout(const rnnwf_handle* h, Fn&& fn) {
    return with_row<NotRiders>(SplitKernels(), h, [&](auto r) { fn(K<decltype(r)::NF32, decltype(r)::RJ, decltype(r)::WAVES, decltype(r)::MODE>()); });
}

// widths served by the riders form (split_stream.hip: the table's MODE 3 rows, 53..100 units); every caller of with_layout asks this first
bool riders(const rnnwf_handle* h) { return with_row<Riders>(SplitKernels(), h, [](auto) {}); }

}  // namespace

// ---- cooperative base pass on the bf16 matrix core (gru_kernels.h: coop_base_pass_bf) ---------------------------------
namespace {
template <int NFULL>
struct BfBase {
    using B = BaseBfLayout<NFULL>;
    static constexpr int NF = NFULL;
    template <int NOUT> static size_t lds_bytes() {
        return GruLayout<float, NFULL, NOUT>::BYTES + B::BYTES + (size_t)B::NB * (B::PB_BYTES + (size_t)2 * (4 * NFULL + 1) * 64 * 4 + 2 * 64 * 4);
    }
    template <typename Args, typename Kern>
    static int launch(rnnwf_handle* h, const Args& a, Kern kern, size_t lds) {
        const int threads = B::NB * (B::NW + 1) * 64;              // per block: NW product / gate waves + the sampler
        // every CU gets work before any workgroup gets a second block: grid = min(blocks, CUs x resident workgroups)
        unsigned grid = 0;
        if (int rc = persistent_grid(h, kern, threads, lds, a.nsb, 1, &grid)) return rc;
#ifdef RNNWF_DIAGNOSTICS
        if constexpr (std::is_same<Args, PrnnArgs>::value) {
            if (getenv("RNNWF_STAMPS_BASE")) {    // median over the waves of each role -> stderr (tools/stamps_base.py)
                const size_t nwv = (size_t)grid * B::NB * (B::NW + 1);
                std::vector<unsigned long long> st;
                if (int rc = read_stamps(h, [&](unsigned long long* buf) { Args b = a; b.stamps = buf; kern<<<grid, threads, lds, h->stream>>>(b); }, nwv, 8, st)) return rc;
                const char* names[7] = {"products", "wait_barrier_B", "gates_writes", "wait_barrier_A", "site", "total_cycles", "realtime_100MHz"};
                for (int role = 0; role < 3; ++role) {
                    fprintf(stderr, "RNNWF_STAMPS_BASE grid=%u %s waves:", grid, role == 2 ? "sampler" : role ? "remainder" : "gate");
                    for (int k = 0; k < 7; ++k) {
                        std::vector<unsigned long long> v;
                        for (size_t w = 0; w < nwv; ++w) {
                            const int mm = (int)st[w * 8 + 7], r_ = mm < NFULL ? 0 : mm == NFULL ? 1 : 2;
                            if (st[w * 8 + 5] && r_ == role) v.push_back(st[w * 8 + k]);
                        }
                        if (v.empty()) continue;
                        std::sort(v.begin(), v.end());
                        fprintf(stderr, " %s med %llu max %llu;", names[k], v[v.size() / 2], v.back());
                    }
                    fprintf(stderr, "\n");
                }
                return 0;
            }
        }
#endif
        return timed_launch(h, kTimerBase, kern, grid, threads, lds, a);
    }
};
// fn(BfBase<NFULL>()) for the handle's row of the cooperative bf16 base pass's table (shapes.h); false for a width without kernels
template <class Fn>
bool with_bf_base(const rnnwf_handle* h, Fn&& fn) {
    return with_row(BaseBfKernels(), h, [&](auto row) { fn(BfBase<decltype(row)::NFULL>()); });
}
int no_bf_base(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no bf16 cooperative base kernel for NFULL=%d", h->NFULL); }
}  // namespace

bool rnnwf::base_bf_available(const rnnwf_handle* h) { return h->base_bf; }

int rnnwf::base_bf_pack(rnnwf_handle* h) {
    h->base_bf = false;
    // measured (profiles/r03_g_base_pass.md): at 37..52 units the pass gains 14 - 16 % (configs 2, 3); at 20 units and 500 samples
    // (config 1) the f32 cooperative kernel is 9 % faster - its image is three times smaller to stage - so narrower models keep it
    if (h->f64 || h->NL != 1 || h->NFULL != 3 || h->knobs.base_f32 || h->knobs.no_coop || h->knobs.engine == 1) return 0;
    std::vector<char> img;
    if (!with_bf_base(h, [&](auto b) { img = pack_base_bf_image<decltype(b)::NF>(h); })) return 0;
    if (int rc = ensure(h, h->wbasebf, img.size())) return rc;
    if (int rc = upload(h, h->wbasebf.p, img.data(), img.size())) return rc;
    h->base_bf = true;
    return 0;
}

int rnnwf::prnn_base_coop_bf(rnnwf_handle* h, const PrnnArgs& a0) {
    PrnnArgs a = a0;
    a.wbf = h->wbasebf.p;
    int rc = 0;
    return with_bf_base(h, [&](auto b) {
        using B = decltype(b);
        rc = B::launch(h, a, prnn_base_coop_kernel<B::NF, true>, B::template lds_bytes<1>());
    }) ? rc : no_bf_base(h);
}

int rnnwf::crnn_base_coop_bf(rnnwf_handle* h, const CrnnArgs& a0) {
    CrnnArgs a = a0;
    a.wbf = h->wbasebf.p;
    int rc = 0;
    return with_bf_base(h, [&](auto b) {
        using B = decltype(b);
        rc = B::launch(h, a, crnn_base_coop_kernel<B::NF, true>, B::template lds_bytes<3>());
    }) ? rc : no_bf_base(h);
}

// ---- device-resident training (train.hip): the tables of the engine's images over Lin into the active PackTrace, each from the row
// its host packer takes (pack_value.h); != 0: no such row ---------------------------------------------------------------------
int rnnwf::base_bf_pack_table(rnnwf_handle* h) {             // h->wbasebf
    return with_bf_base(h, [&](auto b) { pack_base_bf_image<decltype(b)::NF, Lin>(h); }) ? 0 : 1;
}
int rnnwf::split_pack_table(rnnwf_handle* h) {               // h->wsplit of one layer, the riders rows too
    const bool cplx = h->model == RNNWF_MODEL_CRNN_U1;
    return with_row(SplitKernels(), h, [&](auto row) {
        using R = decltype(row);
        if (cplx) pack_split_image<R::NF32, R::RJ, 3, R::MODE, Lin>(h);
        else pack_split_image<R::NF32, R::RJ, 1, R::MODE, Lin>(h);
    }) ? 0 : 1;
}

// the positive RNN's g-state image (h->wsplit_g) once more from h->wsplit as the re-pack kernel has just left it, on the stream: the
// host packer's own fold (pack_split.h: gstate_word), one thread per word.  Nothing to do for a handle without that image.
namespace {
__global__ void gstate_refold_kernel(GstateLayout g, const char* __restrict__ img, uint32_t* __restrict__ out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < g.BYTES / 4) out[w] = gstate_word(g, img, w);
}
// the range word of that image (pack_split.h: gstate_range): one thread per owned unit of the two lane halves, the largest bound through
// LDS, one vector store.  One block, launched behind the refold on the same stream - the flip pass that reads the word is behind both.
__global__ void __launch_bounds__(128) gstate_range_kernel(GstateLayout g, const char* __restrict__ img, uint32_t* __restrict__ out) {
    __shared__ double bound[128];
    const int NU = 16 * g.NF32 + g.RJ, t = threadIdx.x;
    bound[t] = t < 2 * NU ? gstate_range_unit(g, img, t % NU, t / NU) : 0.0;
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (t < s) bound[t] = gstate_max(bound[t], bound[t + s]);
        __syncthreads();
    }
    if (t == 0) out[gstate_range_word_index(g)] = gstate_range_word(bound[0]);
}
}  // namespace
static bool gstate_of(const rnnwf_handle* h, GstateLayout* g) {
    bool has = false;
    if (h->model != RNNWF_MODEL_CRNN_U1 && h->NL == 1 && !riders(h)) with_layout<SLaunch>(h, [&](auto k) { has = decltype(k)::gstate(g); });
    return has;
}
bool rnnwf::prnn_split_gstate_layout(const rnnwf_handle* h, int32_t* layout10) {
    GstateLayout g{};
    static_assert(offsetof(GstateLayout, NF32) == 40, "ten 32-bit fields, then the packer's own");
    if (!gstate_of(h, &g)) return false;
    memcpy(layout10, &g, 40);
    return true;
}
bool rnnwf::prnn_split_gstate_range(const rnnwf_handle* h, const std::vector<char>& simg, const std::vector<char>& simg_g, double* bound, uint32_t* word) {
    GstateLayout g{};
    if (!gstate_of(h, &g) || simg.size() < g.BYTES || simg_g.size() < g.BYTES) return false;
    *bound = gstate_range(g, simg.data());
    *word = reinterpret_cast<const uint32_t*>(simg_g.data())[gstate_range_word_index(g)];
    return true;
}
int rnnwf::split_gstate_refold(rnnwf_handle* h) {
    GstateLayout g{};
    if (!h->wsplit_g.p || !gstate_of(h, &g)) return 0;
    if (g.BYTES > h->wsplit.cap || g.BYTES > h->wsplit_g.cap) return h->fail(RNNWF_ERR_STATE, "g-state image larger than its buffers");
    if (2 * (16 * g.NF32 + g.RJ) > 128) return h->fail(RNNWF_ERR_STATE, "g-state range kernel: more than 128 owned units");
    gstate_refold_kernel<<<(g.BYTES / 4 + 255) / 256, 256, 0, h->stream>>>(g, (const char*)h->wsplit.p, (uint32_t*)h->wsplit_g.p);
    RNNWF_HIP(h, hipGetLastError());
    gstate_range_kernel<<<1, 128, 0, h->stream>>>(g, (const char*)h->wsplit.p, (uint32_t*)h->wsplit_g.p);
    RNNWF_HIP(h, hipGetLastError());
    return 0;
}

// ---- stacked layers on the bf16x3 engine: a pipeline of one kernel per layer (split_core.h: SplitUpperLayout) -----------------
namespace {
constexpr int kStackNF32 = 1, kStackRJ = 9;                  // the K-packed layout of 37..50 units (SplitLayout MODE 2)
using StackL0 = SplitLayout<kStackNF32, kStackRJ, 1, 2>;
using StackU1 = SplitUpperLayout<kStackNF32, kStackRJ, 1>;
using StackU3 = SplitUpperLayout<kStackNF32, kStackRJ, 3>;

}  // namespace

bool rnnwf::stack_split_available(const rnnwf_handle* h) {
    return !h->f64 && h->NL > 1 && h->NFULL == 3 && h->H <= 50 && h->knobs.engine != 1 &&
           (h->model == RNNWF_MODEL_GRU1D || h->model == RNNWF_MODEL_GRU1D_PARITY || h->model == RNNWF_MODEL_CRNN_U1);
}
size_t rnnwf::stack_record_bytes_per_32_chains(const rnnwf_handle* h, int64_t steps) {
    return (size_t)steps * StackU1::RECORD_FLOATS * 4 * (h->NL > 2 ? 2 : 1);
}
double rnnwf::stack_split_flops_per_step(rnnwf_handle* h) {
    return ((double)StackL0::NT * StackL0::KS + (double)(h->NL - 1) * 2.0 * StackU1::NTB * StackL0::KS) * 32768.0;
}

template <int NOUT>
int rnnwf::stack_pack(rnnwf_handle* h) {
    {
        const std::vector<char> img = pack_split_image<kStackNF32, kStackRJ, NOUT, 2>(h);
        if (int rc = ensure(h, h->wsplit, img.size())) return rc;
        if (int rc = upload(h, h->wsplit.p, img.data(), img.size())) return rc;
    }
    for (int l = 1; l < h->NL; ++l) {
        const std::vector<char> img = pack_split_upper_image<kStackNF32, kStackRJ, NOUT>(h, l, l == h->NL - 1);
        if (int rc = ensure(h, h->wsplit_up[l - 1], img.size())) return rc;
        if (int rc = upload(h, h->wsplit_up[l - 1].p, img.data(), img.size())) return rc;
    }
    return 0;
}
template int rnnwf::stack_pack<1>(rnnwf_handle*);
template int rnnwf::stack_pack<3>(rnnwf_handle*);
// the table of one of those images: layer 0 -> h->wsplit, layer l >= 1 -> h->wsplit_up[l - 1]
int rnnwf::stack_pack_table(rnnwf_handle* h, int layer) {
    const bool cplx = h->model == RNNWF_MODEL_CRNN_U1, top = layer == h->NL - 1;
    if (layer == 0) {
        if (cplx) pack_split_image<kStackNF32, kStackRJ, 3, 2, Lin>(h);
        else pack_split_image<kStackNF32, kStackRJ, 1, 2, Lin>(h);
    } else {
        if (cplx) pack_split_upper_image<kStackNF32, kStackRJ, 3, Lin>(h, layer, top);
        else pack_split_upper_image<kStackNF32, kStackRJ, 1, Lin>(h, layer, top);
    }
    return 0;
}

namespace {
// The layer pipeline over `tiles` 32-chain tiles: first (the first layer's kernel, STACK form), then one upper kernel per further layer -
// middle below the top, last at the top - each reading the records (h->xrec, record_bytes each, two buffers alternating) the one below
// wrote.  The whole pipeline is the "flip pass" of the timers.
template <class Args, class K0, class KU>
int stack_pipeline(rnnwf_handle* h, const Args& a, K0 first, KU middle, KU last, size_t lds_first, size_t lds_upper, int64_t tiles, size_t record_bytes) {
    const int kt16 = 4 * h->NFULL + 1, NL = h->NL;
    if (StackL0::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", StackL0::HP, 4 * kt16);
    if (int rc = ensure(h, h->xrec[0], record_bytes)) return rc;
    if (NL > 2) if (int rc = ensure(h, h->xrec[1], record_bytes)) return rc;
    unsigned g0 = 0, gu = 0, gl = 0;
    if (int rc = persistent_grid(h, first, 512, lds_first, tiles, 8, &g0)) return rc;
    if (int rc = persistent_grid(h, middle, 512, lds_upper, tiles, 8, &gu)) return rc;
    if (int rc = persistent_grid(h, last, 512, lds_upper, tiles, 8, &gl)) return rc;
    TimedLaunch tl(h, kTimerFlip);
    StackArgs st{nullptr, (float*)h->xrec[0].p, NL * kt16, 0};
    if (int rc = plain_launch(h, first, g0, 512, lds_first, a, h->wsplit.p, kt16, st)) return rc;
    for (int l = 1; l < NL; ++l) {
        const bool top = l == NL - 1;
        st.xin = (const float*)h->xrec[(l - 1) & 1].p;
        st.xout = top ? nullptr : (float*)h->xrec[l & 1].p;
        st.koff = l * kt16;
#ifdef RNNWF_DIAGNOSTICS
        if constexpr (std::is_same<Args, PrnnArgs>::value) {
            if (top && getenv("RNNWF_STAMPS")) {                  // the top layer's kernel
                const void* wup = h->wsplit_up[l - 1].p;
                if (int rc = read_stamps(h, [&](unsigned long long* buf) { Args b = a; b.stamps = buf; last<<<gl, 512, lds_upper, h->stream>>>(b, wup, kt16, st); },
                                         (size_t)gl * 8, 16, "RNNWF_STAMPS upper kernel", gl,
                                         {"mfma_seg", "barrier_after_mfma", "valu_seg_split_part", "barrier_after_valu", "tile_switch", "total_cycles",
                                          "realtime_ticks_100MHz", "iterations", "valu_seg_head_gates", "valu_seg_store_head"})) return rc;
                continue;
            }
        }
#endif
        if (int rc = plain_launch(h, top ? last : middle, top ? gl : gu, 512, lds_upper, a, h->wsplit_up[l - 1].p, kt16, st)) return rc;
    }
    return 0;
}
}  // namespace

int rnnwf::prnn_stack_flip(rnnwf_handle* h, const PrnnArgs& a) {
    const int64_t nsb32 = (a.ns + 31) / 32;
    const int64_t nrec = nsb32 * (int64_t)a.N * (a.N - 1) / 2;
    return stack_pipeline(h, a, prnn_flip_pp_kernel<kStackNF32, kStackRJ, true>, prnn_flip_pp_upper_kernel<kStackNF32, kStackRJ, false>,
                          prnn_flip_pp_upper_kernel<kStackNF32, kStackRJ, true>, StackL0::BYTES, StackU1::LDS_BYTES, (int64_t)(a.N - 1) * nsb32,
                          (size_t)nrec * StackU1::RECORD_FLOATS * 4);
}

// max_records: upper bound of the wave-steps of all tiles (crnn.hip derives it from the bonds a first-changed site can have)
int rnnwf::crnn_stack_swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int64_t max_records) {
    return stack_pipeline(h, a, crnn_swap_pp_kernel<kStackNF32, kStackRJ, true>, crnn_swap_pp_upper_kernel<kStackNF32, kStackRJ, false>,
                          crnn_swap_pp_upper_kernel<kStackNF32, kStackRJ, true>, SplitPP<kStackNF32, kStackRJ, 3>::LDS_WITH_SLOTS, StackU3::LDS_BYTES,
                          max_tiles, (size_t)max_records * StackU3::RECORD_FLOATS * 4);
}

int rnnwf::prnn_split_flip(rnnwf_handle* h, const PrnnArgs& a) {
    const int kt16 = 4 * h->NFULL + 1;
    if (riders(h)) return prnn_split_flip_stream(h, a, kt16);
    int rc = 0;
    if (with_layout<SLaunch>(h, [&](auto k) { rc = decltype(k)::flip_pp(h, a, kt16); })) return rc;
    return h->fail(RNNWF_ERR_INVALID, "no bf16x3 kernel for NFULL=%d", h->NFULL);
}
double rnnwf::prnn_split_flops_per_step(rnnwf_handle* h) {
    if (riders(h)) return prnn_split_stream_flops_per_step(h);
    double f = 0;
    with_layout<SLaunch>(h, [&](auto k) { f = decltype(k)::mfma_flops_per_step(); });
    return f;
}


int rnnwf::prnn_split_pack(rnnwf_handle* h, std::vector<char>& simg, std::vector<char>& simg_g) {
    simg_g.clear();
    if (riders(h)) return prnn_split_stream_pack(h, simg);
    if (with_layout<SLaunch>(h, [&](auto k) {
            simg = decltype(k)::pack(h);
            GstateLayout g;
            if (decltype(k)::gstate(&g)) simg_g = gstate_image(g, simg);
        })) return 0;
    return h->fail(RNNWF_ERR_INVALID, "no bf16x3 layout for NFULL=%d", h->NFULL);
}

int rnnwf::crnn_split_swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles) {
    const int kt16 = 4 * h->NFULL + 1;
    if (riders(h)) return crnn_split_swap_stream(h, a, max_tiles, kt16);
    int rc = 0;
    if (with_layout<CSLaunch>(h, [&](auto k) { rc = decltype(k)::swap_pp(h, a, max_tiles, kt16); })) return rc;
    return h->fail(RNNWF_ERR_INVALID, "no bf16x3 cRNN kernel for NFULL=%d", h->NFULL);
}
double rnnwf::crnn_split_flops_per_step(rnnwf_handle* h) {
    if (riders(h)) return crnn_split_stream_flops_per_step(h);
    double f = 0;
    with_layout<CSLaunch>(h, [&](auto k) { f = decltype(k)::mfma_flops_per_step(); });
    return f;
}


int rnnwf::crnn_split_pack(rnnwf_handle* h, std::vector<char>& simg) {
    if (riders(h)) return crnn_split_stream_pack(h, simg);
    if (with_layout<CSLaunch>(h, [&](auto k) { simg = decltype(k)::pack(h); })) return 0;
    return h->fail(RNNWF_ERR_INVALID, "no bf16x3 layout for NFULL=%d", h->NFULL);
}
