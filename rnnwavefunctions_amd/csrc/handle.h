// handle.h - the opaque handle behind include/rnnwf.h (host side).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <cstdio>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rnnwf.h"

namespace rnnwf {

struct Family;   // models.h

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// The kernel groups of rnnwf_timing_get (include/rnnwf.h), the index of rnnwf_handle::timers
enum TimerId : int { kTimerBase = 0, kTimerFlip = 1, kTimerAssembly = 2, kTimerBackprop = 3, kTimerGemm = 4, kTimerCount };

// Default bytes of checkpointed states per pass of the GRU, complex RNN, LSTM and Renyi swap passes (RNNWF_STATE_BUDGET_MB
// overrides it: models.h: state_budget_bytes)
constexpr size_t kDefaultStateBudget = (size_t)48 << 30;

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double total_ms = 0.0;
    int64_t launches = 0;
};

// Environment switches, read ONCE in rnnwf_create (never on the per-step path).
struct Knobs {
    int engine = 0;               // RNNWF_ENGINE: 0 default, 1 "f32" (f32-input MFMA everywhere), 2 "bf16x3" (pinned); any other value is refused.  The measured-negative
                                  // kernel variants and their A/B switches (four engines, the 2D RNN's prefetch) were removed after commit f88b60d: DESIGN.md 10
    bool no_coop = false;         // RNNWF_NO_COOP=1: base pass always on the one-wave-per-block kernel
    bool base_f32 = false;        // RNNWF_BASE=f32: the base pass keeps the f32-input MFMA (no bf16 cooperative kernel): A/B, and the
                                  // bit-identity test of the two f32 kernels
    size_t state_budget = 0;      // RNNWF_STATE_BUDGET_MB << 20 (0: the family's default)
    int ablate = 0, ablate_base = 0;   // RNNWF_ABLATE / RNNWF_ABLATE_BASE: only in -DRNNWF_DIAGNOSTICS builds (tools/)
};

// Device-resident training (train.hip): the parameters, Adam's moments and the flat gradient live on the device; after every update
// the kernels' weight images are rebuilt there by replaying the host packers' recorded element tables (pack_value.h).
struct TrainImage {
    DevBuf table;                 // PackEntry[n]
    int64_t n = 0;
    DevBuf* target = nullptr;     // the image it rebuilds (h->wimg, h->wsplit, ...)
};
struct TrainState {
    bool built = false, supported = false;
    std::string why;              // why not supported
    DevBuf P, M, V, G;            // flat f64: parameters (order of rnnwf_set_params_flat), Adam's m and v, gradient
    DevBuf gidx;                  // int32[nparams]: +-(k + 1) = element k of the dW image (sign: the head's logit difference), 0: none
    int64_t nparams = 0;
    size_t dw_count = 0;
    bool dw_f64 = false;
    TrainImage img[8];
    int nimg = 0;
    int64_t adam_t = 0;           // updates applied so far (tf.train.AdamOptimizer's beta powers are beta^(t+1))
    bool host_newer = true;       // the host copy of the parameters changed since the device copy was made
    bool dev_newer = false;       // the device copy was updated by an optimizer step the host copy has not seen
    void* mom_host = nullptr;     // pinned [kMaxSteps][4] doubles: the moments of the K steps of one rnnwf_train_steps call
    void* mom_host_dev = nullptr; // the same memory as the device addresses it
    DevBuf combo;                 // the tables of all images back to back: ONE re-pack launch per update (train.hip: repack_all_kernel)
    int combo_nimg = 0;           // images the combined table was built from
};

struct ParamSpec {
    std::vector<int64_t> shape; // as the caller sees it (the reference's TF variable)
    std::vector<double> value;  // stored in f64, converted to the model type when packed.  Layers of unequal width are held PADDED
                                // to the widest layer (zeros: a padded unit stays exactly 0 and feeds nothing), so that the packers
                                // and kernels see one width; `slot` maps the caller's flat index to the padded one.
    std::vector<int64_t> slot;  // size = number of elements the caller sees
    bool set = false;
};

}  // namespace rnnwf

struct rnnwf_handle {
    rnnwf_config cfg{};
    int model = 0;
    const rnnwf::Family* family = nullptr;   // the model's table of host hooks (models.h)
    bool f64 = false;
    int H = 0;       // num_units
    int NFULL = 0;   // padded hidden size = 16 NFULL + 4
    int NL = 1;      // stacked GRU layers (len(units)); > 1 only for the f32 1D positive RNN
    int N = 0;       // chain length (nx * ny)
    int Nx = 1, Ny = 1;
    int cu_count = 0;
    std::string err;
    hipStream_t stream = nullptr;
    std::map<std::string, rnnwf::ParamSpec> params;
    std::map<std::string, std::vector<int32_t>> param_flat;   // per tensor: padded index -> index in the flat parameter vector
                                                              // (order of rnnwf_set_params_flat), -1 for padding (pack_value.h)
    bool committed = false;

    // device buffers (grown on demand, owned by the handle)
    rnnwf::DevBuf wimg, samples_i32, bits, bits2, hck, lpq, lpq2, out_lp, out_lp2, eloc, moments, coupl, maps;
    // J1J2 / cRNN
    rnnwf::DevBuf camp, tiles, tile_count, cbase, cout;
    // MDRNN
    rnnwf::DevBuf rowbuf;
    // gradient (grad.hip)
    rnnwf::DevBuf wbwd, gradP, gradQ, gradW;
    bool wbwd_valid = false;      // the backward image matches the committed parameters (re-packed by the next gradient call otherwise)
    rnnwf::DevBuf gradPart, gradHeadPart;    // per-block partial sums of the weight-gradient GEMM; per-wave head-row sums
    std::vector<double> coupl_host;   // what h->coupl holds (couplings rarely change between steps: skip the upload)
    rnnwf::DevBuf gradDX[2];      // stacked layers: dL/dx of one layer's pass = dL/dh input of the pass below
    // bf16x3 engine (split_core.h): second weight image; engine_split = use it for the flip pass
    rnnwf::DevBuf wsplit;
    rnnwf::DevBuf wsplit_g;       // positive RNN, one layer, 37..50 units: the g-state form of wsplit, which the ping-pong flip kernel reads
                                  // (pack_split.h: gstate_word; rebuilt from wsplit wherever wsplit is)
    rnnwf::DevBuf wsplit16;       // image of the 16x16x32 form of the flip pass at 69..100 units (split16_core.h)
    rnnwf::DevBuf wbasebf;        // bf16x3 A fragments of the cooperative base pass (layout.h: BaseBfLayout); valid iff base_bf
    rnnwf::DevBuf wsplit_up[RNNWF_MAX_LAYERS - 1];   // stacked layers on the bf16x3 engine: image of layer l in [l - 1] (split_core.h: SplitUpperLayout)
    rnnwf::DevBuf xrec[2];        // their layer pipeline: per-step state records of one layer, read by the kernel of the layer above
    rnnwf::TrainState train;      // device-resident training (train.hip)
    bool base_bf = false;
    bool engine_split = false;
    bool engine_forced = false;   // RNNWF_ENGINE=bf16x3: no small-batch fallback to the f32-input MFMA
    int64_t call_ns = 0;          // samples of the whole API call (a call may run several passes: one engine for all)
    int last_flip_engine = -1;    // engine of the last flip / swap launch (1 bf16x3, 0 f32-input MFMA), -1 none yet
    std::map<std::string, std::vector<double>> grads;
    int64_t last_ns = 0;          // batch of the last rnnwf_vmc_step still resident (bits, hck, eloc)
    void* pinned = nullptr;  // small pinned staging (moments)
    void* pinned_dev = nullptr;   // the same memory as the device addresses it: kernels write the step's 32 + 24 result bytes there directly
    double* moments_direct = nullptr;   // device address of the pinned row the moments kernel also writes to (set per iteration by rnnwf_train_steps)
    bool j1j2_cnt_clean = false;  // the J1-J2 item counters are zero (left so by the last assembly kernel)
    void* staging = nullptr; // pinned staging of the host-side all-reduces (comm.hip) and of the gradient's download, grown on demand
    size_t staging_cap = 0;
    void* upbuf = nullptr;   // pinned buffer the weight images travel through on their way to the device (upload(), below)
    size_t upbuf_cap = 0, upbuf_off = 0;
    rnnwf::DevBuf reduce_scratch;
    rnnwf::DevBuf renyi;          // rnnwf_renyi2_swap, rnnwf_renyi2_regions, rnnwf_pauli_step: tables, per-site terms, tails, log-ratios and partial sums of one pass
    // stochastic reconfiguration (sr.hip): the per-sample log-derivatives J[sr_ns][D] in image order, the chains' head rows, how many
    // parameters read each image element, column sums [mean | J^T y], the centred Gram matrix, the weights y, and the workspace of the
    // device solve: [ns][ns] Cholesky factor | eps row [ns] | y [ns] | pivot status word | diagonal blocks (sr_solve_kernels.h);
    // srStat: rnnwf_sr_train_steps' pivot status of one call, [0] sticky (1 + the first iteration with a bad pivot), [1 + k] iteration k's word
    rnnwf::DevBuf srJ, srHead, srMask, srCol, srGram, srY, srFac, srStat;
    bool sr_valid = false;        // srJ belongs to the resident batch and the committed parameters (cleared where either changes)
    int64_t sr_ns = 0;
    std::vector<int32_t> sr_sidx; // grad_flat_probe's table, probed once
    rnnwf::DevBuf tck, corr;      // rnnwf_correlations: trunk states [N(N-1)/2][nsb][KT][64]; site / trunk / branch terms, log-ratios and sums of one pass (corr.hip)

    bool timing_on = false;
    int timing_mask = 31;    // which kernel ids get HIP events (rnnwf_timing_enable: 1 = all, 2 = the dominant pass only)
    rnnwf::KernelTimer timers[rnnwf::kTimerCount];   // indexed by rnnwf::TimerId
    double work[2] = {0.0, 0.0};

    rnnwf::Knobs knobs;
    // resident blocks per CU of each kernel this handle has launched (the dynamic-LDS attribute is per device and the
    // handle is single-threaded by contract, so the cache lives here: handles on other host threads share nothing)
    std::map<const void*, int> occupancy;

    void* comm = nullptr;  // ncclComm_t
    int rank = 0, nranks = 1;
    bool reduce_in_step = false;   // rnnwf_vmc_step returns the moments summed over all ranks (one RCCL all-reduce on the
                                   // stream, before the single host synchronisation of the step)

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define RNNWF_HIP(h, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return (h)->fail(RNNWF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace rnnwf {

inline int ensure(rnnwf_handle* h, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) RNNWF_HIP(h, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return h->fail(RNNWF_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    b.cap = want;
    return 0;
}

// Pinned staging of `bytes` (grown on demand, owned by the handle): a pageable source or destination makes hipMemcpyAsync a hidden
// synchronous copy through the runtime's own bounce buffer.
inline int ensure_staging(rnnwf_handle* h, size_t bytes) {
    if (bytes <= h->staging_cap) return 0;
    if (h->staging) RNNWF_HIP(h, hipHostFree(h->staging));
    h->staging = nullptr;
    h->staging_cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipHostMalloc(&h->staging, want, hipHostMallocDefault);
    if (e != hipSuccess) return h->fail(RNNWF_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    h->staging_cap = want;
    return 0;
}

// Host -> device copy of a freshly packed image, asynchronous on the handle's stream: the bytes are copied into the handle's
// pinned upload buffer first (bump-allocated; upload_reset() at the start of a commit waits for the previous commit's copies,
// which have long landed), so the caller's vector may die at once and nothing blocks.  A training iteration re-packs three to
// four images; with blocking hipMemcpy each cost 10-20 us of host time (tools/iter_breakdown.py).
inline int upload_reset(rnnwf_handle* h) {
    if (h->upbuf_off) RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    h->upbuf_off = 0;
    return 0;
}
inline int upload(rnnwf_handle* h, void* dst, const void* src, size_t bytes) {
    const size_t off = (h->upbuf_off + 255) & ~(size_t)255;
    if (off + bytes > h->upbuf_cap) {                     // full: wait for what is in flight, then start over - in the same buffer when the
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));    // image fits it (a caller that packs again and again without a commit in between, which
        if (bytes <= h->upbuf_cap) {                      // alone resets the offset, must not double the buffer at every overflow), else a larger one
            h->upbuf_off = 0;
            return upload(h, dst, src, bytes);
        }
        if (h->upbuf) RNNWF_HIP(h, hipHostFree(h->upbuf));
        h->upbuf = nullptr;
        h->upbuf_cap = 0;
        const size_t want = std::max<size_t>((size_t)1 << 20, 2 * (off + bytes));
        hipError_t e = hipHostMalloc(&h->upbuf, want, hipHostMallocDefault);
        if (e != hipSuccess) return h->fail(RNNWF_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        h->upbuf_cap = want;
        h->upbuf_off = 0;
        return upload(h, dst, src, bytes);
    }
    memcpy((char*)h->upbuf + off, src, bytes);
    RNNWF_HIP(h, hipMemcpyAsync(dst, (char*)h->upbuf + off, bytes, hipMemcpyHostToDevice, h->stream));
    h->upbuf_off = off + bytes;
    return 0;
}

// Resident blocks per CU of kernel `fn` at `threads` per block and `lds` dynamic bytes; raises the kernel's
// dynamic-LDS limit on first use.  Cached per handle.
inline int blocks_per_cu(rnnwf_handle* h, const void* fn, int threads, size_t lds, int* out) {
    auto it = h->occupancy.find(fn);
    if (it != h->occupancy.end()) { *out = it->second; return 0; }
    RNNWF_HIP(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int nb = 0;
    RNNWF_HIP(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds));
    nb = nb < 1 ? 1 : nb;
    h->occupancy[fn] = nb;
    *out = nb;
    return 0;
}

// HIP-event bracket around the launches of its scope on the handle's stream
struct TimedLaunch {
    rnnwf_handle* h;
    TimerId id;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    bool on() const { return h->timing_on && ((h->timing_mask >> id) & 1); }
    TimedLaunch(rnnwf_handle* h_, TimerId id_) : h(h_), id(id_) {
        if (!on()) return;
        KernelTimer& t = h->timers[id];
        if (!t.pool.empty()) {
            ev = t.pool.back();
            t.pool.pop_back();
        } else {
            hipEventCreate(&ev.first);
            hipEventCreate(&ev.second);
        }
        hipEventRecord(ev.first, h->stream);
    }
    ~TimedLaunch() {
        if (!on()) return;
        hipEventRecord(ev.second, h->stream);
        h->timers[id].pending.push_back(ev);
    }
};

// Grid of a persistent kernel: one workgroup per `per_block` items, at most as many workgroups as are resident at once (at
// `threads` per workgroup and `lds` dynamic bytes), at least one.
template <typename Kern>
inline int persistent_grid(rnnwf_handle* h, Kern kern, int threads, size_t lds, int64_t items, int64_t per_block, unsigned* grid) {
    int bpc = 0;
    if (int rc = blocks_per_cu(h, (const void*)kern, threads, lds, &bpc)) return rc;
    *grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, (int64_t)bpc * h->cu_count));
    return 0;
}

// kern<<<grid, threads, lds, h->stream>>>(args...), for a caller that holds the timer bracket itself (a pipeline of kernels under one)
template <typename Kern, typename... Args>
inline int plain_launch(rnnwf_handle* h, Kern kern, dim3 grid, int threads, size_t lds, const Args&... args) {
    kern<<<grid, threads, lds, h->stream>>>(args...);
    RNNWF_HIP(h, hipGetLastError());
    return 0;
}

// the same inside the bracket of timer `id`
template <typename Kern, typename... Args>
inline int timed_launch(rnnwf_handle* h, TimerId id, Kern kern, dim3 grid, int threads, size_t lds, const Args&... args) {
    TimedLaunch tl(h, id);
    return plain_launch(h, kern, grid, threads, lds, args...);
}

// persistent_grid + timed_launch
template <typename Kern, typename... Args>
inline int launch_persistent(rnnwf_handle* h, TimerId id, Kern kern, int threads, size_t lds, int64_t items, int64_t per_block,
                             const Args&... args) {
    unsigned grid = 0;
    if (int rc = persistent_grid(h, kern, threads, lds, items, per_block, &grid)) return rc;
    return timed_launch(h, id, kern, grid, threads, lds, args...);
}

// Items (16-chain blocks or flip tiles) one per wave: WAVES waves per workgroup where there are enough items to fill every
// resident workgroup slot, as few as still keep every slot busy otherwise.  For kernels whose LDS image allows few workgroups per
// CU, where a small batch in full-size workgroups would sit on a few CUs (config 2 with two layers: 625 blocks of 16 chains -> 3
// waves on each of 209 CUs instead of 8 on 79).  The occupancy is that of full workgroups.
template <int WAVES, typename Kern, typename... Args>
inline int launch_shrinking(rnnwf_handle* h, TimerId id, Kern kern, size_t lds, int64_t items, const Args&... args) {
    int bpc = 0;
    if (int rc = blocks_per_cu(h, (const void*)kern, WAVES * 64, lds, &bpc)) return rc;
    const int64_t slots = (int64_t)bpc * h->cu_count;
    const int wpb = (int)std::max<int64_t>(1, std::min<int64_t>(WAVES, (items + slots - 1) / slots));
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + wpb - 1) / wpb, slots));
    return timed_launch(h, id, kern, grid, wpb * 64, lds, args...);
}

// The kernels a family is built for: one row per shape (element type, layers, NFULL) with the waves per workgroup of its kernels.
// The families' tables are in shapes.h; every width-class dispatch of the host code walks one of them.
template <typename T_, int NL_, int NFULL_, int WAVES_>
struct KernelRow {
    using T = T_;
    static constexpr int NL = NL_, NFULL = NFULL_, WAVES = WAVES_;
    static bool serves(const rnnwf_handle* h) { return std::is_same<T, double>::value == (bool)h->f64 && NL == h->NL && NFULL == h->NFULL; }
};
// A row of the bf16x3 engine (f32 models, one layer; the callers ask for no other handle): width class NFULL runs on
// SplitLayout<NF32, RJ, ., MODE> (split_core.h) with WAVES waves per workgroup; HMIN <= num_units <= HMAX where a width class has two
// layouts.  MODE 3: the riders form (split_stream.hip)
template <int NFULL_, int NF32_, int RJ_, int WAVES_, int MODE_, int HMIN_ = 0, int HMAX_ = 1 << 30>
struct SplitRow {
    static constexpr int NFULL = NFULL_, NF32 = NF32_, RJ = RJ_, WAVES = WAVES_, MODE = MODE_, HMIN = HMIN_, HMAX = HMAX_;
    static bool serves(const rnnwf_handle* h) { return NFULL == h->NFULL && HMIN <= h->H && h->H <= HMAX; }
};
template <class R> struct Riders : std::bool_constant<R::MODE == 3> {};
template <class R> struct NotRiders : std::bool_constant<R::MODE != 3> {};
template <class... Rows> struct KernelTable {};

// fn(Row()) for the row of this handle's shape among the rows Keep admits (no code of another row is instantiated); false (fn not
// called) for a shape without kernels
template <class R> struct AnyRow : std::true_type {};
template <class R> struct OneLayer : std::bool_constant<R::NL == 1> {};
template <template <class> class Keep = AnyRow, class Fn, class... Rows>
inline bool with_row(KernelTable<Rows...>, const rnnwf_handle* h, Fn&& fn) {
    auto hit = [&](auto row) {
        if constexpr (Keep<decltype(row)>::value)
            if (decltype(row)::serves(h)) return fn(row), true;
        return false;
    };
    return (hit(Rows()) || ...);
}

// the same with fn(K<T, NFULL, NL, WAVES>()): a family's launch class of the row
template <template <typename, int, int, int> class K, class Table, class Fn>
inline bool with_kernels(Table t, const rnnwf_handle* h, Fn&& fn) {
    return with_row(t, h, [&](auto r) { fn(K<typename decltype(r)::T, decltype(r)::NFULL, decltype(r)::NL, decltype(r)::WAVES>()); });
}
// one-layer passes: fn(K<T, NFULL, WAVES>()) for the handle's row among the table's one-layer rows; false for a stack as well
template <template <typename, int, int> class K, class Table, class Fn>
inline bool with_layer_kernels(Table t, const rnnwf_handle* h, Fn&& fn) {
    return with_row<OneLayer>(t, h, [&](auto r) { fn(K<typename decltype(r)::T, decltype(r)::NFULL, decltype(r)::WAVES>()); });
}
// the same with fn(K<NFULL, WAVES>()): families of one element type
template <template <int, int> class K, class Table, class Fn>
inline bool with_width_kernels(Table t, const rnnwf_handle* h, Fn&& fn) {
    return with_row<OneLayer>(t, h, [&](auto r) { fn(K<decltype(r)::NFULL, decltype(r)::WAVES>()); });
}

}  // namespace rnnwf
