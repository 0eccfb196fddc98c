// split_stream.hip - the "riders" form of the bf16x3 engine (split_core.h: SplitLayout mode 3, SplitCore::step_stream): one wave
// per SIMD whose VALU work rides between its own MFMAs.  Flip pass of the positive RNN and swap pass of the complex RNN at
// 69..100 units (config 5; regular w3 fragments read through L2) and at 53..68 units (whole image in LDS).  A translation unit
// of its own: built WITHOUT -amdgpu-mfma-vgpr-form (build.py), so that the accumulators live in AGPRs next to ~250 VGPRs.
#include <algorithm>

#include "models.h"
#include "pack.h"
#include "pack_split.h"
#include "shapes.h"
#include "crnn_split_kernels.h"
#include "split_kernels.h"

using namespace rnnwf;

namespace {
// 32-chain flip tiles of one pass
int64_t ntiles(const PrnnArgs& a) { return (int64_t)(a.N - 1) * ((a.ns + 31) / 32); }
template <int NF32, int RJ, int WAVES>
struct RLaunch {
    using L = SplitLayout<NF32, RJ, 1, 3>;
    using LC = SplitLayout<NF32, RJ, 3, 3>;                  // complex RNN: three head rows
    static_assert(L::STREAM == LC::STREAM && L::STREAM == (L::HP > 68),
                  "layout mode 3 is LDS-resident up to 68 units and streams its regular w3 fragments above");
    // 69..100 units: the 16x16x32 form (generated asm step); 53..68 units: the compiler-scheduled riders step, image resident in LDS
    static int flip(rnnwf_handle* h, const PrnnArgs& a, int kt16) {
        if constexpr (L::STREAM) {
            return flip_asm16(h, a, kt16);
        } else {
            if (L::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", L::HP, 4 * kt16);
            return launch_persistent(h, kTimerFlip, prnn_flip_split_kernel<NF32, RJ, WAVES, 3>, WAVES * 64, L::LDS_BYTES, ntiles(a), WAVES, a,
                                     h->wsplit.p, kt16);
        }
    }
    // the 16x16x32 form (split16_core.h), 69..100 units
    static int flip_asm16(rnnwf_handle* h, const PrnnArgs& a, int kt16) {
        using L16 = S16Layout<1>;
        if (kt16 != L16::NJ) return h->fail(RNNWF_ERR_INVALID, "the 16x16x32 form expects %d checkpoint k-steps, got %d", L16::NJ, kt16);
        return launch_persistent(h, kTimerFlip, prnn_flip_riders16_asm_kernel<WAVES>, WAVES * 64, L16::LDS_BYTES, ntiles(a), WAVES, a,
                                 h->wsplit16.p, kt16);
    }
    static int swap(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int kt16) {
        if (LC::HP > 4 * kt16) return h->fail(RNNWF_ERR_INVALID, "bf16x3 layout wider than the checkpoint rows (%d > %d)", LC::HP, 4 * kt16);
        return launch_persistent(h, kTimerFlip, crnn_swap_split_kernel<NF32, RJ, WAVES, 3>, WAVES * 64, LC::LDS_BYTES, max_tiles, WAVES, a,
                                 h->wsplit.p, kt16);
    }
    // MFMA flops issued per 32-chain wave-step
    static double flip_flops_per_step() {
        // the 16x16x32 form: 19 tiles x 19 k-steps x 2 chain sets of 16 x 16 x 32 x 2 flop
        if constexpr (L::STREAM) return (double)S16Layout<1>::NT * S16Layout<1>::KS * 2 * 16384.0;
        else return (double)L::NT * L::KS * 32768.0;
    }
    static double swap_flops_per_step() { return (double)LC::NT * LC::KS * 32768.0; }
    static int flip_pack(rnnwf_handle* h, std::vector<char>& simg) {
        simg = pack_split_image<NF32, RJ, 1, 3>(h);
        if constexpr (L::STREAM) {
            // the flip pass reads only the 16x16x32 form's image (split16_core.h), uploaded here; no kernel reads the mode-3 image, which
            // goes to h->wsplit all the same: device-resident training (split.hip: split_pack_table) rebuilds that buffer at every width
            const std::vector<char> img16 = pack_split16_image<1>(h);
            if (int rc = ensure(h, h->wsplit16, img16.size())) return rc;
            if (int rc = upload(h, h->wsplit16.p, img16.data(), img16.size())) return rc;
        }
        return 0;
    }
    static std::vector<char> swap_pack(const rnnwf_handle* h) { return pack_split_image<NF32, RJ, 3, 3>(h); }
};

// fn(RLaunch<NF32, RJ, WAVES>()) for the handle's row among the riders rows (MODE 3) of the bf16x3 table (shapes.h); false for another width
template <class Fn>
bool with_riders(const rnnwf_handle* h, Fn&& fn) {
    return with_row<Riders>(SplitKernels(), h, [&](auto r) { fn(RLaunch<decltype(r)::NF32, decltype(r)::RJ, decltype(r)::WAVES>()); });
}
int no_riders(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no bf16x3 riders kernel for NFULL=%d", h->NFULL); }
}  // namespace

int rnnwf::prnn_split_flip_stream(rnnwf_handle* h, const PrnnArgs& a, int kt16) {
    int rc = 0;
    return with_riders(h, [&](auto k) { rc = decltype(k)::flip(h, a, kt16); }) ? rc : no_riders(h);
}
double rnnwf::prnn_split_stream_flops_per_step(rnnwf_handle* h) {
    double f = 0;
    with_riders(h, [&](auto k) { f = decltype(k)::flip_flops_per_step(); });
    return f;
}
int rnnwf::prnn_split_stream_pack(rnnwf_handle* h, std::vector<char>& simg) {
    int rc = 0;
    return with_riders(h, [&](auto k) { rc = decltype(k)::flip_pack(h, simg); }) ? rc : no_riders(h);
}

// ---- swap pass of the complex RNN -----------------------------------------------------------------------------------
int rnnwf::crnn_split_swap_stream(rnnwf_handle* h, const CrnnArgs& a, int64_t max_tiles, int kt16) {
    int rc = 0;
    return with_riders(h, [&](auto k) { rc = decltype(k)::swap(h, a, max_tiles, kt16); }) ? rc : no_riders(h);
}
double rnnwf::crnn_split_stream_flops_per_step(rnnwf_handle* h) {
    double f = 0;
    with_riders(h, [&](auto k) { f = decltype(k)::swap_flops_per_step(); });
    return f;
}
int rnnwf::crnn_split_stream_pack(rnnwf_handle* h, std::vector<char>& simg) {
    return with_riders(h, [&](auto k) { simg = decltype(k)::swap_pack(h); }) ? 0 : no_riders(h);
}
