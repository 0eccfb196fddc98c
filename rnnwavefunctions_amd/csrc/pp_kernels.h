// pp_kernels.h - what the four ping-pong kernels of the bf16x3 engine share (split_kernels.h: prnn_flip_pp_kernel,
// prnn_flip_pp_upper_kernel; crnn_split_kernels.h: crnn_swap_pp_kernel, crnn_swap_pp_upper_kernel).  All of them run 8 waves per
// workgroup, two per SIMD, in lock step: [MFMA segment] barrier [VALU segment] barrier, waves 4-7 one segment behind waves 0-3.
//
//   StackArgs, flip_record_start, store_record : the layer pipeline's records (split_core.h: SplitUpperLayout)
//   PPWalk                                     : the snake walk over the length-sorted tiles and the workgroup's lock-step count
//   checkpoint_src, checkpoint_entry           : where a chain's checkpointed state lies (the base pass's layout)
//   PPSlot                                     : a wave's LDS staging slot - checkpoints and records arrive by LDS-DMA
//   PPStamps, pp_begin / pp_barrier / pp_end   : the lock-step frame (every barrier of the scheme) and its cycle stamps
//
// What stays with each kernel: how a tile is named and entered, what the VALU segment adds up, where the result goes.  The kernels
// sit at 252 of 256 VGPRs: the helpers take the kernel's arrays by reference and keep nothing of their own around the loop.
#pragma once
#include "split_core.h"

namespace rnnwf {

#define RNNWF_RECORD_AUX 2      // cache policy of the record loads (LDS-DMA aux): nt - the record stream is read once

// Stacked layers (layer pipeline, split_core.h: SplitUpperLayout): what a layer's kernel needs besides its model's arguments.
struct StackArgs {
    const float* xin;     // records of the layer below: [wave-step][NU][64] f32, nullptr for the first layer
    float* xout;          // this layer's records for the layer above, nullptr for the top layer
    int32_t kstride;      // checkpoint rows (of 64 floats) per 16-chain block and site: layers x kt16
    int32_t koff;         // first row of this layer's state in a block
};
// record index of the first step of flip tile (i, sb): tiles in (i, sb) order, N - 1 - i steps each
__device__ __forceinline__ int64_t flip_record_start(int N, int64_t nsb32, int i, int64_t sb) {
    const int64_t before = (int64_t)i * (N - 1) - (int64_t)i * (i - 1) / 2;        // sum over i' < i of (N - 1 - i')
    return nsb32 * before + sb * (N - 1 - i);
}

// record `rec` <- this lane's NU state values: [NG][64 lanes][4] f32 (one dwordx4 store per group), then [NU % 4][64 lanes] f32
template <int NU>
__device__ __forceinline__ void store_record(float* xout, int64_t rec, const float (&h)[NU], int lane) {
    constexpr int NG = NU / 4;
    float* base = xout + rec * (int64_t)(NU * 64);
    float4* dst = reinterpret_cast<float4*>(base) + lane;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        // non-temporal: a record is written once and read once, by the next kernel, gigabytes later (measured against plain stores
        // and loads on one box, alternating: 7.31 / 7.33 vs 7.42 / 7.39 ms at two layers, 12.39 / 12.48 vs 12.60 / 12.60 ms at three;
        // profiles/r04_d_ab_nt.txt)
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 v = {h[4 * g], h[4 * g + 1], h[4 * g + 2], h[4 * g + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<f4*>(dst + g * 64));
    }
#pragma unroll
    for (int e = 4 * NG; e < NU; ++e) base[NG * 256 + (e - 4 * NG) * 64 + lane] = h[e];
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// Tiles are sorted by chain length (longest first); round r of the walk hands wave gw the tile r nw + gw in even rounds and
// r nw + (nw - 1 - gw) in odd ones, so every wave gets the same total length within a step or two.
struct PPWalk {
    static constexpr int WAVES = 8;
    const int64_t gw, nw, ntiles;
    __device__ __forceinline__ PPWalk(int wave, int64_t ntiles_)
        : gw((int64_t)blockIdx.x * WAVES + wave), nw((int64_t)gridDim.x * WAVES), ntiles(ntiles_) {}
    __device__ __forceinline__ int64_t tile_of(int64_t r) const { return r * nw + ((r & 1) ? nw - 1 - gw : gw); }
    // this wave's next tile after round r (a round may hold none for it): false when the walk is over
    __device__ __forceinline__ bool next(int64_t r, int64_t& r_out, int64_t& t_out) const {
        for (;;) {
            ++r;
            if (r * nw >= ntiles) return false;
            const int64_t t = tile_of(r);
            if (t < ntiles) { r_out = r; t_out = t; return true; }
        }
    }
    // All waves execute the same number of barriers: the workgroup iterates to the largest per-wave step count.  `counter` is a
    // shared int zeroed before the kernel's staging barrier; steps_of_tile(t) = the chain length of tile t.
    template <class Steps>
    __device__ __forceinline__ int lockstep_iters(int* counter, Steps&& steps_of_tile) const {
        int mine = 0;
        for (int64_t r = 0; r * nw < ntiles; ++r) {
            const int64_t t = tile_of(r);
            if (t < ntiles) mine += steps_of_tile(t);
        }
        if ((threadIdx.x & 63) == 0) atomicMax(counter, mine);
        __syncthreads();
        return *counter;
    }
};

// first-changed site of swap tile t: the last lo with tile_start[lo] <= t (tile_start[0..N], ascending)
__device__ __forceinline__ int lo_of(const int32_t* tile_start, int N, int64_t t) {
    int l = 0, r = N;
    while (r - l > 1) {
        const int mid = (l + r) >> 1;
        if (tile_start[mid] <= t) l = mid; else r = mid;
    }
    return l;
}

// ---- checkpoint addressing --------------------------------------------------------------------------------------------------
// Unit u of a chain sits at float off(u) of the chain's 16-chain block ([kt][lane (q << 4) | chain], unit 4 kt + q).
__device__ __forceinline__ constexpr int checkpoint_off(int u) { return (u >> 2) * 64 + ((u & 3) << 4); }
// the state of `chain` after `site`: a block holds kstride rows of 64 floats per site, this layer's from row koff on
__device__ __forceinline__ const float* checkpoint_src(const float* hck, int64_t site, int64_t nsb, int chain, int kstride, int koff) {
    return hck + ((site * nsb + (chain >> 4)) * kstride + koff) * 64 + (chain & 15);
}
// entry e of this lane's state (layout L): the upper lane half owns units shifted by a constant per group (full tiles +4, remainder
// +(RJ-1), special +1): per-lane base pointers and immediate offsets, instead of one 64-bit address per load (HP <= 4 kt16: host-checked)
template <class L>
__device__ __forceinline__ const float* checkpoint_entry(const float* src, int hh, int e) {
    const int u0 = L::unit_of(e, 0), u1 = L::unit_of(e, 1);
    const int d = checkpoint_off(u1) - checkpoint_off(u0);     // compile-time constant per entry
    return src + (hh ? d : 0) + checkpoint_off(u0);
}

// ---- the staging slot -------------------------------------------------------------------------------------------------------
// NU x 256 bytes of LDS per wave behind the weight image (IMAGE_BYTES): a checkpoint lands as entry e of every lane at
// slot + 256 e + 4 lane, a record as lane l's 16 bytes of group g at slot + g KB + 16 l, then the NU % 4 tail entries.  Both travel
// global memory -> LDS by LDS-DMA (no register destination).
template <class L, int NU, size_t IMAGE_BYTES>
struct PPSlot {
    static constexpr int NG = NU / 4, NTAIL = NU % 4;
    typedef __attribute__((address_space(3))) void* LdsVoid;
    typedef const __attribute__((address_space(1))) void* GlobVoid;
    char* const slot;
    const int lane;
    __device__ __forceinline__ PPSlot(char* lds, int wave, int lane_)
        : slot(lds + ((IMAGE_BYTES + 15) / 16) * 16 + (size_t)wave * NU * 256), lane(lane_) {}

    __device__ __forceinline__ void dma_checkpoint(const float* src) const {
        const int hh = lane >> 5;
#pragma unroll
        for (int e = 0; e < NU; ++e) __builtin_amdgcn_global_load_lds((GlobVoid)checkpoint_entry<L>(src, hh, e), (LdsVoid)(slot + e * 256), 4, 0, 0);
    }
    __device__ __forceinline__ void read_checkpoint(float (&x)[NU]) const {
        const float* p = reinterpret_cast<const float*>(slot) + lane;
#pragma unroll
        for (int e = 0; e < NU; ++e) x[e] = p[e * 64];
    }
    __device__ __forceinline__ void dma_record(const float* xin, int64_t r) const {
        const float* base = xin + r * (int64_t)(NU * 64);
#pragma unroll
        for (int g = 0; g < NG; ++g) __builtin_amdgcn_global_load_lds((GlobVoid)(base + g * 256 + lane * 4), (LdsVoid)(slot + g * 1024), 16, 0, RNNWF_RECORD_AUX);
#pragma unroll
        for (int t = 0; t < NTAIL; ++t)
            __builtin_amdgcn_global_load_lds((GlobVoid)(base + NG * 256 + t * 64 + lane), (LdsVoid)(slot + NG * 1024 + t * 256), 4, 0, 0);
    }
    __device__ __forceinline__ void read_record(float (&x)[NU]) const {
        const float4* p = reinterpret_cast<const float4*>(slot) + lane;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float4 v = p[g * 64];
            x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
        }
#pragma unroll
        for (int t = 0; t < NTAIL; ++t) x[4 * NG + t] = reinterpret_cast<const float*>(slot + NG * 1024)[t * 64 + lane];
    }
    static __device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt(0x0F70); asm volatile("" ::: "memory"); }      // vmcnt(0)
    static __device__ __forceinline__ void wait_lds() { __builtin_amdgcn_s_waitcnt(0xC07F); asm volatile("" ::: "memory"); }     // lgkmcnt(0)
    // BH <- the quads of h, then BX <- the quads of the record in flight (h is overwritten with it).  Behind the record's transfer only
    // this segment's NG + NTAIL record stores may still be on their way; a fresh tile's record was requested a moment ago: wait for all
    template <class PU, bool LAST, int NB>
    __device__ __forceinline__ void load_quads(bool fresh, float (&h)[NU], u32x4 (&BH)[NB], u32x4 (&BX)[NB]) const {
        PU::split(h, BH);
        if (LAST || fresh) __builtin_amdgcn_s_waitcnt(0x0F70);
        else __builtin_amdgcn_s_waitcnt(0x0F70 | (NG + NTAIL));
        asm volatile("" ::: "memory");
        read_record(h);
        PU::split(h, BX);
        wait_lds();                                            // the slot has been read before the next request overwrites it
    }
};

// ---- the frame --------------------------------------------------------------------------------------------------------------
// In-kernel cycle stamps (diagnostics builds, tools/stamps.py): where a wave-step's cycles go, and the clock held.  mark(k) adds
// the cycles since the previous mark to counter k; write() leaves 10 words per wave at out + 16 gw:
//   mfma, b1, valu, b2, switch, total cycles, realtime ticks (100 MHz), iterations, gates, head
enum PPStamp : int { kStampMfma = 0, kStampB1, kStampValu, kStampB2, kStampSwitch, kStampGates, kStampHead, kStampCount };
struct PPNoStamps {                                           // release builds, and the kernels that keep no stamps
    __device__ __forceinline__ explicit PPNoStamps(unsigned long long* = nullptr) {}
    __device__ __forceinline__ void mark(PPStamp) {}
    __device__ __forceinline__ void write(int64_t, int, int) const {}
};
#ifdef RNNWF_DIAGNOSTICS
struct PPStamps {
    unsigned long long* const out;
    unsigned long long t[kStampCount] = {}, ts, t_begin, r_begin;
    __device__ __forceinline__ explicit PPStamps(unsigned long long* out_)
        : out(out_), t_begin(__builtin_amdgcn_s_memtime()), r_begin(__builtin_amdgcn_s_memrealtime()) { ts = t_begin; }
    __device__ __forceinline__ void mark(PPStamp k) {
        if (out) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); t[k] += t_ - ts; ts = t_; }
    }
    __device__ __forceinline__ void write(int64_t gw, int lane, int iters) const {
        if (out && lane == 0) {
            unsigned long long* o = out + gw * 16;
            o[0] = t[kStampMfma]; o[1] = t[kStampB1]; o[2] = t[kStampValu]; o[3] = t[kStampB2]; o[4] = t[kStampSwitch];
            o[5] = __builtin_amdgcn_s_memtime() - t_begin; o[6] = __builtin_amdgcn_s_memrealtime() - r_begin; o[7] = (unsigned long long)iters;
            o[8] = t[kStampGates]; o[9] = t[kStampHead];
        }
    }
};
#else
using PPStamps = PPNoStamps;
#endif

// The lock step: every iteration of a kernel's loop is  [MFMA segment] pp_barrier [VALU segment] pp_barrier  between pp_begin and
// pp_end; the late half (waves 4-7) runs one barrier behind the early one, so that on every SIMD one wave multiplies while the other
// does vector work.  An idle wave executes the barriers only.  Every barrier of the scheme is here; the segments stay in the kernel's
// own scope (inside closures the allocator lays the kernels' 252 registers out differently).
template <class Stamps>
__device__ __forceinline__ void pp_begin(bool late, Stamps& stamps) {
    if (late) { __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }
    stamps.mark(kStampB2);
}
// the segment before it ends here (its cycles go to stamp `seg`), the wait for the workgroup to stamp `wait`
template <class Stamps>
__device__ __forceinline__ void pp_barrier(Stamps& stamps, PPStamp seg, PPStamp wait) {
    __builtin_amdgcn_sched_barrier(0);
    stamps.mark(seg);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    stamps.mark(wait);
}
__device__ __forceinline__ void pp_end(bool late) {
    if (!late) __builtin_amdgcn_s_barrier();
}

}  // namespace rnnwf
