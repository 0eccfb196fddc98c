// lstm.hip - host side of the LSTM wave function over the raster path (model LSTM1D_F64, one layer, 1..68 units, float64):
// weight image, base pass, fused 2D TFIM local energies (driven through lstm_family by rnnwf_api.hip).  The kernels are lstm_kernels.h;
// everything downstream of them (bit packing, local-energy assembly, moments) is shared with the GRU models.
#include <algorithm>
#include <cstdlib>

#include "lstm_kernels.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

const char* kLstmPre = "multi_rnn_cell/cell_0/lstm_cell/";

// Packs LSTMCell + Dense(2) into LstmLayout<NFULL>.  TF's kernel is [2 + H, 4H]: rows 0..1 the one-hot input, rows 2.. the
// hidden state; columns i | j | f | o in blocks of H.  S = double: the image; S = Lin: its table for device-resident training
// (pack_value.h), every element with the operations the double run performs, in their order
template <int NFULL, class S = double>
std::vector<char> pack_lstm_image(const rnnwf_handle* h) {
    using L = LstmLayout<NFULL>;
    using Out = PackSink<S>;
    const int H = h->H;
    std::vector<char> img(L::BYTES, 0);
    Out::begin(img);
    const auto K = pvs<S>(h, std::string(kLstmPre) + "kernel");
    const auto b = pvs<S>(h, std::string(kLstmPre) + "bias");
    const size_t W = (size_t)4 * H;
    auto decode = [&](int tile, int q, int r, int& gate, int& unit) -> bool {
        if (tile < 4 * NFULL) {
            gate = tile / NFULL;
            unit = 16 * (tile % NFULL) + 4 * r + q;
        } else {
            gate = r;
            unit = 16 * NFULL + q;
        }
        return unit < H;
    };
    auto wt = [&](int gate, int unit, int k) -> S {           // W^T[row(gate, unit)][k] over the hidden rows of K
        return k < H ? K[(size_t)(2 + k) * W + (size_t)gate * H + unit] : S(0.0);
    };
    double* avec = reinterpret_cast<double*>(img.data() + L::OFF_AVEC);
    double* arem = reinterpret_cast<double*>(img.data() + L::OFF_AREM);
    for (int tile = 0; tile < L::NT; ++tile)
        for (int row = 0; row < 16; ++row) {
            int q, r, gate, unit;
            row_to_qr<double>(row, q, r);
            if (!decode(tile, q, r, gate, unit)) continue;
            for (int kq = 0; kq < 4; ++kq) {       // lane quarter of the A operand = k mod 4
                const int lane = (kq << 4) | row;
                for (int g = 0; g < L::NG; ++g)
                    for (int j = 0; j < L::VW; ++j)
                        Out::put(&avec[(((size_t)tile * L::NG + g) * 64 + lane) * L::VW + j], wt(gate, unit, 4 * (g * L::VW + j) + kq));
                Out::put(&arem[(size_t)tile * 64 + lane], wt(gate, unit, 4 * (L::KT - 1) + kq));
            }
        }
    for (int v = 0; v < 3; ++v) {  // v = 0: zero input; v = 1, 2: one-hot of spin 0, 1
        double* binit = reinterpret_cast<double*>(img.data() + L::OFF_BINIT + v * L::SZ_BINIT_VARIANT);
        for (int tile = 0; tile < L::NT; ++tile)
            for (int q = 0; q < 4; ++q)
                for (int r = 0; r < 4; ++r) {
                    int gate, unit;
                    if (!decode(tile, q, r, gate, unit)) continue;
                    const size_t col = (size_t)gate * H + unit;
                    // v = 0 adds the zero input's 0.0 (a bias of -0.0 becomes +0.0): recorded as such, not skipped
                    S x = v ? b[col] + K[(size_t)(v - 1) * W + col] : add_const(b[col], 0.0);
                    if (gate == 2) x = add_const(x, 1.0);   // forget_bias = 1.0, folded into the f rows (lstm_core.h)
                    Out::put(&binit[tile * 16 + q * 4 + r], x);
                }
    }
    double* wd = reinterpret_cast<double*>(img.data() + L::OFF_WD);
    double* bd = reinterpret_cast<double*>(img.data() + L::OFF_BD);
    const auto Wd = pvs<S>(h, "wf_dense/kernel");   // [H, 2]
    const auto bdv = pvs<S>(h, "wf_dense/bias");    // [2]
    for (int kt = 0; kt < L::KT; ++kt)
        for (int q = 0; q < 4; ++q) {
            const int unit = 4 * kt + q;
            if (unit < H) Out::put(&wd[q * L::WD_Q + kt], Wd[(size_t)unit * 2 + 1] - Wd[(size_t)unit * 2]);
        }
    Out::put(&bd[0], bdv[1] - bdv[0]);
    return img;
}

// WAVES: waves per workgroup of the flip pass (shapes.h); BWAVES: of the base pass - at 68 units one wave per SIMD: with its
// checkpoint stores and sampler beside h, c and h' it needs more than the 256 registers of two waves per SIMD (scratch otherwise); it
// is the short pass (N steps per chain against the flip pass's N (N - 1) / 2).  The image takes most of a CU's LDS (one workgroup per
// CU from 37 units up): both passes shrink their workgroups for small batches (handle.h: launch_shrinking; the run script's 4x4 /
// 500 samples would sit on 60 of 256 CUs in full-size workgroups)
template <int NFULL, int WAVES>
struct LLaunch {
    using L = LstmLayout<NFULL>;
    static constexpr int BWAVES = NFULL == 4 ? 4 : WAVES;
    static int base(rnnwf_handle* h, const LstmArgs& a) {
        return launch_shrinking<BWAVES>(h, kTimerBase, lstm_base_kernel<NFULL, BWAVES>, L::BYTES, a.nsb, a);
    }
    static int flip(rnnwf_handle* h, const LstmArgs& a) {
        return launch_shrinking<WAVES>(h, kTimerFlip, lstm_flip_kernel<NFULL, WAVES>, L::BYTES, a.ntiles, a);
    }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_lstm_image<NFULL>(h); }
    static void pack_table(const rnnwf_handle* h) { pack_lstm_image<NFULL, Lin>(h); }
    static size_t hck_bytes_per_block() { return (size_t)2 * L::KT * 64 * sizeof(double); }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// fn(K()) for this handle's launch class K, false (fn not called) for a width without kernels
template <class Fn>
bool with_launch(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<LLaunch>(LstmKernels(), h, fn); }

int no_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no LSTM kernel for NFULL=%d (one layer, <= 68 units)", h->NFULL); }
int launch_base(rnnwf_handle* h, const LstmArgs& a) {
    int rc = 0;
    return with_launch(h, [&](auto k) { rc = decltype(k)::base(h, a); }) ? rc : no_kernel(h);
}
int launch_flip(rnnwf_handle* h, const LstmArgs& a) {
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

LstmArgs base_args(rnnwf_handle* h, int64_t ns) {
    LstmArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    return a;
}

int64_t max_chains_per_pass(rnnwf_handle* h) {
    const size_t per_block = (size_t)std::max(h->N - 1, 1) * hck_bytes_per_block(h);
    const int64_t blocks = std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kDefaultStateBudget) / per_block));
    return blocks * kChains;
}

// Fused local energies of ns chains whose packed spins are in h->bits (drawn into it when `d`): base pass with checkpoints
// -> flip pass -> assembly.  Leaves E_loc in h->eloc and the log-prob queue in h->lpq.
int eloc_on_device(rnnwf_handle* h, int64_t ns, const Draw* d, const double* couplings) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    const double Bx = couplings[N];
    if (int rc = ensure(h, h->lpq, (size_t)(N + 1) * ns * 8)) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * hck_bytes_per_block(h))) return rc;
    LstmArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.hck = (double*)h->hck.p;
    a.lpq = (double*)h->lpq.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    if (int rc = launch_base(h, a)) return rc;
    if (Bx != 0.0 && N > 1) {
        a.ntiles = (int64_t)(N - 1) * nsb;
        a.sampling = 0;
        if (int rc = launch_flip(h, a)) return rc;
        h->work[0] += (double)ns * N * (N - 1) / 2.0;
        h->work[1] += (double)nsb * N * (N - 1) / 2.0 * mfma_flops_per_step(h);
    }
    return run_tfim_eloc(h, (const uint32_t*)h->bits.p, (const double*)h->lpq.p, ns, h->Nx, h->Ny, nullptr, (const double*)h->coupl.p,
                         Bx, (double*)h->eloc.p);
}

// base pass alone: log P of every chain -> h->out_lp (the spins drawn into h->bits when `d`)
int log_prob_pass(rnnwf_handle* h, int64_t ns, const Draw* d) {
    if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
    LstmArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.out_lp = (double*)h->out_lp.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    return launch_base(h, a);
}

int pack_image(rnnwf_handle* h, std::vector<char>& img) {
    return with_launch(h, [&](auto k) { img = decltype(k)::pack(h); }) ? 0 : no_kernel(h);
}

}  // namespace

// the table of h->wimg over Lin into the active PackTrace (train.hip: the LSTM's builder; lstm_family()'s pack_table stays nullptr, so
// the entries that ask the family keep refusing an LSTM handle)
int rnnwf::lstm_pack_table(rnnwf_handle* h) {
    return with_launch(h, [&](auto k) { decltype(k)::pack_table(h); }) ? 0 : no_kernel(h);
}

// base pass with checkpoints on the spins packed into h->bits, nothing else: the states the gradient's backward pass starts from
int rnnwf::lstm_teacher_base(rnnwf_handle* h, int64_t ns) {
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->hck, (size_t)std::max(h->N - 1, 1) * nsb * hck_bytes_per_block(h))) return rc;
    LstmArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.hck = (double*)h->hck.p;
    return launch_base(h, a);
}

const Family* rnnwf::lstm_family() {
    static const Family f = {
        "LSTM cell", pack_image, nullptr, log_prob_pass, nullptr, eloc_on_device, max_chains_per_pass, nullptr, nullptr,
        1, 1,                 // Jz per site; Bx
        false, false, nullptr,  // float64 E_loc; the base pass alone keeps no states; no gradient (nothing stays resident)
    };
    return &f;
}
