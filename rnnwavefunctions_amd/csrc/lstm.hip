// lstm.hip - host side of the LSTM wave function over the raster path (model LSTM1D_F64, one layer, 1..68 units, float64):
// weight image, base pass, fused 2D TFIM local energies (driven through lstm_family by rnnwf_api.hip).  The kernels are lstm_kernels.h;
// everything downstream of them (bit packing, local-energy assembly, moments) is shared with the GRU models.
#include <algorithm>
#include <cstdlib>

#include "lstm_kernels.h"
#include "models.h"
#include "pack.h"

using namespace rnnwf;

namespace {

constexpr size_t kHckBudget = (size_t)48 << 30;  // bytes of (h, c) checkpoints per pass (prnn.hip's budget)
const char* kLstmPre = "multi_rnn_cell/cell_0/lstm_cell/";

// Packs LSTMCell + Dense(2) into LstmLayout<NFULL>.  TF's kernel is [2 + H, 4H]: rows 0..1 the one-hot input, rows 2.. the
// hidden state; columns i | j | f | o in blocks of H.
template <int NFULL>
std::vector<char> pack_lstm_image(const rnnwf_handle* h) {
    using L = LstmLayout<NFULL>;
    const int H = h->H;
    std::vector<char> img(L::BYTES, 0);
    const std::vector<double>& K = pv(h, std::string(kLstmPre) + "kernel");
    const std::vector<double>& b = pv(h, std::string(kLstmPre) + "bias");
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
    auto wt = [&](int gate, int unit, int k) -> double {      // W^T[row(gate, unit)][k] over the hidden rows of K
        return k < H ? K[(size_t)(2 + k) * W + (size_t)gate * H + unit] : 0.0;
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
                        avec[(((size_t)tile * L::NG + g) * 64 + lane) * L::VW + j] = wt(gate, unit, 4 * (g * L::VW + j) + kq);
                arem[(size_t)tile * 64 + lane] = wt(gate, unit, 4 * (L::KT - 1) + kq);
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
                    double x = b[col] + (v ? K[(size_t)(v - 1) * W + col] : 0.0);
                    if (gate == 2) x += 1.0;         // forget_bias = 1.0, folded into the f rows (lstm_core.h)
                    binit[tile * 16 + q * 4 + r] = x;
                }
    }
    double* wd = reinterpret_cast<double*>(img.data() + L::OFF_WD);
    double* bd = reinterpret_cast<double*>(img.data() + L::OFF_BD);
    const std::vector<double>& Wd = pv(h, "wf_dense/kernel");   // [H, 2]
    const std::vector<double>& bdv = pv(h, "wf_dense/bias");    // [2]
    for (int kt = 0; kt < L::KT; ++kt)
        for (int q = 0; q < 4; ++q) {
            const int unit = 4 * kt + q;
            if (unit < H) wd[q * L::WD_Q + kt] = Wd[(size_t)unit * 2 + 1] - Wd[(size_t)unit * 2];
        }
    bd[0] = bdv[1] - bdv[0];
    return img;
}

// WAVES: waves per workgroup of the flip pass; BWAVES: of the base pass
template <int NFULL, int WAVES, int BWAVES = WAVES>
struct LLaunch {
    using L = LstmLayout<NFULL>;
    // items (16-chain blocks or flip tiles) one per wave: NW waves per workgroup where there are enough of them to fill every
    // resident workgroup slot, fewer otherwise - the image takes most of a CU's LDS (one workgroup per CU from 37 units up), so
    // a small batch in full-size workgroups would sit on a few CUs, two waves per SIMD (the run script's 4x4 / 500 samples:
    // 60 of 256 CUs)
    template <int NW, class Kern>
    static int run(rnnwf_handle* h, Kern kern, int64_t items, int id, const LstmArgs& a) {
        int bpc = 0;
        if (int rc = blocks_per_cu(h, (const void*)kern, NW * 64, L::BYTES, &bpc)) return rc;
        const int64_t slots = (int64_t)bpc * h->cu_count;
        const int wpb = (int)std::max<int64_t>(1, std::min<int64_t>(NW, (items + slots - 1) / slots));
        const int64_t need = (items + wpb - 1) / wpb;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(need, slots));
        TimedLaunch tl(h, id);
        kern<<<grid, wpb * 64, L::BYTES, h->stream>>>(a);
        RNNWF_HIP(h, hipGetLastError());
        return 0;
    }
    static int base(rnnwf_handle* h, const LstmArgs& a) { return run<BWAVES>(h, lstm_base_kernel<NFULL, BWAVES>, a.nsb, 0, a); }
    static int flip(rnnwf_handle* h, const LstmArgs& a) { return run<WAVES>(h, lstm_flip_kernel<NFULL, WAVES>, a.ntiles, 1, a); }
    static std::vector<char> pack(const rnnwf_handle* h) { return pack_lstm_image<NFULL>(h); }
    static size_t hck_bytes_per_block() { return (size_t)2 * L::KT * 64 * sizeof(double); }
    static double mfma_flops_per_step() { return (double)L::NT * L::KT * 2048.0; }
};

// NFULL 1..4 (<= 20, 36, 52, 68 units); 8 waves where one workgroup fills a CU's LDS (two per SIMD).  The base pass at 68 units
// runs one wave per SIMD: with its checkpoint stores and sampler beside h, c and h' it needs more than the 256 registers of two
// waves per SIMD (scratch otherwise); it is the short pass (N steps per chain against the flip pass's N (N - 1) / 2).
#define LSTM_DISPATCH(h, EXPR)                                                 \
    do {                                                                       \
        switch ((h)->NFULL) {                                                  \
            case 1: { using K = LLaunch<1, 4>; EXPR; }                         \
            case 2: { using K = LLaunch<2, 4>; EXPR; }                         \
            case 3: { using K = LLaunch<3, 8>; EXPR; }                         \
            case 4: { using K = LLaunch<4, 8, 4>; EXPR; }                      \
        }                                                                      \
    } while (0)

int no_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "no LSTM kernel for NFULL=%d (one layer, <= 68 units)", h->NFULL); }
int launch_base(rnnwf_handle* h, const LstmArgs& a) { LSTM_DISPATCH(h, return K::base(h, a)); return no_kernel(h); }
int launch_flip(rnnwf_handle* h, const LstmArgs& a) { LSTM_DISPATCH(h, return K::flip(h, a)); return no_kernel(h); }
size_t hck_bytes_per_block(rnnwf_handle* h) { LSTM_DISPATCH(h, return K::hck_bytes_per_block()); return 0; }
double mfma_flops_per_step(rnnwf_handle* h) { LSTM_DISPATCH(h, return K::mfma_flops_per_step()); return 0; }

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
    const int64_t blocks = std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kHckBudget) / per_block));
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
    LSTM_DISPATCH(h, { img = K::pack(h); return 0; });
    return no_kernel(h);
}

}  // namespace

const Family* rnnwf::lstm_family() {
    static const Family f = {
        "LSTM cell", pack_image, log_prob_pass, nullptr, eloc_on_device, max_chains_per_pass, nullptr, nullptr,
        1, 1,                 // Jz per site; Bx
        false, false, nullptr,  // float64 E_loc; the base pass alone keeps no states; no gradient (nothing stays resident)
    };
    return &f;
}
