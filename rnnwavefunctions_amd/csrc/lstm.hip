// lstm.hip - host side of the LSTM wave function over the raster path (model LSTM1D_F64, one layer, 1..68 units, float64):
// weight image, sample / log_probability / fused 2D TFIM local energies / fused VMC step.  The kernels are lstm_kernels.h;
// everything downstream of them (bit packing, local-energy assembly, moments) is shared with the GRU models.
#include <algorithm>
#include <cstdlib>

#include "lstm_kernels.h"
#include "models.h"
#include "pack.h"

using namespace rnnwf;

namespace {

constexpr size_t kHckBudget = (size_t)48 << 30;  // bytes of (h, c) checkpoints per pass (prnn.hip's budget)
constexpr int64_t kLogProbChunk = (int64_t)1 << 20;
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

// Fused local energies of ns chains whose packed spins are in h->bits (or are drawn into it): base pass with checkpoints
// -> flip pass -> assembly.  Leaves E_loc in h->eloc and the log-prob queue in h->lpq.
int eloc_on_device(rnnwf_handle* h, int64_t ns, bool sampling, uint64_t seed, uint64_t step, int64_t offset, const double* Jz_dev,
                   double Bx) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->lpq, (size_t)(N + 1) * ns * 8)) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    if (int rc = ensure(h, h->hck, (size_t)std::max(N - 1, 1) * nsb * hck_bytes_per_block(h))) return rc;
    LstmArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.hck = (double*)h->hck.p;
    a.lpq = (double*)h->lpq.p;
    a.sampling = sampling ? 1 : 0;
    a.seed = seed; a.step = step; a.sample_offset = offset;
    if (int rc = launch_base(h, a)) return rc;
    if (Bx != 0.0 && N > 1) {
        a.ntiles = (int64_t)(N - 1) * nsb;
        a.sampling = 0;
        if (int rc = launch_flip(h, a)) return rc;
        h->work[0] += (double)ns * N * (N - 1) / 2.0;
        h->work[1] += (double)nsb * N * (N - 1) / 2.0 * mfma_flops_per_step(h);
    }
    return run_tfim_eloc(h, (const uint32_t*)h->bits.p, (const double*)h->lpq.p, ns, h->Nx, h->Ny, nullptr, Jz_dev, Bx,
                         (double*)h->eloc.p);
}

}  // namespace

int rnnwf::lstm_pack_image(rnnwf_handle* h, std::vector<char>& img) {
    LSTM_DISPATCH(h, { img = K::pack(h); return 0; });
    return no_kernel(h);
}

int rnnwf::lstm_log_prob(rnnwf_handle* h, const int32_t* samples, int64_t B, double* out) {
    const int N = h->N;
    h->last_ns = 0;
    for (int64_t off = 0; off < B; off += kLogProbChunk) {
        const int64_t nb = std::min(kLogProbChunk, B - off);
        if (int rc = upload_and_pack(h, samples + off * N, nb, h->bits, 0, nullptr)) return rc;
        if (int rc = ensure(h, h->out_lp, (size_t)nb * 8)) return rc;
        LstmArgs a = base_args(h, nb);
        a.bits = (uint32_t*)h->bits.p;
        a.out_lp = (double*)h->out_lp.p;
        if (int rc = launch_base(h, a)) return rc;
        RNNWF_HIP(h, hipMemcpyAsync(out + off, h->out_lp.p, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    return RNNWF_OK;
}

int rnnwf::lstm_sample(rnnwf_handle* h, int64_t ns, uint64_t seed, uint64_t step, int64_t offset, int32_t* out, double* out_log) {
    const int W = (h->N + 31) / 32;
    h->last_ns = 0;
    if (int rc = ensure(h, h->bits, (size_t)W * ns * 4)) return rc;
    if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
    LstmArgs a = base_args(h, ns);
    a.bits = (uint32_t*)h->bits.p;
    a.out_lp = (double*)h->out_lp.p;
    a.sampling = 1;
    a.seed = seed; a.step = step; a.sample_offset = offset;
    if (int rc = launch_base(h, a)) return rc;
    if (int rc = unpack_and_download(h, h->bits, ns, out, nullptr)) return rc;
    if (out_log) RNNWF_HIP(h, hipMemcpyAsync(out_log, h->out_lp.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    return RNNWF_OK;
}

int rnnwf::lstm_tfim_eloc(rnnwf_handle* h, const int32_t* samples, int64_t ns, const double* Jz, double Bx, double* eloc,
                          double* log_probs) {
    const int N = h->N;
    h->last_ns = 0;
    if (int rc = upload_couplings(h, Jz, (size_t)N)) return rc;
    const int64_t chunk = max_chains_per_pass(h);
    for (int64_t off = 0; off < ns; off += chunk) {
        const int64_t nb = std::min(chunk, ns - off);
        if (int rc = upload_and_pack(h, samples + off * N, nb, h->bits, 0, nullptr)) return rc;
        if (int rc = eloc_on_device(h, nb, false, 0, 0, 0, (const double*)h->coupl.p, Bx)) return rc;
        RNNWF_HIP(h, hipMemcpyAsync(eloc + off, h->eloc.p, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
        if (log_probs)
            RNNWF_HIP(h, hipMemcpy2DAsync(log_probs + off, (size_t)ns * 8, h->lpq.p, (size_t)nb * 8, (size_t)nb * 8,
                                          (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    return RNNWF_OK;
}

int rnnwf::lstm_vmc_step(rnnwf_handle* h, int64_t ns, uint64_t seed, uint64_t step, int64_t offset, const double* couplings,
                         int32_t* out_samples, double* out_eloc, double* moments) {
    const int N = h->N;
    const int W = (N + 31) / 32;
    h->last_ns = 0;
    if (ns > max_chains_per_pass(h))
        return h->fail(RNNWF_ERR_NOMEM, "rnnwf_vmc_step: %lld samples exceed the checkpoint budget; split the batch", (long long)ns);
    if (int rc = ensure(h, h->bits, (size_t)W * ns * 4)) return rc;
    if (int rc = upload_couplings(h, couplings, (size_t)N)) return rc;
    if (int rc = eloc_on_device(h, ns, true, seed, step, offset, (const double*)h->coupl.p, couplings[N])) return rc;
    if (out_samples) if (int rc = unpack_and_download(h, h->bits, ns, out_samples, nullptr)) return rc;
    if (out_eloc) RNNWF_HIP(h, hipMemcpyAsync(out_eloc, h->eloc.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream));
    return run_moments(h, h->eloc.p, ns, false, moments);
}
