// lstm_grad.hip - host side of the LSTM wave function's gradient (docs/lstm.md, "Gradient"): the backward operand, the one driver
// behind rnnwf_lstm_gradient and rnnwf_lstm_vmc_gradient_step (backward pass -> P^T Q -> download -> TF-named tensors), and the two
// entries.  The kernel is lstm_grad_kernels.h; backward_launch, tn_gemm_launch and the head rows' reduction are the GRU's (tn_gemm.h).
// The existing gradient entries keep refusing an LSTM handle (lstm_family()'s `gradient` stays nullptr): these entries carry their
// own hooks, as rnnwf_pauli_step_stack does for stacks.
#include <algorithm>
#include <cmath>

#include "lstm_grad_kernels.h"
#include "tn_gemm.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

const char* kLstmPre = "multi_rnn_cell/cell_0/lstm_cell/";

// Every backward kernel runs four waves per workgroup (one per SIMD), whatever the forward kernels of its row run: from 37 units
// the wave's state (h_in, dh, dc, the head sums and two MFMA chains' operands) takes more than the 256 registers of two waves per SIMD
constexpr int kLstmGradWaves = 4;

template <int NFULL, int>
struct LGrad {
    using L = LstmLayout<NFULL>;
    using G = LstmGradLayout<NFULL>;
    static constexpr size_t DW = (size_t)G::PCOLS * G::QCOLS;        // elements of the dW image; the head row follows it
    static constexpr size_t COUNT = DW + G::HEAD_ROW;

    // pack_bwd_side's operand (grad.hip) with four gates: in the A fragment of output tile t (hidden unit kout receives dL/dh),
    // k-step 4 kt + gate holds K[2 + kout][gate H + u], u = 4 kt + lane quarter.  S = Lin: the operand's table (pack_value.h)
    template <class S = double>
    static std::vector<char> pack_bwd(const rnnwf_handle* h) {
        using Out = PackSink<S>;
        const int H = h->H;
        std::vector<char> img(G::BWD_BYTES, 0);
        Out::begin(img);
        double* A = reinterpret_cast<double*>(img.data());
        const auto K = pvs<S>(h, std::string(kLstmPre) + "kernel");      // [2 + H, 4H], columns i | j | f | o
        for (int t = 0; t < G::NTO; ++t)
            for (int row = 0; row < 16; ++row) {
                int q, r;
                row_to_qr<double>(row, q, r);
                if (t == NFULL && r != 0) continue;
                const int kout = t < NFULL ? 16 * t + 4 * r + q : 16 * NFULL + q;
                if (kout >= H) continue;
                for (int kq = 0; kq < 4; ++kq) {
                    const int lane = (kq << 4) | row;
                    for (int kk = 0; kk < G::KB; ++kk) {
                        const int kt = kk / 4, gate = kk % 4, u = 4 * kt + kq;
                        if (u >= H) continue;
                        Out::put(&A[(((size_t)t * G::KBG + kk / G::VW) * 64 + lane) * G::VW + (kk % G::VW)],
                                 K[(size_t)(2 + kout) * 4 * H + (size_t)gate * H + u]);
                    }
                }
            }
        return img;
    }

    // backward pass over the resident checkpoints, then dW += P^T Q; everything is added into the cleared h->gradW
    static int run(rnnwf_handle* h, LstmGradArgs a) {
        const int64_t R = a.ns * a.N;
        if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * 8)) return rc;
        if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * 8)) return rc;
        a.P = (double*)h->gradP.p;
        a.Q = (double*)h->gradQ.p;
        a.head_grad = (double*)h->gradW.p + DW;
        if (int rc = backward_launch<double>(h, lstm_bwd_kernel<NFULL, kLstmGradWaves>, kLstmGradWaves * 64, G::LDS, a.nsb, kLstmGradWaves,
                                             G::HEAD_ROW, a.head_grad, a))
            return rc;
        return tn_gemm_launch<double, G::PCOLS / 16, G::QCOLS / 16>(h, a.P, a.Q, R, (double*)h->gradW.p);
    }

    // the unit-weight pass of stochastic reconfiguration (sr.hip): the same P and Q rows, every chain's head row into head_rows
    // [ns][HEAD_ROW]; no reduction follows, so the launch is the persistent one without head_reduce_kernel
    static int sr_run(rnnwf_handle* h, LstmGradArgs a, double* head_rows) {
        const int64_t R = a.ns * a.N;
        if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * 8)) return rc;
        if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * 8)) return rc;
        a.P = (double*)h->gradP.p;
        a.Q = (double*)h->gradQ.p;
        a.head_part = head_rows;
        return launch_persistent(h, kTimerBackprop, lstm_bwd_kernel<NFULL, kLstmGradWaves, true>, kLstmGradWaves * 64, G::LDS, a.nsb,
                                 kLstmGradWaves, a);
    }

    // dW image [PCOLS][QCOLS] + head row -> TF-named gradient arrays
    static void unpack(rnnwf_handle* h, const double* dW) {
        const int H = h->H;
        const double* hg = dW + DW;
        auto at = [&](int prow, int col) { return dW[(size_t)prow * G::QCOLS + col]; };
        auto& gK = h->grads[std::string(kLstmPre) + "kernel"];
        auto& gb = h->grads[std::string(kLstmPre) + "bias"];
        auto& gWd = h->grads["wf_dense/kernel"];
        auto& gbd = h->grads["wf_dense/bias"];
        gK.assign((size_t)(2 + H) * 4 * H, 0.0);
        gb.assign((size_t)4 * H, 0.0);
        gWd.assign((size_t)H * 2, 0.0);
        gbd.assign(2, 0.0);
        const size_t W = (size_t)4 * H;
        for (int u = 0; u < H; ++u) {
            const int m = u / 16, r = (u % 16) / 4, q = u % 4;
            const bool full = u < 16 * NFULL;
            const int uq = u - 16 * NFULL;                       // remainder units: lane quarter = uq
            for (int gate = 0; gate < 4; ++gate) {
                const int prow = full ? (gate * NFULL + m) * 16 + 4 * q + r : (G::NT - 1) * 16 + 4 * uq + gate;
                const size_t col = (size_t)gate * H + u;
                for (int k = 0; k < H; ++k) gK[(size_t)(2 + k) * W + col] = at(prow, col_of_unit(NFULL, k));
                for (int i = 0; i < 2; ++i) gK[(size_t)i * W + col] = at(prow, 16 * NFULL + 1 + i);
                gb[col] = at(prow, 16 * NFULL + 3);            // (the forget bias's constant 1 has no gradient)
            }
            // head: the image holds the logit difference z1 - z0, so d/dWd[:,1] = +v and d/dWd[:,0] = -v (GLaunch::unpack)
            const double v = hg[u];
            gWd[(size_t)u * 2 + 1] = v;
            gWd[(size_t)u * 2] = -v;
        }
        gbd[1] = hg[4 * G::KT];
        gbd[0] = -hg[4 * G::KT];
    }
};

template <class Fn>
int with_lstm_grad(rnnwf_handle* h, const char* what, Fn&& fn) {
    int rc = 0;
    if (with_width_kernels<LGrad>(LstmKernels(), h, [&](auto k) { rc = fn(k); })) return rc;
    return h->fail(RNNWF_ERR_INVALID, "%s: no LSTM gradient kernel for NFULL=%d (one layer, <= 68 units)", what, h->NFULL);
}

int require_lstm(rnnwf_handle* h, const char* what) {
    if (h->model == RNNWF_MODEL_LSTM1D_F64) return 0;
    return h->fail(RNNWF_ERR_INVALID, "%s: needs an LSTM1D_F64 handle, this one is %s (its gradient: rnnwf_vmc_gradient)", what,
                   model_name(h->model));
}

}  // namespace

// the backward operand in h->wbwd, packed from the host's parameters and uploaded when a commit has left it stale (a device re-pack
// keeps it current: train.hip)
int rnnwf::lstm_bwd_image(rnnwf_handle* h, const char* what) {
    if (h->wbwd_valid) return 0;
    return with_lstm_grad(h, what, [&](auto k) -> int {
        const std::vector<char> img = decltype(k)::pack_bwd(h);
        if (int rc = ensure(h, h->wbwd, img.size())) return rc;
        if (int rc = upload(h, h->wbwd.p, img.data(), img.size())) return rc;
        h->wbwd_valid = true;
        return 0;
    });
}
// its table over Lin into the active PackTrace
int rnnwf::lstm_bwd_pack_table(rnnwf_handle* h) {
    return with_lstm_grad(h, "device training", [&](auto k) -> int { decltype(k)::template pack_bwd<Lin>(h); return 0; });
}
// grad_flat_probe (grad.hip) for the LSTM: LGrad::unpack on an image whose element k holds k + 1 - sidx[i] = +-(1 + the h->gradW
// element flat parameter i is read from; the sign: the head's two columns), *count = LGrad::COUNT.  h->grads is left as it was
int rnnwf::lstm_grad_flat_probe(rnnwf_handle* h, std::vector<int32_t>& sidx, size_t* count) {
    return with_lstm_grad(h, "device training", [&](auto k) -> int {
        using K = decltype(k);
        *count = K::COUNT;
        static_assert(K::COUNT < ((size_t)1 << 31), "the indices must fit int32_t");
        std::vector<double> img(K::COUNT);
        for (size_t i = 0; i < K::COUNT; ++i) img[i] = (double)(i + 1);
        const auto saved = h->grads;
        K::unpack(h, img.data());
        sidx.clear();
        int rc = 0;
        for (auto& kv : h->params) {
            auto it = h->grads.find(kv.first);
            if (it == h->grads.end() || it->second.size() != kv.second.value.size()) {
                rc = h->fail(RNNWF_ERR_STATE, "device training: no gradient for '%s'", kv.first.c_str());
                break;
            }
            for (int64_t s : kv.second.slot) sidx.push_back((int32_t)std::llround(it->second[(size_t)s]));
        }
        h->grads = saved;
        return rc;
    });
}

// The one driver: the backward pass on the ns chains whose spins (h->bits) and checkpoints (h->hck) the base pass just left, with
// the weights in w_dev, or (w_dev == nullptr) formed from h->eloc and the step's moments still on the device; the dW image and the
// head row are queued for download into h->staging.  The caller synchronises once and calls lstm_grad_finish.  (Declared in models.h:
// rnnwf_lstm_pauli_gradient_step, lstm_pauli.hip, runs it on the batch of its Pauli pass.)
// download = false (device-resident training, rnnwf_lstm_train_steps): the result stays in h->gradW, where Adam reads it.
namespace {
// what every backward pass reads of the batch in h->bits / h->hck
LstmGradArgs batch_args(rnnwf_handle* h, int64_t ns) {
    LstmGradArgs a{};
    a.wimg = h->wimg.p;
    a.wbwd = h->wbwd.p;
    a.N = h->N;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = (const double*)h->hck.p;
    return a;
}
}  // namespace

int rnnwf::lstm_grad_queue(rnnwf_handle* h, const char* what, int64_t ns, const double* w_dev, bool download) {
    return with_lstm_grad(h, what, [&](auto k) -> int {
        using K = decltype(k);
        if (int rc = lstm_bwd_image(h, what)) return rc;
        if (int rc = ensure(h, h->gradW, K::COUNT * 8)) return rc;
        RNNWF_HIP(h, hipMemsetAsync(h->gradW.p, 0, K::COUNT * 8, h->stream));
        LstmGradArgs a = batch_args(h, ns);
        a.weights = w_dev;
        a.eloc = (const double*)h->eloc.p;
        a.mom = (const double*)h->moments.p;
        if (int rc = K::run(h, a)) return rc;
        if (!download) return 0;
        if (int rc = ensure_staging(h, K::COUNT * 8)) return rc;      // pinned: the copy is a plain DMA, the one wait is the caller's
        RNNWF_HIP(h, hipMemcpyAsync(h->staging, h->gradW.p, K::COUNT * 8, hipMemcpyDeviceToHost, h->stream));
        return 0;
    });
}
// stochastic reconfiguration (sr.hip): the backward pass in its unit-weight mode over the resident batch (h->last_ns chains in
// h->bits / h->hck); the rows of P and Q into h->gradP / h->gradQ, every chain's head row into head_rows.  h->wbwd is current
// (lstm_bwd_image: sr_build_shape)
int rnnwf::lstm_sr_backward(rnnwf_handle* h, double* head_rows) {
    return with_lstm_grad(h, "stochastic reconfiguration", [&](auto k) -> int {
        return decltype(k)::sr_run(h, batch_args(h, h->last_ns), head_rows);
    });
}
void rnnwf::lstm_grad_finish(rnnwf_handle* h) {
    with_lstm_grad(h, "", [&](auto k) -> int { decltype(k)::unpack(h, (const double*)h->staging); return 0; });
}

namespace {

int check_ready(rnnwf_handle* h, const char* what) {
    if (int rc = require_lstm(h, what)) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "%s: parameters not committed (call rnnwf_commit_params)", what);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    return 0;
}

}  // namespace

extern "C" int rnnwf_lstm_gradient(rnnwf_handle* h, const int32_t* samples, int64_t B, const double* weights) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = check_ready(h, "rnnwf_lstm_gradient")) return rc;
    if (B < 1 || !samples || !weights) return h->fail(RNNWF_ERR_INVALID, "rnnwf_lstm_gradient: bad arguments");
    if (int rc = refuse_past_budget(h, B, "rnnwf_lstm_gradient")) return rc;
    h->last_ns = 0;
    h->call_ns = B;
    if (int rc = upload_and_pack(h, samples, B, h->bits, 0, nullptr)) return rc;
    if (int rc = lstm_teacher_base(h, B)) return rc;
    if (int rc = ensure(h, h->out_lp, (size_t)B * 8)) return rc;      // the weights' place on the device (this base pass leaves it free)
    RNNWF_HIP(h, hipMemcpyAsync(h->out_lp.p, weights, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
    if (int rc = lstm_grad_queue(h, "rnnwf_lstm_gradient", B, (const double*)h->out_lp.p)) return rc;
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    lstm_grad_finish(h);
    return RNNWF_OK;
}

extern "C" int rnnwf_lstm_vmc_gradient_step(rnnwf_handle* h, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                            const double* couplings, double* moments, int32_t* out_samples, double* out_eloc) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = check_ready(h, "rnnwf_lstm_vmc_gradient_step")) return rc;
    if (ns < 1 || !couplings || !moments) return h->fail(RNNWF_ERR_INVALID, "rnnwf_lstm_vmc_gradient_step: bad arguments");
    if (h->comm || h->nranks > 1 || h->reduce_in_step)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_lstm_vmc_gradient_step: single process only (the weights are centred with this handle's "
                                          "moments); with a communicator use rnnwf_vmc_step and rnnwf_lstm_gradient with globally centred weights");
    // the fused step without its synchronisation: the moments kernel writes the step's pinned row as well as h->moments
    h->moments_direct = (double*)h->pinned_dev;
    const int rc_step = vmc_step(h, ns, Draw{seed, step, sample_offset}, couplings, out_samples, out_eloc, nullptr);
    h->moments_direct = nullptr;
    if (rc_step) return rc_step;
    if (int rc = lstm_grad_queue(h, "rnnwf_lstm_vmc_gradient_step", ns, nullptr)) return rc;
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(moments, h->pinned, 4 * sizeof(double));
    lstm_grad_finish(h);
    return RNNWF_OK;
}

// K whole Adam iterations with one host synchronisation: rnnwf_train_steps for the LSTM (docs/lstm.md, "Device-resident training").
// Per iteration, nothing waiting for the host: rnnwf_lstm_vmc_gradient_step's kernels - the fused step with its moments written into
// row k of train.hip's pinned table, the backward pass and P^T Q with the dW image left in h->gradW -, then train.hip's Adam and the
// re-pack of h->wimg and h->wbwd from the tables the LSTM's builder recorded (train_prepare_lstm).
extern "C" int rnnwf_lstm_train_steps(rnnwf_handle* h, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                      const double* couplings, int64_t n_couplings, const double* learning_rates, double beta1,
                                      double beta2, double epsilon, double* moments) {
    constexpr const char* kEntry = "rnnwf_lstm_train_steps";
    // everything is validated before anything is touched: a refused call leaves the parameters and Adam's state
    if (!h) return RNNWF_ERR_INVALID;
    if (h->model != RNNWF_MODEL_LSTM1D_F64)
        return h->fail(RNNWF_ERR_INVALID, "%s: needs an LSTM1D_F64 handle, this one is %s (its device-resident training: rnnwf_train_steps)",
                       kEntry, model_name(h->model));
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "%s: parameters not committed (call rnnwf_commit_params)", kEntry);
    if (h->comm || h->nranks > 1 || h->reduce_in_step)
        return h->fail(RNNWF_ERR_INVALID, "%s: single process only (the weights are centred with this handle's moments), this handle has "
                                          "a communicator", kEntry);
    if (K < 1 || K > kTrainMaxSteps) return h->fail(RNNWF_ERR_INVALID, "%s: K must be 1..%d", kEntry, kTrainMaxSteps);
    if (numsamples < 1 || !couplings || !learning_rates || !moments)
        return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments (numsamples >= 1; couplings, learning_rates and moments non-null)", kEntry);
    if (n_couplings != (int64_t)h->family->coupl_per_site * h->N + h->family->coupl_tail)
        return h->fail(RNNWF_ERR_INVALID, "%s: wrong number of couplings", kEntry);
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(learning_rates[k])) return h->fail(RNNWF_ERR_INVALID, "%s: learning_rates[%d] must be finite", kEntry, k);
    if (int rc = refuse_past_budget(h, numsamples, kEntry)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    if (int rc = train_prepare_lstm(h)) return rc;
    int rc = 0, applied = 0;
    for (int k = 0; k < K && !rc; ++k) {
        h->moments_direct = train_moments_row(h, k);          // as rnnwf_train_steps: the moments kernel writes the pinned row itself
        rc = vmc_step(h, numsamples, Draw{seed, step0 + (uint64_t)k, sample_offset}, couplings, nullptr, nullptr, nullptr);
        h->moments_direct = nullptr;
        if (!rc) rc = lstm_grad_queue(h, kEntry, numsamples, nullptr, false);
        if (!rc) rc = train_adam_update(h, k, learning_rates[k], beta1, beta2, epsilon);
        if (!rc) ++applied;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = h->fail(RNNWF_ERR_HIP, "%s: stream synchronisation failed", kEntry);
    if (rc) {                                                 // the updates that were applied count; no batch belongs to the new weights
        train_steps_failed(h, applied);
        return rc;
    }
    train_steps_done(h, K, moments);
    return RNNWF_OK;
}
