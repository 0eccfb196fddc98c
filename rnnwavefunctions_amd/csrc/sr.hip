// sr.hip - stochastic reconfiguration (docs/sr.md): rnnwf_log_derivatives, rnnwf_sr_gram, rnnwf_sr_apply, rnnwf_sr_solve,
// rnnwf_sr_direction on the resident batch of the one-layer positive GRU (GRU1D, GRU1D_F64; up to 68 units), and rnnwf_sr_train_steps,
// K whole minSR iterations on batches it draws itself (the update and the images' re-pack are train.hip's).  The per-sample
// log-derivatives J[ns][D] stay on the device in the order of the gradient image (grad.hip) and are read through the table
// grad_flat_probe builds; the ns x ns solve is the caller's (rnnwf_sr_gram + rnnwf_sr_apply) or the device's (rnnwf_sr_solve,
// rnnwf_sr_direction: blocked f64 Cholesky, sr_solve_kernels.h).
// The complex RNN (CRNN_U1, one layer, up to 68 units) has the same five calls as rnnwf_*_complex (docs/sr_complex.md): J[2 ns][D_c]
// = [Re O ; Im O], each half centred with its own mean, and the same solve path on a system of order 2 ns.
// The 2D RNN (MDRNN2D, float64, up to 84 units) has them as rnnwf_*_2d (docs/sr_2d.md): J[ns][D_2] in the order of its gradient image,
// from mdrnn_bwd_kernel's unit-weight mode (mdrnn.hip: mdrnn_sr_backward); one row block, everything behind J as for the positive GRU.
// The LSTM wave function (LSTM1D_F64, up to 68 units) has them as rnnwf_*_lstm (docs/sr_lstm.md): J[ns][D_l] from lstm_bwd_kernel's
// unit-weight mode (lstm_grad.hip: lstm_sr_backward).  Its resident batch comes from two entries of its own, rnnwf_lstm_load_batch and
// rnnwf_sr_step_lstm (the fused step and the whole direction in one call): rnnwf_vmc_step leaves an LSTM handle none.
#include <cmath>
#include <cstring>

#include "sr_kernels.h"
#include "sr_solve_kernels.h"
#include "models.h"
#include "shapes.h"
#include "tn_gemm.h"

using namespace rnnwf;

namespace {

constexpr int64_t kSrMaxSamples = 4096;   // the largest order of the Gram matrix and the solve
static_assert(2 * RNNWF_SR_COMPLEX_MAX_SAMPLES == kSrMaxSamples, "the complex RNN's system has 2 ns rows");
constexpr int kSrMaxNFULL = 4;             // up to 68 units
constexpr int kSrMaxSteps = 1024;          // iterations of one rnnwf_sr_train_steps call: the rows of train.hip's pinned moments table (kMaxSteps)

// An entry point: its name, and the family it belongs to - the positive GRU's, the complex RNN's (rnnwf_*_complex, docs/sr_complex.md)
// the 2D RNN's (rnnwf_*_2d, docs/sr_2d.md) or the LSTM's (rnnwf_*_lstm, docs/sr_lstm.md).  Which handles an entry serves depends on the entry; once it has accepted a handle, the
// handle's model decides everything else (sr_halves, with_sr_shape).
enum SrFamily { kSrPositive, kSrComplex, kSr2D, kSrLstm };
struct SrEntry {
    const char* name;
    SrFamily family;
};

// the row blocks of J with a column mean of their own: [Re O ; Im O] for the complex RNN, whose system has 2 ns rows
int64_t sr_halves(const rnnwf_handle* h) { return h->model == RNNWF_MODEL_CRNN_U1 ? 2 : 1; }
int64_t sr_order(const rnnwf_handle* h) { return sr_halves(h) * h->sr_ns; }

// 0, or RNNWF_ERR_INVALID "<entry>: <why>" for a handle these entry points do not serve; called before anything is touched
int sr_refuse(rnnwf_handle* h, const SrEntry& e) {
    const char* entry = e.name;
    const char* why = nullptr;
    if (e.family == kSr2D) {
        if (h->model != RNNWF_MODEL_MDRNN2D) why = "only for the 2D RNN (RNNWF_MODEL_MDRNN2D)";
        else if (h->comm) why = "not implemented for a handle with a communicator";
        return why ? h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why) : 0;
    }
    if (e.family == kSrLstm) {                             // (one layer, up to 68 units: every LSTM handle there is)
        if (h->model != RNNWF_MODEL_LSTM1D_F64) why = "only for the LSTM wave function (RNNWF_MODEL_LSTM1D_F64)";
        else if (h->comm) why = "not implemented for a handle with a communicator";
        return why ? h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why) : 0;
    }
    if (e.family == kSrComplex) {
        if (h->model != RNNWF_MODEL_CRNN_U1) why = "only for the complex RNN (RNNWF_MODEL_CRNN_U1)";
        else if (h->NL > 1) why = "not implemented for stacked layers (one GRU layer only)";
        else if (h->NFULL > kSrMaxNFULL) why = "not implemented for layers wider than 68 units";
        else if (h->comm) why = "not implemented for a handle with a communicator";
        return why ? h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why) : 0;
    }
    switch (h->model) {
        case RNNWF_MODEL_GRU1D_PARITY: why = "not implemented for the parity model (its symmetrised P has two directions per sample)"; break;
        case RNNWF_MODEL_CRNN_U1: why = "not implemented for the complex RNN"; break;
        case RNNWF_MODEL_MDRNN2D: why = "not implemented for the 2D RNN (MDRNN)"; break;
        case RNNWF_MODEL_LSTM1D_F64: why = "not implemented for the LSTM cell"; break;
        default:
            if (h->NL > 1) why = "not implemented for stacked layers (one GRU layer only)";
            else if (h->NFULL > kSrMaxNFULL) why = "not implemented for layers wider than 68 units";
            else if (h->comm) why = "not implemented for a handle with a communicator";
    }
    return why ? h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why) : 0;
}

// fn(SrShape<T, NFULL, NOUT>()) for the handle's row among the one-layer rows of its family's table up to kSrMaxNFULL (shapes.h):
// the positive GRU's (NOUT 1) or the complex RNN's (NOUT 3); fn(MdSrShape<NFULL>()) for every row of the 2D RNN's table,
// fn(LstmSrShape<NFULL>()) for every row of the LSTM's
template <class R> struct SrRow : std::bool_constant<R::NL == 1 && R::NFULL <= kSrMaxNFULL> {};
template <class Fn>
int with_sr_shape(rnnwf_handle* h, Fn&& fn) {
    int rc = 0;
    const bool hit = h->model == RNNWF_MODEL_MDRNN2D
        ? with_row<OneLayer>(MdKernels(), h, [&](auto r) { rc = fn(MdSrShape<decltype(r)::NFULL>()); })
        : h->model == RNNWF_MODEL_LSTM1D_F64
        ? with_row<SrRow>(LstmKernels(), h, [&](auto r) { rc = fn(LstmSrShape<decltype(r)::NFULL>()); })
        : h->model == RNNWF_MODEL_CRNN_U1
        ? with_row<SrRow>(CrnnKernels(), h, [&](auto r) { rc = fn(SrShape<typename decltype(r)::T, decltype(r)::NFULL, 3>()); })
        : with_row<SrRow>(GruKernels(), h, [&](auto r) { rc = fn(SrShape<typename decltype(r)::T, decltype(r)::NFULL>()); });
    if (hit) return rc;
    return h->fail(RNNWF_ERR_INVALID, "stochastic reconfiguration: no kernel for NFULL=%d", h->NFULL);
}

int64_t sr_image_size(rnnwf_handle* h) {
    int64_t D = 0;
    with_sr_shape(h, [&](auto s) { D = decltype(s)::D; return 0; });
    return D;
}

// RNNWF_ERR_NOMEM unless the workspace of a batch of ns samples fits; `factor`: with the ns x ns Cholesky factor
int sr_workspace(rnnwf_handle* h, const char* entry, int64_t ns, bool factor) {
    const size_t es = h->f64 ? 8 : 4;
    const size_t n = (size_t)(sr_halves(h) * ns);              // rows of J, order of the Gram matrix and of the solve
    // the factor's workspace: n^2 doubles, eps, y, the status word and the diagonal blocks (sr_solve_device), all counted
    const size_t nb = (n + kSrNB - 1) / kSrNB;
    const size_t fac = factor ? (n * n + 2 * n + 1 + nb * kSrNB * kSrNB) * 8 : 0;
    const size_t need = n * (size_t)sr_image_size(h) * es + n * n * 8 + fac;
    if ((int64_t)n > kSrMaxSamples || need > state_budget_bytes(h, kDefaultStateBudget))
        return h->fail(RNNWF_ERR_NOMEM, "%s: ns too large for the SR workspace (%lld samples: Jacobian + Gram matrix%s take %zu bytes; at most %lld samples)",
                       entry, (long long)ns, factor ? " + Cholesky factor" : "", need, (long long)(kSrMaxSamples / sr_halves(h)));
    return 0;
}

int sr_committed(rnnwf_handle* h, const char* entry) {
    return h->committed ? 0 : h->fail(RNNWF_ERR_STATE, "%s: parameters not committed (call rnnwf_commit_params)", entry);
}

// refusals, then the state checks every entry point on the resident batch shares; `factor`: the entry also holds the Cholesky factor
int sr_ready(rnnwf_handle* h, const SrEntry& e, bool factor = false) {
    const char* entry = e.name;
    if (int rc = sr_refuse(h, e)) return rc;
    if (int rc = sr_committed(h, entry)) return rc;
    if (h->last_ns <= 0)
        return e.family == kSrLstm
            ? h->fail(RNNWF_ERR_STATE, "%s: call rnnwf_lstm_load_batch or rnnwf_sr_step_lstm first (their samples, states and E_loc are reused)", entry)
            : h->fail(RNNWF_ERR_STATE, "%s: call rnnwf_vmc_step first (its samples, states and E_loc are reused)", entry);
    if (int rc = sr_workspace(h, entry, h->last_ns, factor)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    return 0;
}

// the flat-order table and, on the device, how many parameters read each image element (0: padding)
int sr_table(rnnwf_handle* h, int64_t D) {
    if (!h->sr_sidx.empty()) return 0;
    std::vector<int32_t> sidx;
    GradImage im{};
    if (h->model == RNNWF_MODEL_LSTM1D_F64) {              // no hook table: the probe of its own unpacker (lstm_grad.hip), +- for the head's two columns
        im.f64 = true;
        if (int rc = lstm_grad_flat_probe(h, sidx, &im.count)) return rc;
    } else if (int rc = grad_flat_probe(h, sidx, &im)) {
        return rc;
    }
    if ((int64_t)im.count != D || im.f64 != h->f64) return h->fail(RNNWF_ERR_INVALID, "stochastic reconfiguration: gradient image of %zu elements, expected %lld", im.count, (long long)D);
    std::vector<uint8_t> used((size_t)D, 0);
    for (int32_t v : sidx)
        if (v) ++used[(size_t)std::abs(v) - 1];
    if (int rc = ensure(h, h->srMask, (size_t)D)) return rc;
    if (int rc = upload(h, h->srMask.p, used.data(), (size_t)D)) return rc;
    h->sr_sidx = std::move(sidx);
    return 0;
}

// The backward pass over the resident batch in its unit-weight mode: the rows of P and Q, every chain's head rows into h->srHead.
// GRU families: gru_bwd_kernel<SR>; `half` is the complex RNN's seed
template <typename T, int NFULL, int NOUT>
int sr_backward(rnnwf_handle* h, SrShape<T, NFULL, NOUT>, int half) {
    using G = GradLayout<NFULL, T>;
    using L = GruLayout<T, NFULL, NOUT>;
    const int64_t ns = h->last_ns, R = ns * h->N, nsb = (ns + kChains - 1) / kChains;
    if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * sizeof(T))) return rc;
    if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * sizeof(T))) return rc;
    GradArgs a{};
    grad_batch_args(h, &a);                                // (one layer: sr_refuse)
    a.wimg = h->wimg.p;
    a.head_part = h->srHead.p;                             // [ns][NOUT][HEAD_ROW]: the head rows of every chain (gru_bwd_kernel<SR>)
    a.sr_im = half;
    constexpr size_t lds = L::LDS_BYTES + (GradStream<T, NFULL, NOUT>::value ? 0 : G::BWD_BYTES);
    static_assert(lds <= 160 * 1024, "forward + backward weight images exceed the LDS");
    return launch_persistent(h, kTimerBackprop, gru_bwd_kernel<T, NFULL, 4, NOUT, false, true>, 4 * 64, lds, nsb, 4, a);
}
// 2D RNN: mdrnn_bwd_kernel<SR> behind the set-up of its gradient launch (the site maps, the ring in HBM)
template <int NFULL>
int sr_backward(rnnwf_handle* h, MdSrShape<NFULL>, int) {
    return mdrnn_sr_backward(h, (double*)h->srHead.p);
}
// LSTM: lstm_bwd_kernel<SR> behind the arguments of its gradient launch
template <int NFULL>
int sr_backward(rnnwf_handle* h, LstmSrShape<NFULL>, int) {
    return lstm_sr_backward(h, (double*)h->srHead.p);
}

template <class S>
int sr_build_shape(rnnwf_handle* h) {
    using T = typename S::Elem;
    using G = typename S::G;
    const int N = h->N;
    const int64_t ns = h->last_ns;
    if (int rc = sr_table(h, S::D)) return rc;
    if (int rc = h->model == RNNWF_MODEL_LSTM1D_F64 ? lstm_bwd_image(h, "stochastic reconfiguration") : grad_bwd_image(h)) return rc;
    if (int rc = ensure(h, h->srHead, (size_t)ns * S::NOUT * G::HEAD_ROW * sizeof(T))) return rc;
    if (int rc = ensure(h, h->srJ, (size_t)sr_halves(h) * ns * S::D * sizeof(T))) return rc;
    // complex RNN: one backward pass and one outer-product pass per seed, Re O into the rows [0, ns) and Im O into [ns, 2 ns).  Both
    // go through the same P, Q and head rows - the second pass starts after the first half is written (one stream); Q is the same twice
    for (int half = 0; half < (int)sr_halves(h); ++half) {
        if (int rc = sr_backward(h, S(), half)) return rc;
        if (int rc = launch_persistent(h, kTimerGemm, sr_outer_kernel<S>, S::WAVES * 64, 0, ns, 1, (const T*)h->gradP.p,
                                       (const T*)h->gradQ.p, (const T*)h->srHead.p, (const uint8_t*)h->srMask.p, N, ns,
                                       (T*)h->srJ.p + (size_t)half * ns * S::D))
            return rc;
    }
    h->sr_ns = ns;
    h->sr_valid = true;
    return 0;
}

// J for the resident batch and the committed parameters, built when it is stale
int sr_build(rnnwf_handle* h) {
    if (h->sr_valid && h->sr_ns == h->last_ns) return 0;
    h->sr_valid = false;
    return with_sr_shape(h, [&](auto s) { return sr_build_shape<decltype(s)>(h); });
}

// out[k] = scale sum_s w_s J[row0 + s][k] over `rows` rows of the resident Jacobian
int sr_colsum(rnnwf_handle* h, int64_t D, int64_t row0, int64_t rows, const double* w, double scale, double* out) {
    return h->f64 ? launch_persistent(h, kTimerGemm, sr_colsum_kernel<double>, 256, 0, (D + 63) / 64, 1, (const double*)h->srJ.p + row0 * D, rows, D,
                                      w, scale, out)
                  : launch_persistent(h, kTimerGemm, sr_colsum_kernel<float>, 256, 0, (D + 63) / 64, 1, (const float*)h->srJ.p + row0 * D, rows, D,
                                      w, scale, out);
}

template <typename T, bool HALVES>
int sr_gram_launch(rnnwf_handle* h, int64_t n, int64_t D, const double* mean) {
    const int64_t nb = (n + 31) / 32, nblocks = nb * (nb + 1) / 2;
    return launch_persistent(h, kTimerGemm, sr_gram_kernel<T, HALVES>, 256, 0, nblocks, 1, (const T*)h->srJ.p, mean, (const uint8_t*)h->srMask.p, n, D,
                             nblocks, (double*)h->srGram.p);
}

// the column mean(s) and the centred Gram matrix of the resident Jacobian, into h->srCol[0 .. halves D) and h->srGram; h->srCol has
// room for one more image behind the means (sr_direction_image)
int sr_gram_device(rnnwf_handle* h) {
    const int64_t ns = h->sr_ns, halves = sr_halves(h), n = sr_order(h), D = sr_image_size(h);
    if (int rc = ensure(h, h->srCol, (size_t)(halves + 1) * D * 8)) return rc;
    if (int rc = ensure(h, h->srGram, (size_t)n * n * 8)) return rc;
    double* mean = (double*)h->srCol.p;
    for (int64_t half = 0; half < halves; ++half)
        if (int rc = sr_colsum(h, D, half * ns, ns, nullptr, 1.0 / (double)ns, mean + half * D)) return rc;
    if (halves == 2) return sr_gram_launch<float, true>(h, n, D, mean);         // (the complex RNN is float32)
    return h->f64 ? sr_gram_launch<double, false>(h, n, D, mean) : sr_gram_launch<float, false>(h, n, D, mean);
}

// (gram + ns diag_shift I) y = eps on the device, of order n = sr_order: eps from the resident local energies into the eps row of the
// workspace, per panel the diagonal factorisation + panel solve and the trailing update, then the backward sweep.  Leaves y and the pivot
// status word behind the eps row (sr_y / sr_status), the factors of the diagonal blocks behind those; nothing is synchronised here.
double* sr_y(rnnwf_handle* h) { return (double*)h->srFac.p + (size_t)sr_order(h) * sr_order(h) + (size_t)sr_order(h); }
long long* sr_status(rnnwf_handle* h) { return (long long*)(sr_y(h) + sr_order(h)); }

int sr_solve_device(rnnwf_handle* h, double diag_shift) {
    const int64_t ns = h->sr_ns, n = sr_order(h);
    const int nb = (int)((n + kSrNB - 1) / kSrNB);
    if (int rc = ensure(h, h->srFac, ((size_t)n * n + 2 * (size_t)n + 1 + (size_t)nb * kSrNB * kSrNB) * 8)) return rc;
    double* F = (double*)h->srFac.p;
    double* Ld = (double*)(sr_status(h) + 1);                // the factorised diagonal blocks
    const double* gram = (const double*)h->srGram.p;
    const double shift = (double)ns * diag_shift;            // ns, not the order: the shift of S = O^T O / ns
    if (int rc = sr_halves(h) == 2
            ? timed_launch(h, kTimerGemm, sr_centre_complex_kernel, 2, 256, 0, (const float2*)h->eloc.p, ns, F + (size_t)n * n, sr_status(h))
            : timed_launch(h, kTimerGemm, sr_centre_kernel, 1, 256, 0, (const double*)h->eloc.p, ns, F + (size_t)n * n, sr_status(h)))
        return rc;
    for (int k = 0; k < nb; ++k) {
        const double* src = k == 0 ? gram : F;
        if (int rc = launch_persistent(h, kTimerGemm, sr_chol_panel_kernel, 256, 0, nb - k, 1, src, F, n, k, shift, Ld, sr_status(h))) return rc;
        const int64_t m = nb - k - 1, nitems = m * (m + 1) / 2 + m;
        if (nitems > 0)
            if (int rc = launch_persistent(h, kTimerGemm, sr_chol_update_kernel, 256, 0, nitems, 1, src, F, n, k, nitems)) return rc;
    }
    for (int k = nb - 1; k >= 0; --k)
        if (int rc = launch_persistent(h, kTimerGemm, sr_chol_back_kernel, 64, 0, k + 1, 1, F, (const double*)Ld, n, k, sr_y(h))) return rc;
    return 0;
}

int sr_check_shift(rnnwf_handle* h, const char* entry, double diag_shift) {
    if (!(diag_shift > 0.0) || !std::isfinite(diag_shift)) return h->fail(RNNWF_ERR_INVALID, "%s: diag_shift must be positive and finite", entry);
    return 0;
}

// the device work the solving entries share once their checks have passed, up to y on the device
int sr_solve_queue(rnnwf_handle* h, double diag_shift) {
    if (int rc = sr_build(h)) return rc;
    if (int rc = sr_gram_device(h)) return rc;
    return sr_solve_device(h, diag_shift);
}

int sr_solve_common(rnnwf_handle* h, const SrEntry& e, double diag_shift) {
    if (int rc = sr_check_shift(h, e.name, diag_shift)) return rc;
    if (int rc = sr_ready(h, e, true)) return rc;
    return sr_solve_queue(h, diag_shift);
}

// behind sr_solve_queue: dO^T y = J^T (y - mean y), as rnnwf_sr_apply, with the centring on the device (each half of y with its own
// mean); the direction's image is left in sr_direction_image(h), nothing is synchronised
double* sr_direction_image(rnnwf_handle* h) { return (double*)h->srCol.p + sr_halves(h) * sr_image_size(h); }

int sr_direction_queue(rnnwf_handle* h) {
    const int64_t ns = h->sr_ns, n = sr_order(h), D = sr_image_size(h);
    if (int rc = ensure(h, h->srY, (size_t)n * 8)) return rc;
    for (int64_t half = 0; half < sr_halves(h); ++half)
        if (int rc = timed_launch(h, kTimerGemm, sr_centre_kernel, 1, 256, 0, (const double*)sr_y(h) + half * ns, ns, (double*)h->srY.p + half * ns,
                                  (long long*)nullptr))
            return rc;
    return sr_colsum(h, D, 0, n, (const double*)h->srY.p, 1.0, sr_direction_image(h));
}

// rnnwf_sr_train_steps: iteration k's pivot status word into its slot of the call's table, and into the sticky word when that is
// still clear (sr_centre_kernel clears the solve's own word at the start of every iteration)
__global__ void sr_record_status_kernel(const long long* __restrict__ status, int k, long long* __restrict__ table) {
    if (blockIdx.x || threadIdx.x) return;
    const long long s = *status;
    table[1 + k] = s;
    if (s && !table[0]) table[0] = k + 1;
}

int sr_pivot_error(rnnwf_handle* h, const char* entry, long long status, double diag_shift) {
    return h->fail(RNNWF_ERR_NUMERIC, "%s: pivot %lld of the shifted Gram matrix is not positive and finite (diag_shift %g, %lld samples)", entry,
                   status - 1, diag_shift, (long long)h->sr_ns);
}

// flat[i] = +-img[|sidx[i]| - 1] (0 where the parameter has no source): the gather of rnnwf_get_grads_flat
template <typename T>
void sr_gather(const std::vector<int32_t>& sidx, const T* img, double* flat) {
    for (size_t i = 0; i < sidx.size(); ++i) {
        const int32_t v = sidx[i];
        flat[i] = v > 0 ? (double)img[v - 1] : v < 0 ? -(double)img[-v - 1] : 0.0;
    }
}

}  // namespace

extern "C" int64_t rnnwf_resident_samples(const rnnwf_handle* h) { return h ? h->last_ns : 0; }

// ---- the five calls on the resident batch, each behind the positive GRU's entry, the complex RNN's (docs/sr_complex.md), the 2D
// RNN's (docs/sr_2d.md) and the LSTM's (docs/sr_lstm.md).  Below the refusal the four run the same code on sr_halves(h) row blocks of ns rows: n = sr_order(h) rows of J, a Gram matrix and a
// solve of order n, y and eps of n entries ([Re ; Im] for the complex RNN).

static int sr_log_derivatives(rnnwf_handle* h, const SrEntry& e, double* out, int64_t ns, int64_t nparams) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, e)) return rc;
    if (out && (ns != h->last_ns || nparams != rnnwf_num_params(h)))
        return h->fail(RNNWF_ERR_INVALID, "%s: the resident batch has %lld samples and the model %lld parameters, caller passed %lld and %lld", e.name,
                       (long long)h->last_ns, (long long)rnnwf_num_params(h), (long long)ns, (long long)nparams);
    if (int rc = sr_build(h)) return rc;
    if (!out) return RNNWF_OK;
    const int64_t D = sr_image_size(h), n = sr_order(h);
    const size_t bytes = (size_t)n * D * (h->f64 ? 8 : 4);
    if (int rc = ensure_staging(h, bytes)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, h->srJ.p, bytes, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t s = 0; s < n; ++s) {
        if (h->f64) sr_gather(h->sr_sidx, (const double*)h->staging + s * D, out + s * nparams);
        else sr_gather(h->sr_sidx, (const float*)h->staging + s * D, out + s * nparams);
    }
    return RNNWF_OK;
}

// v[s] -= the mean of the ns entries, the sum taken in order
static void sr_centre_host(double* v, int64_t ns) {
    double sum = 0.0;
    for (int64_t s = 0; s < ns; ++s) sum += v[s];
    const double mean = sum / (double)ns;
    for (int64_t s = 0; s < ns; ++s) v[s] -= mean;
}

static int sr_gram(rnnwf_handle* h, const SrEntry& e, double* gram, double* eps) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, e)) return rc;
    if (!gram || !eps) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", e.name);
    if (int rc = sr_build(h)) return rc;
    if (int rc = sr_gram_device(h)) return rc;
    const int64_t ns = h->sr_ns, n = sr_order(h);
    RNNWF_HIP(h, hipMemcpyAsync(gram, h->srGram.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, h->stream));
    if (sr_halves(h) == 2) {                                  // complex64 local energies -> [Re eps ; Im eps]
        if (int rc = ensure_staging(h, (size_t)ns * sizeof(float2))) return rc;
        RNNWF_HIP(h, hipMemcpyAsync(h->staging, h->eloc.p, (size_t)ns * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        const float2* el = (const float2*)h->staging;
        for (int64_t s = 0; s < ns; ++s) {
            eps[s] = (double)el[s].x;
            eps[ns + s] = (double)el[s].y;
        }
    } else {
        RNNWF_HIP(h, hipMemcpyAsync(eps, h->eloc.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    for (int64_t half = 0; half < sr_halves(h); ++half) sr_centre_host(eps + half * ns, ns);
    return RNNWF_OK;
}

static int sr_apply(rnnwf_handle* h, const SrEntry& e, const double* y, double* out_direction) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, e)) return rc;
    if (!y || !out_direction) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", e.name);
    if (int rc = sr_build(h)) return rc;
    const int64_t ns = h->sr_ns, n = sr_order(h), D = sr_image_size(h);
    // dO^T y = J^T (y - mean y): the centring moves from the rows of the matrix to the weights (each half with its own mean)
    std::vector<double> yc(y, y + n);
    for (int64_t half = 0; half < sr_halves(h); ++half) sr_centre_host(yc.data() + half * ns, ns);
    if (int rc = ensure(h, h->srY, (size_t)n * 8)) return rc;
    if (int rc = ensure(h, h->srCol, (size_t)(sr_halves(h) + 1) * D * 8)) return rc;
    if (int rc = upload(h, h->srY.p, yc.data(), (size_t)n * 8)) return rc;
    double* col = sr_direction_image(h);
    if (int rc = sr_colsum(h, D, 0, n, (const double*)h->srY.p, 1.0, col)) return rc;
    if (int rc = ensure_staging(h, (size_t)D * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, col, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    sr_gather(h->sr_sidx, (const double*)h->staging, out_direction);
    return RNNWF_OK;
}

static int sr_solve(rnnwf_handle* h, const SrEntry& e, double diag_shift, double* y) {
    if (!h) return RNNWF_ERR_INVALID;
    if (!y) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", e.name);
    if (int rc = sr_solve_common(h, e, diag_shift)) return rc;
    const int64_t n = sr_order(h);
    if (int rc = ensure_staging(h, (size_t)(n + 1) * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, sr_y(h), (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, h->stream));      // y | status
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    const long long status = ((const long long*)h->staging)[n];
    if (status) return sr_pivot_error(h, e.name, status, diag_shift);
    memcpy(y, h->staging, (size_t)n * 8);
    return RNNWF_OK;
}

// behind sr_direction_queue: the one synchronisation, the pivot status, the gather into flat order
static int sr_direction_finish(rnnwf_handle* h, const char* entry, double diag_shift, double* out_direction) {
    const int64_t D = sr_image_size(h);
    const double* col = sr_direction_image(h);
    if (int rc = ensure_staging(h, (size_t)(D + 1) * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, col, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync((double*)h->staging + D, sr_status(h), 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    const long long status = ((const long long*)h->staging)[D];
    if (status) return sr_pivot_error(h, entry, status, diag_shift);
    sr_gather(h->sr_sidx, (const double*)h->staging, out_direction);
    return RNNWF_OK;
}

static int sr_direction(rnnwf_handle* h, const SrEntry& e, double diag_shift, double* out_direction) {
    if (!h) return RNNWF_ERR_INVALID;
    if (!out_direction) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", e.name);
    if (int rc = sr_solve_common(h, e, diag_shift)) return rc;
    if (int rc = sr_direction_queue(h)) return rc;
    return sr_direction_finish(h, e.name, diag_shift, out_direction);
}

extern "C" int rnnwf_log_derivatives(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams) {
    return sr_log_derivatives(h, {"rnnwf_log_derivatives", kSrPositive}, out, ns, nparams);
}
extern "C" int rnnwf_sr_gram(rnnwf_handle* h, double* gram, double* eps) { return sr_gram(h, {"rnnwf_sr_gram", kSrPositive}, gram, eps); }
extern "C" int rnnwf_sr_apply(rnnwf_handle* h, const double* y, double* out_direction) {
    return sr_apply(h, {"rnnwf_sr_apply", kSrPositive}, y, out_direction);
}
extern "C" int rnnwf_sr_solve(rnnwf_handle* h, double diag_shift, double* y) { return sr_solve(h, {"rnnwf_sr_solve", kSrPositive}, diag_shift, y); }
extern "C" int rnnwf_sr_direction(rnnwf_handle* h, double diag_shift, double* out_direction) {
    return sr_direction(h, {"rnnwf_sr_direction", kSrPositive}, diag_shift, out_direction);
}

extern "C" int rnnwf_log_derivatives_complex(rnnwf_handle* h, double* out_re_im, int64_t ns, int64_t nparams) {
    return sr_log_derivatives(h, {"rnnwf_log_derivatives_complex", kSrComplex}, out_re_im, ns, nparams);
}
extern "C" int rnnwf_sr_gram_complex(rnnwf_handle* h, double* gram, double* eps) {
    return sr_gram(h, {"rnnwf_sr_gram_complex", kSrComplex}, gram, eps);
}
extern "C" int rnnwf_sr_apply_complex(rnnwf_handle* h, const double* y, double* out_direction) {
    return sr_apply(h, {"rnnwf_sr_apply_complex", kSrComplex}, y, out_direction);
}
extern "C" int rnnwf_sr_solve_complex(rnnwf_handle* h, double diag_shift, double* y) {
    return sr_solve(h, {"rnnwf_sr_solve_complex", kSrComplex}, diag_shift, y);
}
extern "C" int rnnwf_sr_direction_complex(rnnwf_handle* h, double diag_shift, double* out_direction) {
    return sr_direction(h, {"rnnwf_sr_direction_complex", kSrComplex}, diag_shift, out_direction);
}

extern "C" int rnnwf_log_derivatives_2d(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams) {
    return sr_log_derivatives(h, {"rnnwf_log_derivatives_2d", kSr2D}, out, ns, nparams);
}
extern "C" int rnnwf_sr_gram_2d(rnnwf_handle* h, double* gram, double* eps) { return sr_gram(h, {"rnnwf_sr_gram_2d", kSr2D}, gram, eps); }
extern "C" int rnnwf_sr_apply_2d(rnnwf_handle* h, const double* y, double* out_direction) {
    return sr_apply(h, {"rnnwf_sr_apply_2d", kSr2D}, y, out_direction);
}
extern "C" int rnnwf_sr_solve_2d(rnnwf_handle* h, double diag_shift, double* y) { return sr_solve(h, {"rnnwf_sr_solve_2d", kSr2D}, diag_shift, y); }
extern "C" int rnnwf_sr_direction_2d(rnnwf_handle* h, double diag_shift, double* out_direction) {
    return sr_direction(h, {"rnnwf_sr_direction_2d", kSr2D}, diag_shift, out_direction);
}

extern "C" int rnnwf_log_derivatives_lstm(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams) {
    return sr_log_derivatives(h, {"rnnwf_log_derivatives_lstm", kSrLstm}, out, ns, nparams);
}
extern "C" int rnnwf_sr_gram_lstm(rnnwf_handle* h, double* gram, double* eps) { return sr_gram(h, {"rnnwf_sr_gram_lstm", kSrLstm}, gram, eps); }
extern "C" int rnnwf_sr_apply_lstm(rnnwf_handle* h, const double* y, double* out_direction) {
    return sr_apply(h, {"rnnwf_sr_apply_lstm", kSrLstm}, y, out_direction);
}
extern "C" int rnnwf_sr_solve_lstm(rnnwf_handle* h, double diag_shift, double* y) {
    return sr_solve(h, {"rnnwf_sr_solve_lstm", kSrLstm}, diag_shift, y);
}
extern "C" int rnnwf_sr_direction_lstm(rnnwf_handle* h, double diag_shift, double* out_direction) {
    return sr_direction(h, {"rnnwf_sr_direction_lstm", kSrLstm}, diag_shift, out_direction);
}

// ---- the LSTM's resident batch (docs/sr_lstm.md, "The resident batch").  lstm_family() has no gradient hook, so rnnwf_vmc_step
// leaves an LSTM handle no batch and rnnwf_load_batch refuses it; these two entries are the only ones that set h->last_ns on one.
// Every place that overwrites h->bits, h->hck or h->eloc clears it (rnnwf_api.hip), and so does a commit.

// rnnwf_load_batch for the LSTM: the caller's samples packed into h->bits, the teacher-forced base pass with its (h, c) checkpoints,
// the caller's E_loc (float64) into h->eloc.  Everything is validated before anything is touched.
extern "C" int rnnwf_lstm_load_batch(rnnwf_handle* h, const int32_t* samples, int64_t ns, const double* eloc) {
    if (!h) return RNNWF_ERR_INVALID;
    const char* entry = "rnnwf_lstm_load_batch";
    if (int rc = sr_refuse(h, SrEntry{entry, kSrLstm})) return rc;
    if (int rc = sr_committed(h, entry)) return rc;
    if (ns < 1 || !samples || !eloc) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", entry);
    if (int rc = refuse_past_budget(h, ns, entry)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    h->last_ns = 0;
    h->call_ns = ns;
    if (int rc = upload_and_pack(h, samples, ns, h->bits, 0, nullptr)) return rc;
    if (int rc = lstm_teacher_base(h, ns)) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->eloc.p, eloc, (size_t)ns * 8, hipMemcpyHostToDevice, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    h->last_ns = ns;
    h->sr_valid = false;
    return RNNWF_OK;
}

// One minSR iteration's device work with one host synchronisation: the fused VMC step (its moments written into the step's pinned row,
// as rnnwf_lstm_vmc_gradient_step has them), then on its batch the Jacobian, the Gram matrix, the solve and dO^T y as
// rnnwf_sr_direction_lstm queues them.  The batch and its Jacobian stay resident.
extern "C" int rnnwf_sr_step_lstm(rnnwf_handle* h, int64_t numsamples, uint64_t seed, uint64_t step, int64_t sample_offset,
                                  const double* couplings, int64_t n_couplings, double diag_shift, double* moments, double* out_direction,
                                  int64_t nparams) {
    if (!h) return RNNWF_ERR_INVALID;
    const char* entry = "rnnwf_sr_step_lstm";
    if (int rc = sr_refuse(h, SrEntry{entry, kSrLstm})) return rc;
    if (int rc = sr_committed(h, entry)) return rc;
    if (numsamples < 1 || !couplings || !moments || !out_direction) return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments", entry);
    if (n_couplings != (int64_t)h->family->coupl_per_site * h->N + h->family->coupl_tail)
        return h->fail(RNNWF_ERR_INVALID, "%s: wrong number of couplings", entry);
    if (nparams != rnnwf_num_params(h))
        return h->fail(RNNWF_ERR_INVALID, "%s: the model has %lld parameters, caller passed %lld", entry, (long long)rnnwf_num_params(h),
                       (long long)nparams);
    if (h->nranks > 1 || h->reduce_in_step) return h->fail(RNNWF_ERR_INVALID, "%s: single process only", entry);
    if (int rc = sr_check_shift(h, entry, diag_shift)) return rc;
    if (int rc = sr_workspace(h, entry, numsamples, true)) return rc;
    if (int rc = refuse_past_budget(h, numsamples, entry)) return rc;
    // nothing was touched so far: a refused call leaves the resident batch and its Jacobian as they were
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    h->moments_direct = (double*)h->pinned_dev;
    const int rc_step = vmc_step(h, numsamples, Draw{seed, step, sample_offset}, couplings, nullptr, nullptr, nullptr);
    h->moments_direct = nullptr;
    if (rc_step) return rc_step;
    h->last_ns = numsamples;                                  // (vmc_step cleared sr_valid: keep_resident)
    if (int rc = sr_solve_queue(h, diag_shift)) return rc;
    if (int rc = sr_direction_queue(h)) return rc;
    if (int rc = sr_direction_finish(h, entry, diag_shift, out_direction)) return rc;
    memcpy(moments, h->pinned, 4 * sizeof(double));
    return RNNWF_OK;
}

// K whole minSR iterations with one host synchronisation (docs/sr.md, "Iterations on the device"): per iteration the fused VMC step,
// the Jacobian, the Gram matrix, the solve with diag_shifts[k] and dO^T y as rnnwf_sr_direction queues them, then train.hip's update
// theta <- theta - learning_rates[k] delta on the flat device parameters and the re-pack of every weight image.  The iteration's
// moments go to row k of train.hip's pinned table, its pivot status to h->srStat; from a bad pivot on nothing more is stored.
extern "C" int rnnwf_sr_train_steps(rnnwf_handle* h, int32_t K, int64_t numsamples, uint64_t seed, uint64_t step0, int64_t sample_offset,
                                    const double* couplings, int64_t n_couplings, const double* learning_rates, const double* diag_shifts,
                                    double* moments) {
    if (!h) return RNNWF_ERR_INVALID;
    const char* entry = "rnnwf_sr_train_steps";
    if (int rc = sr_refuse(h, SrEntry{entry, kSrPositive})) return rc;
    if (int rc = sr_committed(h, entry)) return rc;
    if (K < 1 || K > kSrMaxSteps || numsamples < 1 || !couplings || !learning_rates || !diag_shifts || !moments)
        return h->fail(RNNWF_ERR_INVALID, "%s: bad arguments (1 <= K <= %d)", entry, kSrMaxSteps);
    if (n_couplings != (int64_t)h->family->coupl_per_site * h->N + h->family->coupl_tail)
        return h->fail(RNNWF_ERR_INVALID, "%s: wrong number of couplings", entry);
    for (int k = 0; k < K; ++k) {
        if (int rc = sr_check_shift(h, entry, diag_shifts[k])) return rc;
        if (!std::isfinite(learning_rates[k])) return h->fail(RNNWF_ERR_INVALID, "%s: learning_rate must be finite", entry);
    }
    if (int rc = sr_workspace(h, entry, numsamples, true)) return rc;
    if (int rc = refuse_past_budget(h, numsamples, entry)) return rc;
    // nothing was touched so far: a refused call leaves the parameters, the resident batch and its Jacobian as they were
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    if (int rc = train_prepare(h)) return rc;
    const int64_t D = sr_image_size(h);
    if (int rc = sr_table(h, D)) return rc;                 // (its check: the flat table train.hip applies the direction through reads an image of D elements)
    if (int rc = ensure(h, h->srStat, (size_t)(kSrMaxSteps + 1) * 8)) return rc;
    if (int rc = ensure_staging(h, (size_t)(kSrMaxSteps + 1) * 8)) return rc;
    long long* stat = (long long*)h->srStat.p;
    RNNWF_HIP(h, hipMemsetAsync(stat, 0, (size_t)(K + 1) * 8, h->stream));
    int rc = 0;
    for (int k = 0; k < K && !rc; ++k) {
        h->moments_direct = (double*)h->train.mom_host_dev + 4 * k;      // as rnnwf_train_steps: the moments kernel writes the pinned row itself
        rc = vmc_step(h, numsamples, Draw{seed, step0 + (uint64_t)k, sample_offset}, couplings, nullptr, nullptr, nullptr);
        h->moments_direct = nullptr;
        if (!rc) rc = sr_solve_queue(h, diag_shifts[k]);
        if (!rc) rc = timed_launch(h, kTimerGemm, sr_record_status_kernel, 1, 64, 0, (const long long*)sr_status(h), k, stat);
        if (!rc) rc = sr_direction_queue(h);
        if (!rc) rc = train_apply_direction(h, sr_direction_image(h), (size_t)D, learning_rates[k], stat);
        h->sr_valid = false;                                               // the Jacobian belongs to the parameters before the update
    }
    if (!rc && hipMemcpyAsync(h->staging, stat, (size_t)(K + 1) * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = h->fail(RNNWF_ERR_HIP, "%s: status download failed", entry);
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = h->fail(RNNWF_ERR_HIP, "%s: stream synchronisation failed", entry);
    h->last_ns = 0;                       // the resident batch belongs to the weights before the last update
    if (rc) return rc;
    memcpy(moments, h->train.mom_host, (size_t)K * 4 * sizeof(double));
    const long long* st = (const long long*)h->staging;
    if (st[0]) {
        const int k = (int)st[0] - 1;
        char where[64];
        snprintf(where, sizeof where, "%s: iteration %d", entry, k);
        return sr_pivot_error(h, where, st[1 + k], diag_shifts[k]);
    }
    return RNNWF_OK;
}
