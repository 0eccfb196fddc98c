// sr.hip - stochastic reconfiguration (docs/sr.md): rnnwf_log_derivatives, rnnwf_sr_gram, rnnwf_sr_apply, rnnwf_sr_solve,
// rnnwf_sr_direction on the resident batch of the one-layer positive GRU (GRU1D, GRU1D_F64; up to 68 units), and rnnwf_sr_train_steps,
// K whole minSR iterations on batches it draws itself (the update and the images' re-pack are train.hip's).  The per-sample
// log-derivatives J[ns][D] stay on the device in the order of the gradient image (grad.hip) and are read through the table
// grad_flat_probe builds; the ns x ns solve is the caller's (rnnwf_sr_gram + rnnwf_sr_apply) or the device's (rnnwf_sr_solve,
// rnnwf_sr_direction: blocked f64 Cholesky, sr_solve_kernels.h).
#include <cmath>
#include <cstring>

#include "sr_kernels.h"
#include "sr_solve_kernels.h"
#include "models.h"
#include "shapes.h"
#include "tn_gemm.h"

using namespace rnnwf;

namespace {

constexpr int64_t kSrMaxSamples = 4096;
constexpr int kSrMaxNFULL = 4;             // up to 68 units
constexpr int kSrMaxSteps = 1024;          // iterations of one rnnwf_sr_train_steps call: the rows of train.hip's pinned moments table (kMaxSteps)

// 0, or RNNWF_ERR_INVALID "<entry>: <why>" for a handle these entry points do not serve; called before anything is touched
int sr_refuse(rnnwf_handle* h, const char* entry) {
    const char* why = nullptr;
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

// fn(SrShape<T, NFULL>()) for the handle's row among the one-layer rows of the positive GRU's table up to kSrMaxNFULL (shapes.h)
template <class R> struct SrRow : std::bool_constant<R::NL == 1 && R::NFULL <= kSrMaxNFULL> {};
template <class Fn>
int with_sr_shape(rnnwf_handle* h, Fn&& fn) {
    int rc = 0;
    if (with_row<SrRow>(GruKernels(), h, [&](auto r) { rc = fn(SrShape<typename decltype(r)::T, decltype(r)::NFULL>()); })) return rc;
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
    // the factor's workspace: ns^2 doubles, eps, y, the status word and the diagonal blocks (sr_solve_device), all counted
    const size_t nb = (size_t)(ns + kSrNB - 1) / kSrNB;
    const size_t fac = factor ? ((size_t)ns * ns + 2 * (size_t)ns + 1 + nb * kSrNB * kSrNB) * 8 : 0;
    const size_t need = (size_t)ns * (size_t)sr_image_size(h) * es + (size_t)ns * ns * 8 + fac;
    if (ns > kSrMaxSamples || need > state_budget_bytes(h, kDefaultStateBudget))
        return h->fail(RNNWF_ERR_NOMEM, "%s: ns too large for the SR workspace (%lld samples: Jacobian + Gram matrix%s take %zu bytes; at most %lld samples)",
                       entry, (long long)ns, factor ? " + Cholesky factor" : "", need, (long long)kSrMaxSamples);
    return 0;
}

int sr_committed(rnnwf_handle* h, const char* entry) {
    return h->committed ? 0 : h->fail(RNNWF_ERR_STATE, "%s: parameters not committed (call rnnwf_commit_params)", entry);
}

// refusals, then the state checks every entry point on the resident batch shares; `factor`: the entry also holds the ns x ns Cholesky factor
int sr_ready(rnnwf_handle* h, const char* entry, bool factor = false) {
    if (int rc = sr_refuse(h, entry)) return rc;
    if (int rc = sr_committed(h, entry)) return rc;
    if (h->last_ns <= 0) return h->fail(RNNWF_ERR_STATE, "%s: call rnnwf_vmc_step first (its samples, states and E_loc are reused)", entry);
    if (int rc = sr_workspace(h, entry, h->last_ns, factor)) return rc;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    return 0;
}

// the flat-order table and, on the device, how many parameters read each image element (0: padding)
int sr_table(rnnwf_handle* h, int64_t D) {
    if (!h->sr_sidx.empty()) return 0;
    std::vector<int32_t> sidx;
    GradImage im;
    if (int rc = grad_flat_probe(h, sidx, &im)) return rc;
    if ((int64_t)im.count != D || im.f64 != h->f64) return h->fail(RNNWF_ERR_INVALID, "stochastic reconfiguration: gradient image of %zu elements, expected %lld", im.count, (long long)D);
    std::vector<uint8_t> used((size_t)D, 0);
    for (int32_t v : sidx)
        if (v) ++used[(size_t)std::abs(v) - 1];
    if (int rc = ensure(h, h->srMask, (size_t)D)) return rc;
    if (int rc = upload(h, h->srMask.p, used.data(), (size_t)D)) return rc;
    h->sr_sidx = std::move(sidx);
    return 0;
}

template <typename T, int NFULL>
int sr_build_shape(rnnwf_handle* h) {
    using S = SrShape<T, NFULL>;
    using G = typename S::G;
    using L = GruLayout<T, NFULL, 1>;
    const int N = h->N;
    const int64_t ns = h->last_ns, R = ns * N, nsb = (ns + kChains - 1) / kChains;
    if (int rc = sr_table(h, S::D)) return rc;
    if (int rc = grad_bwd_image(h)) return rc;
    if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * sizeof(T))) return rc;
    if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * sizeof(T))) return rc;
    if (int rc = ensure(h, h->srHead, (size_t)ns * G::HEAD_ROW * sizeof(T))) return rc;
    if (int rc = ensure(h, h->srJ, (size_t)ns * S::D * sizeof(T))) return rc;
    GradArgs a{};
    grad_batch_args(h, &a);                                // (one layer: sr_refuse)
    a.wimg = h->wimg.p;
    a.head_part = h->srHead.p;                             // [ns][HEAD_ROW]: one row per chain (gru_bwd_kernel<SR>)
    constexpr size_t lds = L::LDS_BYTES + (GradStream<T, NFULL, 1>::value ? 0 : G::BWD_BYTES);
    static_assert(lds <= 160 * 1024, "forward + backward weight images exceed the LDS");
    if (int rc = launch_persistent(h, kTimerBackprop, gru_bwd_kernel<T, NFULL, 4, 1, false, true>, 4 * 64, lds, nsb, 4, a)) return rc;
    if (int rc = launch_persistent(h, kTimerGemm, sr_outer_kernel<T, NFULL>, S::WAVES * 64, 0, ns, 1, (const T*)h->gradP.p, (const T*)h->gradQ.p,
                                   (const T*)h->srHead.p, (const uint8_t*)h->srMask.p, N, ns, (T*)h->srJ.p))
        return rc;
    h->sr_ns = ns;
    h->sr_valid = true;
    return 0;
}

// J for the resident batch and the committed parameters, built when it is stale
int sr_build(rnnwf_handle* h) {
    if (h->sr_valid && h->sr_ns == h->last_ns) return 0;
    h->sr_valid = false;
    return with_sr_shape(h, [&](auto s) { return sr_build_shape<typename decltype(s)::Elem, decltype(s)::NF>(h); });
}

template <typename T>
int sr_colsum(rnnwf_handle* h, int64_t D, const double* w, double scale, double* out) {
    return launch_persistent(h, kTimerGemm, sr_colsum_kernel<T>, 256, 0, (D + 63) / 64, 1, (const T*)h->srJ.p, h->sr_ns, D, w, scale, out);
}

// the column mean and the centred Gram matrix of the resident Jacobian, into h->srCol[0 .. D) and h->srGram
int sr_gram_device(rnnwf_handle* h) {
    const int64_t ns = h->sr_ns, D = sr_image_size(h);
    if (int rc = ensure(h, h->srCol, (size_t)2 * D * 8)) return rc;
    if (int rc = ensure(h, h->srGram, (size_t)ns * ns * 8)) return rc;
    double* mean = (double*)h->srCol.p;
    if (int rc = h->f64 ? sr_colsum<double>(h, D, nullptr, 1.0 / (double)ns, mean) : sr_colsum<float>(h, D, nullptr, 1.0 / (double)ns, mean)) return rc;
    const int64_t nb = (ns + 31) / 32, nblocks = nb * (nb + 1) / 2;
    if (int rc = h->f64 ? launch_persistent(h, kTimerGemm, sr_gram_kernel<double>, 256, 0, nblocks, 1, (const double*)h->srJ.p, (const double*)mean,
                                            (const uint8_t*)h->srMask.p, ns, D, nblocks, (double*)h->srGram.p)
                        : launch_persistent(h, kTimerGemm, sr_gram_kernel<float>, 256, 0, nblocks, 1, (const float*)h->srJ.p, (const double*)mean,
                                            (const uint8_t*)h->srMask.p, ns, D, nblocks, (double*)h->srGram.p))
        return rc;
    return 0;
}

// (gram + ns diag_shift I) y = eps on the device: eps from the resident local energies into the eps row of the workspace, per
// panel the diagonal factorisation + panel solve and the trailing update, then the backward sweep.  Leaves y and the pivot
// status word behind the eps row (sr_y / sr_status), the factors of the diagonal blocks behind those; nothing is synchronised here.
double* sr_y(rnnwf_handle* h) { return (double*)h->srFac.p + (size_t)h->sr_ns * h->sr_ns + (size_t)h->sr_ns; }
long long* sr_status(rnnwf_handle* h) { return (long long*)(sr_y(h) + h->sr_ns); }

int sr_solve_device(rnnwf_handle* h, double diag_shift) {
    const int64_t ns = h->sr_ns;
    const int nb = (int)((ns + kSrNB - 1) / kSrNB);
    if (int rc = ensure(h, h->srFac, ((size_t)ns * ns + 2 * (size_t)ns + 1 + (size_t)nb * kSrNB * kSrNB) * 8)) return rc;
    double* F = (double*)h->srFac.p;
    double* Ld = (double*)(sr_status(h) + 1);                // the factorised diagonal blocks
    const double* gram = (const double*)h->srGram.p;
    const double shift = (double)ns * diag_shift;
    if (int rc = timed_launch(h, kTimerGemm, sr_centre_kernel, 1, 256, 0, (const double*)h->eloc.p, ns, F + (size_t)ns * ns, sr_status(h))) return rc;
    for (int k = 0; k < nb; ++k) {
        const double* src = k == 0 ? gram : F;
        if (int rc = launch_persistent(h, kTimerGemm, sr_chol_panel_kernel, 256, 0, nb - k, 1, src, F, ns, k, shift, Ld, sr_status(h))) return rc;
        const int64_t m = nb - k - 1, nitems = m * (m + 1) / 2 + m;
        if (nitems > 0)
            if (int rc = launch_persistent(h, kTimerGemm, sr_chol_update_kernel, 256, 0, nitems, 1, src, F, ns, k, nitems)) return rc;
    }
    for (int k = nb - 1; k >= 0; --k)
        if (int rc = launch_persistent(h, kTimerGemm, sr_chol_back_kernel, 64, 0, k + 1, 1, F, (const double*)Ld, ns, k, sr_y(h))) return rc;
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

int sr_solve_common(rnnwf_handle* h, const char* entry, double diag_shift) {
    if (int rc = sr_check_shift(h, entry, diag_shift)) return rc;
    if (int rc = sr_ready(h, entry, true)) return rc;
    return sr_solve_queue(h, diag_shift);
}

// behind sr_solve_queue: dO^T y = J^T (y - mean y), as rnnwf_sr_apply, with the centring on the device; the direction's image is
// left in sr_direction_image(h), nothing is synchronised
double* sr_direction_image(rnnwf_handle* h) { return (double*)h->srCol.p + sr_image_size(h); }

int sr_direction_queue(rnnwf_handle* h) {
    const int64_t ns = h->sr_ns, D = sr_image_size(h);
    if (int rc = ensure(h, h->srY, (size_t)ns * 8)) return rc;
    if (int rc = timed_launch(h, kTimerGemm, sr_centre_kernel, 1, 256, 0, (const double*)sr_y(h), ns, (double*)h->srY.p, (long long*)nullptr)) return rc;
    double* col = sr_direction_image(h);
    return h->f64 ? sr_colsum<double>(h, D, (const double*)h->srY.p, 1.0, col) : sr_colsum<float>(h, D, (const double*)h->srY.p, 1.0, col);
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

extern "C" int rnnwf_log_derivatives(rnnwf_handle* h, double* out, int64_t ns, int64_t nparams) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, "rnnwf_log_derivatives")) return rc;
    if (out && (ns != h->last_ns || nparams != rnnwf_num_params(h)))
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_log_derivatives: the resident batch has %lld samples and the model %lld parameters, caller passed %lld and %lld",
                       (long long)h->last_ns, (long long)rnnwf_num_params(h), (long long)ns, (long long)nparams);
    if (int rc = sr_build(h)) return rc;
    if (!out) return RNNWF_OK;
    const int64_t D = sr_image_size(h);
    const size_t bytes = (size_t)h->sr_ns * D * (h->f64 ? 8 : 4);
    if (int rc = ensure_staging(h, bytes)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, h->srJ.p, bytes, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t s = 0; s < h->sr_ns; ++s) {
        if (h->f64) sr_gather(h->sr_sidx, (const double*)h->staging + s * D, out + s * nparams);
        else sr_gather(h->sr_sidx, (const float*)h->staging + s * D, out + s * nparams);
    }
    return RNNWF_OK;
}

extern "C" int rnnwf_sr_gram(rnnwf_handle* h, double* gram, double* eps) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, "rnnwf_sr_gram")) return rc;
    if (!gram || !eps) return h->fail(RNNWF_ERR_INVALID, "rnnwf_sr_gram: bad arguments");
    if (int rc = sr_build(h)) return rc;
    if (int rc = sr_gram_device(h)) return rc;
    const int64_t ns = h->sr_ns;
    RNNWF_HIP(h, hipMemcpyAsync(gram, h->srGram.p, (size_t)ns * ns * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync(eps, h->eloc.p, (size_t)ns * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    double sum = 0.0;
    for (int64_t s = 0; s < ns; ++s) sum += eps[s];
    const double mean_e = sum / (double)ns;
    for (int64_t s = 0; s < ns; ++s) eps[s] -= mean_e;
    return RNNWF_OK;
}

extern "C" int rnnwf_sr_apply(rnnwf_handle* h, const double* y, double* out_direction) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = sr_ready(h, "rnnwf_sr_apply")) return rc;
    if (!y || !out_direction) return h->fail(RNNWF_ERR_INVALID, "rnnwf_sr_apply: bad arguments");
    if (int rc = sr_build(h)) return rc;
    const int64_t ns = h->sr_ns, D = sr_image_size(h);
    // dO^T y = J^T (y - mean y): the centring moves from the ns x D matrix to the ns weights
    double sum = 0.0;
    for (int64_t s = 0; s < ns; ++s) sum += y[s];
    std::vector<double> yc((size_t)ns);
    for (int64_t s = 0; s < ns; ++s) yc[(size_t)s] = y[s] - sum / (double)ns;
    if (int rc = ensure(h, h->srY, (size_t)ns * 8)) return rc;
    if (int rc = ensure(h, h->srCol, (size_t)2 * D * 8)) return rc;
    if (int rc = upload(h, h->srY.p, yc.data(), (size_t)ns * 8)) return rc;
    double* col = (double*)h->srCol.p + D;
    if (int rc = h->f64 ? sr_colsum<double>(h, D, (const double*)h->srY.p, 1.0, col) : sr_colsum<float>(h, D, (const double*)h->srY.p, 1.0, col)) return rc;
    if (int rc = ensure_staging(h, (size_t)D * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, col, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    sr_gather(h->sr_sidx, (const double*)h->staging, out_direction);
    return RNNWF_OK;
}

extern "C" int rnnwf_sr_solve(rnnwf_handle* h, double diag_shift, double* y) {
    if (!h) return RNNWF_ERR_INVALID;
    if (!y) return h->fail(RNNWF_ERR_INVALID, "rnnwf_sr_solve: bad arguments");
    if (int rc = sr_solve_common(h, "rnnwf_sr_solve", diag_shift)) return rc;
    const int64_t ns = h->sr_ns;
    if (int rc = ensure_staging(h, (size_t)(ns + 1) * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, sr_y(h), (size_t)(ns + 1) * 8, hipMemcpyDeviceToHost, h->stream));      // y | status
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    const long long status = ((const long long*)h->staging)[ns];
    if (status) return sr_pivot_error(h, "rnnwf_sr_solve", status, diag_shift);
    memcpy(y, h->staging, (size_t)ns * 8);
    return RNNWF_OK;
}

extern "C" int rnnwf_sr_direction(rnnwf_handle* h, double diag_shift, double* out_direction) {
    if (!h) return RNNWF_ERR_INVALID;
    if (!out_direction) return h->fail(RNNWF_ERR_INVALID, "rnnwf_sr_direction: bad arguments");
    if (int rc = sr_solve_common(h, "rnnwf_sr_direction", diag_shift)) return rc;
    if (int rc = sr_direction_queue(h)) return rc;
    const int64_t D = sr_image_size(h);
    const double* col = sr_direction_image(h);
    if (int rc = ensure_staging(h, (size_t)(D + 1) * 8)) return rc;
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, col, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipMemcpyAsync((double*)h->staging + D, sr_status(h), 8, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    const long long status = ((const long long*)h->staging)[D];
    if (status) return sr_pivot_error(h, "rnnwf_sr_direction", status, diag_shift);
    sr_gather(h->sr_sidx, (const double*)h->staging, out_direction);
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
    if (int rc = sr_refuse(h, entry)) return rc;
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
