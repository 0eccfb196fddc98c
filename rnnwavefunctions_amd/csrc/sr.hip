// sr.hip - stochastic reconfiguration (docs/sr.md): rnnwf_log_derivatives, rnnwf_sr_gram, rnnwf_sr_apply on the resident batch of the
// one-layer positive GRU (GRU1D, GRU1D_F64; up to 68 units).  The per-sample log-derivatives J[ns][D] stay on the device in the order
// of the gradient image (grad.hip) and are read through the table grad_flat_probe builds; the ns x ns solve is the caller's.
#include <cmath>

#include "sr_kernels.h"
#include "models.h"

using namespace rnnwf;

namespace {

constexpr int64_t kSrMaxSamples = 4096;

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
            else if (h->NFULL > 4) why = "not implemented for layers wider than 68 units";
            else if (h->comm) why = "not implemented for a handle with a communicator";
    }
    return why ? h->fail(RNNWF_ERR_INVALID, "%s: %s", entry, why) : 0;
}

template <class Fn>
int with_sr_shape(rnnwf_handle* h, Fn&& fn) {
    const bool f64 = h->model == RNNWF_MODEL_GRU1D_F64;
    switch (h->NFULL) {
        case 1: return f64 ? fn(SrShape<double, 1>()) : fn(SrShape<float, 1>());
        case 2: return f64 ? fn(SrShape<double, 2>()) : fn(SrShape<float, 2>());
        case 3: return f64 ? fn(SrShape<double, 3>()) : fn(SrShape<float, 3>());
        case 4: return f64 ? fn(SrShape<double, 4>()) : fn(SrShape<float, 4>());
    }
    return h->fail(RNNWF_ERR_INVALID, "stochastic reconfiguration: no kernel for NFULL=%d", h->NFULL);
}

int64_t sr_image_size(rnnwf_handle* h) {
    int64_t D = 0;
    with_sr_shape(h, [&](auto s) { D = decltype(s)::D; return 0; });
    return D;
}

// refusals, then the state checks every entry point shares
int sr_ready(rnnwf_handle* h, const char* entry) {
    if (int rc = sr_refuse(h, entry)) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "%s: parameters not committed (call rnnwf_commit_params)", entry);
    if (h->last_ns <= 0) return h->fail(RNNWF_ERR_STATE, "%s: call rnnwf_vmc_step first (its samples, states and E_loc are reused)", entry);
    const int64_t ns = h->last_ns;
    const size_t es = h->f64 ? 8 : 4;
    const size_t need = (size_t)ns * (size_t)sr_image_size(h) * es + (size_t)ns * ns * 8;
    if (ns > kSrMaxSamples || need > state_budget_bytes(h, kDefaultStateBudget))
        return h->fail(RNNWF_ERR_NOMEM, "%s: ns too large for the SR workspace (%lld samples: Jacobian + Gram matrix take %zu bytes; at most %lld samples)",
                       entry, (long long)ns, need, (long long)kSrMaxSamples);
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
    if (!h->wbwd_valid) {                                  // the backward image, as grad_device packs it
        std::vector<char> img;
        if (int rc = h->family->gradient->pack(h, &img)) return rc;
        if (int rc = ensure(h, h->wbwd, img.size())) return rc;
        if (int rc = upload(h, h->wbwd.p, img.data(), img.size())) return rc;
        h->wbwd_valid = true;
    }
    if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * sizeof(T))) return rc;
    if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * sizeof(T))) return rc;
    if (int rc = ensure(h, h->srHead, (size_t)ns * G::HEAD_ROW * sizeof(T))) return rc;
    if (int rc = ensure(h, h->srJ, (size_t)ns * S::D * sizeof(T))) return rc;
    GradArgs a{};
    a.wimg = h->wimg.p;
    a.wbwd = h->wbwd.p;
    a.N = N; a.ns = ns; a.nsb = nsb;
    a.bits = (const uint32_t*)h->bits.p;
    a.hck = h->hck.p;
    a.P = h->gradP.p;
    a.Q = h->gradQ.p;
    a.head_part = h->srHead.p;                             // [ns][HEAD_ROW]: one row per chain (gru_bwd_kernel<SR>)
    a.hck_nl = 1;
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
