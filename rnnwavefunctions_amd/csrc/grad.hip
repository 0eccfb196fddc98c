// grad.hip - host side of the VMC-cost gradient: the shared driver (grad_device, grad_bwd_image), rnnwf_vmc_gradient,
// the flat-gradient probe, rnnwf_get_grad / rnnwf_get_grads_flat, and the gradient hooks (models.h: Gradient) of the GRU RNNs
// (f32 1D positive / parity / complex, f64 2D-lattice GRU; one layer or a stack).  The 2D RNN's hooks live in mdrnn.hip.
// Every layer's backward image comes from pack_bwd_side, every layer's tensors from unpack_cell, every backward pass - the 2D RNN's
// too - is launched by backward_launch (tn_gemm.h).
#include <algorithm>

#include "grad_kernels.h"
#include "tn_gemm.h"
#include "ml_grad_kernels.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

// One backward operand [NTO][KBG][64] x 16 B at A: in the A fragment of output tile t (hidden unit kout receives dL/dh), k-step
// kk = (gate g, unit quad kt) holds weight(g, kout, u), the weight from pre-activation (gate g, unit u) back to unit kout.
// S: double, or Lin - the device re-pack tables of train.hip are this code run over Lin (pack_value.h).
template <typename T, int NFULL, class S, class W>
void pack_bwd_side(T* A, int H, W&& weight) {
    using G = GradLayout<NFULL, T>;
    for (int t = 0; t < G::NTO; ++t)
        for (int row = 0; row < 16; ++row) {
            int q, r;
            row_to_qr<T>(row, q, r);
            if (t == NFULL && r != 0) continue;
            const int kout = t < NFULL ? 16 * t + 4 * r + q : 16 * NFULL + q;
            if (kout >= H) continue;
            for (int kq = 0; kq < 4; ++kq) {
                const int lane = (kq << 4) | row;
                for (int kk = 0; kk < G::KB; ++kk) {
                    const int g = kk / G::KT, kt = kk % G::KT, u = 4 * kt + kq;
                    if (u >= H) continue;
                    PackSink<S>::put(&A[(((size_t)t * G::KBG + kk / G::VW) * 64 + lane) * G::VW + (kk % G::VW)], weight(g, kout, u));
                }
            }
        }
}

// One GRU cell's tensors (TF names under `pre`) from its dW image [PCOLS][qcols]: unit u's P rows (gate tiles, dy tiles) against
// the Q columns of the `nin` input rows (xcol(i)), of the recurrent state (hoff + col_of_unit) and of the constant 1 (onecol).
template <typename T, int NFULL, class XCol>
void unpack_cell(rnnwf_handle* h, const T* dW, int qcols, const std::string& pre, int nin, XCol&& xcol, int hoff, int onecol) {
    const int H = h->H;
    constexpr int NT = GradLayout<NFULL, T>::NT;
    auto at = [&](int prow, int col) { return (double)dW[(size_t)prow * qcols + col]; };
    auto& gWg = h->grads[pre + "gates/kernel"];
    auto& gbg = h->grads[pre + "gates/bias"];
    auto& gWci = h->grads[pre + "candidate/input_projection/kernel"];
    auto& gbci = h->grads[pre + "candidate/input_projection/bias"];
    auto& gWch = h->grads[pre + "candidate/hidden_projection/kernel"];
    auto& gbch = h->grads[pre + "candidate/hidden_projection/bias"];
    gWg.assign((size_t)(nin + H) * 2 * H, 0.0); gbg.assign(2 * H, 0.0);
    gWci.assign((size_t)nin * H, 0.0); gbci.assign(H, 0.0);
    gWch.assign((size_t)H * H, 0.0); gbch.assign(H, 0.0);
    for (int u = 0; u < H; ++u) {
        const int m = u / 16, r = (u % 16) / 4, q = u % 4;
        const bool full = u < 16 * NFULL;
        const int uq = u - 16 * NFULL;                       // remainder units: lane quarter = uq
        int prow[3];
        for (int g = 0; g < 3; ++g) prow[g] = full ? (g * NFULL + m) * 16 + 4 * q + r : (NT - 1) * 16 + 4 * uq + g;
        const int prow_y = full ? (NT + m) * 16 + 4 * q + r : (NT + NFULL) * 16 + 4 * uq;
        for (int k = 0; k < H; ++k) {
            const int ch = hoff + col_of_unit(NFULL, k);
            gWg[(size_t)(nin + k) * 2 * H + u] = at(prow[0], ch);
            gWg[(size_t)(nin + k) * 2 * H + H + u] = at(prow[1], ch);
            gWch[(size_t)k * H + u] = at(prow[2], ch);
        }
        for (int i = 0; i < nin; ++i) {
            gWg[(size_t)i * 2 * H + u] = at(prow[0], xcol(i));
            gWg[(size_t)i * 2 * H + H + u] = at(prow[1], xcol(i));
            gWci[(size_t)i * H + u] = at(prow_y, xcol(i));
        }
        gbg[u] = at(prow[0], onecol);
        gbg[H + u] = at(prow[1], onecol);
        gbch[u] = at(prow[2], onecol);
        gbci[u] = at(prow_y, onecol);
    }
}

template <typename T, int NFULL, int WAVES, int NOUT>
struct GLaunch {
    using L = GruLayout<T, NFULL, NOUT>;
    using G = GradLayout<NFULL, T>;
    static constexpr bool STREAM = GradStream<T, NFULL, NOUT>::value;       // backward operand read through L2 (grad_kernels.h)
    static constexpr size_t LDS = L::LDS_BYTES + (STREAM ? 0 : G::BWD_BYTES);

    template <class S = double>
    static std::vector<char> pack_bwd(const rnnwf_handle* h) {
        const size_t H = h->H;
        std::vector<char> img(G::BWD_BYTES, 0);
        PackSink<S>::begin(img);
        const std::string pre = kGruPre;
        const auto Wg = pvs<S>(h, pre + "gates/kernel");                         // [2+H, 2H]
        const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");  // [H, H]
        pack_bwd_side<T, NFULL, S>(reinterpret_cast<T*>(img.data()), h->H, [&](int g, int kout, int u) -> S {
            if (g == 2) return Wch[kout * H + u];
            return Wg[(2 + kout) * 2 * H + g * H + u];
        });
        return img;
    }

    // the wide shapes' kernels live in grad_wide.hip's translation unit (see there)
    static constexpr bool WIDE = kGradWide<T, NFULL>;
    static_assert(!WIDE || WAVES == kGradWaves, "grad_wide.hip instantiates its kernels at kGradWaves waves per workgroup");
    static GradKernel kernel(const rnnwf_handle* h) {
        if constexpr (WIDE) return grad_wide_kernel(h);
        else return gru_bwd_kernel<T, NFULL, WAVES, NOUT>;
    }

    // small batches: two waves per block of 16 chains (grad_kernels.h: GradPair) while every pair still gets SIMDs of its own
    static constexpr bool PAIR_OK = !WIDE && std::is_same<T, float>::value && WAVES == 4 && GradPair<T, NFULL, NOUT>::FITS;

    // one pass of `kern` (per_wg 16-chain blocks per workgroup), then dW += P^T Q
    static int run_kernel(rnnwf_handle* h, GradKernel kern, int threads, size_t lds, int per_wg, const GradArgs& a, int64_t R, void* dW) {
        if (int rc = backward_launch<T>(h, kern, threads, lds, a.nsb, per_wg, NOUT * G::HEAD_ROW, (T*)a.head_grad, a)) return rc;
        return tn_gemm_launch<T, G::PCOLS / 16, G::QCOLS / 16>(h, (const T*)a.P, (const T*)a.Q, R, (T*)dW);
    }
    static int run(rnnwf_handle* h, const GradArgs& a, int64_t R, void* dW) {
        if constexpr (PAIR_OK) {
            using GP = GradPair<T, NFULL, NOUT>;
            if (a.nsb <= (int64_t)GP::NB * h->cu_count && !h->knobs.no_coop)
                return run_kernel(h, gru_bwd_kernel<T, NFULL, 2 * GP::NB, NOUT, true>, 2 * GP::NB * 64, GP::LDS, GP::NB, a, R, dW);
        }
        if (LDS > 160 * 1024)
            return h->fail(RNNWF_ERR_INVALID, "rnnwf_vmc_gradient: forward + backward weight images (%zu B) exceed the 160 KB LDS", LDS);
        return run_kernel(h, kernel(h), WAVES * 64, LDS, WAVES, a, R, dW);
    }

    // dW image [PCOLS][QCOLS] + head gradients -> TF-named gradient arrays
    static void unpack(rnnwf_handle* h, const void* dW_, size_t head_off) {
        const T* dW = (const T*)dW_;
        const T* hg = dW + head_off;
        const int H = h->H;
        unpack_cell<T, NFULL>(h, dW, G::QCOLS, kGruPre, 2, [](int sgm) { return 16 * NFULL + 1 + sgm; }, 0, 16 * NFULL + 3);
        const char* amp = NOUT == 1 ? "wf_dense" : "wf_dense_ampl";
        auto& gWd = h->grads[std::string(amp) + "/kernel"];
        auto& gbd = h->grads[std::string(amp) + "/bias"];
        gWd.assign((size_t)H * 2, 0.0); gbd.assign(2, 0.0);
        std::vector<double>* gWp = nullptr;
        std::vector<double>* gbp = nullptr;
        if (NOUT == 3) {
            gWp = &h->grads["wf_dense_phase/kernel"];
            gbp = &h->grads["wf_dense_phase/bias"];
            gWp->assign((size_t)H * 2, 0.0);
            gbp->assign(2, 0.0);
        }
        for (int u = 0; u < H; ++u) {
            // head: the image holds the logit difference z1 - z0, so d/dWd[:,1] = +v and d/dWd[:,0] = -v
            const double v = hg[u];          // slot 4 kt + q == unit index
            gWd[(size_t)u * 2 + 1] = v;
            gWd[(size_t)u * 2] = -v;
            if (NOUT == 3) {
                (*gWp)[(size_t)u * 2] = hg[G::HEAD_ROW + u];
                (*gWp)[(size_t)u * 2 + 1] = hg[2 * G::HEAD_ROW + u];
            }
        }
        gbd[1] = hg[4 * G::KT];
        gbd[0] = -hg[4 * G::KT];
        if (NOUT == 3) {
            (*gbp)[0] = hg[G::HEAD_ROW + 4 * G::KT];
            (*gbp)[1] = hg[2 * G::HEAD_ROW + 4 * G::KT];
        }
    }
};

// ---- the GRU's gradient: one backward pass per layer, top first (ml_grad_kernels.h); one layer is a stack of one -------------
// NOUT = 1: positive RNN; NOUT = 3: complex RNN (heads on the top layer, complex weights w_s as in gru_bwd_kernel).
// T = float, or double for the 2D-lattice GRU (NOUT = 1).  The upper layers' code is compiled for NL > 1 only: no upper-layer
// kernel at a width that has no stack.
template <int NFULL, int NL, int WAVES, int NOUT = 1, typename T = float>
struct MLGrad {
    using G0 = GLaunch<T, NFULL, WAVES, NOUT>;
    using L0 = GruLayout<T, NFULL, NOUT>;
    using U = UpperLayout<NFULL, T>;
    using GU = UpperGradLayout<NFULL, NOUT, T>;
    static constexpr size_t ES = sizeof(T);
    static constexpr size_t DW0 = (size_t)G0::G::PCOLS * G0::G::QCOLS;     // elements
    static constexpr size_t HEAD = (size_t)NOUT * G0::G::HEAD_ROW;
    static constexpr size_t DWU = (size_t)GU::PCOLS * GU::QCOLS;
    static constexpr size_t DW_FLOATS = DW0 + HEAD + (NL - 1) * DWU;       // [dW layer 0 | head | dW layer 1 | ...]
    // a stack's layer-0 pass has no head term: it adds its zeros into a scratch head row past the result
    static constexpr size_t DW_ALLOC = DW_FLOATS + (NL > 1 ? HEAD : 0);

    static GradImage layout() { return {std::is_same<T, double>::value, DW_FLOATS, DW_ALLOC}; }

    template <class S = double>
    static std::vector<char> pack_upper_bwd(const rnnwf_handle* h, int layer) {
        const size_t H = h->H;
        std::vector<char> img(GU::BWD_BYTES, 0);
        PackSink<S>::begin(img);
        const std::string pre = "multi_rnn_cell/cell_" + std::to_string(layer) + "/cudnn_compatible_gru_cell/";
        const auto Wg = pvs<S>(h, pre + "gates/kernel");                         // [H + H, 2H]
        const auto Wci = pvs<S>(h, pre + "candidate/input_projection/kernel");   // [H, H]
        const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");  // [H, H]
        for (int side = 0; side < 2; ++side)                                  // 0: H side (-> dh), 1: X side (-> dx)
            pack_bwd_side<T, NFULL, S>(reinterpret_cast<T*>(img.data() + side * GU::SIDE_BYTES), h->H, [&](int g, int kout, int u) -> S {
                if (g == 2) return (side == 0 ? Wch : Wci)[kout * H + u];
                return Wg[((side == 0 ? H : 0) + kout) * 2 * H + g * H + u];      // the gates kernel's rows: x, then h
            });
        return img;
    }

    // the backward buffer [layer 0 | upper layers]; img == nullptr: the same images once more over Lin, the table of the whole
    // buffer (pack_value.h; the active PackTrace's shift moves along)
    static void pack(const rnnwf_handle* h, std::vector<char>* img) {
        if (img) {
            *img = G0::template pack_bwd<double>(h);
            for (int l = 1; l < NL; ++l) {
                const std::vector<char> up = pack_upper_bwd<double>(h, l);
                img->insert(img->end(), up.begin(), up.end());
            }
            return;
        }
        const size_t base = pack_trace().shift;
        G0::template pack_bwd<Lin>(h);
        for (int l = 1; l < NL; ++l) {
            pack_trace().shift = base + G0::G::BWD_BYTES + (size_t)(l - 1) * GU::BWD_BYTES;
            pack_upper_bwd<Lin>(h, l);
        }
        pack_trace().shift = base;
    }
    // dW image + head rows (host copy of h->gradW) -> TF-named gradient arrays
    static void unpack(rnnwf_handle* h, const void* img) {
        const T* dW = (const T*)img;
        G0::unpack(h, dW, DW0);                                // layer 0 + head (written by the top layer's pass)
        for (int l = 1; l < NL; ++l) unpack_upper(h, dW + DW0 + HEAD + (size_t)(l - 1) * DWU, l);
    }

    template <bool TOP>
    static int upper_pass(rnnwf_handle* h, const UpperGradArgs& a) {
        const size_t lds = GU::WIDE ? GU::HEAD_BYTES : U::BYTES + GU::BWD_BYTES + (TOP ? GU::HEAD_BYTES : 0);
        if (lds > 160 * 1024) return h->fail(RNNWF_ERR_INVALID, "rnnwf_vmc_gradient: stacked-layer images (%zu B) exceed the 160 KB LDS", lds);
        return backward_launch<T>(h, gru_upper_bwd_kernel<T, NFULL, WAVES, TOP, NOUT>, WAVES * 64, lds, a.nsb, WAVES, NOUT * GU::HEAD_ROW,
                                  TOP ? (T*)a.head_grad : nullptr, a);
    }

    // every kernel of the gradient on the resident batch, added into the cleared h->gradW
    static int launch(rnnwf_handle* h, const GradCost& c) {
        const int N = h->N;
        const int64_t ns = h->last_ns, R = ns * N, nsb = (ns + kChains - 1) / kChains;
        if (int rc = ensure(h, h->gradP, (size_t)R * (NL > 1 ? GU::PCOLS : G0::G::PCOLS) * ES)) return rc;
        if (int rc = ensure(h, h->gradQ, (size_t)R * (NL > 1 ? GU::QCOLS : G0::G::QCOLS) * ES)) return rc;
        const size_t dx_bytes = (size_t)N * nsb * L0::KT * 64 * ES;         // dL/dx of one layer's pass, the dh_in of the next
        for (int i = 0; i < std::min(NL - 1, 2); ++i) if (int rc = ensure(h, h->gradDX[i], dx_bytes)) return rc;
        if constexpr (NOUT == 1 && sizeof(T) == 4)
            if (h->model == RNNWF_MODEL_GRU1D_PARITY) {
                // log P_sym = log(0.5 (P_F + P_R)) (1DTFIM/RNNwavefunction_paritysym.py:145): the gradient is the sum of the two
                // directions' gradients, each sample weighted by the direction's share of P_sym.  The step left the checkpoints of ONE
                // direction: both are redone here, teacher-forced, with the shares from the same two passes.
                if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
                if (int rc = ensure(h, h->out_lp2, (size_t)ns * 8)) return rc;
                double* lpF = (double*)h->out_lp.p;
                double* lpR = (double*)h->out_lp2.p;
                if (int rc = prnn_teacher_base(h, ns, false, lpF)) return rc;
                if (int rc = prnn_teacher_base(h, ns, true, lpR)) return rc;       // the reversed chains' states are resident now
                if (int rc = run_parity_share(h, lpF, lpR, ns)) return rc;
                if (int rc = passes(h, c, (const uint32_t*)h->bits2.p, lpR)) return rc;
                if (int rc = prnn_teacher_base(h, ns, false, nullptr)) return rc;
                return passes(h, c, (const uint32_t*)h->bits.p, lpF);
            }
        return passes(h, c, (const uint32_t*)h->bits.p, nullptr);
    }

    // one backward pass per layer, top first, over the resident checkpoints of the chains in `bits`; everything is ADDED to gradW
    static int passes(rnnwf_handle* h, const GradCost& c, const uint32_t* bits, const double* wfac) {
        const int64_t R = h->last_ns * h->N;
        T* dW = (T*)h->gradW.p;
        // the batch, the chains in `bits` and the cost's weights: the same in every pass
        auto fill = [&](auto& a) {
            grad_batch_args(h, &a);
            a.bits = bits;
            a.eloc = (const double*)h->eloc.p;
            a.eloc_c = (const float2*)h->eloc.p;
            a.mean_e = c.mean_e;
            a.mean_im = c.mean_im;
            a.inv_norm = c.inv_norm;
            a.mom = c.mom;
        };
        const void* dh_in = nullptr;
        if constexpr (NL > 1) {
            for (int l = NL - 1; l >= 1; --l) {
                UpperGradArgs u{};
                fill(u);
                u.wup = (const char*)h->wimg.p + L0::BYTES + (size_t)(l - 1) * U::BYTES;
                u.wbwd = (const char*)h->wbwd.p + G0::G::BWD_BYTES + (size_t)(l - 1) * GU::BWD_BYTES;
                u.whead = (const char*)h->wimg.p + L0::OFF_WD;
                u.layer = l;
                u.wfac = wfac;
                u.dh_in = dh_in;
                u.dx_out = h->gradDX[(NL - 1 - l) & 1].p;
                u.head_grad = dW + DW0;
                if (int rc = l == NL - 1 ? upper_pass<true>(h, u) : upper_pass<false>(h, u)) return rc;
                if (int rc = tn_gemm_launch<T, GU::PCOLS / 16, GU::QCOLS / 16>(h, (const T*)u.P, (const T*)u.Q, R, dW + DW0 + HEAD + (size_t)(l - 1) * DWU))
                    return rc;
                dh_in = u.dx_out;
            }
        }
        GradArgs a{};
        fill(a);
        a.wimg = h->wimg.p;
        a.wfac = NL > 1 ? nullptr : wfac;                  // a stack: w_s only weights the head terms, on the top layer
        a.head_grad = dW + (NL > 1 ? DW_FLOATS : DW0);     // a stack: the scratch row (layer 0 has no head term there; its adds are zeros)
        a.dh_in = dh_in;
        return G0::run(h, a, R, dW);
    }

    static void unpack_upper(rnnwf_handle* h, const T* dW, int layer) {
        const int hoff = 16 * GU::NTO;
        unpack_cell<T, NFULL>(h, dW, GU::QCOLS, "multi_rnn_cell/cell_" + std::to_string(layer) + "/cudnn_compatible_gru_cell/", h->H,
                              [](int k) { return col_of_unit(NFULL, k); }, hoff, hoff + 16 * NFULL + 1);
    }
};

// rc = fn(K()) for this handle's gradient class K: one per row of the family's forward table (shapes.h), at kGradWaves waves per
// workgroup whatever the forward kernels' (the kernels of f32 8..16 and the float64 GRU's 6 are in grad_wide.hip: GLaunch::WIDE)
template <typename T, int NFULL, int NL, int> using PGrad = MLGrad<NFULL, NL, kGradWaves, 1, T>;      // positive GRU, f32 and f64
template <typename T, int NFULL, int NL, int> using CGrad = MLGrad<NFULL, NL, kGradWaves, 3, T>;      // complex RNN
template <class Fn>
int with_gru_grad(rnnwf_handle* h, Fn&& fn) {
    int rc = 0;
    auto call = [&](auto k) { rc = fn(k); };
    if (h->model == RNNWF_MODEL_CRNN_U1 ? with_kernels<CGrad>(CrnnKernels(), h, call) : with_kernels<PGrad>(GruKernels(), h, call)) return rc;
    return h->fail(RNNWF_ERR_INVALID, "rnnwf_vmc_gradient: no gradient kernel for NFULL=%d with %d layers", h->NFULL, h->NL);
}

int grad_layout(rnnwf_handle* h, GradImage* out) {
    return with_gru_grad(h, [&](auto k) { *out = decltype(k)::layout(); return 0; });
}
int grad_pack(rnnwf_handle* h, std::vector<char>* img) {
    return with_gru_grad(h, [&](auto k) { decltype(k)::pack(h, img); return 0; });
}
int grad_launch(rnnwf_handle* h, const GradCost& c) {
    return with_gru_grad(h, [&](auto k) { return decltype(k)::launch(h, c); });
}
void grad_unpack(rnnwf_handle* h, const void* img) {
    with_gru_grad(h, [&](auto k) { decltype(k)::unpack(h, img); return 0; });
}

// fn(parameter, its gradient) in the order of rnnwf_set_params_flat; fails at a parameter without a gradient of its size
template <class Fn>
int each_grad(rnnwf_handle* h, const char* what, Fn&& fn) {
    for (auto& kv : h->params) {
        auto it = h->grads.find(kv.first);
        if (it == h->grads.end() || it->second.size() != kv.second.value.size())
            return h->fail(RNNWF_ERR_STATE, "%s: no gradient for '%s'", what, kv.first.c_str());
        fn(kv.second, it->second);
    }
    return 0;
}

// the family's unpacker on an image whose element k holds k + 1
template <typename T>
void unpack_indices(rnnwf_handle* h, size_t n) {
    std::vector<T> img(n);
    for (size_t k = 0; k < n; ++k) img[k] = (T)(k + 1);
    h->family->gradient->unpack(h, img.data());
}

}  // namespace

const Gradient* rnnwf::gru_gradient() {
    static const Gradient g = {grad_layout, grad_pack, grad_launch, grad_unpack};
    return &g;
}

// the family's backward image in h->wbwd, packed and uploaded when the committed parameters changed since the last one
int rnnwf::grad_bwd_image(rnnwf_handle* h) {
    if (h->wbwd_valid) return 0;
    std::vector<char> img;
    if (int rc = h->family->gradient->pack(h, &img)) return rc;
    if (int rc = ensure(h, h->wbwd, img.size())) return rc;
    if (int rc = upload(h, h->wbwd.p, img.data(), img.size())) return rc;
    h->wbwd_valid = true;
    return 0;
}

// The gradient's kernels on the batch of the last rnnwf_vmc_step: back-propagation through time + weight-gradient GEMMs, the
// result (the family's dW images and head rows) left in h->gradW.
int rnnwf::grad_device(rnnwf_handle* h, double mean_energy, double mean_energy_im, double norm, const double* mom_dev, GradImage* out) {
    if (h->last_ns <= 0)
        return h->fail(RNNWF_ERR_STATE, "rnnwf_vmc_gradient: call rnnwf_vmc_step first (its samples, states and E_loc are reused)");
    if (!mom_dev && !(norm > 0)) return h->fail(RNNWF_ERR_INVALID, "rnnwf_vmc_gradient: norm must be positive");
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const Gradient& g = *h->family->gradient;
    GradImage im;
    if (int rc = g.layout(h, &im)) return rc;
    if (int rc = grad_bwd_image(h)) return rc;
    const size_t bytes = im.alloc * (im.f64 ? 8 : 4);
    if (int rc = ensure(h, h->gradW, bytes)) return rc;
    RNNWF_HIP(h, hipMemsetAsync(h->gradW.p, 0, bytes, h->stream));
    if (out) *out = im;
    const double scale = h->family->complex_eloc ? 2.0 : 1.0;      // the complex cost carries a factor 2 (TrainingRNN_J1J2.py:197)
    return g.launch(h, GradCost{mean_energy, mean_energy_im, mom_dev ? scale : scale / norm, mom_dev});
}

extern "C" int rnnwf_vmc_gradient(rnnwf_handle* h, double mean_energy, double mean_energy_im, double norm) {
    if (!h) return RNNWF_ERR_INVALID;
    if (int rc = require_gradient(h, "rnnwf_vmc_gradient")) return rc;
    if (!h->committed) return h->fail(RNNWF_ERR_STATE, "parameters not committed");
    GradImage im;
    if (int rc = grad_device(h, mean_energy, mean_energy_im, norm, nullptr, &im)) return rc;
    const size_t bytes = im.count * (im.f64 ? 8 : 4);
    if (int rc = ensure_staging(h, bytes)) return rc;        // pinned: the copy is a plain DMA, the one wait is ours
    RNNWF_HIP(h, hipMemcpyAsync(h->staging, h->gradW.p, bytes, hipMemcpyDeviceToHost, h->stream));
    RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    h->family->gradient->unpack(h, h->staging);
    return RNNWF_OK;
}

// Where every entry of the flat gradient (order and shapes of rnnwf_get_grads_flat) sits in the h->gradW image: the family's
// unpacker run on an image whose element k holds k + 1 - sidx[j] = +-(k + 1), 0: no source (stays 0).  The indices must be exact
// in the image's element type and fit int32_t.
int rnnwf::grad_flat_probe(rnnwf_handle* h, std::vector<int32_t>& sidx, GradImage* im) {
    if (int rc = h->family->gradient->layout(h, im)) return rc;
    const size_t n = im->count;
    if (n == 0 || n >= ((size_t)1 << (im->f64 ? 31 : 24))) return h->fail(RNNWF_ERR_INVALID, "gradient image of %zu elements cannot be probed", n);
    const auto saved = h->grads;
    if (im->f64) unpack_indices<double>(h, n);
    else unpack_indices<float>(h, n);
    sidx.clear();
    const int rc = each_grad(h, "grad_flat_probe", [&](const ParamSpec& p, const std::vector<double>& g) {
        for (int64_t s : p.slot) sidx.push_back((int32_t)std::llround(g[(size_t)s]));
    });
    h->grads = saved;
    return rc;
}

extern "C" int rnnwf_get_grad(rnnwf_handle* h, const char* name, void* data, int64_t count, int32_t dtype) {
    if (!h || !name || !data) return RNNWF_ERR_INVALID;
    auto it = h->grads.find(name);
    if (it == h->grads.end()) return h->fail(RNNWF_ERR_STATE, "no gradient for '%s' (call rnnwf_vmc_gradient first)", name);
    auto ps = h->params.find(name);                  // the gradient is computed for the padded parameter; the caller gets its own shape
    if (ps == h->params.end() || it->second.size() != ps->second.value.size())
        return h->fail(RNNWF_ERR_STATE, "gradient '%s' does not match a parameter of this model", name);
    const std::vector<int64_t>& slot = ps->second.slot;
    if ((int64_t)slot.size() != count)
        return h->fail(RNNWF_ERR_INVALID, "gradient '%s' has %lld elements, caller passed %lld", name,
                       (long long)slot.size(), (long long)count);
    if (dtype == RNNWF_F32) for (int64_t i = 0; i < count; ++i) ((float*)data)[i] = (float)it->second[slot[i]];
    else if (dtype == RNNWF_F64) for (int64_t i = 0; i < count; ++i) ((double*)data)[i] = it->second[slot[i]];
    else return h->fail(RNNWF_ERR_INVALID, "unknown dtype %d", dtype);
    return RNNWF_OK;
}

// All gradients in ONE call, in the order and shapes of rnnwf_set_params_flat.
extern "C" int rnnwf_get_grads_flat(rnnwf_handle* h, double* flat, int64_t count) {
    if (!h || !flat) return RNNWF_ERR_INVALID;
    if (h->grads.empty()) return h->fail(RNNWF_ERR_STATE, "rnnwf_get_grads_flat: no gradients (call rnnwf_vmc_gradient first)");
    int64_t total = 0;
    for (auto& kv : h->params) total += (int64_t)kv.second.slot.size();
    if (count != total)
        return h->fail(RNNWF_ERR_INVALID, "rnnwf_get_grads_flat: the model has %lld parameters, caller passed %lld", (long long)total, (long long)count);
    return each_grad(h, "rnnwf_get_grads_flat", [&](const ParamSpec& p, const std::vector<double>& g) {
        for (int64_t s : p.slot) *flat++ = g[(size_t)s];
    });
}

// the weight image changed: the backward image must be rebuilt on the next gradient call
void rnnwf::grad_invalidate(rnnwf_handle* h) {     // (the buffer stays: freeing and re-allocating it cost ~0.1 ms per training iteration)
    h->wbwd_valid = false;
    h->sr_valid = false;          // the per-sample log-derivatives (sr.hip) belong to the old weights too
}
