// mdrnn.hip - host side of the 2D MDRNN wave function (model MDRNN2D, float64): weight image, base pass, fused 2D-TFIM local
// energies (driven through mdrnn_family by rnnwf_api.hip) and the gradient's hooks (driven by grad.hip: grad_device).
#include <algorithm>

#include "grad_kernels.h"
#include "mdrnn_grad_kernels.h"
#include "tn_gemm.h"
#include "mdrnn_kernels.h"
#include "models.h"
#include "pack.h"
#include "shapes.h"

using namespace rnnwf;

namespace {

constexpr size_t kHsBudget = (size_t)24 << 30;   // bytes of per-site hidden states per pass

template <int NFULL, int WAVES>
struct MLaunch {
    using L = MdLayout<NFULL>;
    static int base(rnnwf_handle* h, const MdArgs& a) {
        return launch_persistent(h, kTimerBase, mdrnn_base_kernel<NFULL, WAVES>, WAVES * 64, L::BYTES, a.nsb, WAVES, a);
    }
    static constexpr size_t FLIP_LDS = L::BYTES + (size_t)WAVES * L::WORDS_BYTES;     // image + the waves' spin words
    static int flip(rnnwf_handle* h, MdArgs a) {
        const auto kern = mdrnn_flip_kernel<NFULL, WAVES>;
        unsigned grid = 0;
        if (int rc = persistent_grid(h, kern, WAVES * 64, FLIP_LDS, a.ntiles, WAVES, &grid)) return rc;
        const size_t ring_bytes = (size_t)grid * WAVES * a.Nx * ((L::KT + 1) / 2) * 64 * 16;      // one slot per lattice column
        if (int rc = ensure(h, h->rowbuf, ring_bytes)) return rc;
        a.ring = (double*)h->rowbuf.p;
        a.ablate = h->knobs.ablate;   // 0 unless a -DRNNWF_DIAGNOSTICS build read RNNWF_ABLATE
        return timed_launch(h, kTimerFlip, kern, grid, WAVES * 64, FLIP_LDS, a);
    }
    static size_t hs_bytes_per_block() { return (size_t)((L::KT + 1) / 2) * 64 * 16; }
    static double mfma_flops_per_step() { return (double)NFULL * 2 * L::KT * 2048.0; }

    // S = double: the image of the committed parameters; S = Lin: the same code recording, for the device re-pack kernel of
    // train.hip, which parameters every element is made of (pack_value.h)
    template <class S = double>
    static std::vector<char> pack(const rnnwf_handle* h) {
        using Out = PackSink<S>;
        const int H = h->H;
        std::vector<char> img(L::BYTES, 0);
        Out::begin(img);
        const auto Wh = pvs<S>(h, "Wh_rnn_0");   // [H, H]
        const auto Uh = pvs<S>(h, "Uh_rnn_0");   // [2, H]
        const auto Wv = pvs<S>(h, "Wv_rnn_0");
        const auto Uv = pvs<S>(h, "Uv_rnn_0");
        const auto b = pvs<S>(h, "b_rnn_0");
        const auto Wd = pvs<S>(h, "wf_dense/kernel");
        const auto bd = pvs<S>(h, "wf_dense/bias");
        double* A = reinterpret_cast<double*>(img.data() + L::OFF_A);
        for (int t = 0; t < NFULL; ++t)
            for (int row = 0; row < 16; ++row) {
                const int unit = 16 * t + row;
                if (unit >= H) continue;
                for (int kq = 0; kq < 4; ++kq) {
                    const int lane = (kq << 4) | row;
                    for (int kk = 0; kk < 2 * L::KT; ++kk) {
                        const int k = 4 * (kk < L::KT ? kk : kk - L::KT) + kq;
                        if (k >= H) continue;
                        Out::put(&A[(((size_t)t * L::KT + kk / 2) * 64 + lane) * 2 + (kk & 1)],
                                 kk < L::KT ? Wh[(size_t)k * H + unit] : Wv[(size_t)k * H + unit]);
                    }
                }
            }
        double* WR = reinterpret_cast<double*>(img.data() + L::OFF_WR);
        for (int kk = 0; kk < 2 * L::KT; ++kk)
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * (kk < L::KT ? kk : kk - L::KT) + q;
                if (k >= H) continue;
                for (int j = 0; j < 4; ++j) {
                    const int unit = 16 * NFULL + j;
                    if (unit >= H) continue;
                    Out::put(&WR[(kk * 4 + q) * 4 + j], kk < L::KT ? Wh[(size_t)k * H + unit] : Wv[(size_t)k * H + unit]);
                }
            }
        // b + Uh[x_h] (BH), Uv[x_v] (BV) for x in {none, 0, 1}, and their nine sums (BHV): one accumulator start value per step
        auto bh_of = [&](int v, int unit) -> S { return b[unit] + (v ? Uh[(size_t)(v - 1) * H + unit] : S(0.0)); };
        auto bv_of = [&](int v, int unit) -> S { return v ? Uv[(size_t)(v - 1) * H + unit] : S(0.0); };
        for (int t = 0; t < L::NT; ++t)
            for (int q = 0; q < 4; ++q)
                for (int r = 0; r < 4; ++r) {
                    if (t == NFULL && r != 0) continue;
                    const int unit = t < NFULL ? 16 * t + 4 * r + q : 16 * NFULL + q;
                    if (unit >= H) continue;
                    const int k = t * 16 + q * 4 + r;
                    for (int v = 0; v < 3; ++v) {
                        Out::put(reinterpret_cast<double*>(img.data() + L::OFF_BH + v * L::SZ_B) + k, bh_of(v, unit));
                        Out::put(reinterpret_cast<double*>(img.data() + L::OFF_BV + v * L::SZ_B) + k, bv_of(v, unit));
                    }
                    for (int vh = 0; vh < 3; ++vh)
                        for (int vv = 0; vv < 3; ++vv)
                            Out::put(reinterpret_cast<double*>(img.data() + L::OFF_BHV + (size_t)(vh * 3 + vv) * L::SZ_B) + k,
                                     bh_of(vh, unit) + bv_of(vv, unit));
                }
        double* WD = reinterpret_cast<double*>(img.data() + L::OFF_WD);
        double* BD = reinterpret_cast<double*>(img.data() + L::OFF_BD);
        for (int kt = 0; kt < L::KT; ++kt)
            for (int q = 0; q < 4; ++q) {
                const int unit = 4 * kt + q;
                if (unit >= H) continue;
                Out::put(&WD[(kt * 4 + q) * 2], Wd[(size_t)unit * 2]);
                Out::put(&WD[(kt * 4 + q) * 2 + 1], Wd[(size_t)unit * 2 + 1]);
            }
        Out::put(&BD[0], bd[0]);
        Out::put(&BD[1], bd[1]);
        fill_f64_tables(reinterpret_cast<double*>(img.data() + L::OFF_TAB));
        double* WDD = reinterpret_cast<double*>(img.data() + L::OFF_WDD);
        for (int unit = 0; unit < H; ++unit) Out::put(&WDD[unit], Wd[(size_t)unit * 2 + 1] - Wd[(size_t)unit * 2]);   // slot 4 kt + q
        Out::put(&WDD[L::KT * 4], bd[1] - bd[0]);
        return img;
    }
};

// fn(K<NFULL, WAVES>()) for the handle's row of shapes.h, false (fn not called) for a width without kernels: K = MLaunch (the forward
// passes) or MGrad (the gradient)
template <template <int, int> class K, class Fn>
bool with_width(const rnnwf_handle* h, Fn&& fn) { return with_width_kernels<K>(MdKernels(), h, fn); }

int no_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "MDRNN: num_units > 84 is not implemented on gfx950 yet"); }
int launch_base(rnnwf_handle* h, const MdArgs& a) {
    int rc = 0;
    return with_width<MLaunch>(h, [&](auto k) { rc = decltype(k)::base(h, a); }) ? rc : no_kernel(h);
}
int launch_flip(rnnwf_handle* h, const MdArgs& a) {
    int rc = 0;
    return with_width<MLaunch>(h, [&](auto k) { rc = decltype(k)::flip(h, a); }) ? rc : no_kernel(h);
}
size_t hs_bytes_per_block(rnnwf_handle* h) {
    size_t b = 1;
    with_width<MLaunch>(h, [&](auto k) { b = decltype(k)::hs_bytes_per_block(); });
    return b;
}
double mfma_flops_per_step(rnnwf_handle* h) {
    double f = 0;
    with_width<MLaunch>(h, [&](auto k) { f = decltype(k)::mfma_flops_per_step(); });
    return f;
}

// device maps, 6 x N int32: col_of_pos | pos_of_site | row_of_pos | vert_pos | row_first | (spare)
struct Maps {
    const int32_t *col_of_pos, *pos_of_site, *row_of_pos, *vert_pos, *row_first;
};

int get_maps(rnnwf_handle* h, Maps* m) {
    const int Nx = h->Nx, Ny = h->Ny, N = h->N;
    if (!h->maps.p) {
        std::vector<int32_t> v((size_t)5 * N);
        auto pos_of = [&](int nx, int ny) { return ny * Nx + (ny % 2 == 0 ? nx : Nx - 1 - nx); };
        for (int p = 0; p < N; ++p) {
            const int ny = p / Nx, j = p % Nx;
            const int nx = ny % 2 == 0 ? j : Nx - 1 - j;
            const int k = nx * Ny + ny;                        // samples[b, nx, ny] in C order
            v[p] = k;
            v[(size_t)N + k] = p;
            v[(size_t)2 * N + p] = k + 1;                      // queue row of the flip at (nx, ny): nx*Ny + ny + 1
            v[(size_t)3 * N + p] = ny > 0 ? pos_of(nx, ny - 1) : -1;
            v[(size_t)4 * N + p] = j == 0 ? 1 : 0;
        }
        if (int rc = ensure(h, h->maps, v.size() * 4)) return rc;
        RNNWF_HIP(h, hipMemcpy(h->maps.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    const int32_t* b = (const int32_t*)h->maps.p;
    m->col_of_pos = b;
    m->pos_of_site = b + N;
    m->row_of_pos = b + 2 * (size_t)N;
    m->vert_pos = b + 3 * (size_t)N;
    m->row_first = b + 4 * (size_t)N;
    return 0;
}

int64_t max_chains_per_pass(rnnwf_handle* h) {
    const size_t per_block = (size_t)h->N * hs_bytes_per_block(h);
    return std::max<int64_t>(1, (int64_t)(state_budget_bytes(h, kHsBudget) / per_block)) * kChains;
}

MdArgs base_args(rnnwf_handle* h, int64_t ns, const Maps& m) {
    MdArgs a{};
    a.wimg = h->wimg.p;
    a.N = h->N;
    a.Nx = h->Nx;
    a.rem = h->H - 16 * h->NFULL;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.vert_pos = m.vert_pos;
    a.row_first = m.row_first;
    a.row_of_pos = m.row_of_pos;
    return a;
}

// Fused local energies of ns chains whose packed spins are in h->bits (drawn into it when `d`): base pass keeping every site's
// state -> flip pass -> assembly.  Leaves E_loc in h->eloc and the log-prob queue in h->lpq.
int eloc_on_device(rnnwf_handle* h, int64_t ns, const Draw* d, const double* couplings) {
    const int N = h->N;
    const int64_t nsb = (ns + kChains - 1) / kChains;
    const double Bx = couplings[N];
    Maps m;
    if (int rc = get_maps(h, &m)) return rc;
    if (int rc = ensure(h, h->hck, (size_t)N * nsb * hs_bytes_per_block(h))) return rc;
    if (int rc = ensure(h, h->lpq, (size_t)(N + 1) * ns * 8)) return rc;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    MdArgs a = base_args(h, ns, m);
    a.bits = (uint32_t*)h->bits.p;
    a.hs = (double*)h->hck.p;
    a.lpq = (double*)h->lpq.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    if (int rc = launch_base(h, a)) return rc;
    if (Bx != 0.0 && N > 1) {
        a.sampling = 0;
        a.ntiles = (int64_t)(N - 1) * nsb;
        if (int rc = launch_flip(h, a)) return rc;
        h->work[0] += (double)ns * N * (N - 1) / 2.0;
        h->work[1] += (double)nsb * N * (N - 1) / 2.0 * mfma_flops_per_step(h);
    }
    return run_tfim_eloc(h, (const uint32_t*)h->bits.p, (const double*)h->lpq.p, ns, h->Nx, h->Ny, m.pos_of_site,
                         (const double*)h->coupl.p, Bx, (double*)h->eloc.p);
}

// base pass alone (it, too, keeps every site's state in h->hck): log P of every chain -> h->out_lp (the spins drawn into h->bits
// when `d`)
int log_prob_pass(rnnwf_handle* h, int64_t ns, const Draw* d) {
    const int64_t nsb = (ns + kChains - 1) / kChains;
    Maps m;
    if (int rc = get_maps(h, &m)) return rc;
    if (int rc = ensure(h, h->out_lp, (size_t)ns * 8)) return rc;
    if (int rc = ensure(h, h->hck, (size_t)h->N * nsb * hs_bytes_per_block(h))) return rc;
    MdArgs a = base_args(h, ns, m);
    a.bits = (uint32_t*)h->bits.p;
    a.hs = (double*)h->hck.p;
    a.out_lp = (double*)h->out_lp.p;
    if (d) { a.sampling = 1; a.seed = d->seed; a.step = d->step; a.sample_offset = d->offset; }
    return launch_base(h, a);
}

// the packed bits follow the snake path: samples[b, nx, ny] is bit col_of_pos[p] of position p
int site_maps(rnnwf_handle* h, const int32_t** col_of_pos, const int32_t** pos_of_site) {
    Maps m;
    if (int rc = get_maps(h, &m)) return rc;
    *col_of_pos = m.col_of_pos;
    *pos_of_site = m.pos_of_site;
    return 0;
}

int pack_image(rnnwf_handle* h, std::vector<char>& img) {
    if (h->N > 256) return h->fail(RNNWF_ERR_INVALID, "MDRNN: lattices above 256 sites are not implemented");
    return with_width<MLaunch>(h, [&](auto k) { img = decltype(k)::template pack<double>(h); }) ? 0 : no_kernel(h);
}
// device-resident training (train.hip): the table of that image
int pack_table(rnnwf_handle* h) {
    return with_width<MLaunch>(h, [&](auto k) { decltype(k)::template pack<Lin>(h); }) ? 0 : no_kernel(h);
}

}  // namespace

// ---- gradient of the VMC cost (2DTFIM_2DRNN/Training2DRNN_2DTFIM.py:163-170) ----
namespace {

template <int NFULL, int WAVES>
struct MGrad {
    using G = MdGradLayout<NFULL>;
    static GradImage layout() {
        const size_t n = (size_t)G::PCOLS * G::QCOLS + 2 * G::HEAD_ROW;
        return {true, n, n};
    }

    template <class S = double>
    static std::vector<char> pack(const rnnwf_handle* h) {
        using Out = PackSink<S>;
        const int H = h->H;
        std::vector<char> img(G::BYTES, 0);
        Out::begin(img);
        const auto Wh = pvs<S>(h, "Wh_rnn_0");
        const auto Wv = pvs<S>(h, "Wv_rnn_0");
        const auto Wd = pvs<S>(h, "wf_dense/kernel");
        const auto bd = pvs<S>(h, "wf_dense/bias");
        double* A = reinterpret_cast<double*>(img.data() + G::OFF_A);
        for (int t = 0; t < G::NTO; ++t) {
            const int tt = t % G::NT;
            const auto& Wsrc = t < G::NT ? Wh : Wv;
            for (int row = 0; row < 16; ++row) {
                const int kout = 16 * tt + row;                    // unit receiving dL/dh (C/D row = natural order)
                if (kout >= H || (tt == NFULL && row >= 4)) continue;
                for (int kq = 0; kq < 4; ++kq) {
                    const int lane = (kq << 4) | row;
                    for (int kk = 0; kk < G::KT; ++kk) {
                        const int u = 4 * kk + kq;
                        if (u >= H) continue;
                        Out::put(&A[(((size_t)t * G::KBG + kk / 2) * 64 + lane) * 2 + (kk & 1)], Wsrc[(size_t)kout * H + u]);
                    }
                }
            }
        }
        double* WD = reinterpret_cast<double*>(img.data() + G::OFF_WD);
        double* BD = reinterpret_cast<double*>(img.data() + G::OFF_BD);
        for (int kt = 0; kt < G::KT; ++kt)
            for (int q = 0; q < 4; ++q) {
                const int unit = 4 * kt + q;
                if (unit >= H) continue;
                Out::put(&WD[(kt * 4 + q) * 2], Wd[(size_t)unit * 2]);
                Out::put(&WD[(kt * 4 + q) * 2 + 1], Wd[(size_t)unit * 2 + 1]);
            }
        Out::put(&BD[0], bd[0]);
        Out::put(&BD[1], bd[1]);
        return img;
    }

    // What a backward pass over the resident batch reads and writes, whatever its weights: the site maps, the spins and states, the
    // P / Q rows and the per-wave ring in HBM, sized by the persistent grid of `kern` - the kernel these arguments are launched with
    template <class Kern>
    static int backward_args(rnnwf_handle* h, Kern kern, MdGradArgs* out) {
        Maps m;
        if (int rc = get_maps(h, &m)) return rc;
        const int N = h->N;
        const int64_t ns = h->last_ns, R = ns * N;
        if (int rc = ensure(h, h->gradP, (size_t)R * G::PCOLS * 8)) return rc;
        if (int rc = ensure(h, h->gradQ, (size_t)R * G::QCOLS * 8)) return rc;
        MdGradArgs a{};
        a.wbwd = h->wbwd.p;
        a.N = N;
        a.Nx = h->Nx;
        a.ns = ns;
        a.nsb = (ns + kChains - 1) / kChains;
        a.bits = (const uint32_t*)h->bits.p;
        a.hs = (const double*)h->hck.p;
        a.P = (double*)h->gradP.p;
        a.Q = (double*)h->gradQ.p;
        a.vert_pos = m.vert_pos;
        a.row_first = m.row_first;
        unsigned grid = 0;                                  // the ring is sized by the grid backward_launch will use
        if (int rc = persistent_grid(h, kern, WAVES * 64, G::BYTES, a.nsb, WAVES, &grid)) return rc;
        if (int rc = ensure(h, h->rowbuf, (size_t)grid * WAVES * 2 * a.Nx * G::KT * 64 * 8)) return rc;
        a.ring = (double*)h->rowbuf.p;
        *out = a;
        return 0;
    }

    static int launch(rnnwf_handle* h, const GradCost& c) {
        MdGradArgs a{};
        if (int rc = backward_args(h, mdrnn_bwd_kernel<NFULL, WAVES>, &a)) return rc;
        a.eloc = (const double*)h->eloc.p;
        a.mean_e = c.mean_e;
        a.inv_norm = c.inv_norm;
        a.mom = c.mom;
        a.head_grad = (double*)h->gradW.p + (size_t)G::PCOLS * G::QCOLS;
        if (int rc = backward_launch<double>(h, mdrnn_bwd_kernel<NFULL, WAVES>, WAVES * 64, G::BYTES, a.nsb, WAVES, 2 * G::HEAD_ROW, a.head_grad, a)) return rc;
        return tn_gemm_launch<double, G::PCOLS / 16, G::QCOLS / 16>(h, a.P, a.Q, (int64_t)a.ns * a.N, (double*)h->gradW.p);
    }

    // stochastic reconfiguration (sr.hip): the same pass with unit weights, every chain's two head rows into head_rows [ns][2][HEAD_ROW]
    static int sr_backward(rnnwf_handle* h, double* head_rows) {
        MdGradArgs a{};
        if (int rc = backward_args(h, mdrnn_bwd_kernel<NFULL, WAVES, true>, &a)) return rc;
        a.head_part = head_rows;
        return backward_launch<double>(h, mdrnn_bwd_kernel<NFULL, WAVES, true>, WAVES * 64, G::BYTES, a.nsb, WAVES, 0, (double*)nullptr, a);
    }

    // dW image [PCOLS][QCOLS], then the two head rows -> TF-named gradient arrays
    static void unpack(rnnwf_handle* h, const void* img) {
        const double* dW = (const double*)img;
        const double* hg = dW + (size_t)G::PCOLS * G::QCOLS;
        const int H = h->H;
        const int xcol = 16 * NFULL + 1, onecol = 16 * NFULL + 3, voff = 16 * G::NT;
        auto at = [&](int prow, int col) { return dW[(size_t)prow * G::QCOLS + col]; };
        auto& gWh = h->grads["Wh_rnn_0"];
        auto& gUh = h->grads["Uh_rnn_0"];
        auto& gWv = h->grads["Wv_rnn_0"];
        auto& gUv = h->grads["Uv_rnn_0"];
        auto& gb = h->grads["b_rnn_0"];
        auto& gWd = h->grads["wf_dense/kernel"];
        auto& gbd = h->grads["wf_dense/bias"];
        gWh.assign((size_t)H * H, 0.0); gWv.assign((size_t)H * H, 0.0);
        gUh.assign((size_t)2 * H, 0.0); gUv.assign((size_t)2 * H, 0.0);
        gb.assign(H, 0.0); gWd.assign((size_t)H * 2, 0.0); gbd.assign(2, 0.0);
        for (int u = 0; u < H; ++u) {
            const int prow = col_of_unit(NFULL, u);            // P uses the same tile / quarter / register order as Q
            for (int k = 0; k < H; ++k) {
                gWh[(size_t)k * H + u] = at(prow, col_of_unit(NFULL, k));
                gWv[(size_t)k * H + u] = at(prow, voff + col_of_unit(NFULL, k));
            }
            for (int sg = 0; sg < 2; ++sg) {
                gUh[(size_t)sg * H + u] = at(prow, xcol + sg);
                gUv[(size_t)sg * H + u] = at(prow, voff + xcol + sg);
            }
            gb[u] = at(prow, onecol);
            gWd[(size_t)u * 2] = hg[u];
            gWd[(size_t)u * 2 + 1] = hg[G::HEAD_ROW + u];
        }
        gbd[0] = hg[4 * G::KT];
        gbd[1] = hg[G::HEAD_ROW + 4 * G::KT];
    }
};

int no_grad_kernel(rnnwf_handle* h) { return h->fail(RNNWF_ERR_INVALID, "rnnwf_vmc_gradient: num_units > 84 not implemented"); }

// the gradient hooks (models.h: Gradient)
int grad_layout(rnnwf_handle* h, GradImage* out) {
    return with_width<MGrad>(h, [&](auto k) { *out = decltype(k)::layout(); }) ? 0 : no_grad_kernel(h);
}
int grad_pack(rnnwf_handle* h, std::vector<char>* img) {
    return with_width<MGrad>(h, [&](auto k) {
        using K = decltype(k);
        if (img) *img = K::template pack<double>(h);
        else K::template pack<Lin>(h);
    }) ? 0 : no_grad_kernel(h);
}
int grad_launch(rnnwf_handle* h, const GradCost& c) {
    int rc = 0;
    return with_width<MGrad>(h, [&](auto k) { rc = decltype(k)::launch(h, c); }) ? rc : no_grad_kernel(h);
}
void grad_unpack(rnnwf_handle* h, const void* img) {
    with_width<MGrad>(h, [&](auto k) { decltype(k)::unpack(h, img); });
}

}  // namespace

int rnnwf::mdrnn_sr_backward(rnnwf_handle* h, double* head_rows) {
    int rc = 0;
    return with_width<MGrad>(h, [&](auto k) { rc = decltype(k)::sr_backward(h, head_rows); }) ? rc : no_grad_kernel(h);
}

const Family* rnnwf::mdrnn_family() {
    static const Gradient g = {grad_layout, grad_pack, grad_launch, grad_unpack};
    static const Family f = {
        "2D RNN", pack_image, pack_table, log_prob_pass, nullptr, eloc_on_device, max_chains_per_pass, site_maps, nullptr,
        1, 1,               // Jz per site; Bx
        false, true, &g,    // float64 E_loc; the base pass alone keeps every site's state
    };
    return &f;
}
