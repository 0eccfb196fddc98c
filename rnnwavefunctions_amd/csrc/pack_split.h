// pack_split.h - host-side packing of the GRU parameters into the bf16x3 image of split_core.h.
#pragma once
#include <cmath>
#include <cstring>

#include "pack.h"
#include "split_core.h"
#include "split16_core.h"

namespace rnnwf {

// Image of the 16x16x32 form of the flip pass at 69..100 units (split16_core.h: S16Layout).
template <int NOUT, class S = double>
std::vector<char> pack_split16_image(const rnnwf_handle* h) {
    using L = S16Layout<NOUT>;
    using Out = PackSink<S>;
    static_assert(NOUT == 1, "the 16x16x32 form carries one head row (positive RNN)");
    const int H = h->H;
    std::vector<char> img(L::BYTES, 0);
    Out::begin(img);
    const std::string pre = kGruPre;
    const auto Wg = pvs<S>(h, pre + "gates/kernel");
    const auto bg = pvs<S>(h, pre + "gates/bias");
    const auto Wci = pvs<S>(h, pre + "candidate/input_projection/kernel");
    const auto bci = pvs<S>(h, pre + "candidate/input_projection/bias");
    const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");
    const auto bch = pvs<S>(h, pre + "candidate/hidden_projection/bias");
    const auto Wd = pvs<S>(h, "wf_dense/kernel");
    const auto bd = pvs<S>(h, "wf_dense/bias");
    const double sg = PackScale<float>::gate, sc = PackScale<float>::cand;
    // row (tile t, row i = 4 g + r) -> (gate, unit): gate 0 r, 1 u, 2 candidate, 3 head; unit -1: unused row
    auto decode = [&](int t, int g, int r, int& gate, int& unit) {
        if (t < L::NTF) {
            const int b = t / 6, tau = t % 2;
            gate = (t % 6) / 2;
            unit = 4 * (8 * b + 4 * tau + r) + g;
        } else if (r < 3) {
            gate = r;
            unit = 4 * L::NJA + g;
        } else {
            gate = 3;
            unit = 0;
        }
        if (gate < 3 && unit >= H) unit = -1;
    };
    auto weight = [&](int gate, int uo, int ui) -> S {
        if (ui >= H) return S(0.0);
        if (gate == 0) return sg * Wg[(size_t)(2 + ui) * 2 * H + uo];
        if (gate == 1) return sg * Wg[(size_t)(2 + ui) * 2 * H + H + uo];
        if (gate == 2) return sc * Wch[(size_t)ui * H + uo];
        return Wd[(size_t)ui * 2 + 1] - Wd[(size_t)ui * 2];
    };
    uint16_t* A = reinterpret_cast<uint16_t*>(img.data() + L::OFF_A);
    uint16_t* ASP = reinterpret_cast<uint16_t*>(img.data() + L::OFF_ASP);
    float* CI = reinterpret_cast<float*>(img.data() + L::OFF_CI);
    for (int t = 0; t < L::NT; ++t)
        for (int i = 0; i < 16; ++i) {
            const int go = i >> 2, r = i & 3;
            int gate, uo;
            decode(t, go, r, gate, uo);
            if (uo < 0) continue;
            for (int sgm = 0; sgm < 2; ++sgm) {                  // accumulator start value: bias + one-hot input row
                S v;
                if (gate == 0) v = sg * (bg[uo] + Wg[(size_t)sgm * 2 * H + uo]);
                else if (gate == 1) v = sg * (bg[H + uo] + Wg[(size_t)sgm * 2 * H + H + uo]);
                else if (gate == 2) v = sc * bch[uo];
                else v = bd[1] - bd[0];
                Out::put(&CI[(((size_t)sgm * L::NT + t) * 4 + go) * 4 + r], v);
            }
            for (int g = 0; g < 4; ++g) {                        // K side: lane group g supplies its units 4 j + g
                const int lane = (g << 4) | i;
                for (int o = 0; o < L::NOCT; ++o)
                    for (int e = 0; e < 8; ++e) {
                        auto at = [&](int a) { return &A[((((size_t)t * 3 + a) * L::NOCT + o) * 64 + lane) * 8 + e]; };
                        Out::put_parts(at(0), at(1), at(2), weight(gate, uo, 4 * (8 * o + e) + g));
                    }
                const S ws = weight(gate, uo, 4 * L::NJA + g);
                const int part[6] = {0, 0, 0, 1, 1, 2};          // against the B entries {h1, h2, h3, h1, h2, h1}
                for (int e = 0; e < 6; ++e) Out::put_part(&ASP[((size_t)t * 64 + lane) * 8 + e], ws, part[e]);
            }
        }
    float* XC = reinterpret_cast<float*>(img.data() + L::OFF_XC);
    float* WD = reinterpret_cast<float*>(img.data() + L::OFF_WD);
    float* BD = reinterpret_cast<float*>(img.data() + L::OFF_BD);
    for (int g = 0; g < 4; ++g)
        for (int j = 0; j < L::NJ; ++j) {
            const int u = 4 * j + g;
            if (u >= H) continue;
            for (int sgm = 0; sgm < 2; ++sgm) Out::put(&XC[((size_t)sgm * 4 + g) * L::XCP + j], sc * (bci[u] + Wci[(size_t)sgm * H + u]));
            Out::put(&WD[(size_t)g * L::XCP + j], Wd[(size_t)u * 2 + 1] - Wd[(size_t)u * 2]);
        }
    Out::put(&BD[0], bd[1] - bd[0]);
    return img;
}

// bf16x3 A fragments of the cooperative base pass (layout.h: BaseBfLayout): the rows of pack_gru_image (same scaled f32
// weights), each split exactly into three bf16 parts.
template <int NFULL, class S = double>
std::vector<char> pack_base_bf_image(const rnnwf_handle* h) {
    using B = BaseBfLayout<NFULL>;
    using Out = PackSink<S>;
    const int H = h->H;
    std::vector<char> img(B::BYTES, 0);
    Out::begin(img);
    const std::string pre = kGruPre;
    const auto Wg = pvs<S>(h, pre + "gates/kernel");
    const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");
    const double sg = PackScale<float>::gate, sc = PackScale<float>::cand;
    auto wt = [&](int gate, int unit, int k) -> S {
        if (k >= H) return S(0.0);
        if (gate == 0) return sg * Wg[(size_t)(2 + k) * 2 * H + unit];
        if (gate == 1) return sg * Wg[(size_t)(2 + k) * 2 * H + H + unit];
        return sc * Wch[(size_t)k * H + unit];
    };
    uint16_t* A = reinterpret_cast<uint16_t*>(img.data());
    for (int tile = 0; tile < B::NT; ++tile)
        for (int row = 0; row < 16; ++row) {
            const int q = row >> 2, r = row & 3;                // C/D row 4 q + r of the f32 16x16 output
            int gate, unit;
            if (tile < 3 * NFULL) { gate = tile / NFULL; unit = 16 * (tile % NFULL) + 4 * r + q; }
            else { if (r == 3) continue; gate = r; unit = 16 * NFULL + q; }
            if (unit >= H) continue;
            for (int t = 0; t < B::NKS; ++t)
                for (int g = 0; g < 4; ++g)
                    for (int e = 0; e < 8; ++e) {
                        const int kappa = 32 * t + 8 * g + e, grp = kappa / 16, loc = kappa % 16, kq = loc / 4, kr = loc % 4;
                        int ku = -1;
                        if (grp < NFULL) ku = 16 * grp + 4 * kr + kq;
                        else if (grp == NFULL && kr == 0) ku = 16 * NFULL + kq;
                        if (ku < 0 || ku >= H) continue;
                        const int lane = (g << 4) | row;
                        auto at = [&](int a) { return &A[((((size_t)tile * 3 + a) * B::NKS + t) * 64 + lane) * 8 + e]; };
                        Out::put_parts(at(0), at(1), at(2), wt(gate, unit, ku));      // (the split starts from the value as f32)
                    }
        }
    return img;
}

template <int NF32, int RJ, int NOUT = 1, int MODE = 0, class S = double>
std::vector<char> pack_split_image(const rnnwf_handle* h) {
    using L = SplitLayout<NF32, RJ, NOUT, MODE>;
    using Out = PackSink<S>;
    const int H = h->H;
    std::vector<char> img(L::BYTES, 0);
    Out::begin(img);
    const std::string pre = kGruPre;
    const auto Wg = pvs<S>(h, pre + "gates/kernel");
    const auto bg = pvs<S>(h, pre + "gates/bias");
    const auto Wci = pvs<S>(h, pre + "candidate/input_projection/kernel");
    const auto bci = pvs<S>(h, pre + "candidate/input_projection/bias");
    const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");
    const auto bch = pvs<S>(h, pre + "candidate/hidden_projection/bias");
    const auto Wd = pvs<S>(h, NOUT == 1 ? "wf_dense/kernel" : "wf_dense_ampl/kernel");
    const auto bd = pvs<S>(h, NOUT == 1 ? "wf_dense/bias" : "wf_dense_ampl/bias");
    const double sg = PackScale<float>::gate, sc = PackScale<float>::cand;
    uint16_t* A = reinterpret_cast<uint16_t*>(img.data() + L::OFF_A);
    auto head_w = [&](int o, int ui) -> S {
        if (o == 0) return Wd[(size_t)ui * 2 + 1] - Wd[(size_t)ui * 2];
        return pvs<S>(h, "wf_dense_phase/kernel")[(size_t)ui * 2 + (o - 1)];
    };
    auto head_b = [&](int o) -> S {
        if (o == 0) return bd[1] - bd[0];
        return pvs<S>(h, "wf_dense_phase/bias")[o - 1];
    };
    for (int T = 0; T < L::NT; ++T)
        for (int lane = 0; lane < 64; ++lane) {
            const int r32 = lane & 31, hhk = lane >> 5;
            const int hh_row = (r32 >> 2) & 1, rho = (r32 & 3) + 4 * (r32 >> 3);
            int g = -1, uo = -1;
            if (T < 3 * NF32) {
                g = T % 3;
                uo = L::unit_of(16 * (T / 3) + rho, hh_row);
            } else {
                const int s = 16 * (T - 3 * NF32) + rho;
                if (s < 3 * RJ) { g = s / RJ; uo = L::unit_of(16 * NF32 + s % RJ, hh_row); }
                // modes 2 and 3: the spare slots behind the remainder units carry the HEAD rows
                // (g = 3 + o, both lane halves the same row): their kernels read the head of the state that ENTERED a step
                // from its accumulators
                else if ((MODE == 2 || MODE == 3) && s < L::HEAD_SLOT + NOUT) { g = 3 + (s - L::HEAD_SLOT); uo = 0; }
            }
            if (g < 0 || uo >= H) continue;
            auto weight = [&](int ui) -> S {               // (scaled) recurrent weight from unit ui into row (g, uo)
                if (ui >= H) return S(0.0);
                if (g == 0) return sg * Wg[(size_t)(2 + ui) * 2 * H + uo];
                if (g == 1) return sg * Wg[(size_t)(2 + ui) * 2 * H + H + uo];
                if (g == 2) return sc * Wch[(size_t)ui * H + uo];
                return head_w(g - 3, ui);
            };
            if constexpr (MODE != 0) {
                // accumulator start value of this row: bias + one-hot input row (the same for both K halves)
                if (hhk == 0) {
                    float* CI = reinterpret_cast<float*>(img.data() + L::OFF_CI);
                    for (int sgm = 0; sgm < 2; ++sgm) {
                        S v;
                        if (g == 0) v = sg * (bg[uo] + Wg[(size_t)sgm * 2 * H + uo]);
                        else if (g == 1) v = sg * (bg[H + uo] + Wg[(size_t)sgm * 2 * H + H + uo]);
                        else if (g == 2) v = sc * bch[uo];
                        else v = head_b(g - 3);
                        Out::put(&CI[(((size_t)sgm * L::NT + T) * 2 + hh_row) * 16 + rho], v);
                    }
                }
            }
            if constexpr (MODE == 1) {
                // one chain over the concatenated K axis: lane half hhk's flat register list, product by product
                constexpr int ORD[6][2] = {{2, 0}, {1, 1}, {0, 2}, {1, 0}, {0, 1}, {0, 0}};
                for (int ks = 0; ks < L::KS; ++ks)
                    for (int jj = 0; jj < 8; ++jj) {
                        const int fe = 8 * ks + jj, f = fe / 2;
                        if (f >= 6 * L::NRM) continue;
                        const int o = f / L::NRM, e = 2 * (f % L::NRM) + (fe & 1);
                        Out::put_part(&A[(((size_t)ks * L::NT + T) * 64 + lane) * 8 + jj], weight(L::unit_of(e, hhk)), ORD[o][0]);
                    }
                continue;
            }
            if constexpr (MODE == 2) {
                // special unit of K half hhk: parts {w1, w1, w1, w2, w2, w3} against the B entries {h1, h2, h3, h1, h2, h1}
                const S ws = weight(L::unit_of(L::NU - 1, hhk));
                uint16_t* ASP = reinterpret_cast<uint16_t*>(img.data() + L::OFF_ASP);
                const int part[6] = {0, 0, 0, 1, 1, 2};
                for (int jj = 0; jj < 6; ++jj) Out::put_part(&ASP[((size_t)T * 64 + lane) * 8 + jj], ws, part[jj]);
            }
            if constexpr (MODE == 3) {
                // NS special units per K half: entry 6 s + i of the special k-steps = product i of special unit s,
                // A parts {w1, w1, w1, w2, w2, w3} against the B entries {h1, h2, h3, h1, h2, h1}
                uint16_t* ASP = reinterpret_cast<uint16_t*>(img.data() + L::OFF_ASP);
                const int part[6] = {0, 0, 0, 1, 1, 2};
                for (int sp = 0; sp < L::NS; ++sp) {
                    const S ws = weight(L::unit_of(L::NUA + sp, hhk));
                    for (int i = 0; i < 6; ++i) {
                        const int idx = 6 * sp + i;
                        Out::put_part(&ASP[(((size_t)T * L::KSP + idx / 8) * 64 + lane) * 8 + idx % 8], ws, part[i]);
                    }
                }
            }
            for (int x = 0; x < L::NQ; ++x)
                for (int jj = 0; jj < 8; ++jj) {
                    const int e = 8 * x + jj;
                    S w = S(0.0);
                    if (e < L::NUA) {
                        w = weight(L::unit_of(e, hhk));
                    } else if (MODE != 0) {
                        w = S(0.0);
                    } else if (e == L::NU && hhk == 0) {                    // bias (+ input row of spin 0)
                        if (g == 0) w = sg * (bg[uo] + Wg[uo]);
                        else if (g == 1) w = sg * (bg[H + uo] + Wg[H + uo]);
                        else if (g == 2) w = sc * bch[uo];
                        else w = head_b(g - 3);
                    } else if (e == L::NU + 1 && hhk == 0) {                // input row difference, times sigma
                        if (g == 0) w = sg * (Wg[(size_t)2 * H + uo] - Wg[uo]);
                        else if (g == 1) w = sg * (Wg[(size_t)2 * H + H + uo] - Wg[H + uo]);
                    }
                    auto at = [&](int a) { return &A[((((size_t)T * 3 + a) * L::NQ + x) * 64 + lane) * 8 + jj]; };
                    Out::put_parts(at(0), at(1), at(2), w);
                }
        }
    float* XC = reinterpret_cast<float*>(img.data() + L::OFF_XC);
    float* WD = reinterpret_cast<float*>(img.data() + L::OFF_WD);
    float* BD = reinterpret_cast<float*>(img.data() + L::OFF_BD);
    for (int hh = 0; hh < 2; ++hh)
        for (int e = 0; e < L::NU; ++e) {
            const int u = L::unit_of(e, hh);
            if (u >= H) continue;
            for (int sgm = 0; sgm < 2; ++sgm)
                Out::put(&XC[(size_t)(sgm * 2 + hh) * L::NUP + e], sc * (bci[u] + Wci[(size_t)sgm * H + u]));
            for (int o = 0; o < NOUT; ++o) Out::put(&WD[((size_t)hh * L::NUP + e) * NOUT + o], head_w(o, u));
        }
    for (int o = 0; o < NOUT; ++o) Out::put(&BD[o], head_b(o));
    return img;
}

// ---- the g-state form of the MODE 2 image (split_pp.h: SplitPP<.., GSTATE>) ------------------------------------------------------
// The ping-pong step that carries g = (h + 1) / 2 instead of h reads a second variant of the image.  With h = 2 g - 1 a row's
// pre-activation b + sum_j W_j h_j is (b - sum_j W_j) + sum_j (2 W_j) g_j, so
//   * every weight that multiplies the state is doubled - all bf16 parts of the K entries of the r, u, q and head rows (regular and
//     special fragments) and the VALU head's table OFF_WD; doubling is exact in every part;
//   * every constant such a row starts from - the table OFF_CI that preload reads, the VALU head's OFF_BD - is less the row's weight
//     sum: float64, over the f32 weights w1 + w2 + w3 the image holds, in the order of the image, rounded to f32 once;
//   * OFF_XC (the candidate's input side) never meets the state and stays.
// The variant is a function of the h image alone, word by word (gstate_word), so the host packer and device-resident training
// (split.hip: split_gstate_refold, behind train.hip's re-pack of the h image) run the same code and agree bit for bit; a sum over a
// weight row is nothing an element table (pack_value.h: Lin) could hold.
// Padded units (widths below 50) need no case: their weight columns, rows and constants are zero in the h image, so they add
// nothing to a sum, and their own pre-activations stay 0 - then t = u = 0.5 and g' = t + u (g - t) keeps the g = 0.5 such a unit
// enters with (h = 0 in the checkpoint); whatever it held would feed nothing.
struct GstateLayout {
    int NT, NQ, NUP, NOUT;
    uint32_t OFF_ASP, OFF_CI, OFF_XC, OFF_WD, OFF_BD, BYTES;   // the ten fields rnnwf_host_split_images returns
    int NF32, RJ;                                              // where a unit's gate rows lie (gstate_range_unit)
};
template <class L>
constexpr GstateLayout gstate_layout() {
    static_assert(L::MODE == 2 && L::OFF_A == 0, "the g-state form exists for the K-packed layout of the ping-pong kernels");
    static_assert(L::NOUT <= (int)kGstateRangeSlot, "the range word takes a head-bias word no head row uses");
    return {L::NT, L::NQ, L::NUP, L::NOUT, (uint32_t)L::OFF_ASP, (uint32_t)L::OFF_CI, (uint32_t)L::OFF_XC, (uint32_t)L::OFF_WD, (uint32_t)L::OFF_BD,
            (uint32_t)L::BYTES, L::NF32, L::RJ};   // (the range word: split_core.h, kGstateRangeSlot)
}
__host__ __device__ inline float gstate_bf16(uint16_t b) {
    union { uint32_t u; float f; } x;
    x.u = (uint32_t)b << 16;
    return x.f;
}
__host__ __device__ inline uint32_t gstate_bits(float f) {
    union { uint32_t u; float f; } x;
    x.f = f;
    return x.u;
}
// 32-bit word w of the g-state image, from the h image `img`
__host__ __device__ inline uint32_t gstate_word(const GstateLayout& g, const char* img, uint32_t w) {
    const uint32_t off = 4 * w, in = reinterpret_cast<const uint32_t*>(img)[w];
    const uint16_t* A = reinterpret_cast<const uint16_t*>(img);
    if (off < g.OFF_CI) {                                      // two bf16 weight parts, each doubled (x + x: exact, a bf16 again)
        const float lo = gstate_bf16((uint16_t)(in & 0xffffu)), hi = gstate_bf16((uint16_t)(in >> 16));
        return (gstate_bits(lo + lo) >> 16) | (gstate_bits(hi + hi) & 0xffff0000u);
    }
    if (off < g.OFF_XC) {                                      // CI[sigma][T][hh_row][rho]: less the weight sum of row (T, r32)
        const int i = (int)((off - g.OFF_CI) / 4), rho = i & 15, hh_row = (i >> 4) & 1, T = (i >> 5) % g.NT;
        const int r32 = (rho & 3) | (hh_row << 2) | ((rho >> 2) << 3);
        double sum = 0.0;
        for (int hhk = 0; hhk < 2; ++hhk) {
            const int lane = 32 * hhk + r32;
            for (int x = 0; x < g.NQ; ++x)
                for (int jj = 0; jj < 8; ++jj) {
                    float wv = 0.0f;                           // w3 + w2 + w1: exact, the split was
                    for (int a = 2; a >= 0; --a) wv += gstate_bf16(A[((((size_t)T * 3 + a) * g.NQ + x) * 64 + lane) * 8 + jj]);
                    sum += (double)wv;
                }
            const uint16_t* sp = A + g.OFF_ASP / 2 + ((size_t)T * 64 + lane) * 8;      // special unit: entries {w1, w1, w1, w2, w2, w3}
            sum += (double)((gstate_bf16(sp[5]) + gstate_bf16(sp[3])) + gstate_bf16(sp[0]));
        }
        return gstate_bits((float)((double)reinterpret_cast<const float*>(img)[w] - sum));
    }
    if (off < g.OFF_WD) return in;                             // XC
    const float* WD = reinterpret_cast<const float*>(img + g.OFF_WD);
    if (off < g.OFF_BD) { const float v = reinterpret_cast<const float*>(img)[w]; return gstate_bits(v + v); }
    const int o = (int)((off - g.OFF_BD) / 4);
    if (o >= g.NOUT) return in;
    double sum = 0.0;
    for (int e = 0; e < 2 * g.NUP; ++e) sum += (double)WD[(size_t)e * g.NOUT + o];
    return gstate_bits((float)((double)reinterpret_cast<const float*>(img)[w] - sum));
}
// ---- the range word: may the step take ONE reciprocal for update gate and candidate? (split_pp.h: gate_batch, MERGED) -------------
// With Eu = exp2(a_u) and Ec = exp2(a_c) the merged form divides by (1 + Eu)(1 + Ec), which must stay finite in f32:
// (1 + 2^a)(1 + 2^b) <= 2^(a + b + 2) < 2^128 needs a + b <= 125 for a, b >= 0.  gstate_range_unit bounds that sum for the unit at
// entry e of lane half hh over EVERY state and both input spins, in the exponent units the image is scaled to:
//     A_u >= |a_u|             = max over sigma of |start-table entry of the u row| + sum of |w1 + w2 + w3| over the row's K entries,
//     A_c >= |xc + r q|, r in [0, 1]:  max over sigma of |xc| + max over sigma of |start-table entry of the q row| + the q row's sum.
// (|h| <= 1 in the h form is g in [0, 1] in the g form: the same interval of pre-activations, so the h image gives the bound for the g
// image's step.)  Absolute values throughout, so both bounds are >= 0 and a gate that underflows counts like one that overflows: the
// bound errs to the safe side.  The image is in range iff the largest sum is <= kGstateRangeLimit = 120: five exponents are left for
// the f32 rounding of the accumulated pre-activations (each below 2^-17 of A) and of g itself.  float64, additions and comparisons only,
// in the order of the image: host and device agree bit for bit, as gstate_word's sums do.  Padded units give 0.
constexpr double kGstateRangeLimit = 120.0;
__host__ __device__ inline double gstate_max(double a, double b) { return (a > b || a != a) ? a : b; }      // a NaN stays (then: out of range)
__host__ __device__ inline double gstate_row_abs_sum(const GstateLayout& g, const char* img, int T, int r32) {
    const uint16_t* A = reinterpret_cast<const uint16_t*>(img);
    double sum = 0.0;
    for (int hhk = 0; hhk < 2; ++hhk) {
        const int lane = 32 * hhk + r32;
        for (int x = 0; x < g.NQ; ++x)
            for (int jj = 0; jj < 8; ++jj) {
                float wv = 0.0f;                               // w3 + w2 + w1: exact
                for (int a = 2; a >= 0; --a) wv += gstate_bf16(A[((((size_t)T * 3 + a) * g.NQ + x) * 64 + lane) * 8 + jj]);
                sum += fabs((double)wv);
            }
        const uint16_t* sp = A + g.OFF_ASP / 2 + ((size_t)T * 64 + lane) * 8;
        sum += fabs((double)((gstate_bf16(sp[5]) + gstate_bf16(sp[3])) + gstate_bf16(sp[0])));
    }
    return sum;
}
__host__ __device__ inline double gstate_range_unit(const GstateLayout& g, const char* img, int e, int hh) {
    const float* CI = reinterpret_cast<const float*>(img + g.OFF_CI);
    const float* XC = reinterpret_cast<const float*>(img + g.OFF_XC);
    double A = 0.0;
    for (int gate = 1; gate <= 2; ++gate) {                    // 1: u row, 2: q row of the unit (split_pp.h: slots)
        const int s = gate * g.RJ + (e - 16 * g.NF32);
        const int T = e < 16 * g.NF32 ? 3 * (e / 16) + gate : 3 * g.NF32 + s / 16, rho = e < 16 * g.NF32 ? e % 16 : s % 16;
        const int r32 = (rho & 3) | (hh << 2) | ((rho >> 2) << 3);
        double c = 0.0;
        for (int sgm = 0; sgm < 2; ++sgm) c = gstate_max(c, fabs((double)CI[(((size_t)sgm * g.NT + T) * 2 + hh) * 16 + rho]));
        A += c + gstate_row_abs_sum(g, img, T, r32);
    }
    double xc = 0.0;
    for (int sgm = 0; sgm < 2; ++sgm) xc = gstate_max(xc, fabs((double)XC[(size_t)(sgm * 2 + hh) * g.NUP + e]));
    return A + xc;
}
// the largest bound of the image (host; device-resident training: split.hip, gstate_range_kernel) and the word that says "in range"
inline double gstate_range(const GstateLayout& g, const char* img) {
    double m = 0.0;
    for (int hh = 0; hh < 2; ++hh)
        for (int e = 0; e < 16 * g.NF32 + g.RJ; ++e) m = gstate_max(m, gstate_range_unit(g, img, e, hh));
    return m;
}
__host__ __device__ inline uint32_t gstate_range_word(double bound) { return bound <= kGstateRangeLimit ? 1u : 0u; }
__host__ __device__ inline uint32_t gstate_range_word_index(const GstateLayout& g) { return g.OFF_BD / 4 + kGstateRangeSlot; }

inline std::vector<char> gstate_image(const GstateLayout& g, const std::vector<char>& img) {
    std::vector<char> out(img.size());
    for (uint32_t w = 0; w < g.BYTES / 4; ++w) reinterpret_cast<uint32_t*>(out.data())[w] = gstate_word(g, img.data(), w);
    reinterpret_cast<uint32_t*>(out.data())[gstate_range_word_index(g)] = gstate_range_word(gstate_range(g, img.data()));
    return out;
}

// Image of GRU layer `layer` >= 1 on the bf16x3 engine (split_core.h: SplitUpperLayout): the X block (input = state of the layer
// below) and the H block, each laid out as the MODE 2 image of the first layer, the biases as accumulator start values, and - for
// the top layer - the head rows in the H block's spare mixed-tile slots plus the VALU head's tables.
template <int NF32, int RJ, int NOUT, class S = double>
std::vector<char> pack_split_upper_image(const rnnwf_handle* h, int layer, bool top) {
    using U = SplitUpperLayout<NF32, RJ, NOUT>;
    using L = typename U::L0;
    using Out = PackSink<S>;
    const int H = h->H;
    std::vector<char> img(U::BYTES, 0);
    Out::begin(img);
    const std::string pre = "multi_rnn_cell/cell_" + std::to_string(layer) + "/cudnn_compatible_gru_cell/";
    const auto Wg = pvs<S>(h, pre + "gates/kernel");                         // [H + H, 2H]: input rows first, cols r | u
    const auto bg = pvs<S>(h, pre + "gates/bias");
    const auto Wci = pvs<S>(h, pre + "candidate/input_projection/kernel");   // [H, H]
    const auto bci = pvs<S>(h, pre + "candidate/input_projection/bias");
    const auto Wch = pvs<S>(h, pre + "candidate/hidden_projection/kernel");  // [H, H]
    const auto bch = pvs<S>(h, pre + "candidate/hidden_projection/bias");
    const auto Wd = pvs<S>(h, NOUT == 1 ? "wf_dense/kernel" : "wf_dense_ampl/kernel");
    const auto bd = pvs<S>(h, NOUT == 1 ? "wf_dense/bias" : "wf_dense_ampl/bias");
    const double sg = PackScale<float>::gate, sc = PackScale<float>::cand;
    auto head_w = [&](int o, int ui) -> S {
        if (o == 0) return Wd[(size_t)ui * 2 + 1] - Wd[(size_t)ui * 2];
        return pvs<S>(h, "wf_dense_phase/kernel")[(size_t)ui * 2 + (o - 1)];
    };
    auto head_b = [&](int o) -> S {
        if (o == 0) return bd[1] - bd[0];
        return pvs<S>(h, "wf_dense_phase/bias")[o - 1];
    };
    for (int blk = 0; blk < 2; ++blk) {
        const bool xb = blk == 0;
        uint16_t* A = reinterpret_cast<uint16_t*>(img.data() + (xb ? U::OFF_AX : U::OFF_AH));
        uint16_t* ASP = reinterpret_cast<uint16_t*>(img.data() + (xb ? U::OFF_AX : U::OFF_AH) + L::OFF_ASP);
        for (int T = 0; T < L::NT; ++T)
            for (int lane = 0; lane < 64; ++lane) {
                const int r32 = lane & 31, hhk = lane >> 5;
                const int hh_row = (r32 >> 2) & 1, rho = (r32 & 3) + 4 * (r32 >> 3);
                int g = -1, uo = -1;                            // g: 0 r, 1 u, 2 candidate (X: y, H: q), 3 + o: head row o (H block, top layer)
                if (T < 3 * NF32) {
                    g = T % 3;
                    uo = L::unit_of(16 * (T / 3) + rho, hh_row);
                } else {
                    const int sl = 16 * (T - 3 * NF32) + rho;
                    if (sl < 3 * RJ) { g = sl / RJ; uo = L::unit_of(16 * NF32 + sl % RJ, hh_row); }
                    else if (!xb && top && sl < L::HEAD_SLOT + NOUT) { g = 3 + (sl - L::HEAD_SLOT); uo = 0; }
                }
                if (g < 0 || uo >= H) continue;
                auto weight = [&](int ui) -> S {               // (scaled) weight from input unit ui into row (g, uo)
                    if (ui >= H) return S(0.0);
                    const size_t row = xb ? (size_t)ui : (size_t)(H + ui);
                    if (g == 0) return sg * Wg[row * 2 * H + uo];
                    if (g == 1) return sg * Wg[row * 2 * H + H + uo];
                    if (g == 2) return xb ? sc * Wci[(size_t)ui * H + uo] : sc * Wch[(size_t)ui * H + uo];
                    return head_w(g - 3, ui);
                };
                {   // special unit of K half hhk: parts {w1, w1, w1, w2, w2, w3} against the B entries {h1, h2, h3, h1, h2, h1}
                    const S ws = weight(L::unit_of(L::NU - 1, hhk));
                    const int part[6] = {0, 0, 0, 1, 1, 2};
                    for (int jj = 0; jj < 6; ++jj) Out::put_part(&ASP[((size_t)T * 64 + lane) * 8 + jj], ws, part[jj]);
                    // K entries 6, 7 of both halves meet the constant 1.0: the three parts of the row's bias.  The r / u biases enter
                    // once, through the X block; the H block carries the candidate's hidden bias and the head biases.
                    S bias = S(0.0);
                    if (g == 0) { if (xb) bias = sg * bg[uo]; }
                    else if (g == 1) { if (xb) bias = sg * bg[H + uo]; }
                    else if (g == 2) bias = xb ? sc * bci[uo] : sc * bch[uo];
                    else bias = head_b(g - 3);
                    uint16_t* b6 = &ASP[((size_t)T * 64 + lane) * 8 + 6];
                    uint16_t* b7 = &ASP[((size_t)T * 64 + lane) * 8 + 7];
                    if (hhk == 0) { Out::put_part(b6, bias, 0); Out::put_part(b7, bias, 1); }
                    else { Out::put_part(b6, bias, 2); }
                }
                for (int x = 0; x < L::NQ; ++x)
                    for (int jj = 0; jj < 8; ++jj) {
                        const int e = 8 * x + jj;
                        auto at = [&](int a) { return &A[((((size_t)T * 3 + a) * L::NQ + x) * 64 + lane) * 8 + jj]; };
                        Out::put_parts(at(0), at(1), at(2), e < L::NUA ? weight(L::unit_of(e, hhk)) : S(0.0));
                    }
            }
    }
    if (top) {
        float* WD = reinterpret_cast<float*>(img.data() + U::OFF_WD);
        float* BD = reinterpret_cast<float*>(img.data() + U::OFF_BD);
        for (int hh = 0; hh < 2; ++hh)
            for (int e = 0; e < L::NU; ++e) {
                const int u = L::unit_of(e, hh);
                if (u >= H) continue;
                for (int o = 0; o < NOUT; ++o) Out::put(&WD[((size_t)hh * L::NUP + e) * NOUT + o], head_w(o, u));
            }
        for (int o = 0; o < NOUT; ++o) Out::put(&BD[o], head_b(o));
    }
    return img;
}

}  // namespace rnnwf
