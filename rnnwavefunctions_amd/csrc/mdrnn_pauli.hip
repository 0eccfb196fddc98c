// mdrnn_pauli.hip - host driver of rnnwf_pauli_step_2d (include/rnnwf.h): expectation values of Pauli strings and the local energy
// of any real-symmetric spin-1/2 Hamiltonian given as terms (flip mask, sign mask, coefficient), for the 2D RNN (MDRNN2D, float64);
// kernels in mdrnn_pauli_kernels.h and, from the log-ratios on, pauli_kernels.h; the method in docs/pauli_2d.md.
//
// Per call: the masks, given by LATTICE index k = nx Ny + ny, are checked, mapped to visit order and packed into words; the terms
// are grouped by flip mask and the distinct masks sorted longest tail first.  Per pass of whole 16-chain blocks (the state budget):
// spins (the caller's, or drawn exactly as rnnwf_sample draws them) with the family's base pass, which keeps every position's state
// in h->hck and log P in h->out_lp -> site terms -> masked tails -> log-ratios, per-term sums of v and v^2, E_loc and its moments.
// The sums of the passes are added on the host in pass order.  A call that ran in one pass leaves its batch (bits, states, E_loc)
// resident for rnnwf_vmc_gradient.
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "mdrnn_pauli_kernels.h"
#include "observable.h"
#include "pauli_kernels.h"

using namespace rnnwf;

namespace {

constexpr int kMaxMasks = 65535;         // blockIdx.y of the log-ratio kernel
const char* const kEntry = "rnnwf_pauli_step_2d";

template <int NFULL_, int WAVES_>
struct MdPauliLaunch {
    using L = MdLayout<NFULL_>;
    static constexpr int NFULL = NFULL_, WAVES = WAVES_;
    static constexpr size_t TAIL_LDS = L::BYTES + (size_t)WAVES * L::WORDS_BYTES;     // image + the waves' spin words
    static constexpr size_t HS_BYTES_PER_BLOCK = (size_t)((L::KT + 1) / 2) * 64 * 16;
    static double mfma_flops_per_step() { return (double)NFULL * 2 * L::KT * 2048.0; }
};

// the rows of mdrnn.hip's with_width
template <class Fn>
bool with_md_width(const rnnwf_handle* h, Fn&& fn) {
    switch (h->NFULL) {
        case 1: fn(MdPauliLaunch<1, 4>()); return true;
        case 2: fn(MdPauliLaunch<2, 4>()); return true;
        case 3: fn(MdPauliLaunch<3, 4>()); return true;
        case 4: fn(MdPauliLaunch<4, 4>()); return true;
        case 5: fn(MdPauliLaunch<5, 4>()); return true;
    }
    return false;
}

// The terms of one call as the kernels read them: everything in visit order
struct Terms {
    int K = 0, M = 0, W = 0;
    std::vector<uint32_t> mask, sgn;     // [M][W] distinct non-empty flip masks in order of first appearance; [K][W] sign masks
    std::vector<int32_t> tmask;          // [K]: the term's row of `mask`, -1 for a diagonal term
    std::vector<int32_t> first, order;   // [M]: first flipped position f; the masks f ascending, ties by index
    bool replay = false;                 // some mask has f >= 1: the own suffixes need the replayed site terms
    double steps = 0.0;                  // sum over masks of N - 1 - f: cell evaluations per chain
};

// Scratch of one pass of ns chains in h->renyi; the call's tables lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, sgn, tmask, coeff, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per term
    Scratch(int N, const Terms& g, int64_t ns) {
        Carve c;
        const size_t M = (size_t)std::max(g.M, 1), K = (size_t)g.K;
        nblk = (ns + kPauliThreads - 1) / kPauliThreads;
        mask = c.take(M * g.W * 4);
        order = c.take(M * 4);
        first = c.take(M * 4);
        sgn = c.take(K * g.W * 4);
        tmask = c.take(K * 4);
        coeff = c.take(K * 8);
        terms = c.take((size_t)N * ns * 8);
        tail = c.take(M * ns * 8);
        lr = c.take(M * ns * 8);
        part = c.take(K * nblk * 16);
        sums = c.take(K * 16);
        bytes = c.bytes;
    }
};

// visit position of lattice site k = nx Ny + ny (mdrnn.hip: get_maps)
int pos_of_site(const rnnwf_handle* h, int k) {
    const int nx = k / h->Ny, ny = k % h->Ny;
    return ny * h->Nx + (ny % 2 == 0 ? nx : h->Nx - 1 - nx);
}

// check the (K, N) lattice-indexed flip and sign masks, pack them in visit order, group the terms by flip mask, sort the masks
int prepare(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, int K, Terms& g) {
    const int N = h->N;
    g.K = K;
    g.W = (N + 31) / 32;
    g.sgn.assign((size_t)K * g.W, 0u);
    g.tmask.assign(K, -1);
    std::vector<int> pos(N);
    for (int k = 0; k < N; ++k) pos[k] = pos_of_site(h, k);
    std::map<std::vector<uint32_t>, int32_t> seen;
    std::vector<uint32_t> words(g.W);
    for (int k = 0; k < K; ++k) {
        const int32_t *fk = flip + (size_t)k * N, *sk = sign + (size_t)k * N;
        std::fill(words.begin(), words.end(), 0u);
        int f = N;
        for (int n = 0; n < N; ++n) {
            if (fk[n] != 0 && fk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: flip[%d][%d] = %d, a mask entry must be 0 or 1", kEntry, k, n, (int)fk[n]);
            if (sk[n] != 0 && sk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: sign[%d][%d] = %d, a mask entry must be 0 or 1", kEntry, k, n, (int)sk[n]);
            const int p = pos[n];
            if (fk[n]) {
                words[p >> 5] |= 1u << (p & 31);
                f = std::min(f, p);
            }
            if (sk[n]) g.sgn[(size_t)k * g.W + (p >> 5)] |= 1u << (p & 31);
        }
        if (f == N) continue;                      // diagonal term: no cell evaluation
        auto it = seen.find(words);
        if (it == seen.end()) {
            if (g.M == kMaxMasks) return h->fail(RNNWF_ERR_INVALID, "%s: more than %d distinct flip masks", kEntry, kMaxMasks);
            it = seen.emplace(words, g.M++).first;
            g.mask.insert(g.mask.end(), words.begin(), words.end());
            g.first.push_back(f);
            g.order.push_back(it->second);
            g.steps += (double)(N - 1 - f);
            if (f > 0) g.replay = true;
        }
        g.tmask[k] = it->second;
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    return 0;
}

// one pass over the ns chains packed in h->bits, their states in h->hck and log P in h->out_lp (the family's base pass): sums_host
// (K, 2) of this pass; the log-ratios stay in h->renyi, E_loc in h->eloc
int pauli_pass(rnnwf_handle* h, int64_t ns, const Terms& g, const Scratch& sc, double* sums_host) {
    const int N = h->N, K = g.K, M = g.M;
    if (int rc = ensure(h, h->eloc, (size_t)ns * 8)) return rc;
    char* buf = (char*)h->renyi.p;
    double* lr = (double*)(buf + sc.lr);
    const uint32_t* bits = (const uint32_t*)h->bits.p;
    if (M > 0) {
        MdPauliArgs a{};
        a.wimg = h->wimg.p;
        a.N = N;
        a.Nx = h->Nx;
        a.rem = h->H - 16 * h->NFULL;
        a.W = g.W;
        a.ns = ns;
        a.nsb = (ns + kChains - 1) / kChains;
        a.bits = bits;
        a.hs = (const double*)h->hck.p;
        a.terms = (double*)(buf + sc.terms);
        a.mask = (const uint32_t*)(buf + sc.mask);
        a.order = (const int32_t*)(buf + sc.order);
        a.first = (const int32_t*)(buf + sc.first);
        a.tail = (double*)(buf + sc.tail);
        a.ntiles = (int64_t)M * a.nsb;
        int rc = 0;
        with_md_width(h, [&](auto k) {
            using P = decltype(k);
            using L = typename P::L;
            if (g.replay)
                rc = launch_persistent(h, kTimerBase, mdrnn_site_terms_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::BYTES, a.nsb, P::WAVES, a);
            if (rc) return;
            const auto kern = mdrnn_masked_tail_kernel<P::NFULL, P::WAVES>;
            unsigned grid = 0;
            if ((rc = persistent_grid(h, kern, P::WAVES * 64, P::TAIL_LDS, a.ntiles, P::WAVES, &grid))) return;
            if ((rc = ensure(h, h->rowbuf, (size_t)grid * P::WAVES * a.Nx * P::HS_BYTES_PER_BLOCK))) return;      // one slot per lattice column
            a.ring = (double*)h->rowbuf.p;
            rc = timed_launch(h, kTimerFlip, kern, grid, P::WAVES * 64, P::TAIL_LDS, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * P::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over masks of N - 1 - f cell evaluations per chain
        if (int rc2 = timed_launch(h, kTimerAssembly, pauli_log_ratio_kernel, dim3((unsigned)sc.nblk, (unsigned)M), kPauliThreads, 0,
                                   (const double*)a.tail, (const double*)a.terms, (const double*)h->out_lp.p, a.first, N, ns, lr))
            return rc2;
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        const uint32_t* sgn = (const uint32_t*)(buf + sc.sgn);
        const int32_t* tmask = (const int32_t*)(buf + sc.tmask);
        pauli_term_kernel<<<(unsigned)(K * sc.nblk), kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, lr, g.W, ns, sc.nblk,
                                                                                   (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)K, kPauliThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
        pauli_eloc_kernel<<<(unsigned)sc.nblk, kPauliThreads, 0, h->stream>>>(bits, sgn, tmask, (const double*)(buf + sc.coeff), lr, K, g.W,
                                                                             ns, (double*)h->eloc.p);
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)K * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

const char* model_name(int model) {
    static const char* const names[] = {"GRU1D", "GRU1D_PARITY", "CRNN_U1", "GRU1D_F64", "MDRNN2D", "LSTM1D_F64"};
    return model >= 0 && model < (int)(sizeof names / sizeof *names) ? names[model] : "unknown";
}

}  // namespace

extern "C" int rnnwf_pauli_step_2d(rnnwf_handle* h, const int32_t* flip, const int32_t* sign, const double* coeff, int32_t nterms,
                                   const int32_t* samples, int64_t ns, uint64_t seed, uint64_t step, int64_t sample_offset,
                                   double* term_sums, double* out_eloc, double* moments, double* out_log_ratio, int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck, h->eloc) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (h->model != RNNWF_MODEL_MDRNN2D)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the 2D RNN (MDRNN2D) only, this handle's model is %s; rnnwf_pauli_step serves the GRU models",
                       kEntry, model_name(h->model));
    size_t hs_bytes = 0;
    if (!with_md_width(h, [&](auto k) { hs_bytes = decltype(k)::HS_BYTES_PER_BLOCK; }))
        return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for num_units = %d (the 2D RNN's kernels serve 1..84)", kEntry, h->H);
    if (!h->committed) return h->fail(RNNWF_ERR_INVALID, "%s: parameters not committed (call rnnwf_commit_params)", kEntry);
    if (nterms < 1) return h->fail(RNNWF_ERR_INVALID, "%s: nterms must be >= 1", kEntry);
    if (ns < 1) return h->fail(RNNWF_ERR_INVALID, "%s: ns must be >= 1", kEntry);
    if (!flip || !sign || !coeff || !term_sums)
        return h->fail(RNNWF_ERR_INVALID, "%s: flip, sign, coeff and term_sums must be non-null", kEntry);
    if (!samples && sample_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: sample_offset must be >= 0", kEntry);
    Terms g;
    if (int rc = prepare(h, flip, sign, nterms, g)) return rc;
    const int N = h->N, K = nterms, M = g.M;
    // chains per pass: the family's pass holds N states per block in its budget; beside them, per block, the terms (N x 16 x 8
    // bytes), the tails and log-ratios (2 x M x 16 x 8), log P and E_loc (2 x 16 x 8)
    const size_t budget = (size_t)(h->family->max_chains_per_pass(h) / kChains) * N * hs_bytes;
    const size_t per_block = (size_t)N * hs_bytes + (size_t)(N + 2 + 2 * M) * kChains * 8;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / per_block)) * kChains;
    if ((int64_t)K * ((std::min(chunk, ns) + kPauliThreads - 1) / kPauliThreads) > 0x7fffffffLL)
        return h->fail(RNNWF_ERR_INVALID, "%s: nterms x ceil(ns / %d) exceeds the grid of the term kernel; split the batch", kEntry, kPauliThreads);
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int32_t *col_of_pos, *pos_of_site_dev;
    if (int rc = h->family->site_maps(h, &col_of_pos, &pos_of_site_dev)) return rc;
    // the first pass is the largest: one allocation for the call, the tables uploaded once
    const Scratch big(N, g, std::min(chunk, ns));
    if (int rc = ensure(h, h->renyi, big.bytes)) return rc;
    {
        char* buf = (char*)h->renyi.p;
        if (M) {
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.order, g.order.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
            RNNWF_HIP(h, hipMemcpyAsync(buf + big.first, g.first.data(), (size_t)M * 4, hipMemcpyHostToDevice, h->stream));
        }
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.sgn, g.sgn.data(), g.sgn.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.tmask, g.tmask.data(), (size_t)K * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.coeff, coeff, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits, h->hck and h->eloc are overwritten from here on
    h->call_ns = ns;
    std::vector<double> total((size_t)K * 2, 0.0), pass_sums((size_t)K * 2);
    double mom[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t s0 = 0; s0 < ns; s0 += chunk) {
        const int64_t n = std::min(chunk, ns - s0);
        // spins into h->bits, every position's state into h->hck, log P into h->out_lp
        if (int rc = ensure(h, h->bits, (size_t)g.W * n * 4)) return rc;
        if (samples) {
            if (int rc = upload_and_pack(h, samples + s0 * N, n, h->bits, 0, col_of_pos)) return rc;
            if (int rc = h->family->base(h, n, nullptr)) return rc;
        } else {
            const Draw d{seed, step, sample_offset + s0};      // rnnwf_sample's draw: the same kernel, which keeps the states as it goes
            if (int rc = h->family->base(h, n, &d)) return rc;
            if (out_samples)
                if (int rc = unpack_and_download(h, h->bits, n, out_samples + s0 * N, pos_of_site_dev)) return rc;
        }
        const Scratch sc(N, g, n);
        if (int rc = pauli_pass(h, n, g, sc, pass_sums.data())) return rc;
        if (out_log_ratio && M)
            RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + s0, (size_t)ns * 8, (char*)h->renyi.p + sc.lr, (size_t)n * 8, (size_t)n * 8,
                                          (size_t)M, hipMemcpyDeviceToHost, h->stream));
        if (out_eloc) RNNWF_HIP(h, hipMemcpyAsync(out_eloc + s0, h->eloc.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
        if (moments) {                                               // synchronises the stream
            double pm[4];
            if (int rc = run_moments(h, h->eloc.p, n, false, pm)) return rc;
            for (int k = 0; k < 3; ++k) mom[k] += pm[k];
        }
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass_sums[k];
    }
    memcpy(term_sums, total.data(), total.size() * 8);
    if (moments) memcpy(moments, mom, sizeof mom);
    // one pass: bits, states and E_loc of the whole batch are on the device, as rnnwf_vmc_step leaves them
    if (ns <= chunk) h->last_ns = ns;
    return RNNWF_OK;
}
