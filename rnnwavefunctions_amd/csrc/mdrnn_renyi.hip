// mdrnn_renyi.hip - host driver of rnnwf_renyi2_regions_2d (include/rnnwf.h): the second Renyi entropy of arbitrary lattice regions
// for the 2D RNN (MDRNN2D, float64) by the replica swap trick; kernels in mdrnn_pauli_kernels.h (mdrnn_site_terms_kernel and
// mdrnn_masked_tail_kernel<..., PAIRED = true>) and, from the tails on, renyi_region_kernels.h; the method in docs/renyi_2d.md.
//
// Per call: the masks, given by LATTICE index k = nx Ny + ny, are checked, mapped to visit order, normalised (position 0 of the path
// not in A: r_A = r_complement), packed into words and sorted longest mixed chain first.  Per pass of whole 16-chain blocks (the state
// budget): spins (the caller's, or drawn exactly as rnnwf_sample draws them) with the family's base pass, which keeps every position's
// state in h->hck -> site terms -> paired masked tails -> log-ratios and per-region sums of r and r^2.  The sums of the passes are
// added on the host in pass order.  The launch table and the lattice -> path map restate mdrnn_pauli.hip's, whose driver is its own.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mdrnn_pauli_kernels.h"
#include "observable.h"
#include "renyi_region_kernels.h"

using namespace rnnwf;

namespace {

constexpr int kMaxRegions = 65535;       // blockIdx.y of the assembly
const char* const kEntry = "rnnwf_renyi2_regions_2d";

// mdrnn_pauli.hip's MdPauliLaunch
template <int NFULL_, int WAVES_>
struct MdRenyiLaunch {
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
        case 1: fn(MdRenyiLaunch<1, 4>()); return true;
        case 2: fn(MdRenyiLaunch<2, 4>()); return true;
        case 3: fn(MdRenyiLaunch<3, 4>()); return true;
        case 4: fn(MdRenyiLaunch<4, 4>()); return true;
        case 5: fn(MdRenyiLaunch<5, 4>()); return true;
    }
    return false;
}

// The regions of one call as the kernels read them: everything in visit order
struct Regions {
    int R = 0, W = 0, nact = 0;
    std::vector<uint32_t> mask;          // [R][W], normalised
    std::vector<int32_t> first, order;   // [R]: first position f of A, 0 = empty; [nact]: non-empty regions, f ascending, ties by index
    double steps = 0.0;                  // sum over non-empty regions of N - 1 - f: cell evaluations per chain
};

// Scratch of one pass of ns chains in h->renyi; the call's masks, order and first positions lead, at offsets that do not depend on ns
struct Scratch {
    size_t mask, order, first, terms, tail, lr, part, sums, bytes;
    int64_t nblk;      // assembly blocks per region
    Scratch(int N, int R, int W, int64_t ns) {
        Carve c;
        nblk = (ns / 2 + kRenyiThreads - 1) / kRenyiThreads;
        mask = c.take((size_t)R * W * 4);
        order = c.take((size_t)R * 4);
        first = c.take((size_t)R * 4);
        terms = c.take((size_t)N * ns * 8);
        tail = c.take((size_t)R * ns * 8);
        lr = c.take((size_t)R * (ns / 2) * 8);
        part = c.take((size_t)R * nblk * 16);
        sums = c.take((size_t)R * 16);
        bytes = c.bytes;
    }
};

// visit position of lattice site k = nx Ny + ny (mdrnn.hip: get_maps)
int pos_of_site(const rnnwf_handle* h, int k) {
    const int nx = k / h->Ny, ny = k % h->Ny;
    return ny * h->Nx + (ny % 2 == 0 ? nx : h->Nx - 1 - nx);
}

// check the (R, N) lattice-indexed masks, map them to visit order, normalise, pack and sort them
int prepare(rnnwf_handle* h, const int32_t* regions, int R, Regions& g) {
    const int N = h->N;
    g.R = R;
    g.W = (N + 31) / 32;
    g.mask.assign((size_t)R * g.W, 0u);
    g.first.assign(R, 0);
    std::vector<int> site_of_pos(N);
    for (int k = 0; k < N; ++k) site_of_pos[pos_of_site(h, k)] = k;
    for (int r = 0; r < R; ++r) {
        const int32_t* m = regions + (size_t)r * N;
        for (int k = 0; k < N; ++k)
            if (m[k] != 0 && m[k] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: regions[%d][%d] = %d, a mask entry must be 0 or 1", kEntry, r, k, (int)m[k]);
        const int32_t flip = m[site_of_pos[0]];    // position 0 in A: take the complement
        for (int p = 0; p < N; ++p)
            if (m[site_of_pos[p]] ^ flip) {
                g.mask[(size_t)r * g.W + (p >> 5)] |= 1u << (p & 31);
                if (!g.first[r]) g.first[r] = p;
            }
        if (g.first[r]) {
            g.order.push_back(r);
            g.steps += (double)(N - 1 - g.first[r]);
        }
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    g.nact = (int)g.order.size();
    return 0;
}

// one pass over the ns chains packed in h->bits, their states in h->hck (the family's base pass): sums_host (R, 2) of this pass; the
// log-ratios stay in h->renyi
int region_pass(rnnwf_handle* h, int64_t ns, const Regions& g, const Scratch& sc, double* sums_host) {
    const int N = h->N, R = g.R;
    char* buf = (char*)h->renyi.p;
    MdPauliArgs a{};
    a.wimg = h->wimg.p;
    a.N = N;
    a.Nx = h->Nx;
    a.rem = h->H - 16 * h->NFULL;
    a.W = g.W;
    a.ns = ns;
    a.nsb = (ns + kChains - 1) / kChains;
    a.bits = (const uint32_t*)h->bits.p;
    a.hs = (const double*)h->hck.p;
    a.terms = (double*)(buf + sc.terms);
    a.mask = (const uint32_t*)(buf + sc.mask);
    a.order = (const int32_t*)(buf + sc.order);
    a.first = (const int32_t*)(buf + sc.first);
    a.tail = (double*)(buf + sc.tail);
    a.ntiles = (int64_t)g.nact * a.nsb;
    if (g.nact > 0) {                              // N >= 2
        int rc = 0;
        with_md_width(h, [&](auto k) {
            using P = decltype(k);
            using L = typename P::L;
            rc = launch_persistent(h, kTimerBase, mdrnn_site_terms_kernel<P::NFULL, P::WAVES>, P::WAVES * 64, L::BYTES, a.nsb, P::WAVES, a);
            if (rc) return;
            const auto kern = mdrnn_masked_tail_kernel<P::NFULL, P::WAVES, true>;
            unsigned grid = 0;
            if ((rc = persistent_grid(h, kern, P::WAVES * 64, P::TAIL_LDS, a.ntiles, P::WAVES, &grid))) return;
            if ((rc = ensure(h, h->rowbuf, (size_t)grid * P::WAVES * a.Nx * P::HS_BYTES_PER_BLOCK))) return;      // one slot per lattice column
            a.ring = (double*)h->rowbuf.p;
            rc = timed_launch(h, kTimerFlip, kern, grid, P::WAVES * 64, P::TAIL_LDS, a);
            if (!rc) h->work[1] += (double)a.nsb * g.steps * P::mfma_flops_per_step();
        });
        if (rc) return rc;
        h->work[0] += (double)ns * g.steps;        // sum over non-empty regions of N - 1 - f cell evaluations per chain
    }
    {
        TimedLaunch tl(h, kTimerAssembly);
        renyi_region_assemble_kernel<<<dim3((unsigned)sc.nblk, (unsigned)R), kRenyiThreads, 0, h->stream>>>(
            a.tail, a.terms, a.first, N, ns, (double*)(buf + sc.lr), (double*)(buf + sc.part));
        RNNWF_HIP(h, hipGetLastError());
        renyi_sums_kernel<<<(unsigned)R, kRenyiThreads, 0, h->stream>>>((const double*)(buf + sc.part), sc.nblk, (double*)(buf + sc.sums));
        RNNWF_HIP(h, hipGetLastError());
    }
    RNNWF_HIP(h, hipMemcpyAsync(sums_host, buf + sc.sums, (size_t)R * 16, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

const char* model_name(int model) {
    static const char* const names[] = {"GRU1D", "GRU1D_PARITY", "CRNN_U1", "GRU1D_F64", "MDRNN2D", "LSTM1D_F64"};
    return model >= 0 && model < (int)(sizeof names / sizeof *names) ? names[model] : "unknown";
}

}  // namespace

extern "C" int rnnwf_renyi2_regions_2d(rnnwf_handle* h, const int32_t* regions, int32_t nregions, const int32_t* samples, int64_t npairs,
                                       uint64_t seed, uint64_t step, int64_t pair_offset, double* sums, double* out_log_ratio,
                                       int32_t* out_samples) {
    // everything is validated before the resident batch (h->bits, h->hck) is touched: a refused call leaves it usable
    if (!h) return RNNWF_ERR_INVALID;
    if (h->model != RNNWF_MODEL_MDRNN2D)
        return h->fail(RNNWF_ERR_INVALID, "%s: serves the 2D RNN (MDRNN2D) only, this handle's model is %s; rnnwf_renyi2_regions serves the GRU models",
                       kEntry, model_name(h->model));
    size_t hs_bytes = 0;
    if (!with_md_width(h, [&](auto k) { hs_bytes = decltype(k)::HS_BYTES_PER_BLOCK; }))
        return h->fail(RNNWF_ERR_INVALID, "%s: no kernel for num_units = %d (the 2D RNN's kernels serve 1..84)", kEntry, h->H);
    if (!h->committed) return h->fail(RNNWF_ERR_INVALID, "%s: parameters not committed (call rnnwf_commit_params)", kEntry);
    if (nregions < 1 || nregions > kMaxRegions) return h->fail(RNNWF_ERR_INVALID, "%s: nregions must be in 1..%d", kEntry, kMaxRegions);
    if (npairs < 1) return h->fail(RNNWF_ERR_INVALID, "%s: npairs must be >= 1", kEntry);
    if (!regions || !sums) return h->fail(RNNWF_ERR_INVALID, "%s: regions and sums must be non-null", kEntry);
    if (!samples && pair_offset < 0) return h->fail(RNNWF_ERR_INVALID, "%s: pair_offset must be >= 0", kEntry);
    Regions g;
    if (int rc = prepare(h, regions, nregions, g)) return rc;
    const int N = h->N, R = nregions;
    // pairs per pass: the family's pass holds N states per block in its budget; beside them, per block, the terms (N x 16 x 8 bytes),
    // the tails (R x 16 x 8) and the log-ratios (R x 8 x 8)
    const size_t budget = (size_t)(h->family->max_chains_per_pass(h) / kChains) * N * hs_bytes;
    const size_t per_block = (size_t)N * hs_bytes + (size_t)N * kChains * 8 + (size_t)R * kChains * 8 + (size_t)R * (kChains / 2) * 8;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(budget / per_block)) * kChains / 2;
    RNNWF_HIP(h, hipSetDevice(h->cfg.device));
    const int32_t *col_of_pos, *pos_of_site_dev;
    if (int rc = h->family->site_maps(h, &col_of_pos, &pos_of_site_dev)) return rc;
    // the first pass is the largest: one allocation for the call, the masks uploaded once
    const Scratch big(N, R, g.W, 2 * std::min(chunk, npairs));
    if (int rc = ensure(h, h->renyi, big.bytes)) return rc;
    {
        char* buf = (char*)h->renyi.p;
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.mask, g.mask.data(), g.mask.size() * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipMemcpyAsync(buf + big.first, g.first.data(), (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
        if (g.nact) RNNWF_HIP(h, hipMemcpyAsync(buf + big.order, g.order.data(), (size_t)g.nact * 4, hipMemcpyHostToDevice, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->last_ns = 0;                                   // h->bits and h->hck are overwritten from here on
    h->call_ns = 2 * npairs;
    std::vector<double> total((size_t)R * 2, 0.0), pass_sums((size_t)R * 2);
    for (int64_t p0 = 0; p0 < npairs; p0 += chunk) {
        const int64_t np = std::min(chunk, npairs - p0), ns = 2 * np, s0 = 2 * p0;
        // spins into h->bits, every position's state into h->hck
        if (int rc = ensure(h, h->bits, (size_t)g.W * ns * 4)) return rc;
        if (samples) {
            if (int rc = upload_and_pack(h, samples + s0 * N, ns, h->bits, 0, col_of_pos)) return rc;
            if (int rc = h->family->base(h, ns, nullptr)) return rc;
        } else {
            const Draw d{seed, step, 2 * pair_offset + s0};      // rnnwf_sample's draw: the same kernel, which keeps the states as it goes
            if (int rc = h->family->base(h, ns, &d)) return rc;
            if (out_samples)
                if (int rc = unpack_and_download(h, h->bits, ns, out_samples + s0 * N, pos_of_site_dev)) return rc;
        }
        const Scratch sc(N, R, g.W, ns);
        if (int rc = region_pass(h, ns, g, sc, pass_sums.data())) return rc;
        if (out_log_ratio)
            RNNWF_HIP(h, hipMemcpy2DAsync(out_log_ratio + p0, (size_t)npairs * 8, (char*)h->renyi.p + sc.lr, (size_t)np * 8, (size_t)np * 8,
                                          (size_t)R, hipMemcpyDeviceToHost, h->stream));
        RNNWF_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < total.size(); ++k) total[k] += pass_sums[k];
    }
    memcpy(sums, total.data(), total.size() * 8);
    return RNNWF_OK;
}
