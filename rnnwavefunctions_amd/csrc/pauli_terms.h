// pauli_terms.h - the masks of one call as the kernels read them, for every family: the terms of a Pauli step (pauli_driver.h) and
// the regions of a region-Renyi call (region_driver.h).  The masks are checked, mapped from the caller's site index to the position
// in the order the family visits the sites (`pos`, nullptr: the same; the 2D RNN: its path, mdrnn_observable.h), packed into words
// and sorted longest chain first.  `cells` is the number of cell evaluations of a chain flipped from position 0 on: N for the
// chains, N - 1 for the 2D path.  `entry` names the C entry point in the refusals.  Host code only.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

#include "handle.h"

namespace rnnwf {

constexpr int kPauliMaxMasks = 65535;        // blockIdx.y of the log-ratio kernel
constexpr int kMaxRegions = 65535;           // blockIdx.y of the assembly

// The terms of one call: the terms grouped by flip mask (a mask shared by several terms is evaluated once)
struct PauliTerms {
    int K = 0, M = 0, W = 0;
    std::vector<uint32_t> mask, sgn;     // [M][W] distinct non-empty flip masks in order of first appearance; [K][W] sign masks
    std::vector<int32_t> tmask;          // [K]: the term's row of `mask`, -1 for a diagonal term
    std::vector<int32_t> first, order;   // [M]: first flipped position f; the masks f ascending, ties by index
    bool replay = false;                 // some mask has f >= 1: the own suffixes need the replayed site terms
    double steps = 0.0;                  // sum over masks of cells - f: cell evaluations per chain
};

// check and pack the (K, N) flip and sign masks, group the terms by flip mask, sort the distinct masks
inline int prepare_pauli_terms(rnnwf_handle* h, const char* entry, const int32_t* flip, const int32_t* sign, int K, const int32_t* pos,
                               int cells, PauliTerms& g) {
    const int N = h->N;
    g.K = K;
    g.W = (N + 31) / 32;
    g.sgn.assign((size_t)K * g.W, 0u);
    g.tmask.assign(K, -1);
    std::map<std::vector<uint32_t>, int32_t> seen;
    std::vector<uint32_t> words(g.W);
    for (int k = 0; k < K; ++k) {
        const int32_t *fk = flip + (size_t)k * N, *sk = sign + (size_t)k * N;
        std::fill(words.begin(), words.end(), 0u);
        int f = N;
        for (int n = 0; n < N; ++n) {
            if (fk[n] != 0 && fk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: flip[%d][%d] = %d, a mask entry must be 0 or 1", entry, k, n, (int)fk[n]);
            if (sk[n] != 0 && sk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: sign[%d][%d] = %d, a mask entry must be 0 or 1", entry, k, n, (int)sk[n]);
            const int p = pos ? pos[n] : n;
            if (fk[n]) {
                words[p >> 5] |= 1u << (p & 31);
                f = std::min(f, p);
            }
            if (sk[n]) g.sgn[(size_t)k * g.W + (p >> 5)] |= 1u << (p & 31);
        }
        if (f == N) continue;                      // diagonal term: no cell evaluation
        auto it = seen.find(words);
        if (it == seen.end()) {
            if (g.M == kPauliMaxMasks)
                return h->fail(RNNWF_ERR_INVALID, "%s: more than %d distinct flip masks", entry, kPauliMaxMasks);
            it = seen.emplace(words, g.M++).first;
            g.mask.insert(g.mask.end(), words.begin(), words.end());
            g.first.push_back(f);
            g.order.push_back(it->second);
            g.steps += (double)(cells - f);
            if (f > 0) g.replay = true;
        }
        g.tmask[k] = it->second;
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    return 0;
}

// The regions of one call, normalised: position 0 not in A (r_A = r_complement)
struct Regions {
    int R = 0, W = 0, nact = 0;
    std::vector<uint32_t> mask;          // [R][W]
    std::vector<int32_t> first, order;   // [R]: first position f of A, 0 = empty; [nact]: non-empty regions, f ascending, ties by index
    double steps = 0.0;                  // sum over non-empty regions of cells - f: cell evaluations per chain
};

// check, normalise, pack and sort the (R, N) masks
inline int prepare_regions(rnnwf_handle* h, const char* entry, const int32_t* regions, int R, const int32_t* pos, int cells, Regions& g) {
    const int N = h->N;
    g.R = R;
    g.W = (N + 31) / 32;
    g.mask.assign((size_t)R * g.W, 0u);
    g.first.assign(R, 0);
    int site0 = 0;                                 // the site at position 0
    for (int n = 0; pos && n < N; ++n)
        if (pos[n] == 0) site0 = n;
    for (int r = 0; r < R; ++r) {
        const int32_t* m = regions + (size_t)r * N;
        for (int n = 0; n < N; ++n)
            if (m[n] != 0 && m[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: regions[%d][%d] = %d, a mask entry must be 0 or 1", entry, r, n, (int)m[n]);
        const int32_t flip = m[site0];             // position 0 in A: take the complement
        int f = N;
        for (int n = 0; n < N; ++n)
            if (m[n] ^ flip) {
                const int p = pos ? pos[n] : n;
                g.mask[(size_t)r * g.W + (p >> 5)] |= 1u << (p & 31);
                f = std::min(f, p);
            }
        if (f < N) {
            g.first[r] = f;
            g.order.push_back(r);
            g.steps += (double)(cells - f);
        }
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    g.nact = (int)g.order.size();
    return 0;
}

}  // namespace rnnwf
