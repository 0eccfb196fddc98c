// pauli_terms.h - the terms of one Pauli-step call as the kernels read them, shared by the drivers of rnnwf_pauli_step (pauli.hip)
// and rnnwf_pauli_step_complex (crnn_pauli.hip): the masks are checked and packed into words, the terms grouped by flip mask (a mask
// shared by several terms is evaluated once) and the distinct masks sorted longest chain first.  Host code only.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

#include "handle.h"

namespace rnnwf {

constexpr int kPauliMaxMasks = 65535;        // blockIdx.y of the log-ratio kernel

// The terms of one call as the kernels read them
struct PauliTerms {
    int K = 0, M = 0, W = 0;
    std::vector<uint32_t> mask, sgn;     // [M][W] distinct non-empty flip masks in order of first appearance; [K][W] sign masks
    std::vector<int32_t> tmask;          // [K]: the term's row of `mask`, -1 for a diagonal term
    std::vector<int32_t> first, order;   // [M]: first flipped site f; the masks f ascending, ties by index
    bool replay = false;                 // some mask has f >= 1: the own suffixes need the replayed site terms
    double steps = 0.0;                  // sum over masks of N - f: cell evaluations per chain
};

// check and pack the (K, N) flip and sign masks, group the terms by flip mask, sort the distinct masks; `entry` names the C entry
// point in the refusals
inline int prepare_pauli_terms(rnnwf_handle* h, const char* entry, const int32_t* flip, const int32_t* sign, int K, PauliTerms& g) {
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
        int f = -1;
        for (int n = 0; n < N; ++n) {
            if (fk[n] != 0 && fk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: flip[%d][%d] = %d, a mask entry must be 0 or 1", entry, k, n, (int)fk[n]);
            if (sk[n] != 0 && sk[n] != 1)
                return h->fail(RNNWF_ERR_INVALID, "%s: sign[%d][%d] = %d, a mask entry must be 0 or 1", entry, k, n, (int)sk[n]);
            if (fk[n]) {
                words[n >> 5] |= 1u << (n & 31);
                if (f < 0) f = n;
            }
            if (sk[n]) g.sgn[(size_t)k * g.W + (n >> 5)] |= 1u << (n & 31);
        }
        if (f < 0) continue;                       // diagonal term: no cell evaluation
        auto it = seen.find(words);
        if (it == seen.end()) {
            if (g.M == kPauliMaxMasks)
                return h->fail(RNNWF_ERR_INVALID, "%s: more than %d distinct flip masks", entry, kPauliMaxMasks);
            it = seen.emplace(words, g.M++).first;
            g.mask.insert(g.mask.end(), words.begin(), words.end());
            g.first.push_back(f);
            g.order.push_back(it->second);
            g.steps += (double)(N - f);
            if (f > 0) g.replay = true;
        }
        g.tmask[k] = it->second;
    }
    std::stable_sort(g.order.begin(), g.order.end(), [&](int32_t x, int32_t y) { return g.first[x] < g.first[y]; });
    return 0;
}

}  // namespace rnnwf
