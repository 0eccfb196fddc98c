"""Float64 reference of the 2D RNN's swap estimator of the second Renyi entropy of lattice regions (docs/renyi_2d.md) on the oracle's
MDRNN (oracle.models.mdrnn_log_probability, mdrnn_cell, zigzag_order).  TEST INFRASTRUCTURE ONLY; validated by
tests/test_renyi_2d_reference.py.

    log r_A(sigma, tau) = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)],   A = a mask over the lattice index

Two forms: log_ratio_regions is brute force on purpose - both swapped configurations of every (pair, region) are written out in full
and scored from position 0, without normalisation, first position, state reuse, pairing by lane or packed words.  kernel_form restates
what mdrnn_masked_tail_kernel<..., PAIRED = true> and the assembly compute - the mask mapped to visit order and normalised, restart at
the first position f of the path, states <= f reused, every position > f recomputed - with switches for the defects whose rejection by
the bound the CPU test shows.  Also the weights, regions and region pairs the exact and statistical GPU tests share
(tests/test_gpu_renyi_2d.py), and the regions and coverage rules of the full-size cases on lattices of three to eight spin words
(tests/test_gpu_renyi_2d_full.py).
"""
import numpy as np

import pauli_2d_reference as Q
from oracle import models as M
from renyi_regions_reference import purity_of_region  # noqa: F401  (psi over conftest.all_configs(N): column k = lattice index k)

SCOPE = Q.SCOPE
BOUND = Q.BOUND             # x N: the project's float64 bound on log P and log r
FLOOR = Q.FLOOR             # every exact I2 of the statistical test is at least this large
exact_weights = Q.exact_weights
site = Q.site


def mask_of(Nx, Ny, sites):
    """Lattice-indexed mask of the sites [(nx, ny), ...]."""
    m = np.zeros(Nx * Ny, dtype=np.int32)
    for nx, ny in sites:
        m[site(Nx, Ny, nx, ny)] = 1
    return m


def rectangle(Nx, Ny, x0, x1, y0, y1):
    m = np.zeros((Nx, Ny), dtype=np.int32)
    m[x0:x1, y0:y1] = 1
    return m.reshape(-1)


def row_cuts(Nx, Ny):
    return [rectangle(Nx, Ny, 0, Nx, 0, c) for c in range(1, Ny)]


def column_cuts(Nx, Ny):
    return [rectangle(Nx, Ny, 0, c, 0, Ny) for c in range(1, Nx)]


def log_ratio_regions(log_prob, pairs, masks):
    """(len(masks), npairs) log r_A.  pairs: (2 npairs, Nx, Ny) spins, pair p = rows 2p, 2p + 1; masks: (R, Nx Ny) of 0 / 1 over the
    lattice index; log_prob scores (B, Nx, Ny) configurations.  Every region, the empty and the full one included, takes the same path."""
    pairs, masks = np.asarray(pairs), np.asarray(masks)
    _, Nx, Ny = pairs.shape
    assert masks.ndim == 2 and masks.shape[1] == Nx * Ny and np.all((masks == 0) | (masks == 1))
    sigma, tau = pairs[0::2], pairs[1::2]
    own = log_prob(sigma) + log_prob(tau)
    out = np.empty((len(masks), len(sigma)))
    for k, m in enumerate(masks):
        in_a = m.reshape(1, Nx, Ny).astype(bool)
        a = np.where(in_a, tau, sigma)               # tau_A sigma_B
        b = np.where(in_a, sigma, tau)               # sigma_A tau_B
        out[k] = 0.5 * (log_prob(a) + log_prob(b) - own)
    return out


def normalise(mask_visit):
    """(the visit-order mask with position 0 not in A - complemented when it is; f = its first position, 0 when it is empty)."""
    m = np.asarray(mask_visit).astype(np.int64)
    m = m ^ m[0]
    nz = np.flatnonzero(m)
    return m, (int(nz[0]) if len(nz) else 0)


DEFECTS = ("lattice_order", "partner_is_self", "partner_after_f", "partner_state", "vertical_from_hs", "mask_word_0")
WORD_DEFECTS = Q.WORD_DEFECTS + ("partner_words_from_2_own",)      # invisible on lattices of at most 64 sites (two words)


def kernel_form(prm, pairs, masks, defect=None):
    """log r_A = 1/2 [(tail_sigma - suffix_sigma) + (tail_tau - suffix_tau)] as the paired masked-tail kernel and the assembly compute
    it, (R, npairs).  defect names one deliberate error:
      "lattice_order"     the mask left in lattice order: bit k read as position k of the path
      "partner_is_self"   the partner taken as chain s instead of s ^ 1
      "partner_after_f"   the partner's spins taken at every position >= f
      "partner_state"     the chain restarts from the PARTNER's state after position f
      "vertical_from_hs"  the vertical state of every position taken from the base pass, also where f < pv
      "mask_word_0"       the mask words of positions >= 32 read from word 0
      "word_index_mod_2"  word (p >> 5) & 1 of the mixed configuration read for the own, horizontal and vertical spin of position p
      "words_from_2_zero" the mask words >= 2 (positions >= 64) read as 0
      "partner_words_from_2_own"  the partner's spin words >= 2 taken from the chain itself (another place of the kernel's line than
                          "words_from_2_zero", the same mixed chain: own spins from position 64 on)
    The last three (WORD_DEFECTS) are invisible on lattices of at most 64 sites.
    """
    assert defect is None or defect in DEFECTS + WORD_DEFECTS
    pairs = np.asarray(pairs)
    B, Nx, Ny = pairs.shape
    N = Nx * Ny
    order = M.zigzag_order(Nx, Ny)
    H = prm[SCOPE + "/Wh_rnn_0"].shape[0]
    zeros_h, rows = np.zeros((B, H)), np.arange(B)
    spins = np.stack([pairs[:, nx, ny] for nx, ny, _ in order], axis=1)        # (B, N) in visit order
    partner = spins if defect == "partner_is_self" else spins[rows ^ 1]
    if defect == "partner_words_from_2_own":
        partner = np.where(np.arange(N)[None, :] < 64, partner, spins)
    row_first = [p % Nx == 0 for p in range(N)]
    vert = [-1 if ny == 0 else (ny - 1) * Nx + (nx if (ny - 1) % 2 == 0 else Nx - 1 - nx) for nx, ny, _ in order]
    one_hot = lambda s: np.eye(2)[s]
    none = np.zeros((B, 2))

    def step(p, sp, state_of):
        hh, xh = (zeros_h, none) if row_first[p] else (state_of(p - 1), one_hot(sp[:, p - 1]))
        hv, xv = (zeros_h, none) if vert[p] < 0 else (state_of(vert[p]), one_hot(sp[:, vert[p]]))
        return M.mdrnn_cell(xh, xv, hh, hv, prm, SCOPE)

    hs = []
    for p in range(N):
        hs.append(step(p, spins, lambda i: hs[i]))
    own = np.stack([Q._head(prm, hs[p])[rows, spins[:, p]] for p in range(N)], axis=1)      # (B, N)
    out = np.zeros((len(masks), B // 2))
    for k, mask in enumerate(masks):
        mv, f = normalise(np.asarray(mask) if defect == "lattice_order" else Q.to_visit_order(mask, Nx, Ny))
        if f == 0:
            continue
        if defect == "partner_after_f":
            mv = (np.arange(N) >= f).astype(np.int64)
        elif defect == "mask_word_0":
            mv = mv[np.arange(N) & 31]
        elif defect == "words_from_2_zero":
            mv = np.where(np.arange(N) < 64, mv, 0)
        sp = np.where(mv[None, :].astype(bool), partner, spins)
        if defect == "word_index_mod_2":
            sp = sp[:, Q.word_index_mod_2(N)]
        start = hs[f][rows ^ 1] if defect == "partner_state" else hs[f]
        mine = {f: start}
        tail = Q._head(prm, start)[rows, sp[:, f]]
        for p in range(f + 1, N):
            def state_of(i, p=p):
                if i == p - 1 or (defect != "vertical_from_hs" and i > f):
                    return mine[i]                       # the state just computed, or one this chain produced
                return hs[i]                             # a base-pass state: positions <= f

            mine[p] = step(p, sp, state_of)
            tail = tail + Q._head(prm, mine[p])[rows, sp[:, p]]
        d = tail - own[:, f:].sum(axis=1)
        out[k] = 0.5 * (d[0::2] + d[1::2])
    return out


def case_regions(Nx, Ny):
    """Lattice-indexed masks (R, N) of the log-ratio tests: the row and column cuts, a 2x2 corner and its far twin, the bulk site,
    a two-piece region, a region containing lattice site 0 with a far piece, the empty and the full region; then, built from positions
    along the path, single positions at every row turn (the last of a row and the first of the next), a region whose first position
    is N-1, every other position, and, on lattices of more than 32 sites, regions that straddle positions 31 / 32."""
    N = Nx * Ny
    site_of_pos = np.argsort(Q.visit_positions(Nx, Ny))
    masks = row_cuts(Nx, Ny) + column_cuts(Nx, Ny)
    if Nx > 1 and Ny > 1:
        masks += [rectangle(Nx, Ny, 0, 2, 0, 2), rectangle(Nx, Ny, Nx - 2, Nx, Ny - 2, Ny), mask_of(Nx, Ny, [(min(1, Nx - 1), min(1, Ny - 1))]),
                  rectangle(Nx, Ny, 0, 1, 0, min(2, Ny)) | rectangle(Nx, Ny, Nx - 1, Nx, max(Ny - 2, 0), Ny)]
    masks += [mask_of(Nx, Ny, [(0, 0), (Nx - 1, Ny - 1)]), np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)]
    groups = [[N - 1], list(range(1, N, 2))]
    for ny in range(1, Ny):
        groups += [[ny * Nx - 1], [ny * Nx]]
    if N > 32:
        groups += [[30, 31, 32, 33], [31, 32], [31], [32], [1, 32], [31, N - 1]]
    for g in groups:
        m = np.zeros(N, dtype=np.int32)
        m[site_of_pos[g]] = 1
        masks.append(m)
    out, seen = [], set()
    for m in masks:
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            out.append(m)
    return np.stack(out)


# ---- what the exact and statistical GPU tests share: exact_weights() (10 units, seed 4, kernels x 1) -----------------------------------

EXACT_LATTICES = [(3, 4), (4, 3)]


def exact_regions(Nx, Ny):
    """[(name, mask)]: the regions whose exact S2 the statistical test compares with (docs/renyi_2d.md lists the values)."""
    return [("first-column cut", rectangle(Nx, Ny, 0, 1, 0, Ny)), ("first-row cut", rectangle(Nx, Ny, 0, Nx, 0, 1)),
            ("2x2 corner block", rectangle(Nx, Ny, 0, 2, 0, 2)), ("bulk site (1,1)", mask_of(Nx, Ny, [(1, 1)]))]


# exact S2 of exact_regions and exact I2 of i2_pairs, computed on the CPU with the oracle (tests/test_renyi_2d_reference.py asserts them)
EXACT_S2 = {(3, 4): [0.419, 0.396, 0.326, 0.192], (4, 3): [0.372, 0.433, 0.340, 0.192], (3, 3): [0.274, 0.254, 0.249, 0.161]}
EXACT_I2 = {(3, 4): [0.075], (4, 3): [0.062, 0.077]}


def i2_pairs(Nx, Ny):
    """[(mask A, mask B)] of the mutual-information test: exact I2 >= FLOOR for each (the two-block pair gives 0.025 on 3x4 and is
    used on 4x3 only)."""
    out = [(mask_of(Nx, Ny, [(1, 1)]), mask_of(Nx, Ny, [(1, 2)]))]
    if (Nx, Ny) == (4, 3):
        out.append((mask_of(Nx, Ny, [(0, 0), (0, 1)]), mask_of(Nx, Ny, [(3, 2), (3, 1)])))
    return out


# ---- full-size cases: lattices of three to eight spin words (tests/test_gpu_renyi_2d_full.py) ------------------------------------------

def bulk_positions(Nx, Ny):
    """The positions of the path whose site has four neighbours."""
    return [p for p, (nx, ny, _) in enumerate(M.zigzag_order(Nx, Ny)) if 0 < nx < Nx - 1 and 0 < ny < Ny - 1]


def bulk_block(Nx, Ny):
    """(x0, y0, L) of the centred L x L block that touches no edge, L = max(2, min(Nx, Ny) // 3)."""
    L = max(2, min(Nx, Ny) // 3)
    return (Nx - L) // 2, (Ny - L) // 2, L


def region_set_2d(Nx, Ny, fill=Q.MIN_MASKS, thin=False):
    """[(name, lattice-indexed region)] of a full-size case, distinct: every row cut (the prefixes of the path) and column cut, the 2x2
    corner block (lattice site 0 in it: complemented by the driver), a bulk L x L block, two separated pieces, lattice site 0 with
    the far corner, a single bulk site in every word that holds one, the empty and the full region, and pauli_2d_reference's
    word_masks_2d read as regions (single sites on bit 0 and the last bit of every word - position 0 alone is complemented -, first
    position N-1, a run and a vertical pair across every word boundary, a horizontal pair, (1, N-2), the checkerboard, the second
    half); then single sites spread evenly over the remaining positions until `fill` regions are non-empty after normalisation
    (the tiles of the paired pass).  thin: without the filler (the CPU study's set)."""
    N = Nx * Ny
    out = [("row cut %d" % c, m) for c, m in enumerate(row_cuts(Nx, Ny), start=1)]
    out += [("column cut %d" % c, m) for c, m in enumerate(column_cuts(Nx, Ny), start=1)]
    x0, y0, L = bulk_block(Nx, Ny)
    out += [("2x2 corner block", rectangle(Nx, Ny, 0, 2, 0, 2)), ("bulk %dx%d block at (%d,%d)" % (L, L, x0, y0), rectangle(Nx, Ny, x0, x0 + L, y0, y0 + L)),
            ("two pieces", rectangle(Nx, Ny, 1, 2, 1, 3) | rectangle(Nx, Ny, Nx - 2, Nx - 1, Ny - 3, Ny - 1)),
            ("site 0 and the far corner", mask_of(Nx, Ny, [(0, 0), (Nx - 1, Ny - 1)]))]
    bulk = bulk_positions(Nx, Ny)
    for w in range(Q.num_words(N)):
        inside = [p for p in bulk if p >> 5 == w]
        if inside:
            out.append(("bulk site at position %d (word %d)" % (inside[0], w), Q.from_positions(Nx, Ny, inside[:1])))
    out += [("empty", np.zeros(N, dtype=np.int32)), ("full", np.ones(N, dtype=np.int32))]
    out = Q._distinct(out + Q.word_masks_2d(Nx, Ny))
    if not thin:
        have = {int(np.flatnonzero(Q.to_visit_order(m, Nx, Ny))[0]) for _, m in out if m.sum() == 1}
        rest = [p for p in range(N) if p not in have]
        out += [("position %d (filler)" % p, Q.from_positions(Nx, Ny, [p])) for p in Q._spread(rest, fill - (len(out) - 2))]      # but empty, full
    return Q._distinct(out)


def _pieces(mask, Nx, Ny):
    """The sizes of the 4-connected components of a lattice-indexed mask."""
    left = {(k // Ny, k % Ny) for k in np.flatnonzero(mask)}
    sizes = []
    while left:
        todo, n = [left.pop()], 0
        while todo:
            nx, ny = todo.pop()
            n += 1
            for nb in ((nx + 1, ny), (nx - 1, ny), (nx, ny + 1), (nx, ny - 1)):
                if nb in left:
                    left.remove(nb)
                    todo.append(nb)
        sizes.append(n)
    return sorted(sizes)


def check_case_2d(Nx, Ny, masks):
    """The coverage a full-size region set must have, asserted on the masks themselves: pauli_2d_reference.check_case_2d's word
    coverage on the normalised masks, and a member of every kind region_set_2d names."""
    N = Nx * Ny
    masks = np.asarray(masks)
    Q.check_case_2d(Nx, Ny, masks, regions=True)
    have = {m.tobytes() for m in masks}
    for m in row_cuts(Nx, Ny) + column_cuts(Nx, Ny) + [rectangle(Nx, Ny, 0, 2, 0, 2), np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)]:
        assert m.astype(masks.dtype).tobytes() in have, "a row cut, a column cut, the 2x2 corner, the empty or the full region is missing"
    prefixes = {m.tobytes() for m in Q.to_visit_order(masks, Nx, Ny)}
    assert all((np.arange(N) < c * Nx).astype(masks.dtype).tobytes() in prefixes for c in range(1, Ny)), "the row cuts are not the prefixes"
    blocks, two, bulk_words = False, False, set()
    bulk = set(bulk_positions(Nx, Ny))
    for m, mv in zip(masks, Q.to_visit_order(masks, Nx, Ny)):
        grid = m.reshape(Nx, Ny)
        xs, ys = np.flatnonzero(grid.any(axis=1)), np.flatnonzero(grid.any(axis=0))
        if m.any() and len(xs) == len(ys) == xs[-1] - xs[0] + 1 == ys[-1] - ys[0] + 1 >= 2 and m.sum() == len(xs) * len(ys):
            blocks = blocks or (xs[0] > 0 and ys[0] > 0 and xs[-1] < Nx - 1 and ys[-1] < Ny - 1)      # a filled square off every edge
        sizes = _pieces(m, Nx, Ny)
        two = two or (len(sizes) == 2 and sizes[0] >= 2 and not m[0])
        if m.sum() == 1 and int(np.flatnonzero(mv)[0]) in bulk:
            bulk_words.add(int(np.flatnonzero(mv)[0]) >> 5)
    assert blocks, "no bulk L x L block"
    assert two, "no region of two separated pieces"
    assert bulk_words == {p >> 5 for p in bulk}, "a word with a bulk site has no single bulk site"
    assert any(m[0] and not m.all() for m in masks), "no region contains lattice site 0"
    assert any(normalise(mv)[1] == N - 1 for mv in Q.to_visit_order(masks, Nx, Ny)), "no region starts at position N-1"
