"""Float64 reference of the 2D RNN's Pauli-string estimator (docs/pauli_2d.md) on the oracle's MDRNN (oracle.models.mdrnn_cell,
zigzag_order).  TEST INFRASTRUCTURE ONLY; validated by tests/test_pauli_2d_reference.py.

Two forms: explicit_log_ratio scores every flipped configuration in full with mdrnn_log_probability; kernel_form restates what
mdrnn_pauli_kernels.h computes - restart at the first flipped position f of the path, states <= f reused, every position > f
recomputed - with switches for the defects whose rejection by the bound the CPU test shows.  Also the weights and strings the exact
and statistical GPU tests share (tests/test_gpu_pauli_2d.py), and the masks, strings and coverage rules of the full-size cases on lattices
of three to eight spin words (tests/test_gpu_pauli_2d_full.py).
"""
import numpy as np

from oracle import models as M
from rnnwavefunctions_amd import params as P

SCOPE = "RNNwavefunction"
BOUND = 1e-11               # x N: the project's float64 bound on log P and log r (tests/test_gpu_mdrnn.py, docs/pauli.md)
FLOOR = 0.05                # every exact value of the exact test is at least this large in magnitude
EXACT_H, EXACT_SEED, EXACT_SCALE = 10, 4, 1.0
EXACT_LATTICES = [(3, 4), (4, 3)]


def weights(H, seed, scale):
    return P.randomize_biases(P.scale_kernels(P.init_mdrnn_params(H, seed=seed), scale), seed + 1)


def exact_weights():
    return weights(EXACT_H, EXACT_SEED, EXACT_SCALE)


def site(Nx, Ny, nx, ny):
    return nx * Ny + ny


def exact_strings(Nx, Ny):
    """Sparse strings over the lattice index: X on the first and last lattice site, X at a row turn of the path, ZZ, XX and YY on a
    horizontal and on a vertical bond, XZX, the all-X string, a Z.X pair far apart."""
    k = lambda nx, ny: site(Nx, Ny, nx, ny)
    return [[("X", k(0, 0))], [("X", k(Nx - 1, Ny - 1))], [("X", k(Nx - 1, 1))], [("Z", k(0, 0)), ("Z", k(1, 0))],
            [("X", k(0, 0)), ("X", k(1, 0))], [("Y", k(0, 0)), ("Y", k(1, 0))], [("X", k(1, 1)), ("X", k(1, 2))],
            [("Y", k(1, 1)), ("Y", k(1, 2))], [("X", k(0, 1)), ("Z", k(1, 1)), ("X", k(2, 1))], [("X", i) for i in range(Nx * Ny)],
            [("Z", k(0, 0)), ("X", k(Nx - 1, Ny - 1))]]


def visit_positions(Nx, Ny):
    """pos[k]: position along the zig-zag path of lattice site k = nx * Ny + ny, from oracle.models.zigzag_order."""
    pos = np.empty(Nx * Ny, dtype=np.int64)
    for p, (nx, ny, _) in enumerate(M.zigzag_order(Nx, Ny)):
        pos[site(Nx, Ny, nx, ny)] = p
    return pos


def to_visit_order(mask, Nx, Ny):
    """A lattice-indexed mask (..., N) in visit order."""
    mask = np.asarray(mask)
    out = np.zeros_like(mask)
    out[..., visit_positions(Nx, Ny)] = mask
    return out


def explicit_log_ratio(log_prob, samples, masks):
    """(M, ns) 1/2 [log P(sigma ^ F) - log P(sigma)]; samples (ns, Nx, Ny), masks (M, Nx * Ny) lattice-indexed."""
    samples = np.asarray(samples)
    ns, Nx, Ny = samples.shape
    own = log_prob(samples)
    return np.stack([0.5 * (log_prob(samples ^ np.asarray(m).reshape(1, Nx, Ny).astype(samples.dtype)) - own) for m in masks])


def string_expectation(psi, configs, string):
    """psi^T P psi of one sparse Pauli string with an even number of Y, without the dense matrix: P maps sigma to sigma ^ F with the
    sign of sigma's spins on S and the factor (-i)^n_Y.  configs: conftest.all_configs(N) (row index = the bits, site 0 first)."""
    N = configs.shape[1]
    F, S, ny = np.zeros(N, dtype=configs.dtype), np.zeros(N, dtype=bool), 0
    for letter, i in string:
        F[i], S[i], ny = letter in "XY", letter in "ZY", ny + (letter == "Y")
    assert ny % 2 == 0
    partner = (configs ^ F[None, :]) @ (1 << np.arange(N - 1, -1, -1))
    sgn = np.prod(np.where(S[None, :], 2.0 * configs - 1.0, 1.0), axis=1)
    return (-1.0) ** (ny // 2) * float((psi * sgn * psi[partner]).sum())


def _head(prm, h):
    z = h @ prm[SCOPE + "/wf_dense/kernel"] + prm[SCOPE + "/wf_dense/bias"]
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))          # (B, 2) log p(0), log p(1)


DEFECTS = ("lattice_order", "restart_f_minus_1", "vertical_from_hs", "mask_word_0")
WORD_DEFECTS = ("word_index_mod_2", "words_from_2_zero")          # invisible on lattices of at most 64 sites (two words)


def word_index_mod_2(N):
    """The position whose bit a kernel reads for position p when it takes word (p >> 5) & 1 for word p >> 5."""
    p = np.arange(N)
    return (p & 31) + 32 * ((p >> 5) & 1)


def kernel_form(prm, samples, masks, defect=None):
    """1/2 (tail - suffix) as the masked-tail kernel computes it, (M, ns).  defect names one deliberate error:
      "lattice_order"      the mask left in lattice order: bit k read as position k of the path
      "restart_f_minus_1"  the chain restarts from the state after position f - 1 (zero for f = 0) instead of f
      "vertical_from_hs"   the vertical state of every position taken from the base pass, also where f < pv
      "mask_word_0"        the mask words of positions >= 32 read from word 0
      "word_index_mod_2"   word (p >> 5) & 1 of the flipped configuration read for the own, horizontal and vertical spin of position p
      "words_from_2_zero"  the mask words >= 2 (positions >= 64) read as 0
    The last two (WORD_DEFECTS) are invisible on lattices of at most 64 sites.
    """
    assert defect is None or defect in DEFECTS + WORD_DEFECTS
    samples = np.asarray(samples)
    B, Nx, Ny = samples.shape
    N = Nx * Ny
    order = M.zigzag_order(Nx, Ny)
    H = prm[SCOPE + "/Wh_rnn_0"].shape[0]
    zeros_h, rows = np.zeros((B, H)), np.arange(B)
    spins = np.stack([samples[:, nx, ny] for nx, ny, _ in order], axis=1)      # (B, N) in visit order
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
    own = np.stack([_head(prm, hs[p])[rows, spins[:, p]] for p in range(N)], axis=1)     # (B, N)
    out = np.zeros((len(masks), B))
    for k, mask in enumerate(masks):
        mv = np.asarray(mask) if defect == "lattice_order" else to_visit_order(mask, Nx, Ny)
        f = int(np.flatnonzero(mv)[0])
        if defect == "mask_word_0":
            mv = mv[np.arange(N) & 31]
        elif defect == "words_from_2_zero":
            mv = np.where(np.arange(N) < 64, mv, 0)
        sp = spins ^ mv[None, :].astype(spins.dtype)
        if defect == "word_index_mod_2":
            sp = sp[:, word_index_mod_2(N)]
        start = hs[f]
        if defect == "restart_f_minus_1":
            start = hs[f - 1] if f > 0 else zeros_h
        mine = {f: start}

        tail = _head(prm, start)[rows, sp[:, f]]
        for p in range(f + 1, N):
            def state_of(i, p=p):
                if i == p - 1 or (defect != "vertical_from_hs" and i > f):
                    return mine[i]                       # the state just computed, or one this chain produced
                return hs[i]                             # a base-pass state: positions <= f

            mine[p] = step(p, sp, state_of)
            tail = tail + _head(prm, mine[p])[rows, sp[:, p]]
        out[k] = 0.5 * (tail - own[:, f:].sum(axis=1))
    return out


def case_masks(Nx, Ny):
    """Lattice-indexed masks (M, N) of the log-ratio test, built from positions along the path: every single site (f in the first
    row, at every row turn, f = 0 and f = N-1 among them), a flip in row 0 with the site above it (its vertical dependants span two
    rows), a pair far apart, every other position, everything from the middle on, the full mask and, on lattices of more than 32
    sites, strings and single sites that straddle positions 31 / 32."""
    N = Nx * Ny
    pos = visit_positions(Nx, Ny)
    site_of_pos = np.argsort(pos)
    groups = [[p] for p in range(N)] + [[0, N - 1], list(range(0, N, 2)), list(range(N // 2, N)), list(range(N))]
    if Ny > 1:
        groups.append([min(1, Nx - 1), int(pos[site(Nx, Ny, min(1, Nx - 1), 1)])])
    if N > 32:
        groups += [[30, 31, 32, 33], [31, 32], [1, 32], [31, N - 1]]
    masks, seen = [], set()
    for g in groups:
        m = np.zeros(N, dtype=np.int32)
        m[site_of_pos[g]] = 1
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            masks.append(m)
    return np.stack(masks)


# ---- full-size cases: lattices of three to eight spin words (tests/test_gpu_pauli_2d_full.py, tests/test_gpu_renyi_2d_full.py) ----------

MIN_MASKS = 131             # 12 x 12, 2006 chains: 131 masks x 126 blocks = 16 506 tiles >= 16 384 = 2 x 256 CUs x 32 wave slots
FILL = {(16, 16): 0}        # filler single sites of the GPU cases: none on 256 sites, whose float64 reference would take over 10 s with them


def num_words(N):
    return (N + 31) // 32


def word_edges(N):
    """[(first position, last position that exists)] of every 32-position word: bit 0 and bit 31 (less in a partial last word)."""
    return [(32 * w, min(32 * w + 31, N - 1)) for w in range(num_words(N))]


def above(Nx, p):
    """The position of the site above position p of the path (the kernel's pv), -1 on the first row."""
    ny, j = divmod(p, Nx)
    return p - 2 * j - 1 if ny > 0 else -1


def straddling_run(N, b):
    """4 to 5 consecutive positions with b - 1 and b among them: b-2 .. b+2, moved down where the path ends before b + 2."""
    hi = min(N, b + 3)
    return list(range(min(b - 2, hi - 4), hi))


def cross_word_vertical_pair(Nx, N, b):
    """(pv, p): the first position p >= b off a row turn whose site above, pv, lies in the word before b; None without one."""
    for p in range(b, min(N, b + 32)):
        pv = above(Nx, p)
        if 0 <= pv < b and pv != p - 1:
            return pv, p
    return None


def from_positions(Nx, Ny, positions):
    """The lattice-indexed mask (N,) of a list of positions along the path."""
    m = np.zeros(Nx * Ny, dtype=np.int32)
    m[np.argsort(visit_positions(Nx, Ny))[list(positions)]] = 1
    return m


def checkerboard(Nx, Ny):
    """(nx + ny) odd, by lattice coordinates, over the lattice index."""
    nx, ny = np.divmod(np.arange(Nx * Ny), Ny)
    return ((nx + ny) & 1).astype(np.int32)


def _distinct(named):
    seen, out = set(), []
    for name, m in named:
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            out.append((name, m))
    return out


def _spread(rest, need):
    """need of the positions rest, evenly spread (all of them when there are no more)."""
    return list(rest) if need >= len(rest) else [rest[(i * len(rest)) // need] for i in range(max(need, 0))]


def word_masks_2d(Nx, Ny):
    """[(name, mask)] every full-size set holds, flips and regions alike: a single site on bit 0 and on the last bit of every word,
    position N-1, a run straddling every word boundary, a vertical pair across every word boundary, a horizontal pair, the pair
    (1, N-2), the checkerboard and everything from the middle on."""
    N = Nx * Ny
    out = []
    for w, (a, b) in enumerate(word_edges(N)):
        out += [("position %d (word %d bit 0)" % (a, w), from_positions(Nx, Ny, [a])),
                ("position %d (word %d bit %d)" % (b, w, b & 31), from_positions(Nx, Ny, [b]))]
    out.append(("position %d (the last)" % (N - 1), from_positions(Nx, Ny, [N - 1])))
    for b in range(32, N, 32):
        run = straddling_run(N, b)
        out.append(("run %d..%d (straddles word boundary %d)" % (run[0], run[-1], b), from_positions(Nx, Ny, run)))
        pair = cross_word_vertical_pair(Nx, N, b)
        if pair:
            out.append(("vertical pair %d,%d (across word boundary %d)" % (pair + (b,)), from_positions(Nx, Ny, pair)))
    if Nx > 1:
        p = (Ny // 2) * Nx + (Nx - 1) // 2
        out.append(("horizontal pair %d,%d" % (p, p + 1), from_positions(Nx, Ny, [p, p + 1])))
    out += [("pair 1,%d" % (N - 2), from_positions(Nx, Ny, [1, N - 2])), ("checkerboard", checkerboard(Nx, Ny)),
            ("positions %d..%d (from the middle on)" % (N // 2, N - 1), from_positions(Nx, Ny, range(N // 2, N)))]
    return _distinct(out)


def mask_set_2d(Nx, Ny, fill=MIN_MASKS, thin=False):
    """[(name, lattice-indexed flip mask)] of a full-size case, distinct, built from positions of the path: word_masks_2d, the full
    mask, and single sites at every position of the first two rows and of the last row and at every row turn; then single sites
    spread evenly over the remaining positions until the set holds `fill` masks.  thin: without the rows, the turns and the filler
    (the CPU study's set)."""
    N = Nx * Ny
    out = word_masks_2d(Nx, Ny) + [("full", np.ones(N, dtype=np.int32))]
    if not thin:
        single = lambda p, why: ("position %d (%s)" % (p, why), from_positions(Nx, Ny, [p]))
        out += [single(p, "row %d" % (p // Nx)) for p in range(min(2 * Nx, N))] + [single(p, "last row") for p in range(N - Nx, N)]
        for ny in range(1, Ny):
            out += [single(ny * Nx - 1, "row turn"), single(ny * Nx, "row turn")]
        out = _distinct(out)
        have = {int(np.flatnonzero(to_visit_order(m, Nx, Ny))[0]) for _, m in out if m.sum() == 1}
        out += [single(p, "filler") for p in _spread([p for p in range(N) if p not in have], fill - len(out))]
    return _distinct(out)


def sign_strings_2d(Nx, Ny):
    """Sparse Pauli strings over the lattice index whose Z and Y letters (the sign words of the term and E_loc kernels) sit on
    positions of every word: per word w a Z on its last position with an X on position 1 (for the last word: a Z there with an X in
    word 0) and, where the word holds two positions, a YY bond inside it; a YY bond across every word boundary; a Z alone in the
    last word (a diagonal term); last, one string of odd n_Y (expectation exactly 0)."""
    N = Nx * Ny
    s = np.argsort(visit_positions(Nx, Ny))
    k = lambda p: int(s[p])
    out = []
    for a, b in word_edges(N):
        out.append([("Z", k(b)), ("X", k(1))])
        if b > a:
            out.append([("Y", k(a + (b - a) // 2)), ("Y", k(a + (b - a) // 2 + 1))])
    for b in range(32, N, 32):
        out.append([("Y", k(b - 1)), ("Y", k(b))])
    out.append([("Z", k(N - 1))])
    out.append([("Y", k(N - 1)), ("Z", k(32 * (num_words(N) // 2))), ("X", k(0))])
    return out


def _is_run(nz, b):
    return 4 <= len(nz) <= 5 and nz[-1] - nz[0] + 1 == len(nz) and nz[0] < b <= nz[-1]


def check_case_2d(Nx, Ny, masks, regions=False):
    """The coverage a full-size set must have, asserted on the masks themselves in VISIT order (not only intended): distinct masks; a
    single site on bit 0 and on the last bit of every word; first position N-1; at every word boundary a run of 4 to 5 consecutive
    positions and (Ny > 1) a vertical pair in different words; a horizontal pair; the pair (1, N-2); the checkerboard by lattice
    coordinates; everything from the middle on.  Flip masks: also first position 0, the full mask and single sites on the first two
    rows, the last row and every row turn.  regions: the masks are normalised first (position 0 not in A), so position 0 is no
    single site and the full mask is empty; renyi_2d_reference.check_case_2d adds the kinds of regions."""
    N = Nx * Ny
    masks = np.asarray(masks)
    assert len({m.tobytes() for m in masks}) == len(masks), "masks repeat"
    mv = to_visit_order(masks, Nx, Ny)
    if regions:
        mv = mv ^ mv[:, :1]
    sets = [np.flatnonzero(m) for m in mv if m.any()]
    singles = {int(nz[0]) for nz in sets if len(nz) == 1}
    pairs = {(int(nz[0]), int(nz[1])) for nz in sets if len(nz) == 2}
    firsts = {int(nz[0]) for nz in sets}
    edges = {p for ab in word_edges(N) for p in ab} - ({0} if regions else set())
    assert edges <= singles, "no single site at positions %s" % sorted(edges - singles)
    assert N - 1 in firsts and (regions or 0 in firsts)
    for b in range(32, N, 32):
        assert any(_is_run(nz, b) for nz in sets), "no run of 4 to 5 positions straddles word boundary %d" % b
        if Ny > 1:
            assert any(above(Nx, p) == pv and pv >> 5 != p >> 5 and pv < b <= p for pv, p in pairs), "no vertical pair across %d" % b
    assert Nx == 1 or any(p == pv + 1 and p // Nx == pv // Nx for pv, p in pairs), "no horizontal pair"
    assert (1, N - 2) in pairs
    want = {to_visit_order(checkerboard(Nx, Ny), Nx, Ny).tobytes(), (np.arange(N) >= N // 2).astype(mv.dtype).tobytes()}
    if regions:
        want = {(np.frombuffer(w, dtype=mv.dtype) ^ np.frombuffer(w, dtype=mv.dtype)[0]).tobytes() for w in want}
    assert want <= {m.tobytes() for m in mv}, "the checkerboard or the second half is missing"
    if not regions:
        assert any(len(nz) == N for nz in sets), "the full mask is missing"
        rows = set(range(min(2 * Nx, N))) | set(range(N - Nx, N)) | {p for ny in range(1, Ny) for p in (ny * Nx - 1, ny * Nx)}
        assert rows <= singles, "no single site at positions %s" % sorted(rows - singles)
