"""Float64 reference of the 2D RNN's Pauli-string estimator (docs/pauli_2d.md) on the oracle's MDRNN (oracle.models.mdrnn_cell,
zigzag_order).  TEST INFRASTRUCTURE ONLY; validated by tests/test_pauli_2d_reference.py.

Two forms: explicit_log_ratio scores every flipped configuration in full with mdrnn_log_probability; kernel_form restates what
mdrnn_pauli_kernels.h computes - restart at the first flipped position f of the path, states <= f reused, every position > f
recomputed - with switches for the defects whose rejection by the bound the CPU test shows.  Also the weights and strings the exact
and statistical GPU tests share (tests/test_gpu_pauli_2d.py).
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


def kernel_form(prm, samples, masks, defect=None):
    """1/2 (tail - suffix) as the masked-tail kernel computes it, (M, ns).  defect names one deliberate error:
      "lattice_order"      the mask left in lattice order: bit k read as position k of the path
      "restart_f_minus_1"  the chain restarts from the state after position f - 1 (zero for f = 0) instead of f
      "vertical_from_hs"   the vertical state of every position taken from the base pass, also where f < pv
      "mask_word_0"        the mask words of positions >= 32 read from word 0
    """
    assert defect is None or defect in DEFECTS
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
        sp = spins ^ mv[None, :].astype(spins.dtype)
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
