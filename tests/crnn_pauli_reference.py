"""Float64 reference of the complex RNN's Pauli-string estimator (docs/pauli_complex.md), independent of the library: plain NumPy
on the oracle's complex RNN.  TEST INFRASTRUCTURE ONLY; validated by tests/test_crnn_pauli_reference.py.

    O = (prod_{i in S} sz_i)(prod_{i in F} sx_i),   v(sigma) = prod_{i in S} (2 sigma_i - 1) * psi(sigma ^ F) / psi(sigma)
    d(sigma, F) = log psi(sigma ^ F) - log psi(sigma)   (complex; (-inf, 0) and v = 0 where sigma ^ F leaves the sector)

explicit_log_ratio is brute force: every flipped configuration is written out in full and scored from site 0 with
oracle.models.crnn_log_amplitude(dtype=float64).  That function masks both amplitudes of an out-of-sector row to zero and
l2-normalises with an epsilon, so an out-of-sector row comes out as -inf plus whatever phases followed - not a clean (-inf, 0); the
helper therefore decides the sector itself by counting ups and sets d = (-inf, 0) there.  (A row is outside the sector iff some site
overshoots N/2 ups or N/2 downs, which is where the library's per-site mask puts its -inf.)

kernel_form restates what crnn_pauli_kernels.h computes - restart from the state after site f - 1 with the chain's own spin f - 1
as input, the up-count restarted from the own prefix, the suffix from the replayed own terms - with switches for the defects whose
rejection the CPU test shows.
"""
import numpy as np

from oracle import models as M
from rnnwavefunctions_amd import params as P

SCOPE = "RNNwavefunction"
HEADS = ("wf_dense_ampl", "wf_dense_phase")
F32_BOUND = 1e-5            # x N per component: the project's float32 bound on log-ratios (docs/pauli.md, docs/renyi_regions.md)

I2 = np.eye(2)
SX = np.array([[0.0, 1.0], [1.0, 0.0]])
SZ = np.array([[-1.0, 0.0], [0.0, 1.0]])          # sigma = 0 <-> s = -1
SY = -1j * SZ @ SX
PAULI = {"I": I2, "X": SX, "Y": SY, "Z": SZ}


def weights(H, seed=7, scale=2.0):
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=seed, heads=HEADS), scale), seed + 1)


def to64(prm):
    return {k: np.asarray(v, dtype=np.float64) for k, v in prm.items()}


def all_configs(N):
    return ((np.arange(2 ** N)[:, None] >> np.arange(N)[::-1]) & 1).astype(np.int32)


def sector(N):
    """Every configuration of the zero-magnetisation sector, (C(N, N/2), N) int32, in the order of all_configs."""
    c = all_configs(N)
    return c[c.sum(axis=1) == N // 2]


def in_sector(x):
    x = np.asarray(x)
    return x.sum(axis=-1) == x.shape[-1] // 2


def random_sector_samples(N, ns, seed):
    rng = np.random.RandomState(seed)
    base = np.array([0, 1] * (N // 2), dtype=np.int32)
    return np.stack([rng.permutation(base) for _ in range(ns)])


def log_amp(prm, x):
    """complex128 log psi of in-sector rows, float64 arithmetic on the oracle."""
    return M.crnn_log_amplitude(to64(prm), np.asarray(x), SCOPE, dtype=np.float64)


def explicit_log_ratio(prm, samples, masks):
    """(M, ns) complex128 d(sigma, F), brute force; (-inf + 0j) where sigma ^ F leaves the sector."""
    samples = np.asarray(samples)
    assert np.all(in_sector(samples))
    own = log_amp(prm, samples)
    out = np.empty((len(masks), len(samples)), dtype=np.complex128)
    for k, m in enumerate(masks):
        x = samples ^ np.asarray(m)[None, :].astype(samples.dtype)
        ok = in_sector(x)
        out[k] = complex(-np.inf, 0.0)
        if ok.any():
            out[k, ok] = log_amp(prm, x[ok]) - own[ok]
    return out


def explicit_log_ratio_f32(prm, samples, masks):
    """explicit_log_ratio on the FLOAT32 oracle (complex64 terms, summed as the oracle sums them): the yardstick of the full-size test."""
    samples = np.asarray(samples)
    score = lambda x: M.crnn_log_amplitude(prm, x, SCOPE, dtype=np.float32).astype(np.complex128)
    own = score(samples)
    out = np.full((len(masks), len(samples)), complex(-np.inf, 0.0), dtype=np.complex128)
    for k, m in enumerate(masks):
        x = samples ^ np.asarray(m)[None, :].astype(samples.dtype)
        ok = in_sector(x)
        if ok.any():
            out[k, ok] = score(x[ok]) - own[ok]
    return out


def signs(samples, sign):
    """(K, ns) prod_{i in S_k} (2 sigma_i - 1) of the given configurations."""
    s = 2.0 * np.asarray(samples, dtype=np.float64) - 1.0
    return np.stack([np.prod(np.where(np.asarray(m, dtype=bool)[None, :], s, 1.0), axis=1) for m in sign])


def ratio(d):
    """exp(d) with exactly 0 where d.re = -inf."""
    d = np.asarray(d)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(d.real), 0.0, np.exp(np.where(np.isneginf(d.real), 0.0, d)))


def local_values(d, samples, flip, sign, sign_from_flipped=False):
    """(K, ns) complex v_k from the log-ratios d (K, ns) of the terms' own masks.  sign_from_flipped: the defect that reads the signs
    from sigma ^ F instead of sigma."""
    samples = np.asarray(samples)
    if sign_from_flipped:
        sg = np.stack([signs(samples ^ np.asarray(f)[None, :].astype(samples.dtype), [s])[0] for f, s in zip(flip, sign)])
    else:
        sg = signs(samples, sign)
    return sg * ratio(d)


def dense_string(letters, N):
    """The 2^N x 2^N matrix of a Pauli string given as {site: letter}, a dense "XZIY..." or a sparse [("X", i), ...]."""
    if isinstance(letters, str):
        letters = {i: c for i, c in enumerate(letters) if c != "I"}
    elif not isinstance(letters, dict):
        letters = {i: c for c, i in letters}
    out = np.ones((1, 1), dtype=np.complex128)
    for i in range(N):
        out = np.kron(out, PAULI[letters.get(i, "I")])
    return out


def dense_term(flip, sign):
    """(prod_{sign} sz)(prod_{flip} sx) as a dense matrix, sz to the left."""
    N = len(flip)
    return dense_string({i: "Z" for i in range(N) if sign[i]}, N) @ dense_string({i: "X" for i in range(N) if flip[i]}, N)


def dense_hamiltonian(ham):
    """sum_k coeff_k (prod sz)(prod sx) of an observables_complex.ComplexHamiltonian."""
    return sum(c * dense_term(f, s) for c, f, s in zip(ham.coeff, ham.flip, ham.sign))


def dense_state(prm, N):
    """psi over all_configs(N) (zero outside the sector), complex128, and the sector's row indices."""
    idx = np.flatnonzero(in_sector(all_configs(N)))
    psi = np.zeros(2 ** N, dtype=np.complex128)
    psi[idx] = np.exp(log_amp(prm, all_configs(N)[idx]))
    return psi, idx


# ---- the site-resolved form of the kernels, with defects ------------------------------------------------------------------------------

DEFECTS = ("mask_shifted", "mask_word_0", "checkpoint_f", "num_up_no_prefix")


def _site_terms(prm, out, n, N, num_up):
    """(la (B, 2), ph (B, 2)): crnn_site in float64 - log-amplitudes 1/2 log softmax with the U(1) mask, phases pi softsign."""
    za = out @ prm[SCOPE + "/wf_dense_ampl/kernel"] + prm[SCOPE + "/wf_dense_ampl/bias"]
    za = za - za.max(axis=1, keepdims=True)
    la = 0.5 * (za - np.log(np.exp(za).sum(axis=1, keepdims=True)))
    if 2 * n >= N:
        base = N // 2 - 1
        ok_down, ok_up = base - (n - num_up) >= 0, base - num_up >= 0
        la = la.copy()
        la[~ok_down, 0] = -np.inf
        la[~ok_down & ok_up, 1] = 0.0
        la[~ok_up, 1] = -np.inf
        la[~ok_up & ok_down, 0] = 0.0
    zp = out @ prm[SCOPE + "/wf_dense_phase/kernel"] + prm[SCOPE + "/wf_dense_phase/bias"]
    return la, np.pi * (zp / (1.0 + np.abs(zp)))


def kernel_form(prm, samples, masks, defect=None, wrap_phase=False):
    """(M, ns) complex128 tail - suffix as the masked-tail pass computes it.  defect names one deliberate error:
      "mask_shifted"      every mask shifted by one site (site n flipped where n - 1 was asked; the last site drops out)
      "mask_word_0"       the mask word of sites >= 32 read from word 0 (mask[n & 31] for mask[n])
      "checkpoint_f"      restart from the state after site f (the chain's own spin f fed on top of it) instead of f - 1
      "num_up_no_prefix"  the up-count of the restarted chain starts at 0 instead of the ups of the own sites below f
    wrap_phase: every per-site phase reduced to (-pi, pi] before it is added (see test_crnn_pauli_reference.py: not a defect)."""
    assert defect is None or defect in DEFECTS
    prm = to64(prm)
    samples = np.asarray(samples)
    B, N = samples.shape
    rows = np.arange(B)
    one_hot = lambda s: np.eye(2)[s]
    wrap = (lambda p: p - 2 * np.pi * np.ceil((p - np.pi) / (2 * np.pi))) if wrap_phase else (lambda p: p)

    def run(state, x, spins, n0, num_up):
        """sites n0..N-1 teacher-forced on `spins` from `state` and input x: per-site (re, im) terms (B, N - n0) and the states"""
        re, im, states = [], [], []
        num_up = num_up.copy()
        for n in range(n0, N):
            state = M.gru_cell(x, state, prm, SCOPE, 0)
            la, ph = _site_terms(prm, state, n, N, num_up)
            re.append(la[rows, spins[:, n]])
            im.append(wrap(ph[rows, spins[:, n]]))
            states.append(state)
            num_up += spins[:, n]
            x = one_hot(spins[:, n])
        return np.stack(re, axis=1), np.stack(im, axis=1), states

    H = prm[SCOPE + "/" + M.GRU % 0 + "candidate/hidden_projection/kernel"].shape[0]
    own_re, own_im, hs = run(np.zeros((B, H)), np.zeros((B, 2)), samples, 0, np.zeros(B, dtype=np.int64))
    out = np.empty((len(masks), B), dtype=np.complex128)
    for k, mask in enumerate(masks):
        m = np.asarray(mask).astype(samples.dtype)
        f = int(np.flatnonzero(m)[0])                  # of the mask that was asked for: the restart point
        if defect == "mask_shifted":
            m = np.concatenate([[0], m[:-1]]).astype(samples.dtype)
        elif defect == "mask_word_0":
            m = m[np.arange(N) & 31]
        x = samples ^ m[None, :]
        if f == 0:
            state, inp = np.zeros((B, H)), np.zeros((B, 2))
        else:
            state, inp = hs[f - 1], one_hot(samples[:, f - 1])
        if defect == "checkpoint_f" and f < N - 1:
            state, inp = hs[f], one_hot(samples[:, f])
        nu = np.zeros(B, dtype=np.int64) if defect == "num_up_no_prefix" else samples[:, :f].sum(axis=1).astype(np.int64)
        re, im, _ = run(state, inp, x, f, nu)
        tail_re, tail_im = re.sum(axis=1), im.sum(axis=1)
        with np.errstate(invalid="ignore"):
            d = (tail_re - own_re[:, f:].sum(axis=1)) + 1j * (tail_im - own_im[:, f:].sum(axis=1))
        out[k] = np.where(np.isneginf(tail_re), complex(-np.inf, 0.0), d)
    return out


def max_abs_diff(a, b):
    """Largest |Re|, |Im| difference over the entries finite in both; the -inf entries must coincide exactly."""
    a, b = np.asarray(a), np.asarray(b)
    inf_a, inf_b = np.isneginf(a.real), np.isneginf(b.real)
    assert np.array_equal(inf_a, inf_b), "the out-of-sector entries differ"
    assert np.all(a.imag[inf_a] == 0.0) and np.all(b.imag[inf_b] == 0.0)
    ok = ~inf_a
    if not ok.any():
        return 0.0
    d = a[ok] - b[ok]
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


# ---- masks of the GPU cases ----------------------------------------------------------------------------------------------------------

def _sites(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def case_masks(N):
    """f = 0 and f = N-1 among them, pairs near and far (in-sector for anti-aligned chains, out of it for aligned ones), a single site
    (always out of the sector), strings crossing every 32-site word boundary, four- and six-site strings, the full mask."""
    groups = [[0, 1], [0, N - 1], [N - 2, N - 1], [1, 2], [N // 2 - 1, N // 2], [1, N - 2], [N // 4, (3 * N) // 4], [N - 1], [0], [N // 2],
              [0, 1, 2, 3], [N // 2 - 2, N // 2 - 1, N // 2, N // 2 + 1], list(range(0, N, 2)), list(range(N))]
    for w in range(32, N, 32):
        groups += [[w - 1, w], [w - 2, w - 1, w, w + 1] if w + 1 < N else [w - 2, w - 1], [w - 1, N - 1], [1, w]]
    masks, seen = [], set()
    for g in groups:
        m = _sites(N, [i for i in g if 0 <= i < N])
        if m.any() and m.tobytes() not in seen:
            seen.add(m.tobytes())
            masks.append(m)
    return np.stack(masks)
