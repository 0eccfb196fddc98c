"""Pauli-string expectation values, energies of arbitrary spin-1/2 Hamiltonians, spin-spin correlations and the structure factor
for the complex RNN with the U(1) mask (model CRNN_U1, one layer; rnnwf_pauli_step_complex, docs/pauli_complex.md), and its second
Renyi entropies of arbitrary regions, their mutual information and their resolution by the U(1) charge of the region
(rnnwf_renyi2_regions_complex, docs/renyi_complex.md; the region builders are observables.interval_region and its kin).

The term convention is observables.py's, O = (prod_{i in S} sz_i)(prod_{i in F} sx_i) with sz to the left; with sigma ~ |psi|^2 and
s = 2 sigma - 1 the estimator is complex:

    v(sigma) = prod_{i in S} s_i * psi(sigma ^ F) / psi(sigma),   E[v] = <psi|O|psi>,   E_loc = sum_k coeff_k v_k.

Strings with an odd number of Y and complex coefficients are legal here: psi carries a phase.  A flipped configuration outside the
zero-magnetisation sector has psi = 0 and contributes exactly 0.

observables.pauli_expectations / energy keep refusing the complex RNN; these are its own entry points.  They accept the
J1J2.ComplexRNNwavefunction facade or a NativeWavefunction of model CRNN_U1 and raise ValueError for every other model.
"""
import warnings

import numpy as np

from . import _lib
from . import _observable_api as _api
from .observables import _disjoint_masks, _native, group_by_mask, mutual_information2_from_values, pauli_terms

__all__ = ["ComplexHamiltonian", "pauli_expectations", "energy", "j1j2_hamiltonian", "spin_correlation_terms", "spin_correlations",
           "structure_factor", "minimize_hamiltonian", "renyi2_from_sums", "renyi2_regions", "renyi2_entropy",
           "renyi2_mutual_information", "symmetry_resolved_renyi2"]


def _native_complex(wf):
    try:
        nat = _native(wf)
    except TypeError as e:
        raise ValueError(str(e))
    if nat.model != _lib.MODEL_CRNN_U1:
        raise ValueError("observables_complex serves the complex RNN (CRNN_U1) only; observables.py serves the GRU models, "
                         "observables_2d.py the 2D RNN")
    return nat


class ComplexHamiltonian:
    """H = sum_k c_k P_k with complex coefficients c_k and Pauli strings P_k (dense or sparse, see observables.pauli_terms) holding
    any number of Y.  .flip, .sign (K, N) and .coeff (K,) complex are rnnwf_pauli_step_complex's arguments; coeff carries the full
    factor (-i)^n_Y of each string."""

    def __init__(self, N, terms):
        self.N = int(N)
        terms = list(terms)
        if not terms:
            raise ValueError("a Hamiltonian needs at least one term")
        self.terms = [(complex(c), st) for c, st in terms]
        self.flip, self.sign, factor = pauli_terms([st for _, st in terms], self.N)
        self.coeff = np.array([c for c, _ in self.terms], dtype=np.complex128) * factor

    def __len__(self):
        return len(self.terms)

    def is_hermitian(self, tol=1e-12):
        """Whether H equals its adjoint, by pairing terms: (c Z_S X_F)^+ = conj(c) (-1)^|S n F| Z_S X_F, so the summed coefficient
        of every distinct (S, F) must be real where |S n F| is even and imaginary where it is odd."""
        total = {}
        for f, s, c in zip(self.flip, self.sign, self.coeff):
            key = (f.tobytes(), s.tobytes())
            odd = int(np.sum(f & s)) & 1
            t = total.setdefault(key, [0j, odd])
            t[0] += c
        scale = max(1.0, float(np.abs(self.coeff).max()))
        return all(abs(c.real if odd else c.imag) <= tol * scale for c, odd in total.values())


def _from_sums(term_sums, numsamples):
    """(mean complex (K,), err of the real part (K,), err of the imaginary part (K,)) from the (K, 4) sums."""
    t = np.asarray(term_sums, dtype=np.float64)
    n = float(numsamples)
    re, im = t[:, 0] / n, t[:, 1] / n
    return (re + 1j * im, np.sqrt(np.maximum(t[:, 2] / n - re * re, 0.0) / n), np.sqrt(np.maximum(t[:, 3] / n - im * im, 0.0) / n))


def pauli_expectations(wf, strings, numsamples, seed=111, step=0, samples=None):
    """<psi|P|psi> of every Pauli string P of `strings` (dense "XZIY..." or sparse [("X", i), ...]) from `numsamples` samples:
    {"value": complex (K,), "err": (K,) standard error of the real part, "err_imag": (K,) of the imaginary part}.  Strings with an
    odd number of Y are evaluated like every other.  samples: (numsamples, N) spins of the zero-magnetisation sector; None draws
    them on the device from (seed, step)."""
    nat = _native_complex(wf)
    flip, sign, factor = pauli_terms(strings, nat.N)
    out = nat.pauli_step_complex(flip, sign, np.ones(len(factor)), int(numsamples), samples=_api.chains(_api.COMPLEX, nat, samples, numsamples),
                                 seed=seed, step=step)
    mean, e_re, e_im = _from_sums(out["term_sums"], numsamples)
    # factor is one of 1, -i, -1, i: it rotates the value and, where imaginary, exchanges the two errors
    swap = factor.imag != 0.0
    return {"value": factor * mean, "err": np.where(swap, e_im, e_re), "err_imag": np.where(swap, e_re, e_im)}


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under `ham` (a ComplexHamiltonian) from `numsamples` samples: {"mean" (complex), "var" (population variance
    of Re E_loc), "err" (sqrt(var / n)), "eloc" (numsamples,) complex64 when want_eloc}.  Warns when `ham` is not Hermitian.  A batch
    that fits one pass stays resident: vmc_gradient(mean, n) then differentiates the complex VMC cost of this Hamiltonian."""
    nat = _native_complex(wf)
    _api.check_sites(nat, ham)
    if not ham.is_hermitian():
        warnings.warn("energy: the Hamiltonian is not Hermitian; its expectation value is complex", stacklevel=2)
    out = _api.local_energies(_api.COMPLEX, nat, ham, numsamples, seed, step, samples, want_eloc)
    m = out["moments"]
    re = m[0] / m[2]
    var = max(m[1] / m[2] - re * re, 0.0)
    res = {"mean": complex(re, m[3] / m[2]), "var": var, "err": float(np.sqrt(var / m[2]))}
    if want_eloc:
        res["eloc"] = out["eloc"]
    return res


def j1j2_hamiltonian(J1, J2, Bz, periodic=False, marshall=False):
    """The J1-J2 chain with the documented semantics of rnnwf_j1j2_eloc (J1, J2, Bz: (N,) each):

        H = sum_i J1_i/4 (m (XX + YY) + ZZ)_{i,i+1} + sum_i J2_i/4 (XX + YY + ZZ)_{i,i+2} + sum_i Bz_i/2 Z_i

    with m = -1 under `marshall` (the Marshall rotation of the nearest-neighbour exchange).  Open boundaries drop the wrapped bonds
    (i + 1 >= N, i + 2 >= N); bonds with a zero coupling are left out."""
    J1, J2, Bz = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (J1, J2, Bz))
    N = len(J1)
    if N < 2 or len(J2) != N or len(Bz) != N:
        raise ValueError("J1, J2 and Bz must have one entry per site of a chain of N >= 2 sites")
    m = -1.0 if marshall else 1.0
    terms = []
    for dist, J, mm in ((1, J1, m), (2, J2, 1.0)):
        for i in range(N if periodic else N - dist):
            j = (i + dist) % N
            if J[i] == 0.0 or i == j:
                continue
            terms += [(mm * J[i] / 4, [("X", i), ("X", j)]), (mm * J[i] / 4, [("Y", i), ("Y", j)]), (J[i] / 4, [("Z", i), ("Z", j)])]
    terms += [(Bz[i] / 2, [("Z", i)]) for i in range(N) if Bz[i] != 0.0]
    if not terms:
        raise ValueError("every coupling is zero")
    return ComplexHamiltonian(N, terms)


def spin_correlation_terms(N):
    """pairs (P, 2) i < j in lexicographic order and the 3 P strings XX, YY, ZZ of every pair, pair-major: XX and YY of a pair share
    one flip mask (one evaluation), ZZ is diagonal (none)."""
    pairs = np.array([(i, j) for i in range(N) for j in range(i + 1, N)], dtype=np.int64).reshape(-1, 2)
    strings = []
    for i, j in pairs:
        strings += [[("X", int(i)), ("X", int(j))], [("Y", int(i)), ("Y", int(j))], [("Z", int(i)), ("Z", int(j))]]
    return pairs, strings


def spin_correlations(wf, numsamples, seed=111, step=0, samples=None):
    """<S_i . S_j> = 1/4 (<XX> + <YY> + <ZZ>) of every pair of sites from one pauli_step_complex call (one flip mask per pair, <ZZ>
    from the samples): {"corr": (N, N) real symmetric with diagonal 3/4, "err": (N, N) standard errors (diagonal 0), "imag": (N, N)
    the imaginary parts of the estimates, which vanish within "err_imag" for a Hermitian operator}.  The errors are those of the
    per-sample value 1/4 [(1 - s_i s_j) psi(sigma ^ {i, j}) / psi(sigma) + s_i s_j]."""
    nat = _native_complex(wf)
    N, n = nat.N, int(numsamples)
    pairs, strings = spin_correlation_terms(N)
    flip, sign, factor = pauli_terms(strings, N)
    out = nat.pauli_step_complex(flip, sign, 0.25 * factor, n, samples=_api.chains(_api.COMPLEX, nat, samples, n), seed=seed, step=step,
                                 want_log_ratio=True, want_samples=True)
    _, index = group_by_mask(flip)
    lr = out["log_ratio"]
    with np.errstate(invalid="ignore"):
        r = np.where(np.isneginf(lr.real), 0.0, np.exp(lr))      # (P, n) psi(sigma ^ {i, j}) / psi(sigma)
    s = 2.0 * out["samples"].reshape(n, N).T - 1.0               # (N, n)
    ss = s[pairs[:, 0]] * s[pairs[:, 1]]
    v = 0.25 * ((1.0 - ss) * r[index[0::3]] + ss)                # (P, n) complex
    corr, err, imag, err_imag = (np.zeros((N, N)) for _ in range(4))
    np.fill_diagonal(corr, 0.75)
    for a, b in ((pairs[:, 0], pairs[:, 1]), (pairs[:, 1], pairs[:, 0])):
        corr[a, b], err[a, b] = v.real.mean(axis=1), v.real.std(axis=1) / np.sqrt(n)
        imag[a, b], err_imag[a, b] = v.imag.mean(axis=1), v.imag.std(axis=1) / np.sqrt(n)
    return {"corr": corr, "err": err, "imag": imag, "err_imag": err_imag, "pairs": pairs}


def structure_factor(corr, q):
    """S(q) = (1/N) sum_{jk} exp(i q (j - k)) <S_j . S_k> of an (N, N) correlation matrix, for one q or an array of them; real for a
    symmetric matrix."""
    corr = np.asarray(corr, dtype=np.float64)
    if corr.ndim != 2 or corr.shape[0] != corr.shape[1] or corr.shape[0] < 1:
        raise ValueError("corr must be a square (N, N) matrix, got shape %r" % (corr.shape,))
    N = corr.shape[0]
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    d = np.arange(N)[:, None] - np.arange(N)[None, :]
    out = np.array([float(np.real((np.exp(1j * x * d) * corr).sum())) / N for x in qs])
    return out if np.ndim(q) else float(out[0])


def minimize_hamiltonian(wf, ham, numsamples, steps, lr, params=None, seed=111, scope="RNNwavefunction", opt=None, verbose=False,
                         device_steps=None):
    """Minimise the energy of the complex RNN `wf` under `ham` (a ComplexHamiltonian) with training.minimize_hamiltonian's loop:
    pauli_step_complex (samples, complex local energies of `ham`, moments; the batch stays resident) -> vmc_gradient(mean_re,
    mean_im, n) of the complex cost -> training.Adam on the host -> set_params.  wf: the J1J2.ComplexRNNwavefunction facade (its own
    parameters and scope are used and updated) or a NativeWavefunction with `params` scoped by `scope`.  Returns (meanEnergy complex,
    varEnergy of the real part), one entry per iteration 0..steps; the trained parameters are left in
    minimize_hamiltonian.last_params.  The batch must fit one pass of the state budget.  Single process.
    device_steps=K (an integer >= 1): the same iterations run on the device in chunks of at most K with one host synchronisation
    each (pauli_train_steps_complex, docs/pauli_train.md) - the same energies, variances and parameters, bit for bit.  The device
    runs Adam from a fresh state: opt= is refused with it."""
    from .training import check_device_steps
    device_steps = check_device_steps(device_steps, opt, _api.COMPLEX.label)
    nat = _native_complex(wf)
    _api.check_sites(nat, ham)
    facade = wf if wf is not nat else None
    if facade is not None:
        params, scope = facade.get_params(), facade.scope
    if params is None:
        raise ValueError("minimize_hamiltonian on a NativeWavefunction needs its parameters (params=...)")
    meanEnergy, varEnergy, params = _api.minimize_loop(nat.pauli_step_complex, nat.pauli_train_steps_complex,
                                                       lambda s1, si, n: complex(s1 / n, si / n), nat, ham, params, scope, int(steps),
                                                       int(numsamples), lr, seed, opt, device_steps, verbose)
    if facade is not None:
        facade.set_params(params)
    minimize_hamiltonian.last_params = params
    return meanEnergy, varEnergy


# ---- second Renyi entropy (rnnwf_renyi2_regions_complex, docs/renyi_complex.md) ---------------------------------------------------
# For pairs (sigma, tau) drawn independently from |psi|^2 the swap estimator is complex,
#     r_A = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)),   exp(-S2(A)) = E[Re r_A],   E[Im r_A] = 0,
# and r_A = 0 exactly unless sigma and tau carry the same number of ups in A (the mixed chains leave the sector otherwise).

def renyi2_from_sums(sums, numpairs):
    """From the (R, 4) sums [sum Re r, sum Im r, sum (Re r)^2, sum (Im r)^2] of numpairs pairs: {"S2": -log(mean Re r) (R,), "err":
    std(Re r) / (sqrt(n) mean Re r) (first-order error propagation), "imag": mean Im r, "err_imag": its standard error}.  The exact
    mean of Im r is 0: "imag" within a few "err_imag" is a check of the sample, not a result.  A region whose mean is not positive
    gives nan."""
    t = np.asarray(sums, dtype=np.float64)
    n = float(numpairs)
    if t.ndim != 2 or t.shape[1] != 4 or n < 1:
        raise ValueError("sums must have shape (R, 4) and numpairs be >= 1")
    re, im = t[:, 0] / n, t[:, 1] / n
    var_re, var_im = np.maximum(t[:, 2] / n - re * re, 0.0), np.maximum(t[:, 3] / n - im * im, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S2 = np.where(re > 0.0, -np.log(np.where(re > 0.0, re, 1.0)), np.nan)
        err = np.where(re > 0.0, np.sqrt(var_re) / (np.sqrt(n) * np.where(re > 0.0, re, 1.0)), np.nan)
    return {"S2": S2, "err": err, "imag": im, "err_imag": np.sqrt(var_im / n)}


def renyi2_regions(wf, regions, numpairs, seed=111, step=0, samples=None, want_log_ratio=False):
    """Second Renyi entropy S2(A) of the regions `regions` ((R, N) masks of 0 / 1, or one mask; observables.interval_region builds
    them) from `numpairs` pairs of independent samples of the complex RNN `wf`: the dict of renyi2_from_sums plus "survivors" (R,),
    the fraction of the pairs whose mixed chains stay in the zero-magnetisation sector (the only ones that cost anything), and, with
    want_log_ratio, "log_ratio" (R, numpairs) complex128 (-inf + 0j outside the sector) and "samples" (2 numpairs, N).  samples:
    (2 numpairs, N) spins of the sector, pair p = rows 2p and 2p + 1; None draws them on the device from (seed, step)."""
    nat = _native_complex(wf)
    out, s = _api.regions(_api.COMPLEX, nat, regions, numpairs, seed, step, samples, log_ratio=want_log_ratio)
    res = renyi2_from_sums(out["sums"], numpairs)
    res["survivors"] = out["in_sector"] / float(numpairs)
    if want_log_ratio:
        res["log_ratio"] = out["log_ratio"]
        res["samples"] = out["samples"] if s is None else s
    return res


def renyi2_entropy(wf, numpairs, seed=111, step=0, samples=None):
    """renyi2_regions of the N - 1 cuts of the chain: row l - 1 is A = the first l sites, l = 1..N-1."""
    nat = _native_complex(wf)
    cuts = (np.arange(nat.N)[None, :] < np.arange(1, nat.N)[:, None]).astype(np.int32)
    return renyi2_regions(nat, cuts, numpairs, seed=seed, step=step, samples=samples)


def renyi2_mutual_information(wf, region_a, region_b, numpairs, seed=111, step=0, samples=None):
    """Renyi-2 mutual information I2(A : B) = S2(A) + S2(B) - S2(A u B) of two DISJOINT regions (masks of N entries) and its standard
    error by the delta method on the shared pairs (observables.mutual_information2_from_values on Re r); A, B and A u B run in one
    call.  Overlapping regions raise ValueError."""
    a, b = _disjoint_masks(region_a, region_b)
    log_ratio = _api.mutual_log_ratios(_api.COMPLEX, _native_complex(wf), a, b, numpairs, seed, step, samples)
    return mutual_information2_from_values(*_ratio(log_ratio).real)


def _ratio(log_ratio):
    """exp of complex log-ratios, exactly 0 where the real part is -inf"""
    lr = np.asarray(log_ratio, dtype=np.complex128)
    zero = np.isneginf(lr.real)
    return np.where(zero, 0.0, np.exp(np.where(zero, 0.0, lr)))


def symmetry_resolved_renyi2(log_ratio_row, samples, region):
    """The second Renyi entropy of region A resolved by the U(1) charge q = number of ups in A, from the per-pair log r_A of ONE
    region ((n,) complex, the "log_ratio" row of renyi2_regions), the pairs' spins ((2 n, N), pair p = rows 2p, 2p + 1) and the mask
    of A as it was asked for ((N,) of 0 / 1).  rho_A is block-diagonal in q; with q_p the charge of sigma_p (equal to tau_p's in every
    pair that survives)

        p_q = P(q) = E[(1(q_sigma = q) + 1(q_tau = q)) / 2],   Tr rho_A(q)^2 = E[Re r 1(q_sigma = q)],
        S2(q) = -log(Tr rho_A(q)^2 / p_q^2)

    for q = 0..|A|: {"q", "p", "p_err", "trace", "trace_err", "S2", "S2_err"}, each (|A| + 1,).  sum_q trace = mean Re r, the total.
    S2_err by the delta method on g = -t / trace + 2 u / p of the per-pair values t, u.  A charge that no chain shows, or whose
    estimated trace is not positive, has S2 = nan."""
    lr = np.asarray(log_ratio_row, dtype=np.complex128)
    m = np.asarray(region)
    s = np.asarray(samples)
    if lr.ndim != 1 or lr.size < 1 or m.ndim != 1 or not np.all((m == 0) | (m == 1)) or s.shape != (2 * lr.size, m.size):
        raise ValueError("symmetry_resolved_renyi2 needs log r of n >= 1 pairs, samples (2 n, N) and a mask of N entries of 0 / 1")
    n = lr.size
    re = _ratio(lr).real
    qs = s[0::2][:, m == 1].sum(axis=1)
    qt = s[1::2][:, m == 1].sum(axis=1)
    if np.any((re != 0.0) & (qs != qt)):
        raise ValueError("a pair with r != 0 carries different charges in the region: log_ratio_row, samples and region do not belong together")
    nq = int(m.sum()) + 1
    out = {k: np.full(nq, np.nan) for k in ("p", "p_err", "trace", "trace_err", "S2", "S2_err")}
    out["q"] = np.arange(nq)
    for q in range(nq):
        t = re * (qs == q)
        u = 0.5 * ((qs == q).astype(np.float64) + (qt == q))
        tr, p = t.mean(), u.mean()
        out["p"][q], out["p_err"][q] = p, u.std() / np.sqrt(n)
        out["trace"][q], out["trace_err"][q] = tr, t.std() / np.sqrt(n)
        if p > 0.0 and tr > 0.0:
            out["S2"][q] = -np.log(tr / (p * p))
            out["S2_err"][q] = (-t / tr + 2.0 * u / p).std() / np.sqrt(n)
    return out
