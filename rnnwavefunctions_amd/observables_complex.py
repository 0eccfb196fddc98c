"""Pauli-string expectation values, energies of arbitrary spin-1/2 Hamiltonians, spin-spin correlations and the structure factor
for the complex RNN with the U(1) mask (model CRNN_U1, one layer; rnnwf_pauli_step_complex, docs/pauli_complex.md).

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
from .observables import _native, group_by_mask, pauli_terms

__all__ = ["ComplexHamiltonian", "pauli_expectations", "energy", "j1j2_hamiltonian", "spin_correlation_terms", "spin_correlations",
           "structure_factor", "minimize_hamiltonian"]


def _native_complex(wf):
    try:
        nat = _native(wf)
    except TypeError as e:
        raise ValueError(str(e))
    if nat.model != _lib.MODEL_CRNN_U1:
        raise ValueError("observables_complex serves the complex RNN (CRNN_U1) only; observables.py serves the GRU models, "
                         "observables_2d.py the 2D RNN")
    return nat


def _samples(nat, samples, numsamples):
    return None if samples is None else np.asarray(samples).reshape(int(numsamples), nat.N)


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
    out = nat.pauli_step_complex(flip, sign, np.ones(len(factor)), int(numsamples), samples=_samples(nat, samples, numsamples), seed=seed,
                                 step=step)
    mean, e_re, e_im = _from_sums(out["term_sums"], numsamples)
    # factor is one of 1, -i, -1, i: it rotates the value and, where imaginary, exchanges the two errors
    swap = factor.imag != 0.0
    return {"value": factor * mean, "err": np.where(swap, e_im, e_re), "err_imag": np.where(swap, e_re, e_im)}


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under `ham` (a ComplexHamiltonian) from `numsamples` samples: {"mean" (complex), "var" (population variance
    of Re E_loc), "err" (sqrt(var / n)), "eloc" (numsamples,) complex64 when want_eloc}.  Warns when `ham` is not Hermitian.  A batch
    that fits one pass stays resident: vmc_gradient(mean, n) then differentiates the complex VMC cost of this Hamiltonian."""
    nat = _native_complex(wf)
    if ham.N != nat.N:
        raise ValueError("the Hamiltonian has %d sites, the wave function %d" % (ham.N, nat.N))
    if not ham.is_hermitian():
        warnings.warn("energy: the Hamiltonian is not Hermitian; its expectation value is complex", stacklevel=2)
    out = nat.pauli_step_complex(ham.flip, ham.sign, ham.coeff, int(numsamples), samples=_samples(nat, samples, numsamples), seed=seed,
                                 step=step, want_eloc=want_eloc)
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
    out = nat.pauli_step_complex(flip, sign, 0.25 * factor, n, samples=_samples(nat, samples, n), seed=seed, step=step, want_log_ratio=True,
                                 want_samples=True)
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


def minimize_hamiltonian(wf, ham, numsamples, steps, lr, params=None, seed=111, scope="RNNwavefunction", opt=None, verbose=False):
    """Minimise the energy of the complex RNN `wf` under `ham` (a ComplexHamiltonian) with training.minimize_hamiltonian's loop:
    pauli_step_complex (samples, complex local energies of `ham`, moments; the batch stays resident) -> vmc_gradient(mean_re,
    mean_im, n) of the complex cost -> training.Adam on the host -> set_params.  wf: the J1J2.ComplexRNNwavefunction facade (its own
    parameters and scope are used and updated) or a NativeWavefunction with `params` scoped by `scope`.  Returns (meanEnergy complex,
    varEnergy of the real part), one entry per iteration 0..steps; the trained parameters are left in
    minimize_hamiltonian.last_params.  The batch must fit one pass of the state budget.  Single process, host optimizer."""
    from .training import Adam, cost_gradient
    nat = _native_complex(wf)
    if ham.N != nat.N:
        raise ValueError("the Hamiltonian has %d sites, the wave function %d" % (ham.N, nat.N))
    facade = wf if wf is not nat else None
    if facade is not None:
        params, scope = facade.get_params(), facade.scope
    if params is None:
        raise ValueError("minimize_hamiltonian on a NativeWavefunction needs its parameters (params=...)")
    opt = opt or Adam()
    params = {k: np.array(v) for k, v in params.items()}
    nat.set_params(params, scope=scope)
    meanEnergy, varEnergy = [], []
    for it in range(int(steps) + 1):
        s1, s2, n, si = nat.pauli_step_complex(ham.flip, ham.sign, ham.coeff, int(numsamples), seed=seed, step=it)["moments"]
        meanE = complex(s1 / n, si / n)
        varE = s2 / n - (s1 / n) ** 2
        meanEnergy.append(meanE)
        varEnergy.append(varE)
        if verbose and it % 10 == 0:
            print("mean(E): {0}, var(E): {1}, #samples {2}, #Step {3} \n\n".format(meanE, varE, numsamples, it))
        grads = cost_gradient(nat, params, scope, meanE, n)
        params = opt.step(params, grads, lr)
        nat.set_params(params, scope=scope)
    if facade is not None:
        facade.set_params(params)
    minimize_hamiltonian.last_params = params
    return meanEnergy, varEnergy
