"""Observables beyond the energy: the second Renyi entropy S2(l) of the region A = the first l sites, every cut at once, by the
replica swap estimator (Hastings, Gonzalez, Kallin, Melko, PRL 104, 157201 (2010)) on the GPU (rnnwf_renyi2_swap).

For pairs (sigma, tau) drawn independently from |psi|^2,  exp(-S2(l)) = E[r_l],
    r_l = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)).
Several devices: each draws its own pairs (pair_offset) and the (N + 1, 2) sums add up - all-reduce them with
NativeWavefunction.allreduce_f64, then call renyi2_from_sums with the global pair count.  docs/renyi.md has the details.
"""
import warnings

import numpy as np

from . import _lib


def _native(wf):
    """The NativeWavefunction behind a reference-named facade (GRUWavefunction1D, GRUWavefunction2DRaster, their aliases)."""
    if isinstance(wf, _lib.NativeWavefunction):
        return wf
    nat = getattr(wf, "_native", None)
    if isinstance(nat, _lib.NativeWavefunction):
        return nat
    raise TypeError("renyi2_entropy needs a wave-function facade or a NativeWavefunction, got %r" % (wf,))


def renyi2_from_sums(sums, npairs):
    """S2 (N+1,) and its standard error (N+1,) from the swap sums (N+1, 2) = [sum_p r_l, sum_p r_l^2] of npairs pairs:
    S2 = -log(mean r),  sigma = std(r) / (sqrt(npairs) mean r)  (first-order error propagation).  A cut whose sums are not
    finite (a pair with log r > 709) gives nan, with a warning."""
    sums = np.asarray(sums, dtype=np.float64)
    n = float(npairs)
    if sums.ndim != 2 or sums.shape[1] != 2 or n < 1:
        raise ValueError("sums must have shape (N+1, 2) and npairs be >= 1")
    bad = ~np.all(np.isfinite(sums), axis=1)
    if bad.any():
        warnings.warn("renyi2: the swap sums of cuts %s are not finite (a pair with log r > 709); S2 is nan there"
                      % np.flatnonzero(bad).tolist(), RuntimeWarning, stacklevel=2)
    s1 = np.where(bad, np.nan, sums[:, 0])
    s2 = np.where(bad, np.nan, sums[:, 1])
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        S2 = -np.log(mean)
        err = np.sqrt(var) / (np.sqrt(n) * mean)
    return S2, err


def renyi2_entropy(wf, numpairs, seed=111, step=0, samples=None):
    """Second Renyi entropy S2(l), l = 0..N, and its standard error, from `numpairs` pairs of independent samples of `wf`
    (a facade such as TFIM1D.RNNwavefunction / TFIM2D_1DRNN.RNNwavefunction, or a NativeWavefunction).  The cut l counts
    sites in the model's order (the raster order ny * Nx + nx for the 2D raster model).  samples: (2 numpairs, N) spins,
    pair p = rows 2p and 2p + 1; None draws them on the device from (seed, step).  Refused models (parity, complex RNN,
    2D RNN, LSTM, stacked layers) raise ValueError with the library's reason."""
    nat = _native(wf)
    if samples is not None:
        samples = np.asarray(samples).reshape(2 * int(numpairs), nat.N)
    out = nat.renyi2_swap(int(numpairs), samples=samples, seed=seed, step=step)
    return renyi2_from_sums(out["sums"], numpairs)
