"""Pauli-string expectation values, energies of arbitrary real spin Hamiltonians, two-point functions and training on such a
Hamiltonian for the LSTM wave function over the raster path: model LSTM1D_F64, one layer of 1..68 units, float64 - the default cell of
the reference's 2D raster constructor (rnnwf_pauli_step_lstm, rnnwf_lstm_pauli_gradient_step; docs/pauli_lstm.md).

The estimator, the strings and the Hamiltonians are observables.py's:  v(sigma) = prod_{i in S} s_i * exp(1/2 [log P(sigma ^ F) -
log P(sigma)]),  E[v] = <psi|O|psi>;  sites in the model's order, the raster index ny * Nx + nx = the column of a (ns, Nx * Ny)
sample.  observables.pauli_expectations / energy / correlations and training.minimize_hamiltonian keep refusing the LSTM; these are
its own entry points.  They accept a facade or a NativeWavefunction of the LSTM model and raise ValueError for everything else,
naming the module that serves that model, before the library is touched.

The second Renyi entropy of arbitrary regions, block entropies and the Renyi-2 mutual information by the replica swap estimator of
observables.py (rnnwf_renyi2_regions_lstm; docs/renyi_lstm.md): renyi2_regions, renyi2_entropy, renyi2_mutual_information, with
observables.py's region builders re-exported.  observables.renyi2_regions / renyi2_mutual_information keep refusing the LSTM.

Every site and every pair at once (rnnwf_correlations_lstm; docs/correlations_lstm.md): correlation_matrix, the trunk / branch pass
that observables.correlations runs for the GRU, and structure_factor of one of its matrices.  `correlations` below stays the
pair-list form on pauli_step_lstm.

Not here: minSR (docs/lstm.md, "Out of scope").  Device-resident Adam on a Hamiltonian is training_lstm.minimize_hamiltonian_device
(docs/lstm.md, "Device-resident training"); minimize_hamiltonian below keeps refusing device_steps.
"""
import numpy as np

from . import _lib
from . import _observable_api as _api
from .observables import Hamiltonian, _native, pauli_terms, tfim_hamiltonian, xxz_hamiltonian  # noqa: F401
from .observables import correlations_from_sums  # noqa: F401
from .observables import _disjoint_masks, column_cut_regions, interval_region, rectangle_region, renyi2_from_sums  # noqa: F401

# tests/test_lstm_pauli_host.py pins this list; the Renyi functions and the re-exported region builders below are public all the same
# (RENYI_API names them)
__all__ = ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]
RENYI_API = ["renyi2_regions", "renyi2_entropy", "renyi2_mutual_information", "interval_region", "rectangle_region", "column_cut_regions",
             "renyi2_from_sums"]
# likewise outside __all__: the all-pair correlation pass (docs/correlations_lstm.md)
CORRELATION_API = ["correlation_matrix", "structure_factor", "correlations_from_sums"]

_SERVED_BY = {
    _lib.MODEL_GRU1D: "observables.py serves the GRU models (observables_stack.py their stacked layers)",
    _lib.MODEL_GRU1D_F64: "observables.py serves the GRU models (observables_stack.py their stacked layers)",
    _lib.MODEL_GRU1D_PARITY: "no Pauli pass serves the parity model",
    _lib.MODEL_CRNN_U1: "observables_complex.py serves the complex RNN",
    _lib.MODEL_MDRNN2D: "observables_2d.py serves the 2D RNN",
}


def _native_lstm(wf):
    try:
        nat = _native(wf)
    except TypeError as e:
        raise ValueError(str(e))
    if nat.model != _lib.MODEL_LSTM1D_F64:
        raise ValueError("observables_lstm serves the LSTM wave function (LSTM1D_F64) only; %s" % _SERVED_BY.get(nat.model, "this model has no module"))
    return nat


def lr_schedule(learningrate, it):
    """the learning rate of iteration `it` in training_lstm.run_2DTFIM_1DRNN_LSTM: 1 / (1 / lr + it / 10)"""
    return 1.0 / ((1.0 / learningrate) + it / 10)


# ---- second Renyi entropy (rnnwf_renyi2_regions_lstm, docs/renyi_lstm.md) --------------------------------------------------------

def renyi2_regions(wf, regions, numpairs, seed=111, step=0, samples=None):
    """Second Renyi entropy S2(A) (R,) and its standard error (R,) of the regions `regions` ((R, N) masks of 0 / 1, or one mask, or
    (R, Nx, Ny); 1 = site in A, sites by chain position: the raster index ny * Nx + nx, the column of a (ns, Nx * Ny) sample) from
    `numpairs` pairs of independent samples.  samples: (2 numpairs, N) or (2 numpairs, Nx, Ny) spins, pair p = rows 2p and 2p + 1;
    None draws them on the device from (seed, step)."""
    return _api.renyi2_regions(_api.LSTM, _native_lstm(wf), regions, numpairs, seed, step, samples)


def renyi2_entropy(wf, numpairs, seed=111, step=0, samples=None):
    """S2(l) of A = the first l sites (chain positions), l = 0..N, and its standard error, (N + 1,) each, in one call: the region of
    cut l is given as its complement, the suffix {l..N-1} (r_A = r_complement).  Cuts 0 and N are exactly 0 +- 0."""
    nat = _native_lstm(wf)
    suffixes = np.stack([interval_region(nat.N, l, nat.N) for l in range(nat.N + 1)])
    return _api.renyi2_regions(_api.LSTM, nat, suffixes, numpairs, seed, step, samples)


def renyi2_mutual_information(wf, region_a, region_b, numpairs, seed=111, step=0, samples=None):
    """Renyi-2 mutual information I2(A : B) = S2(A) + S2(B) - S2(A u B) of two DISJOINT regions (masks of N entries) and its standard
    error (observables.mutual_information2_from_log_ratios), from `numpairs` pairs; A, B and A u B run in one call on the same
    pairs."""
    a, b = _disjoint_masks(region_a, region_b)
    return _api.renyi2_mutual_information(_api.LSTM, _native_lstm(wf), a, b, numpairs, seed, step, samples)


def pauli_expectations(wf, strings, numsamples, seed=111, step=0, samples=None):
    """<psi|P|psi> of every Pauli string P of `strings` (dense "XZIY..." or sparse [("X", i), ...]) with its standard error, from
    `numsamples` samples: {"value": (K,), "err": (K,)}.  A string with an odd number of Y has expectation exactly 0 in the real state
    psi = sqrt(P): 0 +- 0, without device work.  samples: (numsamples, N) or (numsamples, Nx, Ny) spins as lstm_gradient takes them;
    None draws them on the device from (seed, step)."""
    return _api.pauli_expectations(_api.LSTM, _native_lstm(wf), strings, numsamples, seed, step, samples)


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under the Hamiltonian `ham` from `numsamples` samples: {"mean", "var" (population variance of E_loc), "err"
    (sqrt(var / n)), "eloc" (numsamples,) when want_eloc}.  No batch stays resident: the gradient of this energy is
    NativeWavefunction.lstm_pauli_gradient_step's."""
    return _api.energy(_api.LSTM, _native_lstm(wf), ham, numsamples, seed, step, samples, want_eloc)


def minimize_hamiltonian(wf, ham, params, numsteps=1000, numsamples=500, learningrate=5e-3, seed=111, scope="RNNwavefunction",
                         opt=None, comm=None, verbose=False, device_steps=None):
    """training.minimize_hamiltonian for the LSTM wave function: minimise the energy of `wf` (holding `params`, scoped by `scope`)
    under `ham` (observables.Hamiltonian) with the host optimizer loop  lstm_pauli_gradient_step (samples, local energies of `ham`,
    moments and the gradient of the cost, one library call with one host synchronisation) -> training.Adam -> set_params,  the loop
    of training_lstm.run_2DTFIM_1DRNN_LSTM with its learning rate 1 / (1 / learningrate + it / 10) in iteration it.  Returns
    (meanEnergy, varEnergy), one entry per iteration 0..numsteps; the trained parameters are left in
    minimize_hamiltonian.last_params.  The batch of numsamples must fit one pass of the state budget.  Single process only: a
    communicator is refused.  device_steps is refused here, in the words it always was: the same loop with its iterations on the device is
    training_lstm.minimize_hamiltonian_device (docs/lstm.md, "Device-resident training")."""
    _native_lstm(wf)                                  # another model is told its module before it is told about device_steps
    meanEnergy, varEnergy, minimize_hamiltonian.last_params = _api.minimize_family(
        _api.LSTM, _native_lstm, wf, ham, params, numsteps, numsamples, learningrate, seed, scope, opt, comm, verbose, device_steps,
        lr_of_it=lr_schedule)
    return meanEnergy, varEnergy


def correlations(wf, numsamples, pairs=None, seed=111, step=0, samples=None):
    """<sz_k>, <sx_k> of every site and, for the listed pairs of distinct sites, <sz_a sz_b>, <sx_a sx_b> and their connected parts,
    with standard errors, from one pauli_step_lstm call (one X mask per site, one XX mask per pair):

        z, x (N,);  pairs (P, 2);  zz, xx, zz_c = zz - z_a z_b, xx_c = xx - x_a x_b (P,);  "<name>_err" for each.

    pairs: None = every pair (c, k), k != c, with the centre site c = N // 2.  A pair (k, k) raises ValueError.  Errors: the plain
    std / sqrt(n) (population variance) of the per-sample values s_k, r_k = exp(log r_k), s_a s_b, r_ab, which the call returns as
    log-ratios and samples; connected parts to first order (delta method), as observables_2d.correlations."""
    return _api.correlations(_api.LSTM, _native_lstm(wf), numsamples, pairs, seed, step, samples)


# ---- every site and pair at once (rnnwf_correlations_lstm, docs/correlations_lstm.md) --------------------------------------------

def correlation_matrix(wf, numsamples, seed=111, step=0, samples=None):
    """<sz_i>, <sz_i sz_j>, <sx_i>, <sx_i sx_j> of every site and every pair and the connected two-point functions, with standard
    errors (the connected ones' by the delta method, from cross moments reduced on the device), from `numsamples` samples in one
    correlations_lstm call: the dict of observables.correlations_from_sums - z, x (N,); zz, xx, zz_c, xx_c (N, N); "<name>_err" for
    each.  Sites by chain position: the raster index ny * Nx + nx, the column of a (ns, Nx * Ny) sample.  samples: (numsamples, N) or
    (numsamples, Nx, Ny) spins; None draws them on the device from (seed, step)."""
    nat = _native_lstm(wf)
    out = nat.correlations_lstm(int(numsamples), samples=samples, seed=seed, step=step)
    return correlations_from_sums(out["z_sums"], out["zz_sums"], out["x_sums"], out["xx_sums"], numsamples)


def structure_factor(corr, qx, qy, Nx, Ny):
    """S(q) = (1 / N) sum_{jk} exp(i q . (r_j - r_k)) C_jk of an (N, N) matrix `corr` over the sites of correlation_matrix (for
    instance its "zz_c" or "xx_c"), N = Nx Ny, site n at (nx, ny) = (n mod Nx, n div Nx).  qx, qy: one wave vector or arrays of
    them (broadcast against each other).  Returns S(q) in their shape: real for a real symmetric `corr`, complex otherwise."""
    c = np.asarray(corr)
    N = int(Nx) * int(Ny)
    if c.shape != (N, N):
        raise ValueError("corr must have shape (%d, %d) = (Nx Ny, Nx Ny), got %r" % (N, N, c.shape))
    qx, qy = np.broadcast_arrays(np.asarray(qx, dtype=np.float64), np.asarray(qy, dtype=np.float64))
    n = np.arange(N)
    phase = np.exp(1j * (qx[..., None] * (n % int(Nx)) + qy[..., None] * (n // int(Nx))))      # (..., N): exp(i q . r_n)
    sq = np.einsum("...j,jk,...k->...", phase, c, phase.conj()) / N
    if np.isrealobj(c) and np.array_equal(c, c.T):
        sq = sq.real
    return sq[()] if sq.ndim == 0 else sq
