"""Pauli-string expectation values, energies of arbitrary real spin Hamiltonians, two-point functions and training on such a
Hamiltonian for STACKED GRU layers: the positive models GRU1D (float32) and GRU1D_F64 (float64, raster path) with 2..4 layers - what
units=[h] * num_layers builds (rnnwf_pauli_step_stack, rnnwf_pauli_train_steps_stack; docs/pauli_stack.md).

The estimator, the strings and the Hamiltonians are observables.py's:  v(sigma) = prod_{i in S} s_i * exp(1/2 [log P(sigma ^ F) -
log P(sigma)]),  E[v] = <psi|O|psi>;  sites in the model's order.  observables.pauli_expectations / energy / correlations and
training.minimize_hamiltonian keep refusing stacks; these are the stacks' own entry points.  They accept a facade or a
NativeWavefunction of one of the two models with more than one layer and raise ValueError for everything else - a one-layer wave
function included, which observables.py serves - before the library is touched.

The second Renyi entropy of arbitrary regions, block entropies and the Renyi-2 mutual information by the replica swap estimator of
observables.py (rnnwf_renyi2_regions_stack; docs/renyi_stack.md): renyi2_regions, renyi2_entropy, renyi2_mutual_information, with
observables.py's region builders re-exported.
"""
import numpy as np

from . import _lib
from . import _observable_api as _api
from .observables import Hamiltonian, _native, group_by_mask, pauli_from_sums, pauli_terms, tfim_hamiltonian, xxz_hamiltonian  # noqa: F401
from .observables import (_disjoint_masks, column_cut_regions, interval_region, mutual_information2_from_log_ratios,  # noqa: F401
                          rectangle_region, renyi2_from_sums)

# tests/test_pauli_stack_host.py pins this list; the Renyi functions and the re-exported region builders below are public all the same
# (RENYI_API names them)
__all__ = ["pauli_expectations", "energy", "correlations", "minimize_hamiltonian"]
RENYI_API = ["renyi2_regions", "renyi2_entropy", "renyi2_mutual_information", "interval_region", "rectangle_region", "column_cut_regions",
             "renyi2_from_sums"]


def _native_stack(wf):
    nat = _native(wf)
    if nat.model not in (_lib.MODEL_GRU1D, _lib.MODEL_GRU1D_F64):
        raise ValueError("observables_stack serves stacked layers of the positive GRU models (GRU1D, GRU1D_F64) only")
    if len(nat.units) < 2:
        raise ValueError("observables_stack serves stacked layers (2..%d GRU layers), this wave function has one layer; observables.py "
                         "and training.minimize_hamiltonian serve it" % _lib.MAX_LAYERS)
    return nat


# ---- second Renyi entropy (rnnwf_renyi2_regions_stack, docs/renyi_stack.md) ------------------------------------------------------

def renyi2_regions(wf, regions, numpairs, seed=111, step=0, samples=None):
    """Second Renyi entropy S2(A) (R,) and its standard error (R,) of the regions `regions` ((R, N) masks of 0 / 1, or one mask;
    1 = site in A, sites in the model's order: raster ny * Nx + nx for the 2D raster model) from `numpairs` pairs of independent
    samples.  samples: (2 numpairs, N) spins, pair p = rows 2p and 2p + 1; None draws them on the device from (seed, step)."""
    return _api.renyi2_regions(_api.STACK, _native_stack(wf), regions, numpairs, seed, step, samples)


def renyi2_entropy(wf, numpairs, seed=111, step=0, samples=None):
    """S2(l) of A = the first l sites (the model's order), l = 0..N, and its standard error, (N + 1,) each, in one call: the region
    of cut l is given as its complement, the suffix {l..N-1} (r_A = r_complement).  Cuts 0 and N are exactly 0 +- 0."""
    nat = _native_stack(wf)
    suffixes = np.stack([interval_region(nat.N, l, nat.N) for l in range(nat.N + 1)])
    return _api.renyi2_regions(_api.STACK, nat, suffixes, numpairs, seed, step, samples)


def renyi2_mutual_information(wf, region_a, region_b, numpairs, seed=111, step=0, samples=None):
    """Renyi-2 mutual information I2(A : B) = S2(A) + S2(B) - S2(A u B) of two DISJOINT regions (masks of N entries) and its standard
    error (observables.mutual_information2_from_log_ratios), from `numpairs` pairs; A, B and A u B run in one call on the same
    pairs."""
    a, b = _disjoint_masks(region_a, region_b)
    return _api.renyi2_mutual_information(_api.STACK, _native_stack(wf), a, b, numpairs, seed, step, samples)


def pauli_expectations(wf, strings, numsamples, seed=111, step=0, samples=None):
    """<psi|P|psi> of every Pauli string P of `strings` (dense "XZIY..." or sparse [("X", i), ...]) with its standard error, from
    `numsamples` samples: {"value": (K,), "err": (K,)}.  A string with an odd number of Y has expectation exactly 0 in the real state
    psi = sqrt(P): 0 +- 0, without device work.  samples: (numsamples, N) spins; None draws them on the device from (seed, step)."""
    return _api.pauli_expectations(_api.STACK, _native_stack(wf), strings, numsamples, seed, step, samples)


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under the Hamiltonian `ham` from `numsamples` samples: {"mean", "var" (population variance of E_loc), "err"
    (sqrt(var / n)), "eloc" (numsamples,) when want_eloc}.  A batch that fits one pass stays resident: vmc_gradient then
    differentiates the VMC cost of this Hamiltonian."""
    return _api.energy(_api.STACK, _native_stack(wf), ham, numsamples, seed, step, samples, want_eloc)


def minimize_hamiltonian(wf, ham, params, numsteps=1000, numsamples=500, learningrate=5e-3, seed=111, scope="RNNwavefunction",
                         opt=None, comm=None, verbose=False, device_steps=None):
    """training.minimize_hamiltonian for stacked layers: minimise the energy of `wf` (holding `params`, scoped by `scope`) under `ham`
    (observables.Hamiltonian) with the host optimizer loop pauli_step_stack (samples, local energies of `ham`, moments; the batch
    stays resident) -> training.cost_gradient -> training.Adam -> set_params.  Returns (meanEnergy, varEnergy), one entry per
    iteration 0..numsteps; the trained parameters are left in minimize_hamiltonian.last_params.  The batch of numsamples must fit one
    pass of the state budget.  Single process only: a communicator is refused.
    device_steps=K (an integer >= 1): the same iterations run on the device in chunks of at most K with one host synchronisation
    each (NativeWavefunction.pauli_train_steps_stack) - the same energies, variances and parameters, bit for bit.  The device runs
    Adam from a fresh state: opt= is refused with it."""
    meanEnergy, varEnergy, minimize_hamiltonian.last_params = _api.minimize_family(
        _api.STACK, _native_stack, wf, ham, params, numsteps, numsamples, learningrate, seed, scope, opt, comm, verbose, device_steps)
    return meanEnergy, varEnergy


def correlations(wf, numsamples, pairs=None, seed=111, step=0, samples=None):
    """<sz_k>, <sx_k> of every site and, for the listed pairs of distinct sites, <sz_a sz_b>, <sx_a sx_b> and their connected parts,
    with standard errors, from one pauli_step_stack call (one X mask per site, one XX mask per pair):

        z, x (N,);  pairs (P, 2);  zz, xx, zz_c = zz - z_a z_b, xx_c = xx - x_a x_b (P,);  "<name>_err" for each.

    pairs: None = every pair (c, k), k != c, with the centre site c = N // 2.  A pair (k, k) raises ValueError.  Errors: the plain
    std / sqrt(n) (population variance) of the per-sample values s_k, r_k = exp(log r_k), s_a s_b, r_ab, which the call returns as
    log-ratios and samples; connected parts to first order (delta method), as observables_2d.correlations."""
    return _api.correlations(_api.STACK, _native_stack(wf), numsamples, pairs, seed, step, samples)
