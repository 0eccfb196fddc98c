"""Pauli-string expectation values, energies of arbitrary real spin Hamiltonians and two-point functions for the 2D RNN (model
MDRNN2D on the zig-zag path; rnnwf_pauli_step_2d, docs/pauli_2d.md), training on such a Hamiltonian (minimize_hamiltonian: the host
loop, or rnnwf_pauli_train_steps_2d with device_steps=K, docs/pauli_train.md), and the second Renyi entropy of arbitrary lattice
regions (rnnwf_renyi2_regions_2d, docs/renyi_2d.md).

Sites are named by the LATTICE index k = site(Nx, Ny, nx, ny) = nx * Ny + ny, the C-order flattening of samples (ns, Nx, Ny): the
convention of tfim_hamiltonian for a (Nx, Ny) Jz and of rnnwf_tfim2d_eloc.  The library maps k to the position along the path.  The
estimator is observables.py's:  v(sigma) = prod_{i in S} s_i * exp(1/2 [log P(sigma ^ F) - log P(sigma)]),  E[v] = <psi|O|psi>.

Regions are masks over the same lattice index: r_A = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)) on pairs of
independent samples, exp(-S2(A)) = E[r_A] (observables.py's estimator).

observables.pauli_expectations / energy / correlations / renyi2_regions keep refusing the 2D RNN; these are its own entry points.  They accept the
TFIM2D_2DRNN.RNNwavefunction facade or a NativeWavefunction of model MDRNN2D and raise ValueError for every other model.
"""
import numpy as np

from . import _lib
from . import _observable_api as _api
from .observables import (Hamiltonian, _disjoint_masks, _native, group_by_mask, mutual_information2_from_log_ratios,  # noqa: F401
                          pauli_from_sums, pauli_terms, renyi2_from_sums, tfim_hamiltonian)

__all__ = ["site", "xxz_hamiltonian_2d", "tfim_hamiltonian", "Hamiltonian", "pauli_expectations", "energy", "minimize_hamiltonian", "correlations",
           "rectangle_region", "row_cut_regions", "column_cut_regions", "renyi2_regions", "renyi2_mutual_information"]


def site(Nx, Ny, nx, ny):
    """The lattice index of site (nx, ny) of a Nx x Ny lattice: nx * Ny + ny."""
    Nx, Ny = int(Nx), int(Ny)
    if int(nx) != nx or int(ny) != ny or not (0 <= nx < Nx and 0 <= ny < Ny):
        raise ValueError("site (%r, %r) is not on the %d x %d lattice" % (nx, ny, Nx, Ny))
    return int(nx) * Ny + int(ny)


def xxz_hamiltonian_2d(Nx, Ny, Jxy, Jz):
    """H = sum_bonds [Jxy (sx sx + sy sy) + Jz sz sz] in Pauli matrices on the Nx x Ny lattice with open boundaries, bonds
    (i, j)-(i+1, j) and (i, j)-(i, j+1).  Jxy < 0 is the ferromagnetic XY coupling, whose ground state is positive in the sz basis."""
    Nx, Ny = int(Nx), int(Ny)
    if Nx < 1 or Ny < 1 or Nx * Ny < 2:
        raise ValueError("xxz_hamiltonian_2d needs a lattice of at least two sites, got %d x %d" % (Nx, Ny))
    terms = []
    for i in range(Nx):
        for j in range(Ny):
            a = site(Nx, Ny, i, j)
            for b in ([site(Nx, Ny, i + 1, j)] if i + 1 < Nx else []) + ([site(Nx, Ny, i, j + 1)] if j + 1 < Ny else []):
                terms += [(Jxy, [("X", a), ("X", b)]), (Jxy, [("Y", a), ("Y", b)]), (Jz, [("Z", a), ("Z", b)])]
    return Hamiltonian(Nx * Ny, terms)


def _native_2d(wf):
    nat = _native(wf)
    if nat.model != _lib.MODEL_MDRNN2D:
        raise ValueError("observables_2d serves the 2D RNN (MDRNN2D) only; observables.py serves the GRU models")
    return nat


def pauli_expectations(wf, strings, numsamples, seed=111, step=0, samples=None):
    """<psi|P|psi> of every Pauli string P of `strings` (dense "XZIY..." over the lattice index, or sparse [("X", k), ...]) with its
    standard error, from `numsamples` samples: {"value": (K,), "err": (K,)}.  A string with an odd number of Y has expectation exactly
    0 in the real state psi = sqrt(P): 0 +- 0, without device work.  samples: (numsamples, Nx, Ny) or (numsamples, Nx * Ny) spins;
    None draws them on the device from (seed, step)."""
    return _api.pauli_expectations(_api.LATTICE, _native_2d(wf), strings, numsamples, seed, step, samples)


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under the Hamiltonian `ham` (sites = lattice indices) from `numsamples` samples: {"mean", "var" (population
    variance of E_loc), "err" (sqrt(var / n)), "eloc" (numsamples,) when want_eloc}.  A batch that fits one pass stays resident:
    vmc_gradient then differentiates the VMC cost of this Hamiltonian."""
    return _api.energy(_api.LATTICE, _native_2d(wf), ham, numsamples, seed, step, samples, want_eloc)


def minimize_hamiltonian(wf, ham, params, numsteps=1000, numsamples=500, learningrate=5e-3, seed=111, scope="RNNwavefunction",
                         opt=None, comm=None, verbose=False, device_steps=None):
    """training.minimize_hamiltonian for the 2D RNN: minimise the energy of `wf` (holding `params`, scoped by `scope`) under `ham`
    (observables.Hamiltonian over the Nx Ny lattice indices) with the host optimizer loop pauli_step_2d (samples, local energies of
    `ham`, moments; the batch stays resident) -> training.cost_gradient -> training.Adam -> set_params.  Returns (meanEnergy,
    varEnergy), one entry per iteration 0..numsteps; the trained parameters are left in minimize_hamiltonian.last_params.  The batch
    of numsamples must fit one pass of the state budget.  Single process only: a communicator is refused.
    device_steps=K (an integer >= 1): the same iterations run on the device in chunks of at most K with one host synchronisation
    each (NativeWavefunction.pauli_train_steps_2d, docs/pauli_train.md) - the same energies, variances and parameters, bit for bit.
    The device runs Adam from a fresh state: opt= is refused with it."""
    meanEnergy, varEnergy, minimize_hamiltonian.last_params = _api.minimize_family(
        _api.LATTICE, _native_2d, wf, ham, params, numsteps, numsamples, learningrate, seed, scope, opt, comm, verbose, device_steps)
    return meanEnergy, varEnergy


def correlations(wf, numsamples, pairs=None, seed=111, step=0, samples=None):
    """<sz_k>, <sx_k> of every lattice site and, for the listed pairs of distinct sites, <sz_a sz_b>, <sx_a sx_b> and their connected
    parts, with standard errors, from one pauli_step_2d call (one X mask per site, one XX mask per pair):

        z, x (N,);  pairs (P, 2) lattice indices;  zz, xx, zz_c = zz - z_a z_b, xx_c = xx - x_a x_b (P,);  "<name>_err" for each.

    pairs: None = every pair (c, k), k != c, with the lattice's centre site c = site(Nx, Ny, Nx // 2, Ny // 2).  There are no diagonal
    entries: sz^2 = sx^2 = 1, and a pair (k, k) raises ValueError.  Errors: the plain std / sqrt(n) (population variance) of the
    per-sample values s_k, r_k = exp(log r_k), s_a s_b, r_ab, which the call returns as log-ratios and samples - not the cross-moment
    formulas of observables.correlations_from_sums.  Connected parts to first order (delta method): the std / sqrt(n) of
    g = s_a s_b - z_b s_a - z_a s_b and of g = r_ab - x_b r_a - x_a r_b."""
    return _api.correlations(_api.LATTICE, _native_2d(wf), numsamples, pairs, seed, step, samples)


def rectangle_region(Nx, Ny, x0, x1, y0, y1):
    """(Nx Ny,) int32 mask over the lattice index of the sites x0 <= nx < x1, y0 <= ny < y1."""
    Nx, Ny, x0, x1, y0, y1 = (int(v) for v in (Nx, Ny, x0, x1, y0, y1))
    if Nx < 1 or Ny < 1 or not (0 <= x0 <= x1 <= Nx and 0 <= y0 <= y1 <= Ny):
        raise ValueError("rectangle_region needs 0 <= x0 <= x1 <= Nx and 0 <= y0 <= y1 <= Ny, got Nx=%d, Ny=%d, x %d..%d, y %d..%d"
                         % (Nx, Ny, x0, x1, y0, y1))
    m = np.zeros((Nx, Ny), dtype=np.int32)
    m[x0:x1, y0:y1] = 1
    return m.reshape(Nx * Ny)


def row_cut_regions(Nx, Ny):
    """(Ny - 1, Nx Ny) int32 masks of the cuts between rows: row c - 1 = the sites ny < c, c = 1..Ny-1.  The model visits the lattice
    row by row, so these are the prefixes of its path."""
    Nx, Ny = int(Nx), int(Ny)
    if Nx < 1 or Ny < 2:
        raise ValueError("row_cut_regions needs Nx >= 1 and Ny >= 2, got Nx=%d, Ny=%d" % (Nx, Ny))
    return np.stack([rectangle_region(Nx, Ny, 0, Nx, 0, c) for c in range(1, Ny)])


def column_cut_regions(Nx, Ny):
    """(Nx - 1, Nx Ny) int32 masks of the cuts between columns: row c - 1 = the sites nx < c, c = 1..Nx-1."""
    Nx, Ny = int(Nx), int(Ny)
    if Nx < 2 or Ny < 1:
        raise ValueError("column_cut_regions needs Nx >= 2 and Ny >= 1, got Nx=%d, Ny=%d" % (Nx, Ny))
    return np.stack([rectangle_region(Nx, Ny, 0, c, 0, Ny) for c in range(1, Nx)])


def renyi2_regions(wf, regions, numpairs, seed=111, step=0, samples=None):
    """Second Renyi entropy S2(A) (R,) and its standard error (R,) (observables.renyi2_from_sums) of the regions `regions`: (R, Nx Ny)
    masks of 0 / 1 over the lattice index, (R, Nx, Ny), or one mask of Nx Ny entries; 1 = site in A.  From `numpairs` pairs of
    independent samples; samples: (2 numpairs, Nx, Ny) or (2 numpairs, Nx Ny) spins, pair p = rows 2p and 2p + 1; None draws them on
    the device from (seed, step)."""
    return _api.renyi2_regions(_api.LATTICE, _native_2d(wf), regions, numpairs, seed, step, samples)


def renyi2_mutual_information(wf, region_a, region_b, numpairs, seed=111, step=0, samples=None):
    """Renyi-2 mutual information I2(A : B) = S2(A) + S2(B) - S2(A u B) of two DISJOINT regions (masks of Nx Ny entries over the
    lattice index, or (Nx, Ny)) and its standard error by the delta method (observables.mutual_information2_from_log_ratios), from
    `numpairs` pairs; A, B and A u B run in one call on the same pairs.  Overlapping regions raise ValueError before the wave function
    is touched."""
    a, b = _disjoint_masks(np.asarray(region_a).reshape(-1), np.asarray(region_b).reshape(-1))
    return _api.renyi2_mutual_information(_api.LATTICE, _native_2d(wf), a, b, numpairs, seed, step, samples)
