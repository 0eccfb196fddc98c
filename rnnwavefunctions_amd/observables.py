"""Observables beyond the energy: the second Renyi entropy S2(l) of the region A = the first l sites, every cut at once, by the
replica swap estimator (Hastings, Gonzalez, Kallin, Melko, PRL 104, 157201 (2010)) on the GPU (rnnwf_renyi2_swap).

For pairs (sigma, tau) drawn independently from |psi|^2,  exp(-S2(l)) = E[r_l],
    r_l = psi(tau_A sigma_B) psi(sigma_A tau_B) / (psi(sigma) psi(tau)).
Several devices: each draws its own pairs (pair_offset) and the (N + 1, 2) sums add up - all-reduce them with
NativeWavefunction.allreduce_f64, then call renyi2_from_sums with the global pair count.  docs/renyi.md has the details.

Arbitrary regions (rnnwf_renyi2_regions, docs/renyi_regions.md): renyi2_regions takes site masks - interval_region,
rectangle_region and column_cut_regions build the usual ones - and renyi2_mutual_information gives
I2(A : B) = S2(A) + S2(B) - S2(A u B) of two disjoint regions from one set of pairs.

Two-point correlation functions (rnnwf_correlations, docs/correlations.md): with psi = sqrt(P), s = 2 sigma - 1,
    <sz_i> = E[s_i], <sz_i sz_j> = E[s_i s_j], <sx_i> = E[r_i], <sx_i sx_j> = E[r_ij],
    r_i = psi(sigma with i flipped) / psi(sigma),  r_ij = psi(sigma with i and j flipped) / psi(sigma).
Several devices: each draws its own chains (sample_offset), the four sums add up - all-reduce each with
NativeWavefunction.allreduce_f64, then call correlations_from_sums with the global sample count.
"""
import warnings

import numpy as np

from . import _lib
from . import _observable_api as _api


def _native(wf):
    """The NativeWavefunction behind a reference-named facade (GRUWavefunction1D, GRUWavefunction2DRaster, their aliases)."""
    if isinstance(wf, _lib.NativeWavefunction):
        return wf
    nat = getattr(wf, "_native", None)
    if isinstance(nat, _lib.NativeWavefunction):
        return nat
    raise TypeError("observables need a wave-function facade or a NativeWavefunction, got %r" % (wf,))


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


def interval_region(N, a, b):
    """(N,) int32 mask of the sites a..b-1 of a chain of N sites (0 <= a <= b <= N)."""
    N, a, b = int(N), int(a), int(b)
    if N < 1 or not 0 <= a <= b <= N:
        raise ValueError("interval_region needs N >= 1 and 0 <= a <= b <= N, got N=%d, a=%d, b=%d" % (N, a, b))
    m = np.zeros(N, dtype=np.int32)
    m[a:b] = 1
    return m


def rectangle_region(Nx, Ny, x0, x1, y0, y1):
    """(Nx Ny,) int32 mask of the sites x0 <= nx < x1, y0 <= ny < y1 of the 2D raster model, site index ny * Nx + nx."""
    Nx, Ny, x0, x1, y0, y1 = (int(v) for v in (Nx, Ny, x0, x1, y0, y1))
    if Nx < 1 or Ny < 1 or not (0 <= x0 <= x1 <= Nx and 0 <= y0 <= y1 <= Ny):
        raise ValueError("rectangle_region needs 0 <= x0 <= x1 <= Nx and 0 <= y0 <= y1 <= Ny, got Nx=%d, Ny=%d, x %d..%d, y %d..%d"
                         % (Nx, Ny, x0, x1, y0, y1))
    m = np.zeros((Ny, Nx), dtype=np.int32)
    m[y0:y1, x0:x1] = 1
    return m.reshape(Nx * Ny)


def column_cut_regions(Nx, Ny):
    """(Nx - 1, Nx Ny) int32 masks of the vertical cuts of the 2D raster model: row c - 1 = the columns nx < c, c = 1..Nx-1."""
    Nx, Ny = int(Nx), int(Ny)
    if Nx < 2 or Ny < 1:
        raise ValueError("column_cut_regions needs Nx >= 2 and Ny >= 1, got Nx=%d, Ny=%d" % (Nx, Ny))
    return np.stack([rectangle_region(Nx, Ny, 0, c, 0, Ny) for c in range(1, Nx)])


def renyi2_regions(wf, regions, numpairs, seed=111, step=0, samples=None):
    """Second Renyi entropy S2(A) (R,) and its standard error (R,) of the regions `regions` ((R, N) masks of 0 / 1, or one mask;
    1 = site in A, sites in the model's order: raster ny * Nx + nx for the 2D raster model) from `numpairs` pairs of independent
    samples of `wf` (a facade or a NativeWavefunction).  samples: (2 numpairs, N) spins, pair p = rows 2p and 2p + 1; None draws
    them on the device from (seed, step).  Refused models (parity, complex RNN, 2D RNN, LSTM, stacked layers) raise ValueError
    with the library's reason."""
    return _api.renyi2_regions(_api.GRU, _native(wf), regions, numpairs, seed, step, samples)


def mutual_information2_from_log_ratios(lr_a, lr_b, lr_ab):
    """I2 = S2(A) + S2(B) - S2(A u B) and its standard error from the per-pair log r of A, B and A u B on the SAME n pairs ((n,)
    each).  With m the means of r: I2 = -log m_A - log m_B + log m_AB; the error by the delta method on the per-pair values
    g = -r_A / m_A - r_B / m_B + r_AB / m_AB:  err = std(g) / sqrt(n)  (population std; the three estimates share their pairs, so
    their errors do not add in quadrature)."""
    return mutual_information2_from_values(*(np.exp(np.asarray(v, dtype=np.float64)) for v in (lr_a, lr_b, lr_ab)))


def mutual_information2_from_values(r_a, r_b, r_ab):
    """The same from the per-pair values r themselves (observables_complex passes Re r of the complex estimator)."""
    ra, rb, rab = (np.asarray(v, dtype=np.float64) for v in (r_a, r_b, r_ab))
    if ra.ndim != 1 or ra.shape != rb.shape or ra.shape != rab.shape or ra.size < 1:
        raise ValueError("the three log-ratio arrays must be one-dimensional, of the same length >= 1")
    ma, mb, mab = ra.mean(), rb.mean(), rab.mean()
    g = -ra / ma - rb / mb + rab / mab
    return float(-np.log(ma) - np.log(mb) + np.log(mab)), float(g.std() / np.sqrt(g.size))


def _disjoint_masks(region_a, region_b):
    a, b = np.asarray(region_a), np.asarray(region_b)
    if a.ndim != 1 or a.shape != b.shape or not np.all((a == 0) | (a == 1)) or not np.all((b == 0) | (b == 1)):
        raise ValueError("region_a and region_b must be masks of 0 / 1 of the same length")
    a, b = a.astype(np.int32), b.astype(np.int32)
    if np.any(a & b):
        raise ValueError("region_a and region_b must be disjoint; both contain the sites %s" % np.flatnonzero(a & b).tolist())
    return a, b


def renyi2_mutual_information(wf, region_a, region_b, numpairs, seed=111, step=0, samples=None):
    """Renyi-2 mutual information I2(A : B) = S2(A) + S2(B) - S2(A u B) of two DISJOINT regions (masks of N entries) and its standard
    error (mutual_information2_from_log_ratios), from `numpairs` pairs; A, B and A u B run in one call on the same pairs.
    samples, seed, step and the refused models as renyi2_regions."""
    a, b = _disjoint_masks(region_a, region_b)
    return _api.renyi2_mutual_information(_api.GRU, _native(wf), a, b, numpairs, seed, step, samples)


def correlations_from_sums(z_sums, zz_sums, x_sums, xx_sums, numsamples):
    """Means and standard errors from the sums of rnnwf_correlations over numsamples chains.  Returns a dict of
        z (N,), zz (N, N), x (N,), xx (N, N) (symmetric; diagonals 1), zz_c = zz - z z^T, xx_c = xx - x x^T,
    and "<name>_err" for each.  Errors of the means: sqrt(var / n) with the population variance (s^2 = 1, so var s = 1 - z^2;
    var r = mean r^2 - (mean r)^2).  Errors of the connected functions, first order (delta method): zz_c ~ mean of
    g = s_i s_j - z_j s_i - z_i s_j and xx_c ~ mean of g = r_ij - x_j r_i - x_i r_j, whose variances follow from the cross moments
    xx_sums carries; on the diagonal 1 - z_i^2 and 1 - x_i^2 with errors 2 |z_i| err z_i, 2 |x_i| err x_i.  Entries whose sums
    are not finite (a chain with log r > 709) give nan, with a warning."""
    n = float(numsamples)
    z_sums, zz_sums = np.asarray(z_sums, dtype=np.float64), np.asarray(zz_sums, dtype=np.float64)
    x_sums, xx_sums = np.asarray(x_sums, dtype=np.float64), np.asarray(xx_sums, dtype=np.float64)
    N = z_sums.shape[0] if z_sums.ndim == 1 else -1
    if N < 1 or zz_sums.shape != (N, N) or x_sums.shape != (N, 2) or xx_sums.shape != (N, N, 5) or n < 1:
        raise ValueError("sums must have shapes (N,), (N, N), (N, 2), (N, N, 5) and numsamples be >= 1")
    bad_x = ~np.all(np.isfinite(x_sums), axis=1)
    bad_xx = ~np.all(np.isfinite(xx_sums), axis=2)
    if bad_x.any() or bad_xx.any():
        warnings.warn("correlations: the sums of sites %s and of %d pairs are not finite (a chain with log r > 709); x, xx are nan there"
                      % (np.flatnonzero(bad_x).tolist(), int(np.triu(bad_xx, 1).sum())), RuntimeWarning, stacklevel=2)
    x_sums = np.where(bad_x[:, None], np.nan, x_sums)
    xx_sums = np.where(bad_xx[:, :, None], np.nan, xx_sums)
    iu = np.triu_indices(N, 1)
    eye = np.eye(N, dtype=bool)

    def sym(upper, diag):
        out = np.zeros((N, N))
        out[iu] = upper[iu]
        out = out + out.T
        out[eye] = diag
        return out

    def root(v):
        return np.sqrt(np.maximum(v, 0.0) / n)

    z = z_sums / n
    zz = zz_sums / n
    x, x2 = x_sums[:, 0] / n, x_sums[:, 1] / n
    m = xx_sums / n                                        # [r_ij, r_ij^2, r_ij r_i, r_ij r_j, r_i r_j], upper triangle
    xx = sym(m[:, :, 0], 1.0)
    out = {"z": z, "z_err": root(1.0 - z * z), "zz": zz, "zz_err": root(1.0 - zz * zz), "x": x, "x_err": root(x2 - x * x),
           "xx": xx, "xx_err": sym(root(m[:, :, 1] - m[:, :, 0] ** 2), 0.0)}
    zi, zj = z[:, None], z[None, :]
    out["zz_c"] = zz - zi * zj
    # E[g] = zz - 2 z_i z_j,  E[g^2] = 1 - z_i^2 - z_j^2 + 2 z_i z_j zz   (s^2 = 1, s_i s_j s_i = s_j)
    zz_c_err = root(1.0 - zi * zi - zj * zj + 2.0 * zi * zj * zz - (zz - 2.0 * zi * zj) ** 2)
    zz_c_err[eye] = 2.0 * np.abs(z) * out["z_err"]
    out["zz_c_err"] = zz_c_err
    xi, xj = x[:, None], x[None, :]
    out["xx_c"] = xx - xi * xj
    g1 = m[:, :, 0] - 2.0 * xi * xj
    g2 = (m[:, :, 1] + xj * xj * x2[:, None] + xi * xi * x2[None, :] - 2.0 * xj * m[:, :, 2] - 2.0 * xi * m[:, :, 3]
          + 2.0 * xi * xj * m[:, :, 4])
    out["xx_c_err"] = sym(root(g2 - g1 * g1), 2.0 * np.abs(x) * out["x_err"])
    return out


def correlations(wf, numsamples, seed=111, step=0, samples=None):
    """<sz_i>, <sz_i sz_j>, <sx_i>, <sx_i sx_j> and the connected two-point functions of `wf` (a facade such as
    TFIM1D.RNNwavefunction / TFIM2D_1DRNN.RNNwavefunction, or a NativeWavefunction) from `numsamples` samples, with standard errors:
    the dict of correlations_from_sums.  Sites in the model's order (raster order ny * Nx + nx for the 2D raster model).  samples:
    (numsamples, N) spins; None draws them on the device from (seed, step).  Refused models (parity, complex RNN, 2D RNN, LSTM,
    stacked layers) raise ValueError with the library's reason."""
    nat = _native(wf)
    if samples is not None:
        samples = np.asarray(samples).reshape(int(numsamples), nat.N)
    out = nat.correlations(int(numsamples), samples=samples, seed=seed, step=step)
    return correlations_from_sums(out["z_sums"], out["zz_sums"], out["x_sums"], out["xx_sums"], numsamples)


# ---- Pauli strings and arbitrary spin Hamiltonians (rnnwf_pauli_step, docs/pauli.md) ---------------------------------------
# A string is a product of Pauli matrices, one letter per site: dense "XZIY..." of length N, or sparse [("X", i), ("Z", j), ...].
# On a site X flips the spin, Z reads its sign s = 2 sigma - 1 and Y = -i Z X does both, so a string is
#     factor * (prod_{i in S} sz_i)(prod_{i in F} sx_i),   F = sites with X or Y,  S = sites with Z or Y,  factor = (-i)^n_Y
# (sz to the left on every site; operators of different sites commute).  For even n_Y the factor is real, (-1)^(n_Y / 2); for odd
# n_Y the string has imaginary matrix elements in the sz basis and expectation exactly 0 in a real state psi = sqrt(P).
_LETTERS = "IXYZ"


def _string_sites(string, N):
    """{site: letter} of one string, letters I dropped."""
    if isinstance(string, str):
        if len(string) != N:
            raise ValueError("a dense Pauli string needs one letter per site: %d letters for N = %d in %r" % (len(string), N, string))
        items = list(zip(string, range(N)))
    else:
        items = [(p, i) for p, i in string]
    out = {}
    for letter, site in items:
        if not isinstance(letter, str) or len(letter) != 1 or letter.upper() not in _LETTERS:
            raise ValueError("Pauli letter %r is not one of I, X, Y, Z" % (letter,))
        if int(site) != site or not 0 <= int(site) < N:
            raise ValueError("site %r out of range for N = %d" % (site, N))
        site = int(site)
        if site in out:
            raise ValueError("site %d appears twice in the Pauli string %r" % (site, string))
        if letter.upper() != "I":
            out[site] = letter.upper()
    return out


def pauli_terms(strings, N):
    """flip (K, N) int32, sign (K, N) int32 and factor (K,) complex of K Pauli strings on N sites: string k =
    factor[k] * (prod_{sign[k]} sz)(prod_{flip[k]} sx), factor = (-i)^n_Y (real for even n_Y)."""
    N = int(N)
    if N < 1:
        raise ValueError("N must be >= 1")
    strings = list(strings)
    flip = np.zeros((len(strings), N), dtype=np.int32)
    sign = np.zeros((len(strings), N), dtype=np.int32)
    factor = np.ones(len(strings), dtype=np.complex128)
    for k, st in enumerate(strings):
        ny = 0
        for site, letter in _string_sites(st, N).items():
            flip[k, site] = letter in "XY"
            sign[k, site] = letter in "ZY"
            ny += letter == "Y"
        factor[k] = (1.0, -1j, -1.0, 1j)[ny % 4]
    return flip, sign, factor


def group_by_mask(flip):
    """The distinct non-empty rows of flip (K, N) in order of first appearance and, per term, its row (-1: diagonal term): how
    rnnwf_pauli_step shares one evaluation of sigma ^ F between the terms with the same flip mask."""
    flip = np.asarray(flip)
    seen, masks, index = {}, [], []
    for row in flip:
        key = tuple(int(v) for v in row)
        if not any(key):
            index.append(-1)
            continue
        if key not in seen:
            seen[key] = len(masks)
            masks.append(key)
        index.append(seen[key])
    return np.array(masks, dtype=np.int32).reshape(len(masks), flip.shape[1]), np.array(index, dtype=np.int32)


class Hamiltonian:
    """H = sum_k c_k P_k, real coefficients c_k and Pauli strings P_k (dense or sparse, see pauli_terms) with an even number of Y:
    a real-symmetric matrix in the sz basis.  .flip, .sign (K, N) and .coeff (K,) are rnnwf_pauli_step's arguments (coeff carries
    the strings' factors (-1)^(n_Y / 2))."""

    def __init__(self, N, terms):
        self.N = int(N)
        terms = list(terms)
        if not terms:
            raise ValueError("a Hamiltonian needs at least one term")
        coeffs = []
        for c, _ in terms:
            if isinstance(c, complex) and c.imag != 0.0:
                raise ValueError("coefficients must be real, got %r" % (c,))
            coeffs.append(float(np.real(c)))
        self.terms = [(c, st) for c, (_, st) in zip(coeffs, terms)]
        self.flip, self.sign, factor = pauli_terms([st for _, st in terms], self.N)
        odd = np.flatnonzero(factor.imag != 0.0)
        if odd.size:
            raise ValueError("term %d (%r) has an odd number of Y: imaginary matrix elements in the σᶻ basis"
                             % (int(odd[0]), terms[int(odd[0])][1]))
        self.coeff = np.asarray(coeffs, dtype=np.float64) * factor.real

    def __len__(self):
        return len(self.terms)


def tfim_hamiltonian(Jz, Bx):
    """The transverse-field Ising model with open boundaries in the reference's conventions, H = -sum_bonds Jz sz sz - Bx sum sx.
    Jz of shape (N,): the chain, bond (i, i+1) weighted Jz[i] (Jz[N-1] unused).  Jz of shape (Nx, Ny): the lattice of the 2D raster
    model, site (i, j) at i * Ny + j, bonds (i, j)-(i+1, j) and (i, j)-(i, j+1) both weighted Jz[i, j]: E_loc of rnnwf_tfim_eloc /
    rnnwf_tfim2d_eloc."""
    Jz = np.asarray(Jz, dtype=np.float64)
    if Jz.ndim == 1:
        Jz = Jz[None, :]
    if Jz.ndim != 2 or Jz.size < 1:
        raise ValueError("Jz must have shape (N,) or (Nx, Ny)")
    Nx, Ny = Jz.shape
    terms = []
    for i in range(Nx):
        for j in range(Ny):
            k = i * Ny + j
            if i + 1 < Nx:
                terms.append((-Jz[i, j], [("Z", k), ("Z", k + Ny)]))
            if j + 1 < Ny:
                terms.append((-Jz[i, j], [("Z", k), ("Z", k + 1)]))
    terms += [(-float(Bx), [("X", k)]) for k in range(Nx * Ny)]
    return Hamiltonian(Nx * Ny, terms)


def xxz_hamiltonian(N, Jxy, Jz, periodic=False):
    """H = sum_i [Jxy (sx_i sx_{i+1} + sy_i sy_{i+1}) + Jz sz_i sz_{i+1}] in Pauli matrices on a chain of N sites, open or periodic
    (N >= 3).  Jxy < 0 is the ferromagnetic XY coupling, whose ground state is positive in the sz basis."""
    N = int(N)
    if N < 2 or (periodic and N < 3):
        raise ValueError("xxz_hamiltonian needs N >= 2 (N >= 3 with periodic boundaries)")
    terms = []
    for i in range(N if periodic else N - 1):
        j = (i + 1) % N
        terms += [(Jxy, [("X", i), ("X", j)]), (Jxy, [("Y", i), ("Y", j)]), (Jz, [("Z", i), ("Z", j)])]
    return Hamiltonian(N, terms)


def pauli_from_sums(term_sums, numsamples):
    """Mean and standard error (std / sqrt(n), population variance) per term from rnnwf_pauli_step's (K, 2) sums of v and v^2."""
    sums = np.asarray(term_sums, dtype=np.float64)
    n = float(numsamples)
    mean = sums[:, 0] / n
    return mean, np.sqrt(np.maximum(sums[:, 1] / n - mean * mean, 0.0) / n)


def pauli_expectations(wf, strings, numsamples, seed=111, step=0, samples=None):
    """<psi|P|psi> of every Pauli string P of `strings` (dense "XZIY..." or sparse [("X", i), ...]) with its standard error, from
    `numsamples` samples of `wf` (a facade or a NativeWavefunction): {"value": (K,), "err": (K,)}.  Sites in the model's order.  A
    string with an odd number of Y has expectation exactly 0 in the real state psi = sqrt(P): 0 +- 0, without device work.  samples:
    (numsamples, N) spins; None draws them on the device from (seed, step).  Refused models (parity, complex RNN, 2D RNN, LSTM,
    stacked layers) raise ValueError with the library's reason."""
    return _api.pauli_expectations(_api.GRU, _native(wf), strings, numsamples, seed, step, samples)


def energy(wf, ham, numsamples, seed=111, step=0, samples=None, want_eloc=False):
    """Energy of `wf` under the Hamiltonian `ham` from `numsamples` samples: {"mean", "var" (population variance of E_loc), "err"
    (sqrt(var / n)), "eloc" (numsamples,) when want_eloc}.  samples, seed, step and the refused models as pauli_expectations."""
    return _api.energy(_api.GRU, _native(wf), ham, numsamples, seed, step, samples, want_eloc)
