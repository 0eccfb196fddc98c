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
    nat = _native(wf)
    if samples is not None:
        samples = np.asarray(samples).reshape(2 * int(numpairs), nat.N)
    out = nat.renyi2_regions(regions, int(numpairs), samples=samples, seed=seed, step=step)
    return renyi2_from_sums(out["sums"], numpairs)


def mutual_information2_from_log_ratios(lr_a, lr_b, lr_ab):
    """I2 = S2(A) + S2(B) - S2(A u B) and its standard error from the per-pair log r of A, B and A u B on the SAME n pairs ((n,)
    each).  With m the means of r: I2 = -log m_A - log m_B + log m_AB; the error by the delta method on the per-pair values
    g = -r_A / m_A - r_B / m_B + r_AB / m_AB:  err = std(g) / sqrt(n)  (population std; the three estimates share their pairs, so
    their errors do not add in quadrature)."""
    ra, rb, rab = (np.exp(np.asarray(v, dtype=np.float64)) for v in (lr_a, lr_b, lr_ab))
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
    nat = _native(wf)
    if samples is not None:
        samples = np.asarray(samples).reshape(2 * int(numpairs), nat.N)
    out = nat.renyi2_regions(np.stack([a, b, a | b]), int(numpairs), samples=samples, seed=seed, step=step, log_ratio=True)
    return mutual_information2_from_log_ratios(*out["log_ratio"])


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
