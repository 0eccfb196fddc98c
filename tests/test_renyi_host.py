"""Host-side tests of the second Renyi entropy (rnnwf_renyi2_swap, rnnwavefunctions_amd.observables): the C ABI declares and
exports it, the exact reference S2 of the GPU tests (SVD of psi across the cut) is right on states with known entanglement,
the swap estimator as the GPU tests restate it reproduces Tr rho_A^2 exactly, and the statistics of renyi2_from_sums."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT, all_configs
from oracle import models as M
from rnnwavefunctions_amd import params as P


def exact_renyi2(psi, N):
    """S2(l), l = 0..N, of the normalised state psi over all_configs(N) (site 0 most significant): -log sum_i s_i^4, s the
    singular values of psi reshaped to (2^l, 2^(N-l))."""
    psi = np.asarray(psi, dtype=np.float64)
    psi = psi / np.linalg.norm(psi)
    out = np.zeros(N + 1)
    for l in range(N + 1):
        s = np.linalg.svd(psi.reshape(2 ** l, 2 ** (N - l)), compute_uv=False)
        out[l] = -np.log(np.sum(s ** 4))
    return out


def swap_log_ratio(log_p, sigma, tau, l):
    """log r_l = 1/2 [log P(tau_A sigma_B) + log P(sigma_A tau_B) - log P(sigma) - log P(tau)], A = the first l sites."""
    a = np.concatenate([tau[:, :l], sigma[:, l:]], axis=1)
    b = np.concatenate([sigma[:, :l], tau[:, l:]], axis=1)
    return 0.5 * (log_p(a) + log_p(b) - log_p(sigma) - log_p(tau))


def test_header_prototypes_and_library_declare_renyi2_swap():
    header = open(os.path.join(ROOT, "include", "rnnwf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+rnnwf_renyi2_swap\s*\(\s*rnnwf_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*samples\s*,\s*int64_t\s+npairs"
                     r"\s*,\s*uint64_t\s+seed\s*,\s*uint64_t\s+step\s*,\s*int64_t\s+pair_offset\s*,\s*double\s*\*\s*sums\s*,\s*double\s*\*"
                     r"\s*out_log_ratio\s*,\s*int32_t\s*\*\s*out_samples\s*\)\s*;", code)
    assert "#define RNNWF_ABI_VERSION 1" in header
    from rnnwavefunctions_amd import _lib, build
    assert "rnnwf_renyi2_swap" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["rnnwf_renyi2_swap"]
    assert len(args) == 9
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "rnnwf_renyi2_swap")


def test_exact_helper_product_state_has_no_entanglement():
    N = 5
    one = np.array([0.6, 0.8])
    psi = one
    for _ in range(N - 1):
        psi = np.kron(psi, one)
    assert np.abs(exact_renyi2(psi, N)).max() < 1e-13


@pytest.mark.parametrize("k", [1, 2, 3])
def test_exact_helper_counts_bell_pairs_across_the_cut(k):
    # sites (i, 2k-1-i) form Bell pairs: every pair straddles the middle cut l = k
    N = 2 * k
    c = all_configs(N)
    psi = np.ones(2 ** N)
    for i in range(k):
        psi *= (c[:, i] == c[:, N - 1 - i])
    S = exact_renyi2(psi, N)
    assert abs(S[k] - k * np.log(2)) < 1e-12
    for l in range(N + 1):                                        # cut l splits min(l, N - l) of the pairs
        assert abs(S[l] - min(l, N - l) * np.log(2)) < 1e-12


def test_exact_helper_ghz_state_has_log2_at_every_interior_cut():
    N = 6
    psi = np.zeros(2 ** N)
    psi[0] = psi[-1] = 1.0
    S = exact_renyi2(psi, N)
    assert abs(S[0]) < 1e-14 and abs(S[N]) < 1e-14
    assert np.abs(S[1:N] - np.log(2)).max() < 1e-12


@pytest.mark.parametrize("H,scale", [(6, 3.0), (20, 2.5)])
def test_swap_estimator_restated_with_the_oracle_gives_the_exact_purity(H, scale):
    # sum_{sigma, tau} P(sigma) P(tau) r_l(sigma, tau) = Tr rho_A^2, with P the oracle's GRU log P in float64
    N = 4
    prm = P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=H, dtype=np.float64), scale), H + 1)
    log_p = lambda x: M.prnn_log_probability(prm, x, dtype=np.float64)
    c = all_configs(N)
    lp = log_p(c)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    sigma, tau = c[i.ravel()], c[j.ravel()]
    w = np.exp(lp[i.ravel()] + lp[j.ravel()])
    exact = exact_renyi2(np.exp(0.5 * lp), N)
    for l in range(N + 1):
        purity = np.sum(w * np.exp(swap_log_ratio(log_p, sigma, tau, l)))
        assert abs(purity - np.exp(-exact[l])) <= 1e-12, (l, purity, np.exp(-exact[l]))
    assert exact[1:N].max() > 0.05                                # entangled: the identity is not trivially 1 = 1


def test_renyi2_from_sums_on_hand_made_sums():
    from rnnwavefunctions_amd.observables import renyi2_from_sums
    r = np.array([[1.0, 1.0, 1.0, 1.0], [0.5, 0.25, 0.75, 0.5], [2.0, 0.0, 1.0, 1.0]])     # per cut, 4 pairs
    sums = np.stack([r.sum(axis=1), (r * r).sum(axis=1)], axis=1)
    S2, err = renyi2_from_sums(sums, 4)
    mean = r.mean(axis=1)
    assert np.allclose(S2, -np.log(mean), rtol=0, atol=1e-15)
    assert np.allclose(err, r.std(axis=1) / (2.0 * mean), rtol=1e-14, atol=1e-16)
    assert S2[0] == 0.0 and err[0] == 0.0
    # shards add: the sums of two halves give the same statistics
    a = np.stack([r[:, :2].sum(axis=1), (r[:, :2] ** 2).sum(axis=1)], axis=1)
    b = np.stack([r[:, 2:].sum(axis=1), (r[:, 2:] ** 2).sum(axis=1)], axis=1)
    S2b, errb = renyi2_from_sums(a + b, 4)
    assert np.allclose(S2b, S2, atol=1e-15) and np.allclose(errb, err, atol=1e-15)


def test_renyi2_from_sums_warns_and_gives_nan_on_overflow():
    from rnnwavefunctions_amd.observables import renyi2_from_sums
    sums = np.array([[3.0, 3.0], [np.inf, np.inf], [1.5, 0.9]])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        S2, err = renyi2_from_sums(sums, 3)
    assert any("not finite" in str(x.message) for x in w)
    assert np.isnan(S2[1]) and np.isnan(err[1])
    assert np.isfinite(S2[[0, 2]]).all() and S2[0] == 0.0
    with pytest.raises(ValueError):
        renyi2_from_sums(np.zeros((3, 3)), 3)
