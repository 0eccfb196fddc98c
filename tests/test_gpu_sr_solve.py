"""GPU tests of the device solve of stochastic reconfiguration (docs/sr.md, "Solve on the device"): rnnwf_sr_solve /
rnnwf_sr_direction, the blocked float64 Cholesky of sr_solve_kernels.h.

Set-up: N = 12, 10 units, random spin batches and random E_loc through load_batch (a few hundred random configurations of twelve
spins are almost all distinct: the Gram matrix has high rank).  The matrix under test is the device's own sr_gram() output, A =
gram + ns lambda I; the reference solution is sr.solve_shifted on it (LAPACK float64).

Bounds (the project's factor 16; none fitted to the output), with kappa^ = |A|_inf / (ns lambda) >= cond(A), since
lambda_min(A) >= ns lambda:
  residual           |A y - eps|_inf <= 16 ns 2^-53 |A|_inf |y|_inf, formed in float64 on the host (the backward error of a Cholesky solve)
  against LAPACK     |y - y_ref| / |y_ref| <= 16 ns 2^-53 kappa^
  direction          |delta_dev - delta_host| / |delta_host| <= 16 ns 2^-53 kappa^, delta_host = minsr_direction(wf, lambda, "host")
  direction against float64 autograd (N = 6, ns = 37, units 10 / 36, both types): the bound expression of
                     test_gpu_sr.py::test_minsr_direction.
Shapes, NB = _lib.SR_BLOCK the kernels' block width: ns = 1, 2, NB - 1, NB, NB + 1, 2 NB, 2 NB + 1, 3 NB + 5 (the first trailing
update with a block that is not next to the diagonal, and a ragged last panel), 5 NB + 3, float64 model; NB + 1 and 3 NB + 5 on the
float32 model; lambda = 1e-3, and 1e-8 at 3 NB + 5 (ill-conditioned).  test_strided_update: the smallest ns whose first trailing
update has more blocks than workgroups can be resident.

Measured on an MI355X, error / bound (docs/sr.md has the table): residual 4.2e-5 .. 3.3e-4, against LAPACK 4.1e-5 .. 1.4e-4, direction
against the host solver at most 1.2e-4 (ns = 2: 0.16, 0.16 and 0 - the bound is a few units of round-off there); lambda = 1e-8: at most
4.9e-5; ns = 2017: 2.7e-6 / 2.3e-6 / 4.8e-6; direction against autograd 0.016 .. 0.066.  The module's 63 tests take 3.5 s.
"""
import functools

import numpy as np
import pytest
import torch

import autograd_reference as A
import ed
import sr_reference as R
from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

pytestmark = pytest.mark.gpu
SCOPE = A.SCOPE
NB = _lib.SR_BLOCK
EPS64 = 2.0 ** -53
FACTOR = 16
N, UNITS = 12, 10
LAMBDA, LAMBDA_ILL = 1e-3, 1e-8

SIZES = (1, 2, NB - 1, NB, NB + 1, 2 * NB, 2 * NB + 1, 3 * NB + 5, 5 * NB + 3)
CASES = [(ns, True, LAMBDA) for ns in SIZES] + [(ns, False, LAMBDA) for ns in (NB + 1, 3 * NB + 5)]
CASES += [(3 * NB + 5, f64, LAMBDA_ILL) for f64 in (True, False)]
IDS = ["ns%d-%s-lam%g" % (ns, "f64" if f else "f32", lam) for ns, f, lam in CASES]


def make_wf(n, units, f64, layers=1):
    return _lib.NativeWavefunction(_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D, n, 1, (units,) * layers)


def make_params(units, f64, seed):
    prm = P.init_gru_params([units], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0), seed + 1)


def batch(n, ns, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 2, size=(ns, n)).astype(np.int32), rng.standard_normal(ns) * 2.0 - 3.0


@functools.lru_cache(maxsize=None)
def case(ns, f64, lam):
    """one device run per case, shared by the parametrized tests"""
    s, e = batch(N, ns, 1000 * UNITS + ns + N)
    wf = make_wf(N, UNITS, f64)
    wf.set_params(make_params(UNITS, f64, seed=7 + UNITS), scope=SCOPE)
    wf.load_batch(s, e)
    c = dict(ns=ns, lam=lam)
    c["gram"], c["eps"] = wf.sr_gram()
    c["y"] = wf.sr_solve(lam)
    c["delta"] = wf.sr_direction(lam)
    c["gram_after"] = wf.sr_gram()[0]                              # the factorisation must not have written the Gram matrix
    c["delta_host"] = sr.minsr_direction(wf, lam, solver="host")
    c["again"] = (wf.sr_solve(lam), wf.sr_direction(lam), sr.minsr_direction(wf, lam, solver="device"))
    wf.load_batch(s, e)
    c["reload"] = (wf.sr_solve(lam), wf.sr_direction(lam))
    wf.close()
    c["A"] = c["gram"] + ns * lam * np.eye(ns)
    c["y_ref"] = sr.solve_shifted(c["gram"], c["eps"], lam)
    c["kappa"] = np.abs(c["A"]).sum(axis=1).max() / (ns * lam)
    return c


def check_solution(label, Amat, eps, y, y_ref, ns, kappa):
    """the residual and the LAPACK comparison; prints error / bound of both"""
    assert y.shape == (ns,) and np.all(np.isfinite(y))
    norm_a = np.abs(Amat).sum(axis=1).max()
    res, res_bound = np.abs(Amat @ y - eps).max(), FACTOR * ns * EPS64 * norm_a * np.abs(y).max()
    err, bound = np.linalg.norm(y - y_ref), FACTOR * ns * EPS64 * kappa * np.linalg.norm(y_ref)
    print("%s: residual %.3e, bound %.3e, ratio %.3e | |y - y_ref| / |y_ref| %.3e, bound %.3e, ratio %.3e (kappa^ %.3e)"
          % (label, res, res_bound, res / res_bound if res_bound else 0.0, err / max(np.linalg.norm(y_ref), 1e-300),
             FACTOR * ns * EPS64 * kappa, err / bound if bound else 0.0, kappa))
    assert res <= res_bound
    assert err <= bound


@pytest.mark.parametrize("ns,f64,lam", CASES, ids=IDS)
def test_solution_residual_and_lapack(ns, f64, lam):
    c = case(ns, f64, lam)
    check_solution("solve", c["A"], c["eps"], c["y"], c["y_ref"], ns, c["kappa"])


@pytest.mark.parametrize("ns,f64,lam", CASES, ids=IDS)
def test_direction_matches_the_host_solver(ns, f64, lam):
    c = case(ns, f64, lam)
    err, ref = np.linalg.norm(c["delta"] - c["delta_host"]), np.linalg.norm(c["delta_host"])
    bound = FACTOR * ns * EPS64 * c["kappa"]
    print("direction: |d_dev - d_host| / |d_host| %.3e, bound %.3e, ratio %.3e" % (err / max(ref, 1e-300), bound, err / (bound * ref) if ref else 0.0))
    assert c["delta"].shape == c["delta_host"].shape and np.all(np.isfinite(c["delta"]))
    assert err <= bound * ref


@pytest.mark.parametrize("ns,f64,lam", CASES, ids=IDS)
def test_same_batch_same_bits(ns, f64, lam):
    c = case(ns, f64, lam)
    assert np.array_equal(c["again"][0], c["y"]) and np.array_equal(c["again"][1], c["delta"]) and np.array_equal(c["again"][2], c["delta"])
    assert np.array_equal(c["reload"][0], c["y"]) and np.array_equal(c["reload"][1], c["delta"])


@pytest.mark.parametrize("ns,f64,lam", CASES, ids=IDS)
def test_gram_matrix_survives_the_factorisation(ns, f64, lam):
    c = case(ns, f64, lam)
    assert np.array_equal(c["gram_after"], c["gram"])


@pytest.mark.parametrize("units,f64", [(10, False), (10, True), (36, False), (36, True)], ids=["u10-f32", "u10-f64", "u36-f32", "u36-f64"])
def test_direction_against_autograd(units, f64):
    """sr_direction against the float64 autograd Jacobian, with the bound of test_gpu_sr.py::test_minsr_direction: 16 x (the float32 /
    float64 reference spread, x 2^-29 for the float64 model, + the reference's own solve error, LU against eigen-decomposition)"""
    n, ns = 6, 37
    prm = make_params(units, f64, seed=7 + units)
    s, e = batch(n, ns, 1000 * units + ns + n)
    wf = make_wf(n, units, f64)
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    delta = wf.sr_direction(LAMBDA)
    wf.close()
    o64 = R.jacobian(prm, s, torch.float64)
    ref = R.minsr_direction(o64, e, LAMBDA)
    spread = np.linalg.norm(R.minsr_direction(R.jacobian(prm, s, torch.float32), e, LAMBDA) - ref) / np.linalg.norm(ref)
    w, v = np.linalg.eigh(R.gram(o64))
    own = np.linalg.norm(R.centred(o64).T @ (v @ ((v.T @ R.epsilon(e)) / (w + ns * LAMBDA))) - ref) / np.linalg.norm(ref)
    bound = A.FACTOR * (spread * (A.F64_OVER_F32 if f64 else 1.0) + own)
    err = np.linalg.norm(delta - ref) / np.linalg.norm(ref)
    print("direction: |d| / |ref| %.3e, float32 / float64 reference spread %.3e, the reference's own solve error %.3e, bound %.3e, ratio %.3e"
          % (err, spread, own, bound, err / bound))
    assert err <= bound


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_exact_zeros(f64):
    """ns = 1: eps = 0 and the centred Jacobian is zero, so y and delta are exact zeros.  Constant E_loc (not a dyadic number, so its
    sum rounds): eps is formed as (e - e_0) - mean (e - e_0), exactly zero, and so is everything solved from it."""
    wf = make_wf(N, UNITS, f64)
    wf.set_params(make_params(UNITS, f64, seed=7 + UNITS), scope=SCOPE)
    s, e = batch(N, 1, 5)
    wf.load_batch(s, e)
    y, delta = wf.sr_solve(LAMBDA), wf.sr_direction(LAMBDA)
    assert y.shape == (1,) and np.array_equal(y, [0.0])
    assert delta.shape == (wf.num_params(),) and np.array_equal(delta, np.zeros(wf.num_params()))
    for ns in (2, NB + 1, 3 * NB + 5):
        s, _ = batch(N, ns, 6 + ns)
        wf.load_batch(s, np.full(ns, -2.7))
        y, delta = wf.sr_solve(LAMBDA), wf.sr_direction(LAMBDA)
        assert np.array_equal(y, np.zeros(ns)) and np.array_equal(delta, np.zeros(wf.num_params()))
    wf.close()


def test_strided_update():
    """Second trip of the grid-stride loops.  sr_chol_update_kernel has 256 threads (four waves, one per SIMD) and a SIMD holds at most
    eight waves, so at most 8 workgroups are resident per CU and the launch helper's grid is at most 8 x CU count.  The first trailing
    update of nb block rows has m (m + 1) / 2 + m blocks, m = nb - 1 (the lower triangle behind panel 0 and the eps row): ns is the
    smallest with more blocks than that grid, one row into its last block.  (The loops of sr_chol_panel_kernel and
    sr_chol_back_kernel have at most 128 items at ns <= 4096, fewer than any grid: they never take a second trip.)  Residual and
    LAPACK bounds as for the small cases; no eigen-decomposition at this size."""
    wf = make_wf(N, UNITS, True)
    grid = 8 * wf.device_info()["cu_count"]
    m = 1
    while m * (m + 1) // 2 + m <= grid:
        m += 1
    ns = NB * m + 1                                               # nb = m + 1 block rows
    assert ns <= 4096 and m * (m + 1) // 2 + m > grid and (m - 1) * m // 2 + (m - 1) <= grid
    s, e = batch(N, ns, 77)
    wf.set_params(make_params(UNITS, True, seed=7 + UNITS), scope=SCOPE)
    wf.load_batch(s, e)
    gram, eps = wf.sr_gram()
    y = wf.sr_solve(LAMBDA)
    delta = wf.sr_direction(LAMBDA)
    y_ref = sr.solve_shifted(gram, eps, LAMBDA)
    delta_host = wf.sr_apply(y_ref)
    wf.close()
    Amat = gram + ns * LAMBDA * np.eye(ns)
    kappa = np.abs(Amat).sum(axis=1).max() / (ns * LAMBDA)
    print("strided: ns %d, %d blocks in the first trailing update, grid at most %d" % (ns, m * (m + 1) // 2 + m, grid))
    check_solution("strided solve", Amat, eps, y, y_ref, ns, kappa)
    err, ref = np.linalg.norm(delta - delta_host), np.linalg.norm(delta_host)
    print("strided direction: |d_dev - d_host| / |d_host| %.3e, bound %.3e" % (err / ref, FACTOR * ns * EPS64 * kappa))
    assert err <= FACTOR * ns * EPS64 * kappa * ref


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_diag_shift_is_validated():
    wf = make_wf(N, UNITS, False)
    wf.init_params(5)
    wf.vmc_step(48, 3, 0, np.append(np.ones(N), 1.0))
    for bad in (0.0, -1e-3, np.inf, np.nan):
        for call in (wf.sr_solve, wf.sr_direction):
            with pytest.raises(ValueError, match="diag_shift"):
                call(bad)
        with pytest.raises(ValueError, match="diag_shift"):
            sr.minsr_direction(wf, bad, solver="device")
    assert wf.resident_samples() == 48 and np.all(np.isfinite(wf.sr_direction(LAMBDA)))
    wf.close()


def test_workspace_counts_the_factor(monkeypatch):
    """400 samples, 10 units, float32: J = 400 x 3096 x 4 B = 4 953 600 B, one 400 x 400 float64 matrix 1 280 000 B.  7 MiB = 7 340 032 B
    admits J + one matrix (6 233 600 B), not two (7 513 600 B)."""
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "7")
    wf = make_wf(6, UNITS, False)
    wf.init_params(5)
    wf.vmc_step(400, 3, 0, np.append(np.ones(6), 1.0))
    assert wf.sr_gram()[0].shape == (400, 400)
    for call in (wf.sr_direction, wf.sr_solve):
        with pytest.raises(_lib.RnnwfError, match="ns too large for the SR workspace"):
            call(LAMBDA)
    assert wf.resident_samples() == 400
    assert wf.sr_gram()[0].shape == (400, 400)
    wf.vmc_step(48, 3, 1, np.append(np.ones(6), 1.0))
    assert wf.sr_direction(LAMBDA).shape == (wf.num_params(),)
    wf.close()


def test_no_batch_and_refused_family():
    wf = make_wf(N, UNITS, True)
    wf.init_params(5)
    for call in (wf.sr_solve, wf.sr_direction):
        with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
            call(LAMBDA)
    wf.close()
    stack = make_wf(6, UNITS, False, layers=2)
    stack.init_params(5)
    stack.vmc_step(48, 3, 0, np.append(np.ones(6), 1.0))
    for name, call in (("rnnwf_sr_solve", stack.sr_solve), ("rnnwf_sr_direction", stack.sr_direction)):
        with pytest.raises(ValueError, match=name + ": .*stacked layers"):
            call(LAMBDA)
    assert stack.resident_samples() == 48
    stack.close()


# ---- training ---------------------------------------------------------------------------------------------------------------

def test_device_solver_trains_like_the_host_solver():
    """the configuration of test_gpu_sr.py::test_minsr_training_lowers_the_tfim_energy_and_beats_adam with solver="device": the same
    three energy criteria, and iteration 0 (same parameters, same samples) equal to the host run's exactly"""
    from rnnwavefunctions_amd import training
    n, units, ns, steps, seed = 8, 10, 200, 60, 111
    lr, shift = 0.05, 1e-2
    e0 = np.linalg.eigvalsh(ed.tfim_hamiltonian(np.ones(n), 1.0, n))[0]
    prm = P.init_gru_params([units], seed=seed)
    wf = make_wf(n, units, False)
    mean, var = sr.train_tfim(wf, np.ones(n), 1.0, prm, numsteps=steps, numsamples=ns, learningrate=lr, diag_shift=shift, seed=seed, solver="device")
    host, _ = sr.train_tfim(make_wf(n, units, False), np.ones(n), 1.0, prm, numsteps=0, numsamples=ns, learningrate=lr, diag_shift=shift, seed=seed)
    assert len(mean) == len(var) == steps + 1
    err_i, err_f = np.sqrt(var[0] / ns), np.sqrt(var[-1] / ns)
    adam, _ = training.run_1DTFIM(numsteps=steps, systemsize=n, num_units=units, Bx=1, numsamples=ns, learningrate=5e-3, seed=seed, verbose=False)
    print("minSR, device solver: E %.4f +- %.4f -> %.4f +- %.4f, Adam -> %.4f, ground state %.4f" % (mean[0], err_i, mean[-1], err_f, adam[-1], e0))
    assert host[0] == mean[0] == adam[0]
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_i, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
    assert mean[-1] < adam[-1]
