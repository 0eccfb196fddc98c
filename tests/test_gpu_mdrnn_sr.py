"""GPU tests of stochastic reconfiguration for the 2D RNN (docs/sr_2d.md): rnnwf_log_derivatives_2d, rnnwf_sr_gram_2d / _apply_2d /
_solve_2d / _direction_2d and sr.minsr_direction_2d / train_tfim2d against the float64 autograd yardstick of tests/mdrnn_sr_reference.py.

Bounds (the 2D RNN is a float64 model; these are docs/sr.md's float64 bounds, none fitted to the kernels' output):
  Jacobian, every element: the worst row error at most 1e-10 N x the row's largest element.
  tie to rnnwf_vmc_gradient: sum_s 2 w_s O_s against rnnwf_get_grads_flat, per tensor within 16 N 2^-53 x the tensor's largest
      sum_s |2 w_s O_sk| (both sides add the same N ns products per element in different orders).
  Gram matrix: within 1e-10 N x the largest diagonal element, exactly symmetric, row sums within that bound x ns.
  sr_apply_2d (y not centred): within 1e-10 N ns x the largest element of the reference.
  sr_solve_2d on the device's own Gram matrix A = gram + ns lambda I against sr.solve_shifted (LAPACK): residual
      16 ns 2^-53 |A|_inf |y|_inf, error 16 ns 2^-53 kappa^ with kappa^ = |A|_inf / (ns lambda); lambda = 1e-3, once 1e-8.
  sr_direction_2d: against solver="host" on the same handle 16 ns 2^-53 kappa^; against the float64 reference direction
      16 x (2^-29 x the float32 / float64 reference spread + the reference's own solve error, LU against eigen-decomposition).

Cases (one reference and one device run each, shared by the parametrized tests) and the shapes they instantiate (MdSrShape<NFULL>:
P x Q tiles of 8 registers, waves as rows x columns, MP, Q tiles per column of waves, QCH, passes):
  units 10, 20   NFULL 1   2 x 4,   2 x 2 waves, MP 1, QW 2, QCH 2, 1 pass
  units 21, 36   NFULL 2   3 x 6,   2 x 2 waves, MP 2, QW 3, QCH 3, 1 pass    (the second row of waves has one P tile)
  units 37, 52   NFULL 3   4 x 8,   2 x 2 waves, MP 2, QW 4, QCH 4, 1 pass    (64 accumulator registers)
  units 53, 68   NFULL 4   5 x 10,  2 x 4 waves, MP 3, QW 3, QCH 2, 2 passes (2 + 1); the last column of waves owns one Q tile
  units 69, 84   NFULL 5   6 x 12,  2 x 4 waves, MP 3, QW 3, QCH 2, 2 passes (2 + 1)
  all on the 3 x 3 lattice with ns = 37 (a ragged 16-chain block; N = 9: one valid site in the last group of four)
  lattices (20 units, ns 37): 3 x 2 and 2 x 3 (Nx and Ny exchanged), 4 x 4 (no padded k-group), 3 x 3, 5 x 7 (N = 35 crosses a spin
  word; odd rows: both zig-zag directions and the ring's wrap-around)
  batch sizes (10 units, 3 x 2): ns = 2, 16, 17, 32, 33, 65; ns = 1 in test_one_sample; ns = 4096 in test_strided_grid.

Measured on an MI355X: docs/sr_2d.md has the table.
"""
import functools

import numpy as np
import pytest
import torch

import autograd_reference as A
import ed
import mdrnn_sr_reference as R
from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

pytestmark = pytest.mark.gpu
SCOPE = A.SCOPE
LAMBDA, LAMBDA_ILL = 1e-3, 1e-8
EPS64 = 2.0 ** -53
SR_LR, SR_SHIFT = 0.05, 1e-2          # train_tfim2d's learning rate and diagonal shift in the training test (those of the other two)

CASES = [(3, 3, u, 37) for u in (10, 20, 21, 36, 37, 52, 53, 68, 69, 84)]
CASES += [(nx, ny, 20, 37) for nx, ny in ((3, 2), (2, 3), (4, 4), (5, 7))]
CASES += [(3, 2, 10, ns) for ns in (2, 16, 17, 32, 33, 65)]
IDS = ["%dx%d-u%d-ns%d" % c for c in CASES]


def make_wf(nx, ny, units):
    return _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, nx, ny, (units,))


def make_params(units, seed):
    """non-trivial the way tests/test_gpu_gradient_full.py sharpens the 2D RNN: kernels x 1.25 (its elu cell is unbounded), every
    bias randomised"""
    return P.randomize_biases(P.scale_kernels(P.init_mdrnn_params(units, seed=seed), 1.25), seed + 1)


def wf_dict(wf, flat, prm):
    """flat vector(s) in the order of wf._layout() -> {scoped name: array}; the yardstick's order must be the library's"""
    assert [SCOPE + "/" + nm for nm, _ in wf._layout()] == R.names(prm)
    return R.unflatten(flat, prm)


def device_run(wf, s, e, y, lam):
    """everything the device returns for one batch"""
    c = {}
    wf.load_batch(s, e)
    c["O"] = wf.log_derivatives_2d()
    c["gram"], c["eps"] = wf.sr_gram_2d()
    c["ysol"] = wf.sr_solve_2d(lam)
    c["delta"] = wf.sr_direction_2d(lam)
    c["gram_after"] = wf.sr_gram_2d()[0]
    c["delta_host"] = sr.minsr_direction_2d(wf, lam, solver="host")
    c["apply"] = wf.sr_apply_2d(y)
    return c


@functools.lru_cache(maxsize=None)
def case(nx, ny, units, ns, lam=LAMBDA):
    rng = np.random.RandomState(1000 * units + ns + 10 * nx + ny)
    prm = make_params(units, seed=7 + units)
    s = rng.randint(0, 2, size=(ns, nx, ny)).astype(np.int32)
    e = rng.standard_normal(ns) * 2.0 - 3.0
    c = dict(prm=prm, s=s, e=e, y=rng.standard_normal(ns) + 0.5, ns=ns, N=nx * ny, lam=lam)      # y for sr_apply_2d: not centred
    c["o64"] = R.jacobian(prm, s, torch.float64)
    c["o32"] = R.jacobian(prm, s, torch.float32)
    wf = make_wf(nx, ny, units)
    wf.set_params(prm, scope=SCOPE)
    c.update(device_run(wf, s, e, c["y"], lam))
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    c["grad"] = {SCOPE + "/" + k: v for k, v in wf.vmc_gradient(e.mean(), ns, shapes).items()}
    c["again"] = (wf.log_derivatives_2d(), wf.sr_gram_2d()[0], wf.sr_solve_2d(lam), wf.sr_direction_2d(lam),
                  sr.minsr_direction_2d(wf, lam, solver="device"))               # after the gradient reused P and Q
    again = device_run(wf, s, e, c["y"], lam)
    c["reload"] = (again["O"], again["gram"], again["ysol"], again["delta"])
    c["O_dict"] = wf_dict(wf, c["O"], prm)
    wf.close()
    c["A"] = c["gram"] + ns * lam * np.eye(ns)
    c["y_ref"] = sr.solve_shifted(c["gram"], c["eps"], lam)
    c["kappa"] = np.abs(c["A"]).sum(axis=1).max() / (ns * lam)
    return c


def check_jacobian(O, ref, N):
    assert O.shape == ref.shape and np.all(np.isfinite(O)) and np.abs(ref).max() > 0
    rel = np.abs(O - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("jacobian: worst row error / row max %.3e (bound %.1e, ratio %.3e)" % (rel.max(), 1e-10 * N, rel.max() / (1e-10 * N)))
    assert rel.max() <= 1e-10 * N


def check_gram(gram, eps, ref, e, ns, N):
    scale = np.diag(ref).max() or 1.0
    bound = 1e-10 * N
    err = np.abs(gram - ref).max() / scale
    print("gram: error / largest diagonal %.3e (bound %.3e, ratio %.3e)" % (err, bound, err / bound))
    assert gram.shape == (ns, ns) and np.array_equal(gram, gram.T)
    assert err <= bound
    assert np.abs(gram.sum(axis=1)).max() <= bound * ns * scale
    assert np.abs(eps - R.epsilon(e)).max() <= (ns + 8) * EPS64 * np.abs(e).max()


def check_apply(got, ref, ns, N):
    bound = 1e-10 * N * ns * np.abs(ref).max()
    err = np.abs(got - ref).max()
    print("apply: max error %.3e, bound %.3e, ratio %.3e (largest element %.3e)" % (err, bound, err / bound, np.abs(ref).max()))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert err <= bound


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_jacobian_every_element(nx, ny, units, ns):
    c = case(nx, ny, units, ns)
    check_jacobian(c["O"], c["o64"], c["N"])


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_weighted_sum_is_the_vmc_gradient(nx, ny, units, ns):
    c = case(nx, ny, units, ns)
    w = (c["e"] - c["e"].mean()) / ns                              # w_s of rnnwf_vmc_gradient
    worst = 0.0
    for k, g in c["grad"].items():
        terms = 2.0 * w.reshape((ns,) + (1,) * g.ndim) * c["O_dict"][k]
        tie, mag = terms.sum(axis=0), np.abs(terms).sum(axis=0).max()
        bound = 16 * c["N"] * EPS64 * mag
        err = np.abs(tie - g).max()
        worst = max(worst, err / bound)
        print("tie %-60s |d| %.3e bound %.3e (largest summed magnitude %.3e)" % (k, err, bound, mag))
        assert err <= bound, k
    print("tie: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_gram_matrix(nx, ny, units, ns):
    """against the flat-order reference: also confirms that every multiplicity of the image mask is 0 or 1 (the two columns of
    wf_dense read one head row each)"""
    c = case(nx, ny, units, ns)
    check_gram(c["gram"], c["eps"], R.gram(c["o64"]), c["e"], ns, c["N"])
    assert np.array_equal(c["gram_after"], c["gram"])          # the factorisation does not write the Gram matrix


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_apply_matches_the_reference(nx, ny, units, ns):
    c = case(nx, ny, units, ns)
    check_apply(c["apply"], R.centred(c["o64"]).T @ c["y"], ns, c["N"])


def check_solution(c):
    ns = c["ns"]
    y, y_ref, Amat = c["ysol"], c["y_ref"], c["A"]
    assert y.shape == (ns,) and np.all(np.isfinite(y))
    norm_a = np.abs(Amat).sum(axis=1).max()
    res, res_bound = np.abs(Amat @ y - c["eps"]).max(), 16 * ns * EPS64 * norm_a * np.abs(y).max()
    err, bound = np.linalg.norm(y - y_ref), 16 * ns * EPS64 * c["kappa"] * np.linalg.norm(y_ref)
    print("solve: residual %.3e, bound %.3e, ratio %.3e | |y - y_ref| / |y_ref| %.3e, bound %.3e, ratio %.3e (kappa^ %.3e)"
          % (res, res_bound, res / res_bound if res_bound else 0.0, err / max(np.linalg.norm(y_ref), 1e-300),
             16 * ns * EPS64 * c["kappa"], err / bound if bound else 0.0, c["kappa"]))
    assert res <= res_bound
    assert err <= bound
    dh = c["delta_host"]
    derr, dref = np.linalg.norm(c["delta"] - dh), np.linalg.norm(dh)
    dbound = 16 * ns * EPS64 * c["kappa"]
    print("direction: |d_dev - d_host| / |d_host| %.3e, bound %.3e, ratio %.3e" % (derr / max(dref, 1e-300), dbound, derr / (dbound * dref) if dref else 0.0))
    assert c["delta"].shape == dh.shape and np.all(np.isfinite(c["delta"]))
    assert derr <= dbound * dref


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_solve_residual_lapack_and_host_direction(nx, ny, units, ns):
    check_solution(case(nx, ny, units, ns))


def test_solve_ill_conditioned():
    """lambda = 1e-8 at ns = 65 (three panels, a ragged last one)"""
    check_solution(case(3, 2, 10, 65, LAMBDA_ILL))


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_direction_against_autograd(nx, ny, units, ns):
    c = case(nx, ny, units, ns)
    o64 = c["o64"]
    ref = R.minsr_direction(o64, c["e"], LAMBDA)
    spread = np.linalg.norm(R.minsr_direction(c["o32"], c["e"], LAMBDA) - ref) / np.linalg.norm(ref)
    # the reference's own float64 error: the same reference system solved by eigen-decomposition instead of LU
    w, v = np.linalg.eigh(R.gram(o64))
    own = np.linalg.norm(R.centred(o64).T @ (v @ ((v.T @ R.epsilon(c["e"])) / (w + ns * LAMBDA))) - ref) / np.linalg.norm(ref)
    bound = A.FACTOR * (spread * A.F64_OVER_F32 + own)
    for label, d in (("device", c["delta"]), ("host", c["delta_host"])):
        err = np.linalg.norm(d - ref) / np.linalg.norm(ref)
        print("direction (%s solver): |d| / |ref| %.3e, float32 / float64 reference spread %.3e, the reference's own solve error %.3e, "
              "bound %.3e, ratio %.3e" % (label, err, spread, own, bound, err / bound))
        assert err <= bound


@pytest.mark.parametrize("nx,ny,units,ns", CASES, ids=IDS)
def test_same_batch_same_bits(nx, ny, units, ns):
    c = case(nx, ny, units, ns)
    first = (c["O"], c["gram"], c["ysol"], c["delta"])
    for a, b in zip(first, c["again"][:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(c["again"][4], c["delta"])
    for a, b in zip(first, c["reload"]):
        assert np.array_equal(a, b)


def test_one_sample():
    """ns = 1: the centred Jacobian is exactly zero, so the Gram matrix, eps, y, delta and dO^T y are exact zeros; the Jacobian row
    itself meets the reference like any other."""
    nx, ny, units = 3, 2, 10
    prm = make_params(units, seed=7 + units)
    s = np.array([[[1, 0], [1, 1], [0, 0]]], dtype=np.int32)
    e = np.array([-2.5])
    wf = make_wf(nx, ny, units)
    wf.set_params(prm, scope=SCOPE)
    c = device_run(wf, s, e, np.array([3.0]), LAMBDA)
    wf.close()
    check_jacobian(c["O"], R.jacobian(prm, s), nx * ny)
    npar = c["O"].shape[1]
    assert np.array_equal(c["gram"], np.zeros((1, 1))) and np.array_equal(c["eps"], np.zeros(1))
    assert np.array_equal(c["ysol"], np.zeros(1))
    for k in ("delta", "delta_host", "apply"):
        assert c[k].shape == (npar,) and np.array_equal(c[k], np.zeros(npar)), k


def test_constant_energy_gives_no_direction():
    """A constant E_loc (not a dyadic number, so its sum rounds) gives y = 0 and delta = 0 exactly on the device, which forms eps as
    (e - e_0) - mean (e - e_0) (tests/test_gpu_sr_solve.py: test_exact_zeros).  The eps rnnwf_sr_gram_2d hands to a host solver is
    e - mean e in float64 like the positive model's: zero to the rounding of the mean, not exactly."""
    nx, ny, units = 3, 2, 10
    wf = make_wf(nx, ny, units)
    wf.set_params(make_params(units, seed=7 + units), scope=SCOPE)
    rng = np.random.RandomState(3)
    for ns in (2, 17, 65):
        wf.load_batch(rng.randint(0, 2, size=(ns, nx, ny)).astype(np.int32), np.full(ns, -2.7))
        npar = wf.num_params()
        assert np.array_equal(wf.sr_solve_2d(LAMBDA), np.zeros(ns))
        assert np.array_equal(wf.sr_direction_2d(LAMBDA), np.zeros(npar))
        assert np.abs(wf.sr_gram_2d()[1]).max() <= (ns + 8) * EPS64 * 2.7
    wf.close()


@pytest.mark.parametrize("units", [10, 84], ids=["u10", "u84"])
def test_strided_grid(units):
    """ns = 4096, the largest batch (no solve): 8256 Gram blocks, more than any resident grid, so sr_gram_kernel reuses its LDS array
    across items.  The batch is the 64 configurations of the 3 x 2 lattice tiled 64 times: row s holds configuration s mod 64, and
    equal inputs under a fixed summation order give equal bits in whichever trip they land.

    The second trip of sr_outer_kernel's sample loop.  The launch helper's grid is at most (resident workgroups per CU) x CU count,
    and a CU has four SIMDs of eight wave slots.  MdSrShape<1> (10 units) runs four waves per workgroup, so at most eight workgroups
    are resident per CU; MdSrShape<5> (84 units) runs eight waves, so at most four - whatever registers the compiler assigns (the
    argument of docs/sr_complex.md, here from the wave slots alone).  8 x CU count < ns, resp. 4 x CU count < ns, then guarantees
    that the loop strides.  That holds on an MI355X (256 CUs); on a device with more CUs the case checks the same values without
    the second trip, so the test prints which it was and asserts nothing about the grid."""
    nx, ny, ns = 3, 2, 4096
    N = nx * ny
    rng = np.random.RandomState(4096)
    prm = make_params(units, seed=7 + units)
    conf = np.array([[(k >> i) & 1 for i in range(N)] for k in range(64)], dtype=np.int32).reshape(64, nx, ny)
    idx = np.arange(ns) % 64
    s, e, y = conf[idx], rng.standard_normal(ns) * 2.0 - 3.0, rng.standard_normal(ns) + 0.5
    o64 = R.jacobian(prm, conf)
    wf = make_wf(nx, ny, units)
    per_cu, cus = (8 if units == 10 else 4), wf.device_info()["cu_count"]
    print("sr_outer_kernel: at most %d x %d workgroups resident for %d samples: the sample loop %s"
          % (per_cu, cus, ns, "strides" if per_cu * cus < ns else "may run in one trip"))
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    O = wf.log_derivatives_2d()
    gram, eps = wf.sr_gram_2d()
    applied = wf.sr_apply_2d(y)
    wf.close()
    check_jacobian(O[:64], o64, N)
    assert np.array_equal(O, O[idx])                                # O[s] = O[s mod 64]
    # every configuration appears 64 times: the mean of the tiled rows is the mean of the 64
    d64 = R.centred(o64)
    check_gram(gram, eps, (d64 @ d64.T)[np.ix_(idx, idx)], e, ns, N)
    assert np.array_equal(gram, gram[:64, :64][np.ix_(idx, idx)])
    check_apply(applied, d64.T @ np.bincount(idx, weights=y, minlength=64), ns, N)


# ---- state rules and refusals ---------------------------------------------------------------------------------------------

def calls_2d(wf, n=4):
    return (("rnnwf_log_derivatives_2d", wf.log_derivatives_2d), ("rnnwf_sr_gram_2d", wf.sr_gram_2d),
            ("rnnwf_sr_apply_2d", lambda: wf.sr_apply_2d(np.ones(n))), ("rnnwf_sr_solve_2d", lambda: wf.sr_solve_2d(LAMBDA)),
            ("rnnwf_sr_direction_2d", lambda: wf.sr_direction_2d(LAMBDA)))


def test_refused_models_keep_their_batch():
    N, ns = 6, 48
    tfim, j1j2 = np.append(np.ones(N), 1.0), np.concatenate([np.ones(N), 0.2 * np.ones(N), np.zeros(N), [0.0, 0.0]])
    refused = [("gru", _lib.MODEL_GRU1D, tfim), ("gru64", _lib.MODEL_GRU1D_F64, tfim), ("parity", _lib.MODEL_GRU1D_PARITY, tfim),
               ("complex", _lib.MODEL_CRNN_U1, j1j2), ("lstm", _lib.MODEL_LSTM1D_F64, tfim)]
    for label, model, couplings in refused:
        wf = _lib.NativeWavefunction(model, N, 1, (10,))
        wf.init_params(5)
        wf.vmc_step(ns, 3, 0, couplings)
        before = wf.resident_samples()                   # (the LSTM's step leaves no batch: it has no gradient)
        assert before == ns or label == "lstm"
        for name, call in calls_2d(wf, ns):
            with pytest.raises(ValueError, match=name + r": only for the 2D RNN \(RNNWF_MODEL_MDRNN2D\)"):
                call()
        assert wf.resident_samples() == before, label
        if label == "gru":                               # the positive GRU's batch still serves its own entries afterwards
            assert wf.sr_gram()[0].shape == (ns, ns)
        wf.close()


def test_state_rules_and_argument_refusals():
    nx, ny, units, ns = 3, 2, 10, 33
    c = case(nx, ny, units, ns)
    wf = make_wf(nx, ny, units)
    wf.set_params(c["prm"], scope=SCOPE)
    for name, call in calls_2d(wf, ns):                                # no batch
        with pytest.raises(_lib.RnnwfError, match=name + ": call rnnwf_vmc_step first"):
            call()
    wf.load_batch(c["s"], c["e"])
    for bad in (0.0, -1e-3, np.inf, np.nan):
        for name, call in (("rnnwf_sr_solve_2d", wf.sr_solve_2d), ("rnnwf_sr_direction_2d", wf.sr_direction_2d)):
            with pytest.raises(ValueError, match=name + ": diag_shift must be positive and finite"):
                call(bad)
    with pytest.raises(ValueError, match="sr_apply_2d"):
        wf.sr_apply_2d(np.ones(ns + 1))
    assert wf.resident_samples() == ns
    assert np.array_equal(wf.sr_direction_2d(LAMBDA), c["delta"])      # the refusals touched nothing
    # the positive model's and the complex RNN's entries still refuse the 2D handle, in their words
    for name, call in (("rnnwf_log_derivatives", wf.log_derivatives), ("rnnwf_sr_gram", wf.sr_gram),
                       ("rnnwf_sr_apply", lambda: wf.sr_apply(np.ones(ns))), ("rnnwf_sr_solve", lambda: wf.sr_solve(LAMBDA)),
                       ("rnnwf_sr_direction", lambda: wf.sr_direction(LAMBDA))):
        with pytest.raises(ValueError, match=name + ": not implemented for the 2D RNN"):
            call()
    with pytest.raises(ValueError, match="rnnwf_sr_gram_complex: only for the complex RNN"):
        wf.sr_gram_complex()
    assert wf.resident_samples() == ns
    assert np.array_equal(wf.sr_direction_2d(LAMBDA), c["delta"])
    # uncommitted parameters
    name0, cnt0 = wf._layout()[0]
    first = np.asarray(c["prm"][SCOPE + "/" + name0], dtype=np.float64)
    wf._check(wf.lib.rnnwf_set_param(wf.h, name0.encode(), first.ctypes.data_as(_lib._P), first.size, _lib.F64))
    for name, call in calls_2d(wf, ns):
        with pytest.raises(_lib.RnnwfError, match=name + ": parameters not committed"):
            call()
    # new parameters: the batch goes with them, and the Jacobian of the re-loaded batch is the one at the new parameters
    prm2 = make_params(units, seed=99)
    wf.set_params(prm2, scope=SCOPE)
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.sr_gram_2d()
    wf.load_batch(c["s"], c["e"])
    O2 = wf.log_derivatives_2d()
    assert np.abs(O2 - c["O"]).max() > 1e-3 * np.abs(c["O"]).max()
    check_jacobian(O2, R.jacobian(prm2, c["s"]), nx * ny)
    wf.close()


def test_handle_with_a_communicator_is_refused():
    """a one-rank RCCL communicator on one GPU (tests/test_gpu_prnn.py: test_rccl_all_reduce_single_rank): every entry refuses the
    handle before any work and the batch stays resident; a handle without one serves the same batch"""
    nx, ny, units, ns = 3, 2, 10, 33
    c = case(nx, ny, units, ns)
    wf = make_wf(nx, ny, units)
    wf.set_params(c["prm"], scope=SCOPE)
    wf.comm_init(wf.comm_unique_id(), 0, 1)
    wf.load_batch(c["s"], c["e"])
    assert wf.resident_samples() == ns
    for name, call in calls_2d(wf, ns):
        with pytest.raises(ValueError, match=name + ": not implemented for a handle with a communicator"):
            call()
    assert wf.resident_samples() == ns                         # refused, not dropped: the gradient still works on the batch
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in c["prm"].items()}
    grad = wf.vmc_gradient(c["e"].mean(), ns, shapes)
    for k, g in grad.items():
        assert np.array_equal(g, c["grad"][SCOPE + "/" + k]), k
    wf.close()


def test_sample_cap():
    nx, ny, ns = 3, 2, 4097
    wf = make_wf(nx, ny, 10)
    wf.init_params(5)
    wf.vmc_step(ns, 3, 0, np.append(np.ones(nx * ny), 1.0))
    for name, call in calls_2d(wf, ns):
        with pytest.raises(_lib.RnnwfError, match=name + ": ns too large for the SR workspace"):
            call()
    assert wf.resident_samples() == ns                         # refused, not dropped
    wf.close()


# ---- training ----------------------------------------------------------------------------------------------------------------

TRAIN = dict(nx=3, ny=3, Bx=3.0, units=10, ns=200, steps=60, seed=111)


def train(solver, steps):
    t = TRAIN
    prm = P.init_mdrnn_params(t["units"], seed=t["seed"])
    wf = make_wf(t["nx"], t["ny"], t["units"])
    out = sr.train_tfim2d(wf, 1.0, t["Bx"], prm, numsteps=steps, numsamples=t["ns"], learningrate=SR_LR, diag_shift=SR_SHIFT,
                          seed=t["seed"], solver=solver)
    wf.close()
    return out


def test_minsr_training_on_the_3x3_tfim():
    """3 x 3 TFIM, Jz = 1, Bx = 3, 10 units, 200 samples, 60 steps, lr 0.05, shift 1e-2 (the values of the other two training tests,
    not tuned), seed 111; docs/sr_2d.md has the table of three seeds against run_2DTFIM_2DRNN.  Asserted: the final energy is more
    than 5 standard errors below the start, not more than 5 standard errors below the exact ground energy, and below the energy
    run_2DTFIM_2DRNN's Adam reaches at its default learning rate from the same start (that held for all three seeds of the table)."""
    from rnnwavefunctions_amd import training
    t = TRAIN
    e0 = np.linalg.eigvalsh(ed.tfim2d_hamiltonian(np.ones((t["nx"], t["ny"])), t["Bx"], t["nx"], t["ny"]))[0]
    mean, var = train("device", t["steps"])
    assert len(mean) == len(var) == t["steps"] + 1
    err_0, err_f = np.sqrt(var[0] / t["ns"]), np.sqrt(var[-1] / t["ns"])
    adam, _ = training.run_2DTFIM_2DRNN(numsteps=t["steps"], systemsize_x=t["nx"], systemsize_y=t["ny"], Bx=t["Bx"], num_units=t["units"],
                                        numsamples=t["ns"], seed=t["seed"], verbose=False)
    print("minSR: E %.4f +- %.4f -> %.4f +- %.4f, Adam -> %.4f, ground state %.4f" % (mean[0], err_0, mean[-1], err_f, adam[-1], e0))
    assert mean[0] == adam[0]                                    # the same start: same parameters, same samples
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_0, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
    assert mean[-1] < adam[-1]


def test_device_and_host_solver_start_alike():
    """iteration 0 sees the same parameters and draws the same samples whichever solver follows: its moments agree bit for bit"""
    (md, vd), (mh, vh) = train("device", 1), train("host", 1)
    assert md[0] == mh[0] and vd[0] == vh[0]
    assert np.isfinite(md[1]) and np.isfinite(mh[1])
