"""GPU tests of stochastic reconfiguration for the complex RNN (docs/sr_complex.md): rnnwf_log_derivatives_complex,
rnnwf_sr_gram_complex / _apply_complex / _solve_complex / _direction_complex and sr.minsr_direction_complex / train_j1j2 against the
float64 autograd yardstick of tests/crnn_sr_reference.py.

Bounds (the complex RNN is a float32 model; none fitted to the kernels' output, all built as tests/test_gpu_sr.py builds its float32 ones):
  Jacobian, both halves, per tensor and in both norms (autograd_reference.verdict): FACTOR = 16 x the deviation of the float32 autograd
      restatement from the float64 one, with the floor 16 N 2^-24 x the tensor's largest reference magnitude where that difference
      collapses (docs/sr.md: a Jacobian stored in float32 cannot be closer than its own rounding).  The largest |O| of a tensor is a
      lower bound of its largest magnitude summed over the sites, so this floor is not above the one of that sum.  A tensor whose
      reference is exactly zero in both types (Re O on the phase head) has the bound zero: the device must return exact zeros.
  tie to rnnwf_vmc_gradient: sum_s 2 (Re eps_s Re O_s + Im eps_s Im O_s) / ns against rnnwf_get_grads_flat; the larger of FACTOR x the
      tensor's float32 / float64 autograd gradient difference and 16 N 2^-24 x the tensor's largest summed magnitude of the terms.
  Gram matrix: FACTOR x the spread between the Gram matrices of the float32 and float64 reference Jacobians, relative to the largest
      diagonal element; exactly symmetric; the row sums within each half within bound x ns.
  sr_apply_complex (y not centred): FACTOR x the spread of the same product over the two reference Jacobians.
  sr_solve_complex: on the device's own Gram matrix A = gram + ns lambda I, order n = 2 ns, against sr.solve_shifted (LAPACK):
      residual 16 n 2^-53 |A|_inf |y|_inf, error 16 n 2^-53 kappa^, kappa^ = |A|_inf / (ns lambda) (tests/test_gpu_sr_solve.py).
  sr_direction_complex: against solver="host" on the same handle, 16 n 2^-53 kappa^; against the float64 reference direction,
      FACTOR x (float32 / float64 reference spread + the reference's own solve error, LU against eigen-decomposition).

Cases (one reference and one device run each, shared by the parametrized tests) and the shapes they instantiate
(SrShape<float, NFULL, 3>: P x Q tiles, MP, QCH, passes; all four waves, backward operand in LDS):
  units 10, 20       NFULL 1   6 x 2,  MP 2, QCH 2, 1 pass
  units 36           NFULL 2   10 x 3, MP 3, QCH 3, 1 pass
  units 37, 50*, 52  NFULL 3   14 x 4, MP 4, QCH 4, 1 pass               (* N = 8, ns = 48)
  units 53, 68       NFULL 4   18 x 5, MP 5, QCH 3, 2 passes (3 + 2)
  chain lengths (20 units, ns 37): N = 4, 8 (no padded k-group), 6 (one), 34 (across a spin word)
  batch sizes (10 units, N = 6) on the order 2 ns: ns = 2, 8, 16 (one Gram block, the halves meet inside it), 17, 32 (the halves meet
  on a block edge), 33, 50; ns = 1 in test_one_sample; ns = 2048 in test_strided_grid (10 and 37 units).
"""
import functools

import numpy as np
import pytest
import torch

import autograd_reference as A
import crnn_sr_reference as C
import ed
from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

pytestmark = pytest.mark.gpu
SCOPE = A.SCOPE
LAMBDA, LAMBDA_ILL = 1e-3, 1e-8
EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24
SR_LR, SR_SHIFT = 0.05, 1e-2          # train_j1j2's learning rate and diagonal shift in the training test (those of the TFIM test)

CASES = [(6, u, 37) for u in (10, 20, 36, 37, 52, 53, 68)] + [(8, 50, 48)]
CASES += [(N, 20, 37) for N in (4, 8, 34)]
CASES += [(6, 10, ns) for ns in (2, 8, 16, 17, 32, 33, 50)]
IDS = ["N%d-u%d-ns%d" % c for c in CASES]


def make_wf(N, units, layers=1, model=_lib.MODEL_CRNN_U1):
    return _lib.NativeWavefunction(model, N, 1, (units,) * layers)


def make_params(units, seed):
    """trained-like: kernels x 2, every bias randomised (tests/test_gpu_crnn.py)"""
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([units], seed=seed, heads=C.HEADS), 2.0), seed + 1)


def sector_batch(rng, N, ns):
    return np.stack([rng.permutation(np.repeat([0, 1], N // 2)) for _ in range(ns)]).astype(np.int32)


def energies(rng, ns):
    """random complex local energies, exactly representable in the complex64 the device holds"""
    return ((rng.standard_normal(ns) * 2.0 - 3.0) + 1j * rng.standard_normal(ns)).astype(np.complex64).astype(np.complex128)


def wf_dict(wf, flat, prm):
    assert [SCOPE + "/" + nm for nm, _ in wf._layout()] == C.names(prm)
    return C.unflatten(flat, prm)


def device_run(wf, s, e, y, lam):
    """everything the device returns for one batch"""
    c = {}
    wf.load_batch(s, e)
    c["O"] = wf.log_derivatives_complex()
    c["gram"], c["eps"] = wf.sr_gram_complex()
    c["ysol"] = wf.sr_solve_complex(lam)
    c["delta"] = wf.sr_direction_complex(lam)
    c["gram_after"] = wf.sr_gram_complex()[0]
    c["delta_host"] = sr.minsr_direction_complex(wf, lam, solver="host")
    c["apply"] = wf.sr_apply_complex(y)
    return c


@functools.lru_cache(maxsize=None)
def case(N, units, ns, lam=LAMBDA):
    rng = np.random.RandomState(1000 * units + ns + N)
    prm = make_params(units, seed=7 + units)
    s, e = sector_batch(rng, N, ns), energies(rng, ns)
    c = dict(prm=prm, s=s, e=e, y=rng.standard_normal(2 * ns) + 0.5, ns=ns, lam=lam)
    c["re64"], c["im64"] = C.jacobian_dicts(prm, s, torch.float64)
    c["re32"], c["im32"] = C.jacobian_dicts(prm, s, torch.float32)
    c["o64"] = C.flatten(c["re64"]) + 1j * C.flatten(c["im64"])
    c["o32"] = C.flatten(c["re32"]) + 1j * C.flatten(c["im32"])
    c["g64"] = A.gradient("crnn", prm, s, e, dtype=torch.float64)
    c["g32"] = A.gradient("crnn", prm, s, e, dtype=torch.float32)
    wf = make_wf(N, units)
    wf.set_params(prm, scope=SCOPE)
    c.update(device_run(wf, s, e, c["y"], lam))
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    c["grad"] = {SCOPE + "/" + k: v for k, v in wf.vmc_gradient(e.mean(), ns, shapes).items()}
    c["again"] = (wf.log_derivatives_complex(), wf.sr_gram_complex()[0], wf.sr_solve_complex(lam), wf.sr_direction_complex(lam),
                  sr.minsr_direction_complex(wf, lam, solver="device"))          # after the gradient reused P and Q
    again = device_run(wf, s, e, c["y"], lam)
    c["reload"] = (again["O"], again["gram"], again["ysol"], again["delta"])
    c["re"], c["im"] = wf_dict(wf, c["O"].real, prm), wf_dict(wf, c["O"].imag, prm)
    wf.close()
    n = 2 * ns
    c["A"] = c["gram"] + ns * lam * np.eye(n)
    c["y_ref"] = sr.solve_shifted(c["gram"], c["eps"], lam / 2.0)              # solve_shifted shifts by (order) x its argument
    c["kappa"] = np.abs(c["A"]).sum(axis=1).max() / (ns * lam)
    return c


def check_jacobian(re, im, re64, im64, re32, im32, N):
    """both halves of the device Jacobian, by tensor, against the float64 reference"""
    floor = {k: N * EPS32 for k in re64}
    for half, got, ref, ref32 in (("Re", re, re64, re32), ("Im", im, im64, im32)):
        assert all(np.all(np.isfinite(v)) for v in got.values())
        worst, failures = A.verdict(got, ref, ref32, label="jacobian " + half, floor=floor)
        print("jacobian %s: worst deviation / yardstick %.3f (bound %g)" % (half, worst, A.FACTOR))
        assert not failures, (half, failures)


def check_gram(gram, eps, o64, o32, e, ns):
    ref, ref32 = C.gram(o64), C.gram(o32)
    scale = np.diag(ref).max() or 1.0
    bound = A.FACTOR * np.abs(ref32 - ref).max() / scale
    err = np.abs(gram - ref).max() / scale
    print("gram: error / largest diagonal %.3e (bound %.3e, ratio %.3e)" % (err, bound, err / bound if bound else 0.0))
    assert gram.shape == (2 * ns, 2 * ns) and np.array_equal(gram, gram.T)
    assert err <= bound
    for half in (slice(0, ns), slice(ns, 2 * ns)):
        assert np.abs(gram[:, half].sum(axis=1)).max() <= bound * ns * scale
    assert np.abs(eps - C.epsilon(e)).max() <= (ns + 8) * EPS64 * np.abs(e).max()
    return err, bound


def check_apply(got, o64, o32, y):
    ref = C.stacked(o64).T @ y
    bound = A.FACTOR * np.abs(C.stacked(o32).T @ y - ref).max()
    err = np.abs(got - ref).max()
    print("apply: max error %.3e, bound %.3e, ratio %.3e (largest element %.3e)" % (err, bound, err / bound, np.abs(ref).max()))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert err <= bound


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_jacobian_every_element(N, units, ns):
    c = case(N, units, ns)
    assert c["O"].shape == c["o64"].shape
    check_jacobian(c["re"], c["im"], c["re64"], c["im64"], c["re32"], c["im32"], N)


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_weighted_sum_is_the_vmc_gradient(N, units, ns):
    c = case(N, units, ns)
    w = (c["e"] - c["e"].mean()) / ns
    worst = 0.0
    for k, g in c["grad"].items():
        shape = (ns,) + (1,) * g.ndim
        t_re, t_im = 2.0 * w.real.reshape(shape) * c["re"][k], 2.0 * w.imag.reshape(shape) * c["im"][k]
        tie, mag = (t_re + t_im).sum(axis=0), (np.abs(t_re) + np.abs(t_im)).sum(axis=0).max()
        y = A.compare({k: c["g32"][k]}, {k: c["g64"][k]})[k]
        bound = max(A.FACTOR * y["max_abs"], 16 * N * EPS32 * mag)
        err = np.abs(tie - g).max()
        worst = max(worst, err / bound)
        print("tie %-80s |d| %.3e bound %.3e (largest summed magnitude %.3e)" % (k, err, bound, mag))
        assert err <= bound, k
    print("tie: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_gram_matrix(N, units, ns):
    c = case(N, units, ns)
    check_gram(c["gram"], c["eps"], c["o64"], c["o32"], c["e"], ns)
    assert np.array_equal(c["gram_after"], c["gram"])          # the factorisation does not write the Gram matrix


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_apply_matches_the_reference(N, units, ns):
    c = case(N, units, ns)
    check_apply(c["apply"], c["o64"], c["o32"], c["y"])


def check_solution(c):
    ns, n = c["ns"], 2 * c["ns"]
    y, y_ref, Amat = c["ysol"], c["y_ref"], c["A"]
    assert y.shape == (n,) and np.all(np.isfinite(y))
    norm_a = np.abs(Amat).sum(axis=1).max()
    res, res_bound = np.abs(Amat @ y - c["eps"]).max(), 16 * n * EPS64 * norm_a * np.abs(y).max()
    err, bound = np.linalg.norm(y - y_ref), 16 * n * EPS64 * c["kappa"] * np.linalg.norm(y_ref)
    print("solve: residual %.3e, bound %.3e, ratio %.3e | |y - y_ref| / |y_ref| %.3e, bound %.3e, ratio %.3e (kappa^ %.3e)"
          % (res, res_bound, res / res_bound if res_bound else 0.0, err / max(np.linalg.norm(y_ref), 1e-300),
             16 * n * EPS64 * c["kappa"], err / bound if bound else 0.0, c["kappa"]))
    assert res <= res_bound
    assert err <= bound
    dh = c["delta_host"]
    derr, dref = np.linalg.norm(c["delta"] - dh), np.linalg.norm(dh)
    dbound = 16 * n * EPS64 * c["kappa"]
    print("direction: |d_dev - d_host| / |d_host| %.3e, bound %.3e, ratio %.3e" % (derr / max(dref, 1e-300), dbound, derr / (dbound * dref) if dref else 0.0))
    assert c["delta"].shape == dh.shape and np.all(np.isfinite(c["delta"]))
    assert derr <= dbound * dref


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_solve_residual_lapack_and_host_direction(N, units, ns):
    check_solution(case(N, units, ns))


def test_solve_ill_conditioned():
    """lambda = 1e-8 at ns = 50 (order 100: four panels, a ragged last one)"""
    check_solution(case(6, 10, 50, LAMBDA_ILL))


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_direction_against_autograd(N, units, ns):
    c = case(N, units, ns)
    o64 = c["o64"]
    ref = C.minsr_direction(o64, c["e"], LAMBDA)
    spread = np.linalg.norm(C.minsr_direction(c["o32"], c["e"], LAMBDA) - ref) / np.linalg.norm(ref)
    w, v = np.linalg.eigh(C.gram(o64))
    own = np.linalg.norm(C.stacked(o64).T @ (v @ ((v.T @ C.epsilon(c["e"])) / (w + ns * LAMBDA))) - ref) / np.linalg.norm(ref)
    bound = A.FACTOR * (spread + own)
    for label, d in (("device", c["delta"]), ("host", c["delta_host"])):
        err = np.linalg.norm(d - ref) / np.linalg.norm(ref)
        print("direction (%s solver): |d| / |ref| %.3e, float32 / float64 reference spread %.3e, the reference's own solve error %.3e, "
              "bound %.3e, ratio %.3e" % (label, err, spread, own, bound, err / bound))
        assert err <= bound


@pytest.mark.parametrize("N,units,ns", CASES, ids=IDS)
def test_same_batch_same_bits(N, units, ns):
    c = case(N, units, ns)
    first = (c["O"], c["gram"], c["ysol"], c["delta"])
    for a, b in zip(first, c["again"][:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(c["again"][4], c["delta"])
    for a, b in zip(first, c["reload"]):
        assert np.array_equal(a, b)


def test_one_sample():
    """ns = 1: both centred halves are exactly zero, so the Gram matrix, eps, y, delta and Obar^T y are exact zeros; the Jacobian rows
    themselves meet the reference like any other."""
    N, units = 6, 10
    prm = make_params(units, seed=7 + units)
    s = np.array([[1, 0, 1, 1, 0, 0]], dtype=np.int32)
    e = np.array([-2.5 + 0.75j])
    re64, im64 = C.jacobian_dicts(prm, s, torch.float64)
    re32, im32 = C.jacobian_dicts(prm, s, torch.float32)
    wf = make_wf(N, units)
    wf.set_params(prm, scope=SCOPE)
    c = device_run(wf, s, e, np.array([3.0, -2.0]), LAMBDA)
    re, im = wf_dict(wf, c["O"].real, prm), wf_dict(wf, c["O"].imag, prm)
    wf.close()
    check_jacobian(re, im, re64, im64, re32, im32, N)
    npar = c["O"].shape[1]
    assert np.array_equal(c["gram"], np.zeros((2, 2))) and np.array_equal(c["eps"], np.zeros(2))
    assert np.array_equal(c["ysol"], np.zeros(2))
    for k in ("delta", "delta_host", "apply"):
        assert c[k].shape == (npar,) and np.array_equal(c[k], np.zeros(npar)), k


def test_constant_energy_gives_no_direction():
    """A constant complex E_loc (not dyadic: its sums round) gives eps = 0 and delta = 0 exactly, on the device and through the host."""
    N, units = 6, 10
    wf = make_wf(N, units)
    wf.set_params(make_params(units, seed=7 + units), scope=SCOPE)
    rng = np.random.RandomState(3)
    for ns in (2, 17, 50):
        wf.load_batch(sector_batch(rng, N, ns), np.full(ns, -2.7 + 0.3j))
        npar = wf.num_params()
        assert np.array_equal(wf.sr_gram_complex()[1], np.zeros(2 * ns))
        assert np.array_equal(wf.sr_solve_complex(LAMBDA), np.zeros(2 * ns))
        assert np.array_equal(wf.sr_direction_complex(LAMBDA), np.zeros(npar))
        assert np.array_equal(sr.minsr_direction_complex(wf, LAMBDA, solver="host"), np.zeros(npar))
    wf.close()


@pytest.mark.parametrize("units", [10, 37], ids=["u10", "u37"])
def test_strided_grid(units):
    """ns = 2048, the largest batch (order 4096, no solve): 8256 Gram blocks, more than any resident grid, so sr_gram_kernel reuses its
    LDS array across items.  The batch is the 20 configurations of the sector of six spins, tiled (the last tile is cut): row s holds
    configuration s mod 20, and equal inputs under a fixed summation order give equal bits in whichever trip they land - per half,
    for the two halves have their own means.

    The second trip of sr_outer_kernel's sample loop.  The launch helper's grid is at most (resident workgroups per CU) x CU count.
    The generic bound of eight workgroups of four waves per CU (a SIMD holds eight waves) gives 8 x 256 = 2048 on the MI355X, which
    is not below the largest batch these entries take - "8 x CU count < ns" cannot hold at ns = 2048 on 256 CUs, whatever the code
    does.  At 37 units the bound is tighter by construction, not by a compiler's choice: SrShape<float, 3, 3> keeps MP x QCH = 16
    accumulator tiles of four registers, 64 registers, live across its site loop beside the operands of the next step, so a wave
    needs more than 64 of the SIMD's 512 registers per lane and at most seven waves fit.  The test asserts 7 x CU count < ns for
    that width: there the sample loop is certain to stride.  (profiles/crnn_sr_kernel_resources.txt records 255 registers, two
    workgroups per CU, for that kernel, and 72 registers, seven per CU, at 10 units: the 10-unit case strides as well, but nothing
    in the source guarantees it, so it asserts nothing about the grid.)"""
    N, ns = 6, _lib.SR_COMPLEX_MAX_SAMPLES
    rng = np.random.RandomState(2048)
    prm = make_params(units, seed=7 + units)
    conf = np.array([[(k >> i) & 1 for i in range(N)] for k in range(64)], dtype=np.int32)
    conf = conf[conf.sum(axis=1) == N // 2]
    assert len(conf) == 20
    idx = np.arange(ns) % 20
    s, e, y = conf[idx], energies(rng, ns), rng.standard_normal(2 * ns) + 0.5
    tile = lambda d: {k: v[idx] for k, v in d.items()}
    re64, im64 = map(tile, C.jacobian_dicts(prm, conf, torch.float64))
    re32, im32 = map(tile, C.jacobian_dicts(prm, conf, torch.float32))
    o64, o32 = C.flatten(re64) + 1j * C.flatten(im64), C.flatten(re32) + 1j * C.flatten(im32)
    wf = make_wf(N, units)
    if units == 37:
        assert 7 * wf.device_info()["cu_count"] < ns               # the sample loop of sr_outer_kernel strides (docstring)
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    O = wf.log_derivatives_complex()
    gram, eps = wf.sr_gram_complex()
    applied = wf.sr_apply_complex(y)
    re, im = wf_dict(wf, O.real, prm), wf_dict(wf, O.imag, prm)
    wf.close()
    check_jacobian(re, im, re64, im64, re32, im32, N)
    assert np.array_equal(O, O[idx])                                # O[s] = O[s mod 20], both halves
    check_gram(gram, eps, o64, o32, e, ns)
    for a in (slice(0, ns), slice(ns, 2 * ns)):
        for b in (slice(0, ns), slice(ns, 2 * ns)):
            blk = gram[a, b]
            assert np.array_equal(blk, blk[:20, :20][np.ix_(idx, idx)])
    check_apply(applied, o64, o32, y)


# ---- state rules and refusals ---------------------------------------------------------------------------------------------

def complex_calls(wf, n=4):
    return (("rnnwf_log_derivatives_complex", wf.log_derivatives_complex), ("rnnwf_sr_gram_complex", wf.sr_gram_complex),
            ("rnnwf_sr_apply_complex", lambda: wf.sr_apply_complex(np.ones(n))),
            ("rnnwf_sr_solve_complex", lambda: wf.sr_solve_complex(LAMBDA)),
            ("rnnwf_sr_direction_complex", lambda: wf.sr_direction_complex(LAMBDA)))


def test_refused_models_keep_their_batch():
    N, ns = 6, 48
    refused = [("gru", make_wf(N, 10, model=_lib.MODEL_GRU1D)), ("gru64", make_wf(N, 10, model=_lib.MODEL_GRU1D_F64)),
               ("parity", make_wf(N, 10, model=_lib.MODEL_GRU1D_PARITY)), ("lstm", make_wf(N, 10, model=_lib.MODEL_LSTM1D_F64)),
               ("mdrnn", _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 3, 2, (10,)))]
    for label, wf in refused:
        wf.init_params(5)
        wf.vmc_step(ns, 3, 0, np.append(np.ones(N), 1.0))
        before = wf.resident_samples()                   # (the LSTM's step leaves no batch: it has no gradient)
        assert before == ns or label in ("lstm", "mdrnn")
        for name, call in complex_calls(wf, 2 * ns):
            with pytest.raises(ValueError, match=name + ": only for the complex RNN"):
                call()
        assert wf.resident_samples() == before, label
    # the positive GRU's batch still serves its own entries afterwards
    wf = refused[0][1]
    assert wf.sr_gram()[0].shape == (ns, ns)
    for _, wf in refused:
        wf.close()


def j1j2_couplings(N):
    return np.concatenate([np.ones(N), 0.2 * np.ones(N), np.zeros(N), [0.0, 0.0]])


def test_refused_complex_handles_keep_their_batch():
    N, ns = 6, 48
    for wf, why in ((make_wf(N, 10, layers=2), "one GRU layer only"), (make_wf(N, 70), "wider than 68")):
        wf.init_params(5)
        wf.vmc_step(ns, 3, 0, j1j2_couplings(N))
        for name, call in complex_calls(wf, 2 * ns):
            with pytest.raises(ValueError, match=name + ": .*" + why):
                call()
        assert wf.resident_samples() == ns
        wf.close()


def test_state_rules_and_argument_refusals():
    N, units, ns = 6, 10, 37
    c = case(N, units, ns)
    wf = make_wf(N, units)
    wf.set_params(c["prm"], scope=SCOPE)
    for name, call in complex_calls(wf, 2 * ns):                       # no batch
        with pytest.raises(_lib.RnnwfError, match=name + ": call rnnwf_vmc_step first"):
            call()
    wf.load_batch(c["s"], c["e"])
    for bad in (0.0, -1e-3, np.inf, np.nan):
        for name, call in (("rnnwf_sr_solve_complex", wf.sr_solve_complex), ("rnnwf_sr_direction_complex", wf.sr_direction_complex)):
            with pytest.raises(ValueError, match=name + ": diag_shift must be positive and finite"):
                call(bad)
    with pytest.raises(ValueError, match="sr_apply_complex"):
        wf.sr_apply_complex(np.ones(ns))
    assert wf.resident_samples() == ns
    assert np.array_equal(wf.sr_direction_complex(LAMBDA), c["delta"])   # the refusals touched nothing
    # the positive model's entries still refuse the complex handle, in their words
    for name, call in (("rnnwf_log_derivatives", wf.log_derivatives), ("rnnwf_sr_gram", wf.sr_gram),
                       ("rnnwf_sr_apply", lambda: wf.sr_apply(np.ones(ns))), ("rnnwf_sr_solve", lambda: wf.sr_solve(LAMBDA)),
                       ("rnnwf_sr_direction", lambda: wf.sr_direction(LAMBDA))):
        with pytest.raises(ValueError, match=name + ": not implemented for the complex RNN"):
            call()
    assert wf.resident_samples() == ns
    # new parameters: the batch goes with them, and the Jacobian of the re-loaded batch is the one at the new parameters
    prm2 = make_params(units, seed=99)
    wf.set_params(prm2, scope=SCOPE)
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.sr_gram_complex()
    wf.load_batch(c["s"], c["e"])
    O2 = wf.log_derivatives_complex()
    assert np.abs(O2 - c["O"]).max() > 1e-3 * np.abs(c["O"]).max()
    re64, im64 = C.jacobian_dicts(prm2, c["s"], torch.float64)
    re32, im32 = C.jacobian_dicts(prm2, c["s"], torch.float32)
    check_jacobian(wf_dict(wf, O2.real, prm2), wf_dict(wf, O2.imag, prm2), re64, im64, re32, im32, N)
    wf.close()


def test_sample_cap():
    N, ns = 6, _lib.SR_COMPLEX_MAX_SAMPLES + 1
    wf = make_wf(N, 10)
    wf.init_params(5)
    wf.vmc_step(ns, 3, 0, j1j2_couplings(N))
    for name, call in complex_calls(wf, 2 * ns):
        with pytest.raises(_lib.RnnwfError, match=name + ": ns too large for the SR workspace"):
            call()
    assert wf.resident_samples() == ns                         # refused, not dropped
    wf.close()


# ---- training ----------------------------------------------------------------------------------------------------------------

def test_minsr_training_on_the_j1j2_chain_beats_adam():
    """Open J1-J2 chain, N = 8, J2 = 0.2, 10 units, 200 samples, 60 steps, seed 111 (run_J1J2's default); docs/sr_complex.md has the
    table of three seeds.  Asserted: minSR ends below run_J1J2's Adam at its default learning rate from the same start, and its
    last-step energy is not below the exact ground energy by more than 5 standard errors (the variational bound)."""
    from rnnwavefunctions_amd import training
    N, units, ns, steps, seed = 8, 10, 200, 60, 111
    e0 = np.linalg.eigvalsh(ed.j1j2_hamiltonian(np.ones(N), 0.2 * np.ones(N), N))[0]
    prm = P.init_gru_params([units], seed=seed, heads=C.HEADS)
    wf = make_wf(N, units)
    mean, var = sr.train_j1j2(wf, 1.0, 0.2, 0.0, prm, numsteps=steps, numsamples=ns, learningrate=SR_LR, diag_shift=SR_SHIFT, seed=seed)
    wf.close()
    assert len(mean) == len(var) == steps + 1
    err_f = np.sqrt(var[-1] / ns)
    adam, _ = training.run_J1J2(numsteps=steps, systemsize=N, J1_=1.0, J2_=0.2, num_units=units, numsamples=ns, seed=seed, verbose=False)
    print("minSR: E %.4f -> %.4f +- %.4f (Im %.4f), Adam -> %.4f, ground state %.4f"
          % (mean[0].real, mean[-1].real, err_f, mean[-1].imag, np.real(adam[-1]), e0))
    assert np.complex64(mean[0]) == adam[0]                    # the same start: same parameters, same samples
    assert mean[-1].real < np.real(adam[-1])
    assert mean[-1].real >= e0 - 5.0 * err_f


def test_device_and_host_solver_start_alike():
    """iteration 0 sees the same parameters and draws the same samples whichever solver follows: its moments agree bit for bit"""
    N, units, ns, seed = 8, 10, 200, 111
    prm = P.init_gru_params([units], seed=seed, heads=C.HEADS)
    runs = []
    for solver in ("device", "host"):
        wf = make_wf(N, units)
        runs.append(sr.train_j1j2(wf, 1.0, 0.2, 0.0, prm, numsteps=1, numsamples=ns, learningrate=SR_LR, diag_shift=SR_SHIFT, seed=seed,
                                  solver=solver))
        wf.close()
    (md, vd), (mh, vh) = runs
    assert md[0] == mh[0] and vd[0] == vh[0]
    assert np.isfinite(md[1]) and np.isfinite(mh[1])
