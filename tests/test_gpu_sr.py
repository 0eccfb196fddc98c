"""GPU tests of stochastic reconfiguration (docs/sr.md): rnnwf_log_derivatives / rnnwf_sr_gram / rnnwf_sr_apply and
rnnwavefunctions_amd/sr.py against the float64 autograd yardstick of tests/sr_reference.py.

Bounds (none fitted to the kernels' output):
  float64 model: 1e-10 N relative to the row's largest element (Jacobian) or the largest diagonal element (Gram matrix) - the kind
      of bound docs/lstm.md uses for a float64 recurrence of N sites;
  float32 model: autograd_reference.FACTOR x the deviation of the float32 autograd restatement from the float64 one, per tensor
      and in both norms (autograd_reference.verdict) for the Jacobian; the same spread of the derived quantity (Gram matrix,
      direction) computed from the float32 and float64 reference Jacobians for those;
  direction: the spread above (x 2^-29 for the float64 model) PLUS the reference's own float64 error, measured as the difference between
      two float64 solves of the reference system (LU and eigen-decomposition): the shifted Gram matrix has a condition number of
      1e3..1e4 at lambda = 1e-3, so the yardstick itself is only good to ~1e-13;
  tie to rnnwf_vmc_gradient, float64: both sides add the same N ns products per element in different orders, each with relative
      rounding 2^-53 of the running magnitudes: 16 N 2^-53 x the tensor's largest sum_s |2 w_s O_sk|.
  tie, float32: the larger of FACTOR x the tensor's float32 / float64 autograd difference and the float64 branch's expression at the
      float32 unit round-off, 16 N 2^-24 x the tensor's largest sum_s |2 w_s O_sk|.  The autograd difference alone cannot serve: on a
      tensor of two elements (wf_dense/bias) it can come out far below one float32 ulp of what either side adds up, by chance and
      depending on the reference's thread count, while a Jacobian stored in float32 cannot be closer than its own rounding.
  sr_apply (dO^T y, y not centred), every case: float64 1e-10 N ns x the largest element of the reference (the bound of
      test_resident_batch_rules); float32 FACTOR x the largest difference between the same product of the float32 and of the float64
      reference Jacobian.

Cases (CASES; each is one reference and one device run shared by the six parametrized tests) and the SrShape of sr_kernels.h they
instantiate (P x Q tiles, waves, MP, QCH, passes; backward operand of gru_bwd_kernel<SR>):
  units 10, 20   NFULL 1  f32 / f64  6 x 2,  4 waves, MP 2, QCH 2, 1 pass                    LDS
  units 36       NFULL 2  f32        10 x 3, 4 waves, MP 3, QCH 3, 1 pass                    LDS
                          f64        10 x 3, 4 waves, MP 3, QCH 2, 2 passes (2 + 1)          LDS
  units 37, 50*, 52  NFULL 3  f32    14 x 4, 4 waves, MP 4, QCH 4, 1 pass                    LDS          (* f32 only, N = 8, ns = 48)
                          f64        14 x 4, 8 waves, MP 2, QCH 4, 1 pass                    LDS
  units 53, 68   NFULL 4  f32        18 x 5, 4 waves, MP 5, QCH 3, 2 passes (3 + 2)          LDS
                          f64        18 x 5, 8 waves, MP 3, QCH 2, 3 passes (2 + 2 + 1)      global, through L2 (GradStream)
  chain lengths (ns 37): units 20 f32 N = 4, 5, 8, 36 and N = 33; units 68 f64 N = 8
  batch sizes (units 10, N = 6, both types): ns = 2, 16, 32, 33, 65, 100 beside 37 and 48; ns = 1 in test_one_sample; ns = 4096 in
  test_strided_grids (second trip of the grid-stride loops of sr_outer_kernel and sr_gram_kernel).

Measured on an MI355X over the added cases, float64 / float32 model (docs/sr.md has the table and the first cases' figures):
  Jacobian            worst row error / row maximum 5.2e-15 (bound 1e-10 N)   /  deviation / yardstick at most 2.8 (bound 16)
  tie, error / bound  0.034                                                    /  0.050
  Gram matrix         error / largest diagonal 1.0e-15, ns 4096: 2.8e-15      /  error / bound at most 0.10
  direction           error / bound at most 0.13                               /  0.089
  sr_apply            error / largest element 6.7e-15, ns 4096: 7.0e-13       /  error / bound at most 0.12
The module's 243 tests take 8 s (the two ns = 4096 tests 1.3 s each).
"""
import functools

import numpy as np
import pytest
import torch

import autograd_reference as A
import ed
import sr_reference as R
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import sr

pytestmark = pytest.mark.gpu
SCOPE = A.SCOPE
LAMBDA = 1e-3
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
SR_LR, SR_SHIFT = 0.05, 1e-2          # train_tfim's learning rate and diagonal shift in the training test

# (N, units, float64 model, ns): units 10 = mixed tile only (plus a remainder), 20 = one full tile + the whole mixed tile, 36 = two full
# tiles + the mixed tile; ns 37 = a partial last block of 16 chains; N = 33: the packed spins cross a word
CASES = [(6, u, f64, ns) for u in (10, 20, 36) for f64 in (False, True) for ns in (37, 48)] + [(33, 20, False, 37)]
# both ends of NFULL 3 (37..52 units) and NFULL 4 (53..68), the widths at which SrShape changes shape: eight waves per sample and
# waves without an i-th tile (f64), two and three Q passes with a ragged last chunk (NFULL 4), gru_bwd_kernel<SR> with the
# backward operand streamed through L2 (f64 above 52 units); and the width docs/sr.md times (50 units, f32)
CASES += [(6, u, f64, 37) for u in (37, 52, 53, 68) for f64 in (False, True)] + [(8, 50, False, 48)]
# chain lengths: N = 4, 8 multiples of four (no padded k-group in sr_outer_kernel), 5 = one valid site in the last group, 36 = a
# multiple of four that crosses a spin word; N = 8 once more on the widest float64 shape
CASES += [(N, 20, False, 37) for N in (4, 5, 8, 36)] + [(8, 68, True, 37)]
# batch sizes at the edges of the 32 x 32 Gram blocks and the 16-chain blocks: 32 = exactly one Gram block, 33 = one valid row in the
# second, 65 = the first off-diagonal block that is not next to the diagonal (2, 0), 100 = ten blocks
CASES += [(6, 10, f64, ns) for f64 in (False, True) for ns in (2, 16, 32, 33, 65, 100)]
IDS = ["N%d-u%d-%s-ns%d" % (N, u, "f64" if f else "f32", ns) for N, u, f, ns in CASES]


def make_wf(N, units, f64, layers=1, model=None):
    from rnnwavefunctions_amd import _lib
    mid = model if model is not None else (_lib.MODEL_GRU1D_F64 if f64 else _lib.MODEL_GRU1D)
    return _lib.NativeWavefunction(mid, N, 1, (units,) * layers)


def make_params(units, f64, seed):
    prm = P.init_gru_params([units], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0), seed + 1)


def wf_dict(wf, flat, prm):
    """flat vector(s) in the order of wf._layout() -> {scoped name: array}; the yardstick's order must be the library's"""
    assert [SCOPE + "/" + nm for nm, _ in wf._layout()] == R.names(prm)
    return R.unflatten(flat, prm)


@functools.lru_cache(maxsize=None)
def case(N, units, f64, ns):
    """the batch, the reference (computed once, shared by the tests of the case) and everything the device returns for it"""
    rng = np.random.RandomState(1000 * units + ns + N)
    prm = make_params(units, f64, seed=7 + units)
    s = rng.randint(0, 2, size=(ns, N)).astype(np.int32)
    e = rng.standard_normal(ns) * 2.0 - 3.0
    c = dict(prm=prm, s=s, e=e, y=rng.standard_normal(ns) + 0.5)          # y for sr_apply: not centred
    c["o64"] = R.jacobian_dict(prm, s, torch.float64)
    c["o32"] = R.jacobian_dict(prm, s, torch.float32)
    c["g64"] = A.gradient("gru", prm, s, e, dtype=torch.float64)
    c["g32"] = A.gradient("gru", prm, s, e, dtype=torch.float32)
    wf = make_wf(N, units, f64)
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    c["O"] = wf.log_derivatives()
    c["gram"], c["eps"] = wf.sr_gram()
    c["delta"] = sr.minsr_direction(wf, LAMBDA)
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()}
    c["grad"] = {SCOPE + "/" + k: v for k, v in wf.vmc_gradient(e.mean(), ns, shapes).items()}
    c["again"] = (wf.log_derivatives(), wf.sr_gram()[0], sr.minsr_direction(wf, LAMBDA))      # after the gradient reused P and Q
    wf.load_batch(s, e)
    c["reload"] = (wf.log_derivatives(), wf.sr_gram()[0], sr.minsr_direction(wf, LAMBDA))
    c["apply"] = wf.sr_apply(c["y"])
    c["O_dict"] = wf_dict(wf, c["O"], prm)
    wf.close()
    return c


def check_jacobian(O, O_dict, o64, o32, f64, N):
    """every element of the device Jacobian O (O_dict: the same by tensor) against the float64 reference, with the bound of its type"""
    ref = R.flatten(o64)
    assert O.shape == ref.shape and np.all(np.isfinite(O))
    if f64:
        rel = np.abs(O - ref).max(axis=1) / np.abs(ref).max(axis=1)
        print("jacobian f64: worst row error / row max %.3e (bound %.1e)" % (rel.max(), 1e-10 * N))
        assert rel.max() <= 1e-10 * N
    else:
        worst, failures = A.verdict(O_dict, o64, o32, label="jacobian")
        print("jacobian f32: worst deviation / yardstick %.3f (bound %g)" % (worst, A.FACTOR))
        assert not failures, failures


def check_apply(got, o64, o32, y, f64, N):
    """dO^T y against the float64 reference: 1e-10 N ns relative for the float64 model (the bound of test_resident_batch_rules), FACTOR x
    the spread of the same product over the float32 and float64 reference Jacobians for the float32 model"""
    o = R.flatten(o64)
    ns, ref = o.shape[0], R.centred(o).T @ y
    bound = 1e-10 * N * ns * np.abs(ref).max() if f64 else A.FACTOR * np.abs(R.centred(R.flatten(o32)).T @ y - ref).max()
    err = np.abs(got - ref).max()
    print("apply: max error %.3e, bound %.3e, ratio %.3e (largest element %.3e)" % (err, bound, err / bound, np.abs(ref).max()))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert err <= bound


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_jacobian_every_element(N, units, f64, ns):
    c = case(N, units, f64, ns)
    check_jacobian(c["O"], c["O_dict"], c["o64"], c["o32"], f64, N)


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_weighted_sum_is_the_vmc_gradient(N, units, f64, ns):
    c = case(N, units, f64, ns)
    w = (c["e"] - c["e"].mean()) / ns                              # w_s of rnnwf_vmc_gradient
    worst = 0.0
    for k, g in c["grad"].items():
        terms = 2.0 * w.reshape((ns,) + (1,) * g.ndim) * c["O_dict"][k]
        tie, mag = terms.sum(axis=0), np.abs(terms).sum(axis=0).max()
        if f64:
            bound = 16 * N * EPS64 * mag
        else:
            y = A.compare({k: c["g32"][k]}, {k: c["g64"][k]})[k]
            bound = max(A.FACTOR * y["max_abs"], 16 * N * EPS32 * mag)
        err = np.abs(tie - g).max()
        worst = max(worst, err / bound)
        print("tie %-80s |d| %.3e bound %.3e (largest summed magnitude %.3e)" % (k, err, bound, mag))
        assert err <= bound, k
    print("tie: worst error / bound %.3f" % worst)


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_gram_matrix(N, units, f64, ns):
    c = case(N, units, f64, ns)
    ref, ref32 = R.gram(R.flatten(c["o64"])), R.gram(R.flatten(c["o32"]))
    scale = np.diag(ref).max()
    bound = 1e-10 * N if f64 else A.FACTOR * np.abs(ref32 - ref).max() / scale
    err = np.abs(c["gram"] - ref).max() / scale
    print("gram: error / largest diagonal %.3e (bound %.3e), eps error %.3e" % (err, bound, np.abs(c["eps"] - R.epsilon(c["e"])).max()))
    assert c["gram"].shape == (ns, ns) and np.array_equal(c["gram"], c["gram"].T)
    assert err <= bound
    assert np.abs(c["gram"].sum(axis=1)).max() <= bound * ns * scale
    assert np.abs(c["eps"] - R.epsilon(c["e"])).max() <= 8 * EPS64 * np.abs(c["e"]).max()


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_minsr_direction(N, units, f64, ns):
    c = case(N, units, f64, ns)
    o64 = R.flatten(c["o64"])
    ref = R.minsr_direction(o64, c["e"], LAMBDA)
    spread = np.linalg.norm(R.minsr_direction(R.flatten(c["o32"]), c["e"], LAMBDA) - ref) / np.linalg.norm(ref)
    # the reference's own float64 error: the same reference system solved by eigen-decomposition instead of LU
    w, v = np.linalg.eigh(R.gram(o64))
    own = np.linalg.norm(R.centred(o64).T @ (v @ ((v.T @ R.epsilon(c["e"])) / (w + ns * LAMBDA))) - ref) / np.linalg.norm(ref)
    bound = A.FACTOR * (spread * (A.F64_OVER_F32 if f64 else 1.0) + own)
    err = np.linalg.norm(c["delta"] - ref) / np.linalg.norm(ref)
    print("direction: |d| / |ref| %.3e, float32 / float64 reference spread %.3e, the reference's own solve error %.3e, bound %.3e"
          % (err, spread, own, bound))
    assert err <= bound


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_same_batch_same_bits(N, units, f64, ns):
    c = case(N, units, f64, ns)
    for first, other in zip((c["O"], c["gram"], c["delta"]), c["again"]):
        assert np.array_equal(first, other)
    for first, other in zip((c["O"], c["gram"], c["delta"]), c["reload"]):
        assert np.array_equal(first, other)


@pytest.mark.parametrize("N,units,f64,ns", CASES, ids=IDS)
def test_apply_matches_the_reference(N, units, f64, ns):
    c = case(N, units, f64, ns)
    check_apply(c["apply"], c["o64"], c["o32"], c["y"], f64, N)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_one_sample(f64):
    """ns = 1: the centred Jacobian is exactly zero (the column mean of one row is that row), so the Gram matrix, eps and dO^T y are
    exact zeros and there is no direction to compare (the direction test divides by the reference's norm); the Jacobian row itself
    meets the reference like any other."""
    N, units = 6, 10
    prm = make_params(units, f64, seed=7 + units)
    s = np.array([[1, 0, 1, 1, 0, 0]], dtype=np.int32)
    e = np.array([-2.5])
    o64, o32 = R.jacobian_dict(prm, s, torch.float64), R.jacobian_dict(prm, s, torch.float32)
    wf = make_wf(N, units, f64)
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    O = wf.log_derivatives()
    gram, eps = wf.sr_gram()
    applied = wf.sr_apply(np.array([3.0]))
    O_dict = wf_dict(wf, O, prm)
    wf.close()
    assert np.abs(R.flatten(o64)).max() > 0
    check_jacobian(O, O_dict, o64, o32, f64, N)
    assert gram.shape == (1, 1) and np.array_equal(gram, [[0.0]])
    assert np.array_equal(eps, [0.0])
    assert applied.shape == (O.shape[1],) and np.array_equal(applied, np.zeros(O.shape[1]))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_strided_grids(f64):
    """ns = 4096: more samples than sr_outer_kernel has resident workgroups (at most eight of 256 threads per CU), so its sample loop
    makes a second trip, and 8256 Gram blocks, more than any resident grid, so sr_gram_kernel's item loop reuses its LDS array.
    The batch is the 64 configurations of six spins tiled 64 times: row s holds configuration s mod 64, the reference needs the 64
    distinct rows only, and equal inputs under a fixed summation order must give equal bits in whichever grid trip they land.
    No solve here: the host solve is covered by the smaller cases."""
    N, units, reps = 6, 10, 64
    ns = 64 * reps
    rng = np.random.RandomState(4096 + int(f64))
    prm = make_params(units, f64, seed=7 + units)
    conf = ((np.arange(64)[:, None] >> np.arange(N)) & 1).astype(np.int32)
    s = np.tile(conf, (reps, 1))
    e = rng.standard_normal(ns) * 2.0 - 3.0
    y = rng.standard_normal(ns) + 0.5
    o64 = {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in R.jacobian_dict(prm, conf, torch.float64).items()}
    o32 = {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in R.jacobian_dict(prm, conf, torch.float32).items()}
    wf = make_wf(N, units, f64)
    assert 8 * wf.device_info()["cu_count"] < ns                   # the sample loop of sr_outer_kernel strides
    wf.set_params(prm, scope=SCOPE)
    wf.load_batch(s, e)
    O = wf.log_derivatives()
    gram, eps = wf.sr_gram()
    applied = wf.sr_apply(y)
    O_dict = wf_dict(wf, O, prm)
    wf.close()
    assert np.array_equal(s[64:], s[:-64])
    check_jacobian(O, O_dict, o64, o32, f64, N)
    assert np.array_equal(O.reshape(reps, 64, -1), np.broadcast_to(O[:64], (reps, 64, O.shape[1])))
    ref, ref32 = R.gram(R.flatten(o64)), R.gram(R.flatten(o32))
    scale = np.diag(ref).max()
    bound = 1e-10 * N if f64 else A.FACTOR * np.abs(ref32 - ref).max() / scale
    err = np.abs(gram - ref).max() / scale
    print("gram: error / largest diagonal %.3e (bound %.3e)" % (err, bound))
    assert gram.shape == (ns, ns) and np.array_equal(gram, gram.T)
    assert err <= bound
    assert np.array_equal(gram.reshape(reps, 64, reps, 64), np.broadcast_to(gram[:64, :64][None, :, None, :], (reps, 64, reps, 64)))
    # eps: the library's mean is a serial float64 sum of ns terms, at most (ns - 1) 2^-53 sum |e| off, so the mean is within
    # ns 2^-53 max |e|; the few roundings of the division, the subtraction and the reference's own mean are the + 8
    assert np.abs(eps - R.epsilon(e)).max() <= (ns + 8) * EPS64 * np.abs(e).max()
    check_apply(applied, o64, o32, y, f64, N)


def test_qgt_matches_the_reference():
    N, units, ns = 6, 10, 48
    c = case(N, units, True, ns)
    wf = make_wf(N, units, True)
    wf.set_params(c["prm"], scope=SCOPE)
    wf.load_batch(c["s"], c["e"])
    S, ref = sr.qgt(wf), R.qgt(R.flatten(c["o64"]))
    assert np.abs(S - ref).max() <= 1e-10 * N * np.abs(np.diag(ref)).max()


# ---- resident-batch rules and refusals ------------------------------------------------------------------------------------

def test_resident_batch_rules():
    from rnnwavefunctions_amd import _lib
    N, units, ns = 6, 10, 37
    c = case(N, units, True, ns)
    wf = make_wf(N, units, True)
    wf.set_params(c["prm"], scope=SCOPE)
    for call in (wf.log_derivatives, wf.sr_gram, lambda: wf.sr_apply(np.ones(ns))):
        with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
            call()
    wf.load_batch(c["s"], c["e"])
    assert wf.resident_samples() == ns
    ref = R.flatten(c["o64"])
    assert np.abs(wf.log_derivatives() - ref).max() <= 1e-10 * N * np.abs(ref).max()
    with pytest.raises(ValueError, match="sr_apply"):
        wf.sr_apply(np.ones(ns + 1))
    # new parameters: the batch is gone with them, and the Jacobian of the re-loaded batch is the one at the NEW parameters.  (A commit
    # clears the resident batch, so the rebuild always comes through the new batch; grad_invalidate's own sr_valid = false is a
    # second guard that no sequence of public calls reaches alone.)
    prm2 = make_params(units, True, seed=99)
    wf.set_params(prm2, scope=SCOPE)
    with pytest.raises(_lib.RnnwfError, match="vmc_step first"):
        wf.sr_gram()
    wf.load_batch(c["s"], c["e"])
    ref2 = R.jacobian(prm2, c["s"])
    assert np.abs(ref2 - ref).max() > 1e-3 * np.abs(ref).max()
    assert np.abs(wf.log_derivatives() - ref2).max() <= 1e-10 * N * np.abs(ref2).max()
    # a new batch under the same parameters: rebuilt as well (sr_apply alone must not read the old Jacobian)
    s3 = 1 - c["s"]
    wf.load_batch(s3, c["e"])
    y = np.linspace(-1.0, 1.0, ns)
    ref3 = R.centred(R.jacobian(prm2, s3)).T @ y
    assert np.abs(wf.sr_apply(y) - ref3).max() <= 1e-10 * N * ns * np.abs(ref3).max()


def test_refused_handles_keep_their_batch():
    from rnnwavefunctions_amd import _lib
    N = 6
    refused = [("parity", make_wf(N, 10, False, model=_lib.MODEL_GRU1D_PARITY), "parity"),
               ("complex", make_wf(N, 10, False, model=_lib.MODEL_CRNN_U1), "complex RNN"),
               ("mdrnn", _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 3, 2, (10,)), "2D RNN"),
               ("lstm", make_wf(N, 10, True, model=_lib.MODEL_LSTM1D_F64), "LSTM"),
               ("stack", make_wf(N, 10, False, layers=2), "stacked layers"),
               ("wide", make_wf(N, 70, False), "wider than 68")]
    for label, wf, why in refused:
        wf.init_params(5)
        for name, call in (("rnnwf_log_derivatives", wf.log_derivatives), ("rnnwf_sr_gram", wf.sr_gram),
                           ("rnnwf_sr_apply", lambda: wf.sr_apply(np.ones(4)))):
            with pytest.raises(ValueError, match=name + ": .*" + why):
                call()
    # a refused call touches nothing: the parity model's resident batch still serves the gradient, with the same bits
    wf = refused[0][1]
    mom = wf.vmc_step(48, 3, 0, np.append(np.ones(N), 1.0))["moments"]
    shapes = {k[len(SCOPE) + 1:]: v.shape for k, v in P.init_gru_params([10]).items()}
    g0 = wf.vmc_gradient(mom[0] / mom[2], mom[2], shapes)
    with pytest.raises(ValueError, match="rnnwf_sr_gram"):
        wf.sr_gram()
    g1 = wf.vmc_gradient(mom[0] / mom[2], mom[2], shapes)
    assert wf.resident_samples() == 48 and all(np.array_equal(g0[k], g1[k]) for k in g0)


def test_workspace_refusals(monkeypatch):
    from rnnwavefunctions_amd import _lib
    N = 6
    wf = make_wf(N, 10, False)
    wf.init_params(5)
    wf.vmc_step(4112, 3, 0, np.append(np.ones(N), 1.0))
    with pytest.raises(_lib.RnnwfError, match="ns too large for the SR workspace"):
        wf.sr_gram()
    assert wf.resident_samples() == 4112                     # refused, not dropped
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")         # Jacobian 400 x 3096 x 4 B = 4.7 MiB
    small = make_wf(N, 10, False)
    small.init_params(5)
    small.vmc_step(400, 3, 0, np.append(np.ones(N), 1.0))
    with pytest.raises(_lib.RnnwfError, match="ns too large for the SR workspace"):
        small.log_derivatives()
    small.vmc_step(48, 3, 1, np.append(np.ones(N), 1.0))     # 48 x 3096 x 4 B + 48^2 x 8 B fits
    assert small.sr_gram()[0].shape == (48, 48)


# ---- training ----------------------------------------------------------------------------------------------------------------

def test_minsr_training_lowers_the_tfim_energy_and_beats_adam():
    from rnnwavefunctions_amd import training
    N, units, ns, steps, seed = 8, 10, 200, 60, 111
    e0 = np.linalg.eigvalsh(ed.tfim_hamiltonian(np.ones(N), 1.0, N))[0]
    prm = P.init_gru_params([units], seed=seed)
    wf = make_wf(N, units, False)
    mean, var = sr.train_tfim(wf, np.ones(N), 1.0, prm, numsteps=steps, numsamples=ns, learningrate=SR_LR, diag_shift=SR_SHIFT, seed=seed)
    assert len(mean) == len(var) == steps + 1
    err_i, err_f = np.sqrt(var[0] / ns), np.sqrt(var[-1] / ns)
    adam, _ = training.run_1DTFIM(numsteps=steps, systemsize=N, num_units=units, Bx=1, numsamples=ns, learningrate=5e-3, seed=seed,
                                  verbose=False)
    print("minSR: E %.4f +- %.4f -> %.4f +- %.4f, Adam -> %.4f, ground state %.4f" % (mean[0], err_i, mean[-1], err_f, adam[-1], e0))
    assert adam[0] == mean[0]                                # the same start: same parameters, same samples
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_i, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
    assert mean[-1] < adam[-1]

