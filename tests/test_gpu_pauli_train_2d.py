"""GPU tests of device-resident Adam training of the 2D RNN on Pauli-string Hamiltonians (rnnwf_pauli_train_steps_2d,
csrc/mdrnn_pauli.hip: MdPauliTrain, csrc/pauli_driver.h: pauli_train_steps, csrc/pauli_train_kernels.h; docs/pauli_train.md, "2D RNN").

The criterion is the host loop's trajectory bit for bit (np.array_equal), the standard rnnwf_train_steps, rnnwf_sr_train_steps and
rnnwf_pauli_train_steps meet: the host loop is pauli_step_2d -> cost_gradient -> training.Adam -> set_params.  No tolerance appears in
this file; pauli_step_2d itself is tied to the float64 oracle by tests/test_gpu_pauli_2d*.py.  The statistical criteria of the last
test are those of tests/test_gpu_pauli.py: test_minimize_hamiltonian_lowers_the_energy_towards_the_ground_state.
"""
import re

import numpy as np
import pytest

import pauli_reference as PR
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_2d as O2
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
ENTRY = "rnnwf_pauli_train_steps_2d"
NS, K = 37, 4                   # ragged 16-chain blocks; four iterations
LRS = [5e-3, 2e-2, 1e-3, 7e-3]
HEAD = SCOPE + "/wf_dense/kernel"


def weights(H, seed=5):
    return P.randomize_biases(P.scale_kernels(P.init_mdrnn_params(H, seed=seed), 2.0), seed + 1)


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def last_visited(Nx, Ny):
    """the lattice index of the site at position N - 1 of the zig-zag path: row Ny - 1, run forwards if Ny - 1 is even"""
    return O2.site(Nx, Ny, Nx - 1 if (Ny - 1) % 2 == 0 else 0, Ny - 1)


def hamiltonian(name, Nx, Ny):
    N = Nx * Ny
    xxz = O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5)
    zz = [t for t in O2.tfim_hamiltonian(1.0 + 0.1 * np.arange(N).reshape(Nx, Ny), 1.0).terms if t[1][0][0] == "Z"]
    if name == "xxz":                                  # pair masks, XX and YY of a bond share one; vertical bonds lie apart on the path
        return xxz
    if name == "tfim":                                 # single-site masks, path position 0 among them; site-dependent couplings and
        return O.Hamiltonian(N, zz + [(-(0.5 + 0.07 * k), [("X", k)]) for k in range(N)])      # fields: lattice != path order shows
    if name == "diagonal":                             # no flip mask at all: M = 0, no tail launch
        return O.Hamiltonian(N, zz + [(0.3, [("Z", k)]) for k in range(N)])
    if name == "mixed":                                # a three-site string, a long-range XX between the first and last lattice site,
        return O.Hamiltonian(N, xxz.terms + [(0.4, [("X", 0), ("Z", 1), ("X", 2)]), (-0.3, [("X", 0), ("X", N - 1)]),
                                             (0.25, [("X", last_visited(Nx, Ny))])])       # and f = N - 1: the head alone
    raise KeyError(name)


def host_loop(wf, ham, prm, ns, seed, lrs, step0=0):
    """the host loop: (moments (K, 4), term sums (K, nterms, 2), parameters, the optimizer)"""
    opt = T.Adam()
    params = {k: np.array(v) for k, v in prm.items()}
    wf.set_params(params, scope=SCOPE)
    moms, sums = [], []
    for k, lr in enumerate(lrs):
        out = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, seed=seed, step=step0 + k)
        s1, s2, n, si = out["moments"]
        moms.append(out["moments"].copy())
        sums.append(out["term_sums"].copy())
        grads = T.cost_gradient(wf, params, SCOPE, s1 / n, n)
        params = opt.step(params, grads, lr)
        wf.set_params(params, scope=SCOPE)
    return np.array(moms), np.array(sums), params, opt


def assert_state_equals(wf, prm_like, params, opt):
    got = wf.get_params_dict(prm_like, SCOPE)
    for k in params:
        assert got[k].dtype == params[k].dtype and np.array_equal(got[k], params[k]), k
    m, v, t = wf.adam_get_state()
    m0, v0 = opt.to_flat(wf, params, SCOPE)
    assert t == opt.t and np.array_equal(m, m0) and np.array_equal(v, v0)


def reset(wf, prm):
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)


# (Nx, Ny, units): 3x2 at one width of every row of the 2D family's shape table (<= 20, 36, 52, 68, 84 units) and at 20 units, which
# fill the mixed tile; 3x4: an odd row runs reversed and vertical neighbours lie apart on the path; 5x7: 35 sites, two spin words
SHAPES = [(3, 2, 10), (3, 2, 36), (3, 2, 50), (3, 2, 68), (3, 2, 84), (3, 2, 20), (3, 4, 10), (5, 7, 10)]
CASES = [s + ("xxz",) for s in SHAPES] + [(3, 2, 10, h) for h in ("tfim", "diagonal", "mixed")] + \
        [(3, 4, 10, h) for h in ("tfim", "mixed")] + [(5, 7, 10, "mixed")]


@pytest.fixture(scope="module")
def trajectories():
    """the host loop's trajectory of every case, computed once: {case: (prm, moments, sums, params, opt)}"""
    cache = {}

    def get(case, lrs=tuple(LRS)):
        if (case, lrs) not in cache:
            Nx, Ny, H, name = case
            prm = weights(H)
            wf = make_wf(Nx, Ny, H, prm)
            cache[case, lrs] = (prm,) + host_loop(wf, hamiltonian(name, Nx, Ny), prm, NS, 11, lrs)
            wf.close()
        return cache[case, lrs]
    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_trajectory_equals_the_host_loop_bit_for_bit(case, trajectories):
    Nx, Ny, H, name = case
    prm, moms, sums, params, opt = trajectories(case)
    ham = hamiltonian(name, Nx, Ny)
    wf = make_wf(Nx, Ny, H, prm)
    out = wf.pauli_train_steps_2d(ham.flip, ham.sign, ham.coeff, NS, 11, 0, LRS, want_term_sums=True)
    assert np.all(np.isfinite(moms)) and moms[:, 1].min() > 0.0 and not np.array_equal(moms[0], moms[-1])
    assert np.array_equal(out["moments"], moms)
    assert out["term_sums"].shape == (K, len(ham.coeff), 2) and np.array_equal(out["term_sums"], sums)
    assert wf.resident_samples() == 0
    assert_state_equals(wf, prm, params, opt)
    # masks given as (nterms, Nx, Ny), and without the per-term sums: not a bit of the moments or of the state changes, and the
    # per-term kernels are not launched
    reset(wf, prm)
    wf.timing_enable(True)
    wf.timing_reset()
    mom = wf.pauli_train_steps_2d(ham.flip.reshape(-1, Nx, Ny), ham.sign.reshape(-1, Nx, Ny), ham.coeff, NS, 11, 0, LRS)
    without = wf.timing_get(2)["launches"]
    assert isinstance(mom, np.ndarray) and np.array_equal(mom, moms)
    assert_state_equals(wf, prm, params, opt)
    nmasks = len({r.tobytes() for r in ham.flip if r.any()})
    assert (nmasks == 0) == (name == "diagonal")
    assert without == K * (3 if nmasks else 2)                # ratios (where a term flips), E_loc, moments
    assert (wf.timing_get(1)["launches"] == 0) == (nmasks == 0)        # a diagonal Hamiltonian launches no tail pass
    reset(wf, prm)
    wf.timing_reset()
    wf.pauli_train_steps_2d(ham.flip, ham.sign, ham.coeff, NS, 11, 0, LRS, want_term_sums=True)
    assert wf.timing_get(2)["launches"] == without + K         # one timed group (term kernel + reduction) per iteration


def test_chunks_single_calls_and_a_second_call(trajectories):
    case = (3, 4, 10, "xxz")
    Nx, Ny, H, name = case
    prm, moms, sums, params, opt = trajectories(case)
    ham = hamiltonian(name, Nx, Ny)
    args = (ham.flip, ham.sign, ham.coeff)
    wf = make_wf(Nx, Ny, H, prm)
    # four calls of one iteration with step0 = 0..3 and the rates of LRS: the call of four
    rows = [wf.pauli_train_steps_2d(*args, NS, 11, k, [LRS[k]], want_term_sums=True) for k in range(K)]
    assert np.array_equal(np.array([r["moments"][0] for r in rows]), moms)
    assert np.array_equal(np.array([r["term_sums"][0] for r in rows]), sums)
    assert_state_equals(wf, prm, params, opt)
    # a second call continues Adam's count: two calls of four = the host loop of eight; between them the next pauli_step_2d runs on
    # the trained parameters and gives the host loop's next step
    _, moms8, sums8, params8, opt8 = trajectories(case, tuple(LRS + LRS))
    assert np.array_equal(moms8[:K], moms)
    reset(wf, prm)
    first = wf.pauli_train_steps_2d(*args, NS, 11, 0, LRS)
    assert wf.adam_get_state()[2] == K and wf.resident_samples() == 0
    nxt = wf.pauli_step_2d(*args, NS, seed=11, step=K)
    assert wf.resident_samples() == NS
    assert np.array_equal(nxt["moments"], moms8[K]) and np.array_equal(nxt["term_sums"], sums8[K])
    second = wf.pauli_train_steps_2d(*args, NS, 11, K, LRS, want_term_sums=True)
    assert np.array_equal(np.concatenate([first, second["moments"]]), moms8) and np.array_equal(second["term_sums"], sums8[K:])
    assert wf.adam_get_state()[2] == 2 * K == opt8.t
    assert_state_equals(wf, prm, params8, opt8)
    # minimize_hamiltonian(device_steps=3) over four iterations at a constant rate: one call of four
    reset(wf, prm)
    one = wf.pauli_train_steps_2d(*args, NS, 111, 0, [1e-2] * K)
    p_one = wf.get_params_dict(prm, SCOPE)
    mean, var = O2.minimize_hamiltonian(wf, ham, prm, numsteps=K - 1, numsamples=NS, learningrate=1e-2, seed=111, device_steps=3)
    assert mean == [r[0] / r[2] for r in one] and var == [r[1] / r[2] - (r[0] / r[2]) ** 2 for r in one]
    assert all(np.array_equal(O2.minimize_hamiltonian.last_params[k], p_one[k]) for k in prm)


@pytest.mark.parametrize("Nx,Ny,H,name,sharpen", [(3, 4, 10, "mixed", 1.0), (5, 7, 50, "xxz", 1.0), (3, 2, 84, "tfim", 1.0),
                                                  (3, 4, 10, "mixed", 60.0), (3, 2, 20, "xxz", 200.0)])
def test_eloc_of_the_table_reading_kernels(Nx, Ny, H, name, sharpen):
    """One iteration (K = 1) on the batch of (seed, step): E_loc, moments and per-term sums of the ratio-table kernels against
    pauli_step_2d's on the same batch, element for element.  sharpen: the head's kernel scaled so that the ratios span hundreds of
    orders of magnitude and some underflow to 0 (asserted).  300 chains: two blocks of the 256-chain assembly kernels, the second
    ragged."""
    ns = 300
    prm = weights(H)
    if sharpen != 1.0:
        prm[HEAD] = (prm[HEAD] * sharpen).astype(prm[HEAD].dtype)
    ham = hamiltonian(name, Nx, Ny)
    wf = make_wf(Nx, Ny, H, prm)
    ref = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, seed=3, step=7, want_eloc=True, want_log_ratio=True)
    out = wf.pauli_train_steps_2d(ham.flip, ham.sign, ham.coeff, ns, 3, 7, [0.0], want_term_sums=True, want_eloc=True)
    lr = ref["log_ratio"]
    print("%dx%d H=%d %s x%g: log r in [%.1f, %.1f]" % (Nx, Ny, H, name, sharpen, lr.min(), lr.max()))
    if sharpen != 1.0:
        assert lr.min() < -750.0 and lr.max() > -700.0                          # exp underflows to 0 for some, not for all
    else:
        assert np.abs(lr).max() > 0.5                                           # the ratios are not all near 1
    assert out["eloc"].dtype == ref["eloc"].dtype == np.float64 and out["eloc"].shape == (ns,)
    assert np.array_equal(out["eloc"], ref["eloc"], equal_nan=True)
    assert np.array_equal(out["moments"][0], ref["moments"], equal_nan=True)
    assert np.array_equal(out["term_sums"][0], ref["term_sums"], equal_nan=True)
    if sharpen == 1.0:                                                          # lr = 0: the parameters did not move
        got = wf.get_params_dict(prm, SCOPE)
        assert all(np.array_equal(got[k], prm[k]) for k in prm) and wf.adam_get_state()[2] == 1


def snapshot(wf, prm):
    return wf.resident_samples(), wf.get_params_dict(prm, SCOPE), wf.adam_get_state()


def same(a, b):
    return a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1]) and a[2][2] == b[2][2] and \
        np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])


def test_refusals_leave_everything_untouched(monkeypatch):
    from rnnwavefunctions_amd import _lib
    Nx, Ny, H = 3, 2, 10
    N = Nx * Ny
    prm = weights(H)
    ham = hamiltonian("xxz", Nx, Ny)
    wf = make_wf(Nx, Ny, H, prm)
    train = wf.pauli_train_steps_2d
    args = (ham.flip, ham.sign, ham.coeff)
    train(*args, NS, 1, 0, [1e-2, 1e-2])                                        # Adam's state is not trivial
    m = wf.pauli_step_2d(*args, NS, seed=1, step=2)["moments"]                  # a resident batch
    trained = wf.get_params_dict(prm, SCOPE)
    g0 = T.cost_gradient(wf, trained, SCOPE, m[0] / m[2], m[2])
    before = snapshot(wf, prm)
    assert before[0] == NS and before[2][2] == 2
    for call, word in [(lambda: train(*args, NS, 1, 0, []), "K must be"), (lambda: train(*args, NS, 1, 0, [1e-2] * 1025), "K must be"),
                       (lambda: train(*args, 0, 1, 0, [1e-2]), "numsamples"), (lambda: train(*args, NS, 1, 0, [1e-2, np.nan]), "finite"),
                       (lambda: train(*args, NS, 1, 0, [np.inf]), "finite"), (lambda: train(*args, NS, 1, 0, [1e-2], sample_offset=-1), "sample_offset")]:
        with pytest.raises(ValueError, match=ENTRY + ": .*" + word):
            call()
        assert same(snapshot(wf, prm), before)
    I32P, F64P = _lib._I32P, _lib._F64P
    mom = np.zeros((1, 4))
    lr = np.array([1e-2])
    fl, sg = np.ascontiguousarray(ham.flip, dtype=np.int32), np.ascontiguousarray(ham.sign, dtype=np.int32)
    co = np.ascontiguousarray(ham.coeff, dtype=np.float64)
    full = [fl.ctypes.data_as(I32P), sg.ctypes.data_as(I32P), co.ctypes.data_as(F64P), len(fl), 1, NS, 1, 0, 0, lr.ctypes.data_as(F64P),
            0.9, 0.999, 1e-8, mom.ctypes.data_as(F64P), None, None]
    bad_f, bad_s = fl.copy(), sg.copy()
    bad_f[0, 4] = 2                                                             # named by the lattice index (position 3 of the path)
    bad_s[1, 5] = -1
    for idx, value, word in [(0, None, "non-null"), (1, None, "non-null"), (2, None, "non-null"), (9, None, "non-null"), (13, None, "non-null"),
                             (3, 0, "nterms"), (0, bad_f.ctypes.data_as(I32P), r"flip\[0\]\[4\] = 2"),
                             (1, bad_s.ctypes.data_as(I32P), r"sign\[1\]\[5\] = -1")]:
        a = list(full)
        a[idx] = value
        assert wf.lib.rnnwf_pauli_train_steps_2d(wf.h, *a) == -1
        msg = wf.lib.rnnwf_last_error(wf.h).decode()
        assert msg.startswith(ENTRY + ": ") and re.search(word, msg), msg
        assert same(snapshot(wf, prm), before)
    # the batch of the refused calls' predecessor is still the gradient's, and the gradient is the one it gave before
    assert wf.resident_samples() == NS
    g1 = T.cost_gradient(wf, trained, SCOPE, m[0] / m[2], m[2])
    assert all(np.array_equal(g0[k], g1[k]) for k in g0) and same(snapshot(wf, prm), before)
    # more than 65 535 distinct non-empty flip masks (17 sites carry 2^16 of them)
    big = make_wf(5, 4, H, prm)
    many = ((np.arange(1, 65537)[:, None] >> np.arange(20)[None, :]) & 1).astype(np.int32)
    with pytest.raises(ValueError, match=ENTRY + ": .*65535 distinct"):
        big.pauli_train_steps_2d(many, np.zeros_like(many), np.ones(len(many)), NS, 1, 0, [1e-2])
    assert big.resident_samples() == 0 and big.adam_get_state()[2] == 0
    # a handle with a communicator
    wc = make_wf(Nx, Ny, H, prm)
    wc.comm_init(wc.comm_unique_id(), 0, 1)
    with pytest.raises(ValueError, match=ENTRY + ": .*communicator"):
        wc.pauli_train_steps_2d(*args, NS, 1, 0, [1e-2])
    # more samples than one pass holds
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    small = make_wf(Nx, Ny, H, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    with pytest.raises(_lib.RnnwfError, match=ENTRY + ": .*split the batch"):
        small.pauli_train_steps_2d(*args, 200000, 1, 0, [1e-2])
    assert small.resident_samples() == 0 and all(np.array_equal(small.get_params_dict(prm, SCOPE)[k], prm[k]) for k in prm)
    # every other model, by name, with a pointer to the entries that serve it
    for model, nx, ny, name in [(_lib.MODEL_GRU1D, N, 1, "GRU1D"), (_lib.MODEL_CRNN_U1, N, 1, "CRNN_U1"), (_lib.MODEL_GRU1D_PARITY, N, 1, "GRU1D_PARITY"),
                                (_lib.MODEL_LSTM1D_F64, Nx, Ny, "LSTM1D_F64"), (_lib.MODEL_GRU1D_F64, Nx, Ny, "GRU1D_F64")]:
        w = _lib.NativeWavefunction(model, nx, ny, (H,))
        w.init_params(1)
        with pytest.raises(ValueError, match=ENTRY + r": .*model is %s; rnnwf_pauli_train_steps serves .*rnnwf_pauli_train_steps_complex" % name):
            w.pauli_train_steps_2d(*args, NS, 1, 0, [1e-2])
        assert w.resident_samples() == 0
    # the older entries keep refusing the 2D RNN
    with pytest.raises(ValueError, match="rnnwf_pauli_train_steps: .*2D RNN"):
        wf.pauli_train_steps(*args, NS, 1, 0, [1e-2])
    with pytest.raises(ValueError, match="rnnwf_pauli_train_steps_complex: "):
        wf.pauli_train_steps_complex(*args, NS, 1, 0, [1e-2])
    assert same(snapshot(wf, prm), before)
    # uncommitted parameters
    fresh = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    with pytest.raises(_lib.RnnwfError, match="not committed") as e:
        fresh.pauli_train_steps_2d(*args, NS, 1, 0, [1e-2])
    assert not isinstance(e.value, ValueError)                                  # RNNWF_ERR_STATE, as for the other two train entries


def test_state_rules_after_a_successful_call():
    Nx, Ny, H = 3, 4, 20
    prm = weights(H)
    ham = hamiltonian("mixed", Nx, Ny)
    args = (ham.flip, ham.sign, ham.coeff)
    wf = make_wf(Nx, Ny, H, prm)
    wf.pauli_step_2d(*args, NS, seed=1, step=9)                                 # a resident batch from before
    wf.pauli_train_steps_2d(*args, NS, 1, 0, [1e-2, 1e-2])
    assert wf.resident_samples() == 0                                           # the last batch belongs to the weights before the last update
    with pytest.raises(Exception, match="resident|no batch|vmc_step"):
        wf.vmc_gradient(0.0, NS, {k[len(SCOPE) + 1:]: v.shape for k, v in prm.items()})
    trained = wf.get_params_dict(prm, SCOPE)
    assert any(not np.array_equal(trained[k], prm[k]) for k in prm) and all(trained[k].dtype == prm[k].dtype for k in prm)
    on_device = wf.pauli_step_2d(*args, NS, seed=1, step=2)                     # runs on the device's parameters
    assert wf.resident_samples() == NS
    again = make_wf(Nx, Ny, H, trained)
    ref = again.pauli_step_2d(*args, NS, seed=1, step=2)
    assert np.array_equal(ref["moments"], on_device["moments"]) and np.array_equal(ref["term_sums"], on_device["term_sums"])
    # Adam's state carries across calls and through rnnwf_adam_get_state / rnnwf_adam_set_state to a fresh handle
    m, v, t = wf.adam_get_state()
    assert t == 2 and np.abs(m).max() > 0.0
    a = wf.pauli_train_steps_2d(*args, NS, 1, 2, [1e-2, 5e-3])
    again.adam_set_state(m, v, t)
    assert np.array_equal(again.pauli_train_steps_2d(*args, NS, 1, 2, [1e-2, 5e-3]), a)
    assert same(snapshot(again, prm), snapshot(wf, prm)) and wf.adam_get_state()[2] == 4


def test_minimize_hamiltonian_lowers_the_energy_and_device_steps_equals_the_host_loop():
    """3x3 XXZ (ferromagnetic XY coupling) in a transverse field: stoquastic, so the ground state is positive.  The criteria are those
    of tests/test_gpu_pauli.py's chain test; e0 from the dense 512 x 512 matrix."""
    Nx, Ny, H, ns, steps = 3, 3, 20, 1000, 300
    N = Nx * Ny
    ham = O.Hamiltonian(N, O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5).terms + [(-0.8, [("X", i)]) for i in range(N)])
    Hd = sum(c * PR.dense_string({i: p for p, i in st}, N).real for c, st in ham.terms)
    assert Hd.shape == (512, 512) and np.allclose(Hd, Hd.T)
    e0 = np.linalg.eigvalsh(Hd)[0]
    prm = P.init_mdrnn_params(H, seed=111)
    wf = make_wf(Nx, Ny, H, prm)
    mean, var = O2.minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111)
    p_h = O2.minimize_hamiltonian.last_params
    assert len(mean) == len(var) == steps + 1
    err_i, err_f = np.sqrt(var[0] / ns), np.sqrt(var[-1] / ns)
    print("minimize_hamiltonian 2D: E %.4f +- %.4f -> %.4f +- %.4f, ground state %.4f" % (mean[0], err_i, mean[-1], err_f, e0))
    assert mean[-1] < mean[0] - 5.0 * np.hypot(err_i, err_f)
    assert mean[-1] >= e0 - 5.0 * err_f
    mean_d, var_d = O2.minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111, device_steps=16)
    p_d = O2.minimize_hamiltonian.last_params
    assert len(mean_d) == steps + 1 and mean_d == mean and var_d == var
    assert all(np.array_equal(p_d[k], p_h[k]) and p_d[k].dtype == p_h[k].dtype for k in p_h)
