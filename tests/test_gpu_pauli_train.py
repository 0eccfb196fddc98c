"""GPU tests of device-resident Adam training on Pauli-string Hamiltonians (rnnwf_pauli_train_steps,
rnnwf_pauli_train_steps_complex, csrc/pauli_driver.h: pauli_train_steps, csrc/pauli_train_kernels.h,
csrc/crnn_pauli_train_kernels.h; docs/pauli_train.md).

The criterion is the host loop's trajectory bit for bit (np.array_equal), the standard rnnwf_train_steps and rnnwf_sr_train_steps
meet: the host loop is pauli_step* -> cost_gradient -> training.Adam -> set_params.  No tolerance appears in this file.

The +inf branch of the ratio (log r > 709) needs a sampled configuration with P(sigma) < e^-1418, which the device's sampler never
draws; the entries take no caller-supplied samples.  test_eloc_of_the_table_reading_kernels covers the widest ratios sharpened
weights reach (underflow to 0 included); both paths call the same exp on the same argument.
"""
import re

import numpy as np
import pytest

import crnn_pauli_reference as CR
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
NS, K = 37, 4                   # ragged 16-chain blocks; four iterations
LRS = [5e-3, 2e-2, 1e-3, 7e-3]


def weights(H, f64=False, cplx=False, seed=5):
    prm = P.init_gru_params([H], seed=seed, heads=CR.HEADS) if cplx else P.init_gru_params([H], seed=seed, dtype=np.float64 if f64 else np.float32)
    return P.randomize_biases(P.scale_kernels(prm, 2.0), seed + 1)


def make_wf(kind, Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    model = {"f32": _lib.MODEL_GRU1D, "f64": _lib.MODEL_GRU1D_F64, "cplx": _lib.MODEL_CRNN_U1}[kind]
    wf = _lib.NativeWavefunction(model, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def hamiltonian(name, N):
    xxz = O.xxz_hamiltonian(N, -1.0, 0.5)
    if name == "xxz":                                  # pair masks; XX and YY of a bond share one
        return xxz
    if name == "tfim":                                 # single-site masks, the mask at site 0 (first = 0) among them
        return O.tfim_hamiltonian(1.0 + 0.1 * np.arange(N), 0.8)
    if name == "diagonal":                             # no flip mask at all: M = 0
        return O.Hamiltonian(N, [(-1.0, [("Z", i), ("Z", i + 1)]) for i in range(N - 1)] + [(0.3, [("Z", i)]) for i in range(N)])
    if name == "mixed":                                # a three-site string and a long-range XX term
        return O.Hamiltonian(N, xxz.terms + [(0.4, [("X", 0), ("Z", 1), ("X", 2)]), (-0.3, [("X", 1), ("X", N - 1)])])
    if name == "heisenberg":                           # complex: XX, YY (flips that leave the sector give exact zeros), ZZ, a field,
        heis = OC.j1j2_hamiltonian(np.ones(N), 0.3 * np.ones(N), 0.1 * np.arange(N))        # and one complex coefficient
        return OC.ComplexHamiltonian(N, heis.terms + [(0.2 + 0.1j, [("X", 0), ("Y", 3)]), (0.05, [("X", 2)])])
    raise KeyError(name)


def steps_of(wf, kind):
    return (wf.pauli_step_complex, wf.pauli_train_steps_complex) if kind == "cplx" else (wf.pauli_step, wf.pauli_train_steps)


def host_loop(wf, kind, ham, prm, ns, seed, lrs, step0=0):
    """today's loop: (moments (K, 4), term sums (K, nterms, 2 or 4), parameters, the optimizer)"""
    step, _ = steps_of(wf, kind)
    opt = T.Adam()
    params = {k: np.array(v) for k, v in prm.items()}
    wf.set_params(params, scope=SCOPE)
    moms, sums = [], []
    for k, lr in enumerate(lrs):
        out = step(ham.flip, ham.sign, ham.coeff, ns, seed=seed, step=step0 + k)
        s1, s2, n, si = out["moments"]
        moms.append(out["moments"].copy())
        sums.append(out["term_sums"].copy())
        grads = T.cost_gradient(wf, params, SCOPE, complex(s1 / n, si / n) if kind == "cplx" else s1 / n, n)
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


# (kind, Nx, Ny, units): NFULL 1, 3, 4 in float32; the float64 raster model at 10 and 53 units (the 4-wave row); two spin words; the
# complex model at NFULL 1, 3 and 4
SHAPES = [("f32", 6, 1, 10), ("f32", 6, 1, 37), ("f32", 6, 1, 68), ("f64", 3, 2, 10), ("f64", 3, 2, 53), ("f32", 34, 1, 10),
          ("cplx", 6, 1, 10), ("cplx", 6, 1, 37), ("cplx", 8, 1, 53)]
CASES = [s + (("heisenberg",) if s[0] == "cplx" else ("xxz",)) for s in SHAPES] + \
        [("f32", 6, 1, 10, h) for h in ("tfim", "diagonal", "mixed")] + [("f64", 3, 2, 10, "tfim"), ("f32", 34, 1, 10, "mixed")]


@pytest.fixture(scope="module")
def trajectories():
    """the host loop's trajectory of every case, computed once: {case: (prm, moments, sums, params, opt)}"""
    cache = {}

    def get(case):
        if case not in cache:
            kind, Nx, Ny, H, name = case
            prm = weights(H, f64=kind == "f64", cplx=kind == "cplx")
            wf = make_wf(kind, Nx, Ny, H, prm)
            cache[case] = (prm,) + host_loop(wf, kind, hamiltonian(name, Nx * Ny), prm, NS, 11, LRS)
            wf.close()
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_trajectory_equals_the_host_loop_bit_for_bit(case, trajectories):
    kind, Nx, Ny, H, name = case
    prm, moms, sums, params, opt = trajectories(case)
    ham = hamiltonian(name, Nx * Ny)
    wf = make_wf(kind, Nx, Ny, H, prm)
    _, train = steps_of(wf, kind)
    out = train(ham.flip, ham.sign, ham.coeff, NS, 11, 0, LRS, want_term_sums=True)
    assert np.all(np.isfinite(moms)) and moms[:, 1].min() > 0.0 and not np.array_equal(moms[0], moms[-1])
    assert np.array_equal(out["moments"], moms)
    assert np.array_equal(out["term_sums"], sums)
    assert wf.resident_samples() == 0
    assert_state_equals(wf, prm, params, opt)
    # without the per-term sums: not a bit of the moments or of the state changes, and the per-term kernels are not launched
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)
    wf.timing_enable(True)
    wf.timing_reset()
    mom = train(ham.flip, ham.sign, ham.coeff, NS, 11, 0, LRS)
    without = wf.timing_get(2)["launches"]
    assert isinstance(mom, np.ndarray) and np.array_equal(mom, moms)
    assert_state_equals(wf, prm, params, opt)
    nmasks = len({r.tobytes() for r in ham.flip if r.any()})
    assert without == K * (3 if nmasks else 2)                # ratios (where a term flips), E_loc, moments
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)
    wf.timing_reset()
    train(ham.flip, ham.sign, ham.coeff, NS, 11, 0, LRS, want_term_sums=True)
    assert wf.timing_get(2)["launches"] == without + K         # one timed group (term kernel + reduction) per iteration


@pytest.mark.parametrize("case", [("f32", 6, 1, 10, "xxz"), ("cplx", 6, 1, 10, "heisenberg")], ids=lambda c: c[0])
def test_chunks_single_calls_and_per_iteration_rates(case, trajectories):
    kind, Nx, Ny, H, name = case
    prm, moms, _, params, opt = trajectories(case)
    ham = hamiltonian(name, Nx * Ny)
    wf = make_wf(kind, Nx, Ny, H, prm)
    _, train = steps_of(wf, kind)
    # four calls of one iteration with the rates of LRS: the call of four
    rows = [train(ham.flip, ham.sign, ham.coeff, NS, 11, k, [LRS[k]])[0] for k in range(K)]
    assert np.array_equal(np.array(rows), moms)
    assert_state_equals(wf, prm, params, opt)
    # a constant rate: one call of four = four single calls = minimize_hamiltonian(device_steps=2) over four iterations
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)
    one = train(ham.flip, ham.sign, ham.coeff, NS, 111, 0, [1e-2] * K)
    p_one, a_one = wf.get_params_dict(prm, SCOPE), wf.adam_get_state()
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)
    single = np.array([train(ham.flip, ham.sign, ham.coeff, NS, 111, k, [1e-2])[0] for k in range(K)])
    p_single, a_single = wf.get_params_dict(prm, SCOPE), wf.adam_get_state()
    assert np.array_equal(one, single) and a_one[2] == a_single[2] == K
    assert all(np.array_equal(p_one[k], p_single[k]) for k in prm) and all(np.array_equal(a, b) for a, b in zip(a_one[:2], a_single[:2]))
    if kind == "cplx":
        mean, var = OC.minimize_hamiltonian(wf, ham, NS, K - 1, 1e-2, params=prm, seed=111, scope=SCOPE, device_steps=2)
        last = OC.minimize_hamiltonian.last_params
        assert mean == [complex(r[0] / r[2], r[3] / r[2]) for r in one]
    else:
        mean, var = T.minimize_hamiltonian(wf, ham, prm, numsteps=K - 1, numsamples=NS, learningrate=1e-2, seed=111, device_steps=2)
        last = T.minimize_hamiltonian.last_params
        assert mean == [r[0] / r[2] for r in one]
    assert var == [r[1] / r[2] - (r[0] / r[2]) ** 2 for r in one]
    assert all(np.array_equal(last[k], p_one[k]) for k in prm)


@pytest.mark.parametrize("kind,Nx,Ny,H,name,sharpen", [("f32", 6, 1, 10, "mixed", 1.0), ("f32", 34, 1, 37, "xxz", 1.0), ("f64", 3, 2, 53, "tfim", 1.0),
                                                       ("f32", 6, 1, 10, "mixed", 2000.0), ("f64", 3, 2, 10, "xxz", 2000.0),
                                                       ("cplx", 6, 1, 10, "heisenberg", 1.0), ("cplx", 8, 1, 53, "heisenberg", 1.0)])
def test_eloc_of_the_table_reading_kernels(kind, Nx, Ny, H, name, sharpen):
    """One iteration with lr = 0 on the batch of (seed, step): E_loc, moments and per-term sums of the ratio-table kernels against
    pauli_step*'s on the same batch, bit for bit.  sharpen: the head's kernel scaled so that the ratios span hundreds of orders of
    magnitude and underflow to 0.  300 chains: two blocks of the 256-chain assembly kernels, the second ragged."""
    ns = 300
    prm = weights(H, f64=kind == "f64", cplx=kind == "cplx")
    if sharpen != 1.0:
        prm["RNNwavefunction/wf_dense/kernel"] = (prm["RNNwavefunction/wf_dense/kernel"] * sharpen).astype(prm["RNNwavefunction/wf_dense/kernel"].dtype)
    ham = hamiltonian(name, Nx * Ny)
    wf = make_wf(kind, Nx, Ny, H, prm)
    step, train = steps_of(wf, kind)
    ref = step(ham.flip, ham.sign, ham.coeff, ns, seed=3, step=7, want_eloc=True, want_log_ratio=True)
    out = train(ham.flip, ham.sign, ham.coeff, ns, 3, 7, [0.0], want_term_sums=True, want_eloc=True)
    lr = ref["log_ratio"]
    if kind == "cplx":
        assert np.isneginf(lr.real).any() and np.isfinite(lr.real).any()        # flips that leave the sector: exact zeros
        assert np.abs(ref["eloc"].imag).max() > 0.0
    elif sharpen != 1.0:
        assert lr.min() < -750.0                                                # exp underflows to 0
    else:
        assert np.abs(lr).max() > 0.5                                           # the ratios are not all near 1
    assert out["eloc"].dtype == ref["eloc"].dtype and np.array_equal(out["eloc"], ref["eloc"], equal_nan=True)
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


@pytest.mark.parametrize("kind", ["f32", "cplx"])
def test_refusals_leave_everything_untouched_and_state_rules(kind, monkeypatch):
    from rnnwavefunctions_amd import _lib
    N, H = 6, 10
    entry = "rnnwf_pauli_train_steps_complex" if kind == "cplx" else "rnnwf_pauli_train_steps"
    prm = weights(H, cplx=kind == "cplx")
    ham = hamiltonian("heisenberg" if kind == "cplx" else "xxz", N)
    wf = make_wf(kind, N, 1, H, prm)
    step, train = steps_of(wf, kind)
    train(ham.flip, ham.sign, ham.coeff, NS, 1, 0, [1e-2, 1e-2])                # Adam's state is not trivial
    step(ham.flip, ham.sign, ham.coeff, NS, seed=1, step=2)                     # a resident batch
    before = snapshot(wf, prm)
    assert before[0] == NS and before[2][2] == 2
    args = (ham.flip, ham.sign, ham.coeff)
    for call, word in [(lambda: train(*args, NS, 1, 0, []), "K must be"), (lambda: train(*args, NS, 1, 0, [1e-2] * 1025), "K must be"),
                       (lambda: train(*args, 0, 1, 0, [1e-2]), "numsamples"), (lambda: train(*args, NS, 1, 0, [1e-2, np.nan]), "finite"),
                       (lambda: train(*args, NS, 1, 0, [np.inf]), "finite"), (lambda: train(*args, NS, 1, 0, [1e-2], sample_offset=-1), "sample_offset")]:
        with pytest.raises(ValueError, match=entry + ": .*" + word):
            call()
        assert same(snapshot(wf, prm), before)
    I32P, F64P = _lib._I32P, _lib._F64P
    mom = np.zeros((1, 4))
    lr = np.array([1e-2])
    fl, sg = np.ascontiguousarray(ham.flip, dtype=np.int32), np.ascontiguousarray(ham.sign, dtype=np.int32)
    co = np.ascontiguousarray(ham.coeff, dtype=np.complex128 if kind == "cplx" else np.float64)
    full = [fl.ctypes.data_as(I32P), sg.ctypes.data_as(I32P), co.ctypes.data_as(F64P), len(fl), 1, NS, 1, 0, 0, lr.ctypes.data_as(F64P),
            0.9, 0.999, 1e-8, mom.ctypes.data_as(F64P), None, None]
    bad = fl.copy()
    bad[0, 4] = 2
    for idx, value, word in [(0, None, "non-null"), (1, None, "non-null"), (2, None, "non-null"), (9, None, "non-null"), (13, None, "non-null"),
                             (3, 0, "nterms"), (0, bad.ctypes.data_as(I32P), r"flip\[0\]\[4\] = 2")]:
        a = list(full)
        a[idx] = value
        assert getattr(wf.lib, entry)(wf.h, *a) == -1
        msg = wf.lib.rnnwf_last_error(wf.h).decode()
        assert msg.startswith(entry + ": ") and re.search(word, msg), msg
        assert same(snapshot(wf, prm), before)
    # the batch of the refused calls' predecessor is still the gradient's
    assert wf.resident_samples() == NS
    # a handle with a communicator
    wc = make_wf(kind, N, 1, H, prm)
    wc.comm_init(wc.comm_unique_id(), 0, 1)
    with pytest.raises(ValueError, match=entry + ": .*communicator"):
        steps_of(wc, kind)[1](*args, NS, 1, 0, [1e-2])
    # more samples than one pass holds
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    small = make_wf(kind, N, 1, H, prm)
    monkeypatch.delenv("RNNWF_STATE_BUDGET_MB")
    with pytest.raises(_lib.RnnwfError, match=entry + ": .*split the batch"):
        steps_of(small, kind)[1](*args, 200000, 1, 0, [1e-2])
    assert small.resident_samples() == 0 and all(np.array_equal(small.get_params_dict(prm, SCOPE)[k], prm[k]) for k in prm)
    # the other family's handle, stacked layers and uncommitted parameters
    other = make_wf("f32" if kind == "cplx" else "cplx", N, 1, H, weights(H, cplx=kind != "cplx"))
    with pytest.raises(ValueError, match=entry + ": "):
        getattr(other, "pauli_train_steps_complex" if kind == "cplx" else "pauli_train_steps")(*args, NS, 1, 0, [1e-2])
    with pytest.raises(ValueError, match="rnnwf_pauli_step"):                    # the older entries keep refusing what they refuse
        (other.pauli_step_complex if kind == "cplx" else other.pauli_step)(*args, NS)
    stack = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1 if kind == "cplx" else _lib.MODEL_GRU1D, N, 1, (H, H))
    stack.init_params(1)
    with pytest.raises(ValueError, match=entry + ": .*stacked"):
        steps_of(stack, kind)[1](*args, NS, 1, 0, [1e-2])
    fresh = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1 if kind == "cplx" else _lib.MODEL_GRU1D, N, 1, (H,))
    with pytest.raises(_lib.RnnwfError, match="not committed"):
        steps_of(fresh, kind)[1](*args, NS, 1, 0, [1e-2])
    # after a successful call: no resident batch, get_params returns the device's values, the next step runs on the new weights
    wf.set_params(prm, scope=SCOPE)
    wf.adam_set_state(None, None, 0)
    train(*args, NS, 1, 0, [1e-2, 1e-2])
    assert wf.resident_samples() == 0
    trained = wf.get_params_dict(prm, SCOPE)
    assert any(not np.array_equal(trained[k], prm[k]) for k in prm)
    on_device = step(*args, NS, seed=1, step=2)["moments"]
    assert wf.resident_samples() == NS
    again = make_wf(kind, N, 1, H, trained)
    assert np.array_equal(steps_of(again, kind)[0](*args, NS, seed=1, step=2)["moments"], on_device)
    # Adam's state carries across calls and through rnnwf_adam_get_state / rnnwf_adam_set_state
    m, v, t = wf.adam_get_state()
    assert t == 2
    a = train(*args, NS, 1, 2, [1e-2])
    again.adam_set_state(m, v, t)
    assert np.array_equal(steps_of(again, kind)[1](*args, NS, 1, 2, [1e-2]), a)
    assert same(snapshot(again, prm), snapshot(wf, prm))


def test_training_end_to_end_equals_the_host_loop_real():
    """the configuration of tests/test_gpu_pauli.py: test_minimize_hamiltonian_lowers_the_energy_towards_the_ground_state with
    device_steps=16: the host loop's energies element for element, so that test's criteria hold for this path as they stand"""
    from rnnwavefunctions_amd import _lib
    N, H, ns, steps = 8, 20, 1000, 300
    xxz = O.xxz_hamiltonian(N, -1.0, 0.5)
    ham = O.Hamiltonian(N, xxz.terms + [(-0.8, [("X", i)]) for i in range(N)])
    prm = P.init_gru_params([H], seed=111)
    wf = _lib.NativeWavefunction(_lib.MODEL_GRU1D, N, 1, (H,))
    mean_h, var_h = T.minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111)
    p_h = T.minimize_hamiltonian.last_params
    mean_d, var_d = T.minimize_hamiltonian(wf, ham, prm, numsteps=steps, numsamples=ns, learningrate=5e-3, seed=111, device_steps=16)
    p_d = T.minimize_hamiltonian.last_params
    assert len(mean_d) == steps + 1 and mean_d == mean_h and var_d == var_h
    assert all(np.array_equal(p_d[k], p_h[k]) and p_d[k].dtype == p_h[k].dtype for k in p_h)
    assert mean_h[-1] < mean_h[0]


def test_training_end_to_end_equals_the_host_loop_complex():
    """the antiferromagnetic Heisenberg chain of tests/test_gpu_crnn_pauli.py at 60 steps, through the reference-named facade"""
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.J1J2.ComplexRNNwavefunction import RNNwavefunction
    N, H, ns, steps = 8, 20, 500, 60
    ham = OC.j1j2_hamiltonian(np.ones(N), np.zeros(N), np.zeros(N))
    res = []
    for ds in (None, 16):
        fac = RNNwavefunction(N, cell=tf.contrib.cudnn_rnn.CudnnCompatibleGRUCell, units=[H])
        mean, var = OC.minimize_hamiltonian(fac, ham, ns, steps, 5e-3, seed=111, device_steps=ds)
        last = OC.minimize_hamiltonian.last_params
        after = fac.get_params()
        assert all(np.array_equal(np.asarray(after[k]), last[k]) for k in last)
        res.append((mean, var, last))
    assert len(res[1][0]) == steps + 1 and res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert all(np.array_equal(res[0][2][k], res[1][2][k]) for k in res[0][2])
    assert res[0][0][-1].real < res[0][0][0].real
