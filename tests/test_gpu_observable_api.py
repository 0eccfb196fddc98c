"""GPU test of the shared Python layer (rnnwavefunctions_amd/_observable_api.py) under the four observable modules: on one small wave
function per family, energy, pauli_expectations, correlations (spin_correlations for the complex RNN) and renyi2_regions of the module
equal - `==` on every element - what this file computes from a direct call of the family's NativeWavefunction method with the same
arguments.  The layer adds no arithmetic of its own, so there is no tolerance.  Two iterations of minimize_hamiltonian give the same
energies and parameters with device_steps=None and device_steps=2, bit for bit; all four families have a device entry
(rnnwf_pauli_train_steps, _stack, _2d, _complex), so all four are checked.  The module takes a few seconds."""
import numpy as np
import pytest

from rnnwavefunctions_amd import _lib
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_2d as O2
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd import observables_stack as OS
from rnnwavefunctions_amd import params as P
from rnnwavefunctions_amd import training as T

pytestmark = pytest.mark.gpu

SCOPE = "RNNwavefunction"
N, H, NS, NPAIRS, SEED, STEP = 6, 5, 32, 16, 1234, 3
STRINGS = ["XXIIII", "IZZIII", "YIIIII", "IYIYII", [("X", 1), ("Z", 4)], "ZIXXIZ"]
MASKS = np.array([[1, 1, 0, 0, 0, 0], [0, 0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1]])
PAIRS = [(0, 5), (5, 0), (2, 3)]

# family -> (module, model, (nx, ny), units, parameters, NativeWavefunction methods: step and regions)
FAMILIES = {
    "gru": (O, _lib.MODEL_GRU1D, (N, 1), (H,), lambda: P.init_gru_params([H], seed=11), "pauli_step", "renyi2_regions"),
    "stack": (OS, _lib.MODEL_GRU1D, (N, 1), (H, H), lambda: P.init_gru_params([H, H], seed=11), "pauli_step_stack", "renyi2_regions_stack"),
    "2d": (O2, _lib.MODEL_MDRNN2D, (3, 2), (H,), lambda: P.init_mdrnn_params(H, seed=11), "pauli_step_2d", "renyi2_regions_2d"),
    "complex": (OC, _lib.MODEL_CRNN_U1, (N, 1), (H,), lambda: P.init_gru_params([H], seed=11, heads=("wf_dense_ampl", "wf_dense_phase")),
                "pauli_step_complex", "renyi2_regions_complex"),
}


def make(family):
    mod, model, (nx, ny), units, prm, step, regions = FAMILIES[family]
    prm = prm()
    wf = _lib.NativeWavefunction(model, nx, ny, units)
    wf.set_params(prm, scope=SCOPE)
    return mod, wf, prm, getattr(wf, step), getattr(wf, regions)


def hamiltonian(family):
    if family == "complex":                                # stays in the zero-magnetisation sector
        return OC.j1j2_hamiltonian(np.ones(N), 0.5 * np.ones(N), np.zeros(N))
    return O.Hamiltonian(N, [(-1.0, "ZZIIII"), (-0.5, "IXIIII"), (0.25, "IIYYII"), (-0.75, "IIIXXI"), (0.5, [("Z", 0), ("Z", 5)])])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | ((a != a) & (b != b))))


@pytest.mark.parametrize("family", ["gru", "stack", "2d"])
def test_real_families_equal_the_direct_calls(family):
    mod, wf, _, step, regions = make(family)
    ham = hamiltonian(family)
    got = mod.energy(wf, ham, NS, seed=SEED, step=STEP, want_eloc=True)
    out = step(ham.flip, ham.sign, ham.coeff, NS, seed=SEED, step=STEP, want_eloc=True)
    m = out["moments"]
    mean = m[0] / m[2]
    var = max(m[1] / m[2] - mean * mean, 0.0)
    assert got["mean"] == mean and got["var"] == var and got["err"] == float(np.sqrt(var / m[2])) and same(got["eloc"], out["eloc"])
    assert np.isfinite(mean) and got["eloc"].shape == (NS,)

    got = mod.pauli_expectations(wf, STRINGS, NS, seed=SEED, step=STEP)
    flip, sign, factor = O.pauli_terms(STRINGS, N)
    real = np.flatnonzero(factor.imag == 0.0)
    assert 0 < real.size < len(STRINGS)
    t = step(flip[real], sign[real], np.ones(real.size), NS, seed=SEED, step=STEP)["term_sums"]
    value, err = np.zeros(len(STRINGS)), np.zeros(len(STRINGS))
    mean, err[real] = O.pauli_from_sums(t, NS)
    value[real] = factor.real[real] * mean
    assert same(got["value"], value) and same(got["err"], err) and np.any(value != 0.0)

    got = mod.renyi2_regions(wf, MASKS, NPAIRS, seed=SEED, step=STEP)
    want = O.renyi2_from_sums(regions(MASKS, NPAIRS, seed=SEED, step=STEP)["sums"], NPAIRS)
    assert same(got[0], want[0]) and same(got[1], want[1]) and got[0].shape == (3,)

    if family == "gru":
        got = mod.correlations(wf, NS, seed=SEED, step=STEP)
        c = wf.correlations(NS, seed=SEED, step=STEP)
        want = O.correlations_from_sums(c["z_sums"], c["zz_sums"], c["x_sums"], c["xx_sums"], NS)
        assert sorted(got) == sorted(want) and all(same(got[k], want[k]) for k in want)
        return
    for pairs in (None, PAIRS):
        got = mod.correlations(wf, NS, pairs=pairs, seed=SEED, step=STEP)
        centre = N // 2 if family == "stack" else O2.site(3, 2, 1, 1)
        p = np.array(pairs if pairs is not None else [(centre, k) for k in range(N) if k != centre], dtype=np.int64)
        flip = np.zeros((N + len(p), N), dtype=np.int32)
        flip[np.arange(N), np.arange(N)] = 1
        for k, (a, b) in enumerate(p):
            flip[N + k, [a, b]] = 1
        out = step(flip, np.zeros_like(flip), np.ones(len(flip)), NS, seed=SEED, step=STEP, want_log_ratio=True, want_samples=True)
        r = np.exp(out["log_ratio"])[O.group_by_mask(flip)[1]]
        s = 2.0 * out["samples"].reshape(NS, N).T - 1.0
        a, b = p[:, 0], p[:, 1]
        z, x, zz, xx = s.mean(axis=-1), r[:N].mean(axis=-1), (s[a] * s[b]).mean(axis=-1), r[N:].mean(axis=-1)
        want = {"pairs": p, "z": z, "x": x, "zz": zz, "xx": xx, "zz_c": zz - z[a] * z[b], "xx_c": xx - x[a] * x[b],
                "z_err": s.std(axis=-1) / np.sqrt(NS), "x_err": r[:N].std(axis=-1) / np.sqrt(NS),
                "zz_err": (s[a] * s[b]).std(axis=-1) / np.sqrt(NS), "xx_err": r[N:].std(axis=-1) / np.sqrt(NS),
                "zz_c_err": (s[a] * s[b] - z[b][:, None] * s[a] - z[a][:, None] * s[b]).std(axis=-1) / np.sqrt(NS),
                "xx_c_err": (r[N:] - x[b][:, None] * r[a] - x[a][:, None] * r[b]).std(axis=-1) / np.sqrt(NS)}
        assert sorted(got) == sorted(want) and all(same(got[k], want[k]) for k in want), [k for k in want if not same(got[k], want[k])]


def test_complex_family_equals_the_direct_calls():
    mod, wf, _, step, regions = make("complex")
    ham = hamiltonian("complex")
    assert ham.is_hermitian()
    got = OC.energy(wf, ham, NS, seed=SEED, step=STEP, want_eloc=True)
    out = step(ham.flip, ham.sign, ham.coeff, NS, seed=SEED, step=STEP, want_eloc=True)
    m = out["moments"]
    re = m[0] / m[2]
    var = max(m[1] / m[2] - re * re, 0.0)
    assert got["mean"] == complex(re, m[3] / m[2]) and got["var"] == var and got["err"] == float(np.sqrt(var / m[2]))
    assert same(got["eloc"], out["eloc"]) and out["eloc"].dtype == np.complex64

    got = OC.pauli_expectations(wf, STRINGS, NS, seed=SEED, step=STEP)
    flip, sign, factor = O.pauli_terms(STRINGS, N)
    mean, e_re, e_im = OC._from_sums(step(flip, sign, np.ones(len(factor)), NS, seed=SEED, step=STEP)["term_sums"], NS)
    swap = factor.imag != 0.0
    assert same(got["value"], factor * mean) and same(got["err"], np.where(swap, e_im, e_re)) and same(got["err_imag"], np.where(swap, e_re, e_im))

    got = OC.spin_correlations(wf, NS, seed=SEED, step=STEP)
    pairs, strings = OC.spin_correlation_terms(N)
    flip, sign, factor = O.pauli_terms(strings, N)
    out = step(flip, sign, 0.25 * factor, NS, seed=SEED, step=STEP, want_log_ratio=True, want_samples=True)
    lr = out["log_ratio"]
    with np.errstate(invalid="ignore"):
        r = np.where(np.isneginf(lr.real), 0.0, np.exp(lr))
    s = 2.0 * out["samples"].reshape(NS, N).T - 1.0
    ss = s[pairs[:, 0]] * s[pairs[:, 1]]
    v = 0.25 * ((1.0 - ss) * r[O.group_by_mask(flip)[1][0::3]] + ss)
    assert same(got["corr"][pairs[:, 0], pairs[:, 1]], v.real.mean(axis=1)) and same(got["corr"], got["corr"].T)
    assert same(got["err"][pairs[:, 1], pairs[:, 0]], v.real.std(axis=1) / np.sqrt(NS))
    assert same(got["imag"][pairs[:, 0], pairs[:, 1]], v.imag.mean(axis=1)) and same(np.diag(got["corr"]), np.full(N, 0.75))

    got = OC.renyi2_regions(wf, MASKS, NPAIRS, seed=SEED, step=STEP, want_log_ratio=True)
    out = regions(MASKS, NPAIRS, seed=SEED, step=STEP, log_ratio=True)
    want = OC.renyi2_from_sums(out["sums"], NPAIRS)
    assert all(same(got[k], want[k]) for k in want) and same(got["survivors"], out["in_sector"] / float(NPAIRS))
    assert same(got["log_ratio"], out["log_ratio"]) and same(got["samples"], out["samples"]) and got["samples"].shape == (2 * NPAIRS, N)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_two_iterations_on_the_host_and_on_the_device_agree_bit_for_bit(family):
    ham = hamiltonian(family)
    runs = []
    for device_steps in (None, 2):
        mod, wf, prm, _, _ = make(family)
        if family == "complex":
            mean, var = OC.minimize_hamiltonian(wf, ham, NS, 1, 1e-2, params=prm, seed=SEED, scope=SCOPE, device_steps=device_steps)
        else:
            minimize = T.minimize_hamiltonian if family == "gru" else mod.minimize_hamiltonian
            mean, var = minimize(wf, ham, prm, numsteps=1, numsamples=NS, learningrate=1e-2, seed=SEED, scope=SCOPE, device_steps=device_steps)
        last = (T if family == "gru" else mod).minimize_hamiltonian.last_params
        runs.append((np.array(mean), np.array(var), last))
        assert len(mean) == len(var) == 2 and sorted(last) == sorted(prm) and any(not same(last[k], prm[k]) for k in prm)
    (mean_h, var_h, prm_h), (mean_d, var_d, prm_d) = runs
    assert same(mean_h, mean_d) and same(var_h, var_d)
    assert all(same(prm_h[k], prm_d[k]) for k in prm_h)
