"""GPU tests of Pauli-string expectation values and local energies of arbitrary spin Hamiltonians for the 2D RNN
(rnnwf_pauli_step_2d, csrc/mdrnn_pauli_kernels.h, NativeWavefunction.pauli_step_2d, observables_2d).

Tolerances, the project's own for this model (tests/test_gpu_mdrnn.py, docs/pauli.md): log r against flipped configurations scored by
rnnwf_log_prob (the base kernel, independent of the tail kernel) and against rnnwf_tfim2d_eloc's queue: 1e-11 N.  Exact enumeration:
relative 1e-12.  E_loc against rnnwf_tfim2d_eloc: rtol 1e-10.  Sums against sums of the device's own values: rtol 1e-12.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import autograd_reference as A
import pauli_2d_reference as Q
import pauli_reference as PR
from conftest import all_configs
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_2d as O2

pytestmark = pytest.mark.gpu

SCOPE = Q.SCOPE


def make_wf(Nx, Ny, H, prm):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (H,))
    wf.set_params(prm, scope=SCOPE)
    return wf


def flips_only(wf, masks, ns, **kw):
    masks = np.asarray(masks)
    return wf.pauli_step_2d(masks, np.zeros_like(masks), np.ones(len(masks)), ns, **kw)


@functools.lru_cache(maxsize=None)
def exact_state(Nx, Ny):
    """(wave function, all configurations (2^N, Nx, Ny), their log P from the base kernel, strings, exact values from dense operators)"""
    N = Nx * Ny
    wf = make_wf(Nx, Ny, Q.EXACT_H, Q.exact_weights())
    c = all_configs(N).reshape(-1, Nx, Ny)
    lp = wf.log_prob(c)
    psi = np.exp(0.5 * lp)
    strings = Q.exact_strings(Nx, Ny)
    exact = np.array([(psi @ (PR.dense_string({i: p for p, i in st}, N) @ psi)).real for st in strings]) / (psi @ psi)
    return wf, c, lp, strings, exact


# 1. sum over every sigma of P(sigma) v_k(sigma) = psi^T O_k psi from the dense operator
@pytest.mark.parametrize("Nx,Ny", Q.EXACT_LATTICES)
def test_exact_enumeration_against_dense_operators(Nx, Ny):
    N = Nx * Ny
    wf, c, lp, strings, exact = exact_state(Nx, Ny)
    flip, sign, factor = O.pauli_terms(strings, N)
    assert np.all(factor.imag == 0)
    out = wf.pauli_step_2d(flip, sign, factor.real, len(c), samples=c, want_log_ratio=True, want_eloc=True)
    lr = out["log_ratio"]
    _, index = O.group_by_mask(flip)
    cf = c.reshape(-1, N)
    v = PR.signs(cf, sign) * np.where(index[:, None] >= 0, np.exp(lr[np.maximum(index, 0)]), 1.0)
    got = factor.real * (np.exp(lp)[None, :] * v).sum(axis=1) / np.exp(lp).sum()
    rel = np.abs(got / exact - 1.0)
    print("%dx%d: exact values %s, max rel %.2e" % (Nx, Ny, np.round(exact, 4), rel.max()))
    assert np.abs(exact).min() >= Q.FLOOR
    assert rel.max() <= 1e-12
    # term_sums are the plain sums of the same v, E_loc their coefficient-weighted sum
    assert np.allclose(out["term_sums"], PR.sums_from_values(v), rtol=1e-12, atol=0)
    assert np.allclose(out["eloc"], factor.real @ v, rtol=1e-12, atol=1e-12)
    m = out["moments"]
    assert m[2] == len(c) and np.isclose(m[0], out["eloc"].sum(), rtol=1e-12) and np.isclose(m[1], (out["eloc"] ** 2).sum(), rtol=1e-12)
    # raw terms whose sign and flip masks overlap on an odd number of sites (sz_k sx_k; sz_a sx_a sx_b): the sign is the SAMPLED
    # configuration's - read from the flipped one, every v would change sign
    a, b = Q.site(Nx, Ny, Nx - 1, 1), Q.site(Nx, Ny, 1, 2)
    f2, s2, _ = O.pauli_terms([[("Y", a)], [("Y", b), ("X", 0)]], N)
    o2 = wf.pauli_step_2d(f2, s2, [1.0, 1.0], len(c), samples=c, want_log_ratio=True)
    v2 = PR.signs(cf, s2) * np.exp(o2["log_ratio"])
    assert np.allclose(o2["term_sums"], PR.sums_from_values(v2), rtol=1e-12, atol=0)
    assert np.abs(o2["term_sums"][:, 0]).min() > 1.0     # (CPU oracle: -6.7e3, 1.8e4 on 3x4; -2.5e4, 1.7e5 on 4x3)
    # weighted with P these raw terms vanish: sz sx overlapping on an odd number of sites is a real antisymmetric matrix, so
    # psi^T O psi = 0 exactly; the device's pairs psi(sigma) psi(sigma ^ F) s(sigma) cancel to the rounding of log r (sum |psi psi'| <= 1)
    assert np.abs((np.exp(lp)[None, :] * v2).sum(axis=1)).max() <= 1e-12


# 2. log r per chain against explicit flipped configurations scored by the base kernel: every row of the dispatch table and every
# remainder width; lattices without a vertical neighbour, with every site a row start, with two mask words; a partial last block
WIDTHS = [10, 16, 17, 18, 19, 20, 36, 50, 68, 84]
LATTICES = [(4, 3), (3, 3), (2, 2), (1, 5), (5, 1), (5, 7), (7, 5)]


@pytest.mark.parametrize("Nx,Ny", LATTICES)
@pytest.mark.parametrize("H", WIDTHS)
def test_log_ratio_matches_explicit_flipped_configurations(H, Nx, Ny):
    N, ns = Nx * Ny, 37
    wf = make_wf(Nx, Ny, H, Q.weights(H, H + N, 1.0))
    s = np.random.RandomState(H + N).randint(0, 2, size=(ns, Nx, Ny)).astype(np.int32)
    masks = Q.case_masks(Nx, Ny)
    got = flips_only(wf, masks, ns, samples=s, want_log_ratio=True)["log_ratio"]
    ref = Q.explicit_log_ratio(wf.log_prob, s, masks)
    err = np.abs(got - ref).max()
    print("H=%d %dx%d: %d masks, max |log r - explicit| = %.2e (max |log r| %.2f)" % (H, Nx, Ny, len(masks), err, np.abs(ref).max()))
    assert got.shape == (len(masks), ns) and np.all(np.isfinite(ref))
    assert err <= Q.BOUND * N
    assert np.abs(ref).max() > 1e-3


# 3. against the hard-wired 2D TFIM estimator on the same samples
@pytest.mark.parametrize("Nx,Ny,H", [(4, 3, 20), (5, 7, 50)])
def test_single_x_masks_and_tfim_energy_against_tfim2d_eloc(Nx, Ny, H):
    N, ns = Nx * Ny, 100
    wf = make_wf(Nx, Ny, H, Q.weights(H, 5, 1.0))
    s = wf.sample(ns, seed=3)
    Jz = np.random.RandomState(1).uniform(0.5, 1.5, size=(Nx, Ny))      # non-uniform: a transposed lattice index shows
    lpq = np.empty((N + 1, ns))
    e_ref = wf.tfim_eloc(s, Jz, 1.3, log_probs=lpq)
    out = flips_only(wf, np.eye(N, dtype=np.int32), ns, samples=s, want_log_ratio=True)
    ref = 0.5 * (lpq[1:] - lpq[0][None, :])                             # queue row nx*Ny + ny + 1 = the flip of lattice site k
    err = np.abs(out["log_ratio"] - ref).max()
    e = O2.energy(wf, O2.tfim_hamiltonian(Jz, 1.3), ns, samples=s, want_eloc=True)
    rel = np.abs(e["eloc"] / e_ref - 1.0).max()
    print("%dx%d: max |log r_k - queue| = %.2e; max rel |E_loc - tfim2d_eloc| = %.2e" % (Nx, Ny, err, rel))
    assert err <= Q.BOUND * N
    assert np.allclose(e["eloc"], e_ref, rtol=1e-10, atol=0)
    assert np.isclose(e["mean"], e_ref.mean(), rtol=1e-10)


# 4. device-drawn samples
def test_drawn_samples_shards_and_work():
    Nx, Ny, H, ns = 5, 4, 20, 1000
    N = Nx * Ny
    wf = make_wf(Nx, Ny, H, Q.weights(H, 4, 1.0))
    ham = O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5)
    kw = dict(seed=5, step=2, want_eloc=True, want_log_ratio=True, want_samples=True)
    wf.timing_enable(True)
    wf.timing_reset()
    a = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, **kw)
    masks, _ = O.group_by_mask(ham.flip)
    firsts = [int(np.flatnonzero(m)[0]) for m in Q.to_visit_order(masks, Nx, Ny)]
    assert wf.timing_get(1)["cell_evals"] == ns * sum(N - 1 - f for f in firsts) and wf.timing_get(1)["launches"] == 1
    assert a["samples"].shape == (ns, Nx, Ny) and np.array_equal(a["samples"], wf.sample(ns, seed=5, step=2))
    b = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, **kw)
    for k in ("term_sums", "moments", "eloc", "log_ratio", "samples"):
        assert np.array_equal(a[k], b[k]), k
    cut = 336
    s1 = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, cut, sample_offset=0, **kw)
    s2 = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns - cut, sample_offset=cut, **kw)
    assert np.array_equal(np.concatenate([s1["samples"], s2["samples"]]), wf.sample(ns, seed=5, step=2, sample_offset=0))
    assert np.array_equal(s2["samples"], wf.sample(ns - cut, seed=5, step=2, sample_offset=cut))
    assert np.array_equal(np.concatenate([s1["eloc"], s2["eloc"]]), a["eloc"])
    assert np.allclose(s1["term_sums"] + s2["term_sums"], a["term_sums"], rtol=1e-12, atol=0)
    # permuted and duplicated terms read the row of their mask: no per-term bit changes
    perm = np.random.RandomState(0).permutation(len(ham.coeff))[:20]
    perm = np.concatenate([perm, perm[:3]])
    p = wf.pauli_step_2d(ham.flip[perm], ham.sign[perm], ham.coeff[perm], ns, **kw)
    assert np.array_equal(p["term_sums"], a["term_sums"][perm])


@pytest.mark.parametrize("Nx,Ny", Q.EXACT_LATTICES)
def test_device_drawn_expectations_within_five_standard_errors(Nx, Ny):
    ns = 2 ** 16
    wf, c, lp, strings, exact = exact_state(Nx, Ny)
    strings = strings + [[("Y", 3)], [("X", 1), ("Y", 2), ("Z", 3)]]
    out = O2.pauli_expectations(wf, strings, ns, seed=111)
    z = np.abs(out["value"][:-2] - exact) / out["err"][:-2]
    print("%dx%d: exact %s\n  got %s\n  |z| %s" % (Nx, Ny, np.round(exact, 4), np.round(out["value"], 4), np.round(z, 2)))
    assert np.abs(exact).min() >= Q.FLOOR and np.all(out["err"][:-2] > 0)
    assert z.max() <= 5.0
    assert np.all(out["value"][-2:] == 0) and np.all(out["err"][-2:] == 0)          # odd n_Y


# 5. several passes
def test_several_passes_give_the_one_pass_bits_and_leave_no_batch(monkeypatch):
    Nx, Ny, H, ns = 5, 7, 50, 300
    prm = Q.weights(H, 4, 1.0)
    ham = O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5)
    kw = dict(seed=5, step=2, want_eloc=True, want_log_ratio=True, want_samples=True)
    a = make_wf(Nx, Ny, H, prm).pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, **kw)
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf1 = make_wf(Nx, Ny, H, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    m = wf1.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, **kw)
    passes = wf1.timing_get(1)["launches"]
    print("RNNWF_STATE_BUDGET_MB=1: %d passes" % passes)
    assert passes >= 3
    for k in ("eloc", "log_ratio", "samples"):
        assert np.array_equal(m[k], a[k]), k
    assert np.allclose(m["term_sums"], a["term_sums"], rtol=1e-12, atol=0) and np.allclose(m["moments"][:3], a["moments"][:3], rtol=1e-12)
    with pytest.raises(Exception, match="rnnwf_vmc_step first"):
        wf1.vmc_gradient(0.0, ns, {"wf_dense/kernel": (H, 2)})
    # caller's samples through the same passes
    m2 = wf1.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, samples=a["samples"], want_eloc=True, want_log_ratio=True)
    assert np.array_equal(m2["eloc"], a["eloc"]) and np.array_equal(m2["log_ratio"], a["log_ratio"])


# 6. the resident batch: the gradient of an energy that is not hard-wired
def test_gradient_of_a_2d_xxz_energy_against_float64_autograd():
    import torch
    from rnnwavefunctions_amd.training import cost_gradient
    Nx, Ny, H, ns = 4, 3, 20, 2000
    prm = Q.weights(H, 111, 1.0)
    wf = make_wf(Nx, Ny, H, prm)
    ham = O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5)
    out = wf.pauli_step_2d(ham.flip, ham.sign, ham.coeff, ns, seed=111, want_eloc=True, want_samples=True)
    s, e = out["samples"], out["eloc"]
    assert np.isclose(out["moments"][0] / ns, e.mean(), rtol=1e-12) and e.std() > 0.1
    grads = cost_gradient(wf, prm, SCOPE, e.mean(), ns)
    g64 = A.gradient("mdrnn", prm, s, e, dtype=torch.float64)
    g32 = A.gradient("mdrnn", prm, s, e, dtype=torch.float32)
    assert set(grads) == set(prm)
    worst, failures = A.verdict(grads, g64, g32, unit_roundoff_ratio=A.F64_OVER_F32, label="[pauli 2d xxz]")
    print("[pauli 2d xxz] worst ratio deviation / yardstick = %.3f (bound %g)" % (worst, A.FACTOR))
    assert not failures, "tensors beyond %g x the yardstick: %s" % (A.FACTOR, failures)
    # a refused call in between leaves the batch: the same gradient bits
    with pytest.raises(ValueError, match="nterms|shape"):
        wf.pauli_step_2d(np.zeros((0, Nx * Ny)), np.zeros((0, Nx * Ny)), [], ns)
    bad = ham.flip.copy()
    bad[3, 5] = 2
    with pytest.raises(ValueError, match=r"flip\[3\]\[5\] = 2"):
        wf.pauli_step_2d(bad, ham.sign, ham.coeff, ns, seed=1)
    again = cost_gradient(wf, prm, SCOPE, e.mean(), ns)
    for k in grads:
        assert np.array_equal(grads[k], again[k]), k


# 7. refusals
def test_refusals_through_the_c_call_and_the_facade():
    from rnnwavefunctions_amd import _lib
    Nx, Ny, N = 3, 2, 6
    wf = make_wf(Nx, Ny, 10, Q.weights(10, 1, 1.0))
    one = np.zeros((1, N), dtype=np.int32)
    x0 = one.copy()
    x0[0, 0] = 1
    ok = wf.pauli_step_2d(x0, one, [1.0], 32, seed=1)
    shapes = {"wf_dense/kernel": (10, 2)}
    g0 = wf.vmc_gradient(ok["moments"][0] / 32, 32, shapes)["wf_dense/kernel"]
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fp, sp = x0.ctypes.data_as(I32P), one.ctypes.data_as(I32P)
    co = np.ones(1)
    cp = co.ctypes.data_as(F64P)
    sums = np.zeros((1, 2))
    up = sums.ctypes.data_as(F64P)

    def call(h=None, flip=fp, sign=sp, coeff=cp, K=1, ns=32, offset=0, out=up):
        return wf.lib.rnnwf_pauli_step_2d(h or wf.h, flip, sign, coeff, K, None, ns, 1, 0, offset, out, None, None, None, None)

    def last(h=None):
        return wf.lib.rnnwf_last_error(h or wf.h).decode()

    wf.timing_enable(True)
    wf.timing_reset()
    for kwargs, word in [(dict(K=0), "nterms"), (dict(ns=0), "ns must"), (dict(flip=None), "non-null"), (dict(sign=None), "non-null"),
                         (dict(coeff=None), "non-null"), (dict(out=None), "non-null"), (dict(offset=-1), "sample_offset")]:
        assert call(**kwargs) == -1, kwargs
        assert word in last() and "rnnwf_pauli_step_2d" in last(), (kwargs, last())
    bad = x0.copy()
    bad[0, 4] = 2
    assert call(flip=bad.ctypes.data_as(I32P)) == -1 and "flip[0][4] = 2" in last()
    assert call(sign=bad.ctypes.data_as(I32P)) == -1 and "sign[0][4] = 2" in last()
    with pytest.raises(ValueError, match="0 or 1"):
        wf.pauli_step_2d(bad, one, [1.0], 32)
    # more than 65 535 distinct non-empty masks (N = 17 sites)
    w17 = make_wf(17, 1, 10, Q.weights(10, 1, 1.0))
    k = np.arange(1, 65537)
    many = np.ascontiguousarray(((k[:, None] >> np.arange(17)[None, :]) & 1).astype(np.int32))
    w17.timing_enable(True)
    w17.timing_reset()
    with pytest.raises(ValueError, match="more than 65535 distinct flip masks"):
        w17.pauli_step_2d(many, np.zeros_like(many), np.ones(len(many)), 16, seed=1)
    assert sum(w17.timing_get(i)["launches"] for i in range(3)) == 0
    # uncommitted parameters
    raw = _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (10,))
    assert call(h=raw.h) == -1 and "not committed" in last(raw.h)
    with pytest.raises(ValueError, match="not committed"):
        raw.pauli_step_2d(x0, one, [1.0], 32)
    # a width without a kernel cannot be created
    with pytest.raises(ValueError, match="num_units too large"):
        _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, Nx, Ny, (85,))
    # the refused calls launched nothing and left the resident batch usable
    assert sum(wf.timing_get(i)["launches"] for i in range(3)) == 0
    g1 = wf.vmc_gradient(ok["moments"][0] / 32, 32, shapes)["wf_dense/kernel"]
    assert np.array_equal(g0, g1)
    # every other model is refused by the 2D entry point, by name, with a pointer to rnnwf_pauli_step
    for model, nx, ny, units, name in [(_lib.MODEL_GRU1D, N, 1, (10,), "GRU1D"), (_lib.MODEL_GRU1D_F64, Nx, Ny, (10,), "GRU1D_F64"),
                                       (_lib.MODEL_GRU1D_PARITY, N, 1, (10,), "GRU1D_PARITY"), (_lib.MODEL_CRNN_U1, N, 1, (10,), "CRNN_U1"),
                                       (_lib.MODEL_LSTM1D_F64, Nx, Ny, (10,), "LSTM1D_F64")]:
        w = _lib.NativeWavefunction(model, nx, ny, units)
        w.timing_enable(True)
        with pytest.raises(ValueError, match=r"model is %s; rnnwf_pauli_step serves the GRU models" % name):
            w.pauli_step_2d(x0, one, [1.0], 32)
        with pytest.raises(ValueError, match="MDRNN2D"):
            O2.pauli_expectations(w, ["XIIIII"], 32)
        assert sum(w.timing_get(i)["launches"] for i in range(3)) == 0
    # the existing entry points still refuse the 2D RNN
    with pytest.raises(ValueError, match="MDRNN"):
        wf.pauli_step(x0, one, [1.0], 32)
    with pytest.raises(ValueError, match="MDRNN"):
        O.pauli_expectations(wf, ["XIIIII"], 32)
    for fn in (lambda: wf.renyi2_swap(4), lambda: wf.renyi2_regions(x0, 4), lambda: wf.correlations(8)):
        with pytest.raises(ValueError, match="MDRNN"):
            fn()


# 8. two-point functions
def test_correlations_on_3x4_against_exact_enumeration():
    Nx, Ny, ns = 3, 4, 2 ** 16
    N = Nx * Ny
    wf, c, lp, _, _ = exact_state(Nx, Ny)
    psi = np.exp(0.5 * lp)
    psi /= np.linalg.norm(psi)
    cf = c.reshape(-1, N)
    ev = lambda letters: Q.string_expectation(psi, cf, [(p, k) for k, p in letters.items()])
    out = O2.correlations(wf, ns, seed=7)
    centre = O2.site(Nx, Ny, Nx // 2, Ny // 2)
    assert out["pairs"].tolist() == [[centre, k] for k in range(N) if k != centre]
    z = np.array([ev({k: "Z"}) for k in range(N)])
    x = np.array([ev({k: "X"}) for k in range(N)])
    zz_c = np.array([ev({a: "Z", b: "Z"}) - z[a] * z[b] for a, b in out["pairs"]])
    xx_c = np.array([ev({a: "X", b: "X"}) - x[a] * x[b] for a, b in out["pairs"]])
    worst = {}
    for name, exact in [("z", z), ("x", x), ("zz_c", zz_c), ("xx_c", xx_c)]:
        assert np.all(out[name + "_err"] > 0)
        worst[name] = (np.abs(out[name] - exact) / out[name + "_err"]).max()
    print("3x4 correlations, 2^16 samples: worst |z| %s; max |zz_c| %.3f, max |xx_c| %.3f"
          % ({k: round(v, 2) for k, v in worst.items()}, np.abs(zz_c).max(), np.abs(xx_c).max()))
    assert max(worst.values()) <= 5.0
    assert np.abs(zz_c).max() > 0.01 and np.abs(xx_c).max() > 0.01
    # listed pairs, in either order, share one mask
    two = O2.correlations(wf, 1000, pairs=[(0, 5), (5, 0)], seed=7)
    assert two["xx"][0] == two["xx"][1] and two["zz_c"][0] == two["zz_c"][1]
    # the facade of the reference's class is accepted
    from rnnwavefunctions_amd.TFIM2D_2DRNN.Training2DRNN_2DTFIM import MDRNNcell, RNNwavefunction
    fac = RNNwavefunction(Nx, Ny, units=[10], cell=MDRNNcell, seed=111)
    e = O2.energy(fac, O2.xxz_hamiltonian_2d(Nx, Ny, -1.0, 0.5), 500)
    assert np.isfinite(e["mean"]) and e["err"] > 0
