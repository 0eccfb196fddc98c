"""GPU tests of Pauli-string expectation values and energies of arbitrary spin Hamiltonians for the complex RNN
(rnnwf_pauli_step_complex, csrc/crnn_pauli.hip, csrc/crnn_pauli_kernels.h; docs/pauli_complex.md).

Bounds, none derived from the kernels: float32 log-ratios 1e-5 N per component (docs/pauli.md, from docs/renyi_regions.md); exact
enumeration relative 2e-5 (the f32 row of docs/pauli.md), every non-zero exact value at least the floor 0.05 of
tests/pauli_2d_reference.py; J1-J2 local energies
1e-5 per site in both parts (the f32 row of tests/test_gpu_prnn.py); sums 1e-12 relative; statistics |z| <= 5.
"""
import ctypes as C
import math

import numpy as np
import pytest

import crnn_pauli_reference as CR
import ed
from rnnwavefunctions_amd import observables as O
from rnnwavefunctions_amd import observables_complex as OC
from rnnwavefunctions_amd import params as P

pytestmark = pytest.mark.gpu

SCOPE = CR.SCOPE
FLOOR = 0.05


def make_wf(N, H, prm, layers=1):
    from rnnwavefunctions_amd import _lib
    wf = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,) * layers)
    wf.set_params(prm, scope=SCOPE)
    return wf


def host_values(out, flip, sign, samples):
    """(K, ns) complex v_k from the device's own log-ratios and the sampled signs."""
    _, index = O.group_by_mask(flip)
    lr = out["log_ratio"]
    d = np.stack([lr[i] if i >= 0 else np.zeros(lr.shape[1], dtype=np.complex128) for i in index])
    return CR.local_values(d, samples, flip, sign)


# (N, units, chains): NFULL 1, 2, 3 (second mask word; the width whose sampling base pass is the bf16 cooperative kernel), three words,
# then one case per remaining launch row (NFULL 4, 6, 8, 12, 16)
ROWS = [(10, 12, 37), (12, 30, 37), (34, 50, 37), (70, 20, 37), (6, 60, 48), (6, 90, 48), (6, 120, 48), (6, 180, 48), (6, 250, 48)]


# 1. log-ratio against explicit scoring
@pytest.mark.parametrize("N,H,ns", ROWS)
def test_log_ratio_matches_explicit_flipped_configurations(N, H, ns):
    prm = CR.weights(H, seed=H + N, scale=2.0 if H <= 60 else 1.0)
    wf = make_wf(N, H, prm)
    s = CR.random_sector_samples(N, ns, seed=N)
    masks = CR.case_masks(N)
    firsts = {int(np.flatnonzero(m)[0]) for m in masks}
    assert 0 in firsts and N - 1 in firsts
    out = wf.pauli_step_complex(masks, np.zeros_like(masks), np.ones(len(masks)), ns, samples=s, want_log_ratio=True, want_eloc=True)
    lr = out["log_ratio"]
    assert lr.shape == (len(masks), ns) and not np.any(np.isnan(lr.real)) and not np.any(np.isnan(lr.imag))
    assert np.all(np.isfinite(out["term_sums"])) and np.all(np.isfinite(out["moments"])) and np.all(np.isfinite(out["eloc"].view(np.float32)))
    own = wf.log_amp(s).astype(np.complex128)
    worst, n_out, n_in = 0.0, 0, 0
    for k, m in enumerate(masks):
        x = s ^ m[None, :]
        ok = CR.in_sector(x)
        n_out, n_in = n_out + int((~ok).sum()), n_in + int(ok.sum())
        # outside the sector: exactly (-inf, 0)
        assert np.all(np.isneginf(lr[k, ~ok].real)) and np.all(lr[k, ~ok].imag == 0.0), k
        assert np.all(np.isfinite(lr[k, ok].real)), k
        if ok.any():
            ref = wf.log_amp(x[ok]).astype(np.complex128) - own[ok]
            d = lr[k, ok] - ref
            worst = max(worst, float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
        if not ok.any():                                       # v exactly 0: the sums of this term are exactly 0
            assert np.all(out["term_sums"][k] == 0.0), k
    print("[crnn pauli N=%d H=%d] %d masks, %d in-sector / %d out-of-sector entries, max |d| error %.3e, bound %.3e"
          % (N, H, len(masks), n_in, n_out, worst, CR.F32_BOUND * N))
    assert n_out > 0 and n_in > 0
    assert worst <= CR.F32_BOUND * N
    # E_loc = sum_k v_k: exactly zero contributions from outside the sector, complex64
    v = host_values(out, masks, np.zeros_like(masks), s)
    assert np.all(v[:, :][np.isneginf(lr.real)] == 0.0)
    assert np.abs(out["eloc"] - v.sum(axis=0)).max() <= 1e-6 * max(1.0, np.abs(v.sum(axis=0)).max())


# 2. exact enumeration over the whole sector
EXACT_STRINGS = [[("X", 0), ("X", 1)], [("Y", 0), ("Y", 1)], [("X", 4), ("X", 5)], [("Y", 4), ("Y", 5)], [("X", 2), ("Y", 7)],
                 [("Z", 1), ("X", 3), ("Z", 2), ("X", 6)], [("X", 3)], [("Y", 0), ("X", 3)], [("Z", 2), ("Z", 8)],
                 [("X", 0), ("X", 1), ("X", 2), ("X", 3)], [("X", 8), ("X", 9)], [("Y", 1), ("Z", 5), ("X", 8)]]


def exact_state(N=10, H=12):
    prm = CR.weights(H, seed=7, scale=2.0)
    wf = make_wf(N, H, prm)
    cfg = CR.sector(N)
    psi = np.zeros(2 ** N, dtype=np.complex128)
    idx = cfg @ (1 << np.arange(N - 1, -1, -1))
    psi[idx] = np.exp(wf.log_amp(cfg).astype(np.complex128))
    exact = np.array([np.vdot(psi, CR.dense_string(s, N) @ psi) for s in EXACT_STRINGS]) / np.vdot(psi, psi).real
    return wf, cfg, exact


def test_exact_enumeration_against_dense_operators():
    N = 10
    wf, cfg, exact = exact_state(N)
    flip, sign, factor = O.pauli_terms(EXACT_STRINGS, N)
    out = wf.pauli_step_complex(flip, sign, np.ones(len(factor)), len(cfg), samples=cfg, want_log_ratio=True)
    w = np.exp(wf.log_prob(cfg))
    assert abs(w.sum() - 1.0) < 1e-5
    est = factor * (host_values(out, flip, sign, cfg) @ w) / w.sum()
    nz = np.arange(len(exact)) != 6
    assert est[6] == 0.0 and exact[6] == 0.0                    # a single X leaves the sector
    assert np.abs(exact[nz]).min() >= FLOOR                      # (float64 oracle: the smallest is X2 Y7 = -0.056)
    rel = np.where(nz, np.abs(est - exact) / np.where(nz, np.abs(exact), 1.0), 0.0)
    for st, e, x, r in zip(EXACT_STRINGS, est, exact, rel):
        print("[crnn pauli exact] %-40s est %+.6f%+.6fi exact %+.6f%+.6fi rel %.2e" % (st, e.real, e.imag, x.real, x.imag, r))
    assert np.abs(exact.imag).max() < 1e-6                       # Pauli strings are Hermitian
    assert rel.max() <= 2e-5


# 3. J1-J2 cross-check against the hard-wired estimator, on the same samples
@pytest.mark.parametrize("N,H", [(10, 12), (34, 50)])
def test_j1j2_hamiltonian_eloc_against_rnnwf_j1j2_eloc(N, H, monkeypatch):
    monkeypatch.setenv("RNNWF_ENGINE", "f32")        # rnnwf_j1j2_eloc on the f32-input MFMA engine, as the masked-tail pass
    prm = CR.weights(H, seed=N, scale=2.0)
    wf = make_wf(N, H, prm)
    ns = 100
    s = wf.sample(ns, seed=3)
    rng = np.random.RandomState(N)
    J1, J2, Bz = 1.0 + 0.1 * rng.standard_normal(N), 0.4 + 0.1 * rng.standard_normal(N), 0.3 * rng.standard_normal(N)
    for periodic in (False, True):
        for marshall in (False, True):
            ham = OC.j1j2_hamiltonian(J1, J2, Bz, periodic=periodic, marshall=marshall)
            e = wf.pauli_step_complex(ham.flip, ham.sign, ham.coeff, ns, samples=s, want_eloc=True)["eloc"].astype(np.complex128)
            ref, _ = wf.j1j2_eloc(s, J1, J2, Bz, periodic=periodic, marshall=marshall)
            d = e - ref.astype(np.complex128)
            worst = max(np.abs(d.real).max(), np.abs(d.imag).max())
            print("[crnn pauli j1j2 N=%d periodic=%d marshall=%d] max |dE| %.3e (bound %.3e), |E| up to %.2f"
                  % (N, periodic, marshall, worst, 1e-5 * N, np.abs(ref).max()))
            assert np.abs(ref.imag).max() > 1e-3 and np.all(np.isfinite(e.real)) and np.all(np.isfinite(e.imag))
            assert worst <= 1e-5 * N


# 4. bit identities, shards, passes, work counters and timing ids
def test_bit_identities_repeat_order_shards_passes_and_work(monkeypatch):
    N, H, ns = 12, 30, 300
    prm = CR.weights(H, seed=5, scale=2.0)
    wf = make_wf(N, H, prm)
    strings = [[("X", 2), ("X", 3)], [("Y", 2), ("Y", 3)], [("X", 5)], [("Z", 0), ("Z", 7)], [("X", 0), ("Y", 11)], [("X", 4), ("X", 9)],
               [("Y", 4), ("Y", 9)], [("Z", 1), ("X", 6), ("X", 7)]]
    flip, sign, factor = O.pauli_terms(strings, N)
    coeff = factor * (1.0 + 0.1 * np.arange(len(factor)))
    kw = dict(seed=5, step=2, want_eloc=True, want_log_ratio=True, want_samples=True)
    wf.timing_enable(True)
    wf.timing_reset()
    a = wf.pauli_step_complex(flip, sign, coeff, ns, **kw)
    masks, index = O.group_by_mask(flip)
    firsts = [int(np.flatnonzero(m)[0]) for m in masks]
    t = [wf.timing_get(i) for i in range(3)]
    assert t[1]["cell_evals"] == ns * sum(N - f for f in firsts)
    # id 0: the sampling base pass, the checkpointed base pass and the site-term replay; id 1: one masked-tail launch; id 2: log-ratio,
    # term, sums, E_loc and moments kernels under three brackets
    assert t[0]["launches"] == 3 and t[1]["launches"] == 1 and t[2]["launches"] == 3 and t[1]["mfma_flops"] > 0
    s = a["samples"]
    assert np.array_equal(s, wf.sample(ns, seed=5, step=2)) and np.all(CR.in_sector(s))
    b = wf.pauli_step_complex(flip, sign, coeff, ns, **kw)
    for k in ("term_sums", "moments", "eloc", "log_ratio", "samples"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # <X_5>: exactly 0
    assert np.all(a["term_sums"][2] == 0.0)
    # v_YY = v_XX * (-s_i s_j) per sample, to the bit
    sp = 2.0 * s - 1.0
    one = lambda k: wf.pauli_step_complex(flip[k], sign[k], [factor[k]], ns, samples=s, want_eloc=True)["eloc"]      # factor: 1, -1
    for kx, ky, (i, j) in ((0, 1, (2, 3)), (5, 6, (4, 9))):
        vx, vy = one(kx), one(ky)
        assert np.abs(vx).max() > 0.01
        want = (vx * (-sp[:, i] * sp[:, j]).astype(np.float32)).astype(np.complex64)
        assert np.array_equal((vy + 0).view(np.uint32), (want + 0).view(np.uint32))      # + 0: -0.0 and 0.0 are the same value
    # term order and duplication leave per-term bits equal
    perm = np.array([3, 0, 0, 7, 5, 1, 2, 6, 4, 1])
    c = wf.pauli_step_complex(flip[perm], sign[perm], coeff[perm], ns, samples=s)
    assert np.array_equal(c["term_sums"], a["term_sums"][perm])
    # sums against an exactly rounded re-summation of the device's own v
    v = host_values(a, flip, sign, s)
    resum = np.array([[math.fsum(r.real), math.fsum(r.imag), math.fsum(r.real ** 2), math.fsum(r.imag ** 2)] for r in v])
    nz = np.abs(resum) > 0
    assert np.abs(a["term_sums"][nz] / resum[nz] - 1.0).max() <= 1e-12 and np.all(a["term_sums"][~nz] == 0.0)
    e64 = coeff @ v
    m = a["moments"]
    assert m[2] == ns and np.allclose([m[0], m[3]], [a["eloc"].real.astype(np.float64).sum(), a["eloc"].imag.astype(np.float64).sum()], rtol=1e-12)
    assert np.abs(a["eloc"] - e64).max() <= 1e-6 * np.abs(e64).max()
    # two shards add up to the single call
    h1 = wf.pauli_step_complex(flip, sign, coeff, 160, seed=5, step=2)
    h2 = wf.pauli_step_complex(flip, sign, coeff, ns - 160, seed=5, step=2, sample_offset=160)
    tot = h1["term_sums"] + h2["term_sums"]
    assert np.abs(tot[nz] / a["term_sums"][nz] - 1.0).max() <= 1e-12
    # several passes: equal per-sample bits, no resident batch
    monkeypatch.setenv("RNNWF_STATE_BUDGET_MB", "1")
    wf1 = make_wf(N, H, prm)
    wf1.timing_enable(True)
    wf1.timing_reset()
    big = 4000
    one_pass = wf.pauli_step_complex(flip, sign, coeff, big, **kw)
    many = wf1.pauli_step_complex(flip, sign, coeff, big, **kw)
    passes = wf1.timing_get(1)["launches"]
    print("[crnn pauli passes] RNNWF_STATE_BUDGET_MB=1: %d passes" % passes)
    assert passes >= 3
    for k in ("eloc", "log_ratio", "samples"):
        assert np.array_equal(many[k].view(np.uint8), one_pass[k].view(np.uint8)), k
    assert np.allclose(many["term_sums"], one_pass["term_sums"], rtol=1e-12, atol=1e-300)
    with pytest.raises(Exception, match="rnnwf_vmc_step first"):
        wf1.vmc_gradient(0.0, big, {"wf_dense_ampl/kernel": (H, 2)})


# 5. statistics on device-drawn samples
def test_device_drawn_expectations_within_five_standard_errors():
    N, ns = 10, 2 ** 16
    wf, cfg, exact = exact_state(N)
    res = OC.pauli_expectations(wf, EXACT_STRINGS, ns, seed=11, step=3)
    for st, v, e, ei, x in zip(EXACT_STRINGS, res["value"], res["err"], res["err_imag"], exact):
        print("[crnn pauli stats] %-40s %+.5f%+.5fi +- %.5f / %.5f, exact %+.5f" % (st, v.real, v.imag, e, ei, x.real))
        for got, want, err in ((v.real, x.real, e), (v.imag, 0.0, ei)):
            if err == 0.0:
                assert got == want == 0.0                        # a string that leaves the sector for every chain
            else:
                assert abs(got - want) / err <= 5.0, st
    # spin correlations and the structure factor on top, against the dense S_i . S_j of the same state
    sc = OC.spin_correlations(wf, 2 ** 14, seed=12)
    psi = np.zeros(2 ** N, dtype=np.complex128)
    psi[cfg @ (1 << np.arange(N - 1, -1, -1))] = np.exp(wf.log_amp(cfg).astype(np.complex128))
    psi /= np.linalg.norm(psi)
    for i, j in [(0, 1), (3, 7), (0, 9), (4, 5)]:
        want = 0.25 * sum(np.vdot(psi, CR.dense_string([(c, i), (c, j)], N) @ psi).real for c in "XYZ")
        assert abs(sc["corr"][i, j] - want) <= 5.0 * sc["err"][i, j] and sc["corr"][j, i] == sc["corr"][i, j]
        assert abs(sc["imag"][i, j]) <= 5.0 * sc["err_imag"][i, j] + 1e-15
    assert np.all(np.diag(sc["corr"]) == 0.75)
    # total S_z = 0 in the sector: sum_ij <Z_i Z_j> = 0, so S(0) = (1/N) sum_ij <S_i . S_j> is the XY part alone and non-negative
    assert OC.structure_factor(sc["corr"], 0.0) > -5.0 * sc["err"].sum() / N


# 6. the resident batch and the gradient of the complex cost
@pytest.mark.parametrize("N,H", [(10, 12), (12, 30)])
def test_gradient_after_a_one_pass_call_equals_load_batch_bits(N, H):
    """The widths whose rnnwf_load_batch base pass is an f32 kernel (bit-identical to the one-wave kernel the Pauli pass uses).  At
    37..52 units rnnwf_load_batch runs the bf16 cooperative base pass, whose checkpoints differ in the last bits by construction."""
    from rnnwavefunctions_amd.training import cost_gradient
    ns = 400
    prm = CR.weights(H, seed=3, scale=1.5)
    wf = make_wf(N, H, prm)
    ham = OC.j1j2_hamiltonian(np.ones(N), 0.3 * np.ones(N), np.zeros(N))
    out = wf.pauli_step_complex(ham.flip, ham.sign, ham.coeff, ns, seed=4, want_eloc=True, want_samples=True)
    m = out["moments"]
    mean = complex(m[0] / m[2], m[3] / m[2])
    g1 = cost_gradient(wf, prm, SCOPE, mean, ns)
    wf.load_batch(out["samples"], out["eloc"])
    g2 = cost_gradient(wf, prm, SCOPE, mean, ns)
    assert set(g1) == set(prm)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    assert max(np.abs(v).max() for v in g1.values()) > 1e-4


def test_gradient_at_the_width_of_the_bf16_base_pass_agrees_with_load_batch():
    """N = 34 with 50 units (37..52 units): the resident checkpoints come from the one-wave f32 kernel, rnnwf_load_batch takes its own
    from the bf16 cooperative base pass, so the two gradients cannot be equal to the bit.  Bound: 2e-3 of the largest gradient element,
    the bound tests/test_gpu_training.py sets for this family's gradient against exact finite differences at every width (50 units,
    the bf16 base pass, among them) - both gradients lie within it of the exact one, and the difference of the two is held to the
    same figure, not to twice it."""
    from rnnwavefunctions_amd.training import cost_gradient
    N, H, ns = 34, 50, 400
    prm = CR.weights(H, seed=3, scale=1.5)
    wf = make_wf(N, H, prm)
    ham = OC.j1j2_hamiltonian(np.ones(N), 0.3 * np.ones(N), np.zeros(N))
    out = wf.pauli_step_complex(ham.flip, ham.sign, ham.coeff, ns, seed=4, want_eloc=True, want_samples=True)
    m = out["moments"]
    mean = complex(m[0] / m[2], m[3] / m[2])
    g1 = cost_gradient(wf, prm, SCOPE, mean, ns)
    wf.load_batch(out["samples"], out["eloc"])
    g2 = cost_gradient(wf, prm, SCOPE, mean, ns)
    scale = max(np.abs(v).max() for v in g2.values())
    worst = max(np.abs(g1[k] - g2[k]).max() for k in g1) / scale
    print("[crnn pauli gradient N=%d H=%d] max |g(resident) - g(load_batch)| / max |g| = %.2e (bound 2e-3), max |g| = %.3e" % (N, H, worst, scale))
    assert set(g1) == set(prm) and all(np.all(np.isfinite(v)) for v in g1.values()) and scale > 1e-4
    assert worst <= 2e-3


def test_the_reference_named_facade_through_the_module():
    """J1J2.ComplexRNNwavefunction.RNNwavefunction goes through energy, pauli_expectations and minimize_hamiltonian: the same bits as
    its NativeWavefunction gives, and the trained parameters land in the facade."""
    from rnnwavefunctions_amd import compat as tf
    from rnnwavefunctions_amd.J1J2.ComplexRNNwavefunction import RNNwavefunction
    N = 8
    fac = RNNwavefunction(N, cell=tf.contrib.cudnn_rnn.CudnnCompatibleGRUCell, units=[12])
    ham = OC.j1j2_hamiltonian(np.ones(N), 0.2 * np.ones(N), np.zeros(N))
    a, b = OC.energy(fac, ham, 500, seed=5), OC.energy(fac._native, ham, 500, seed=5)
    assert a["mean"] == b["mean"] and a["err"] == b["err"] and np.isfinite(a["mean"].real)
    pa, pb = OC.pauli_expectations(fac, ["XXIIIIII", "YXIIIIII"], 500, seed=5), OC.pauli_expectations(fac._native, ["XXIIIIII", "YXIIIIII"], 500, seed=5)
    assert np.array_equal(pa["value"], pb["value"]) and np.all(np.isfinite(pa["value"].real))
    before = {k: np.array(v) for k, v in fac.get_params().items()}
    meanE, varE = OC.minimize_hamiltonian(fac, ham, 200, 3, 1e-2, seed=7)
    assert len(meanE) == 4 and len(varE) == 4 and np.all(np.isfinite(np.real(meanE)))
    after = fac.get_params()
    assert set(after) == set(before) and any(not np.array_equal(after[k], before[k]) for k in after)
    for k, v in OC.minimize_hamiltonian.last_params.items():
        assert np.array_equal(np.asarray(after[k]), v), k
    # the library holds the facade's parameters: the energy through the facade is the energy of the trained state
    c, d = OC.energy(fac, ham, 500, seed=6), OC.energy(fac._native, ham, 500, seed=6)
    assert c["mean"] == d["mean"] and c["mean"] != a["mean"]


# 7. training on a Hamiltonian no positive model of the project can represent
def test_minimize_hamiltonian_on_the_antiferromagnetic_heisenberg_chain():
    """N = 8, open chain, no Marshall rotation: the ground state has a sign structure.  300 steps; the energy reached is printed
    (docs/pauli_complex.md records it), not asserted."""
    N, H = 8, 20
    prm = P.init_gru_params([H], seed=111, heads=CR.HEADS)
    wf = make_wf(N, H, prm)
    ham = OC.j1j2_hamiltonian(np.ones(N), np.zeros(N), np.zeros(N))
    E0 = float(np.linalg.eigvalsh(ed.j1j2_hamiltonian(np.ones(N), np.zeros(N), N))[0])
    first = OC.energy(wf, ham, 8000, seed=900)
    OC.minimize_hamiltonian(wf, ham, 500, 300, 5e-3, params=prm, seed=111, scope=SCOPE)
    last = OC.energy(wf, ham, 8000, seed=901)
    err = max(first["err"], last["err"])
    print("[crnn pauli training] E0 %.6f, initial %.5f +- %.5f, after 300 steps %.5f +- %.5f (imag %.1e)"
          % (E0, first["mean"].real, first["err"], last["mean"].real, last["err"], last["mean"].imag))
    assert last["mean"].real < first["mean"].real - 10.0 * err
    assert last["mean"].real >= E0 - 5.0 * err


# 8. refusals
def test_refusals_through_the_c_call_and_the_module():
    from rnnwavefunctions_amd import _lib
    N, H, ns = 6, 10, 32
    prm = CR.weights(H, seed=1)
    wf = make_wf(N, H, prm)
    one = np.zeros((1, N), dtype=np.int32)
    x01 = one.copy()
    x01[0, :2] = 1
    ok = wf.pauli_step_complex(x01, one, [1.0], ns, seed=1)
    shapes = {"wf_dense_ampl/kernel": (H, 2)}
    mean = complex(ok["moments"][0] / ns, ok["moments"][3] / ns)
    g0 = wf.vmc_gradient(mean, ns, shapes)["wf_dense_ampl/kernel"]
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    fp, sp = x01.ctypes.data_as(I32P), one.ctypes.data_as(I32P)
    co = np.ones(2)
    cp = co.ctypes.data_as(F64P)
    sums = np.zeros((1, 4))
    up = sums.ctypes.data_as(F64P)

    def call(h=None, flip=fp, sign=sp, coeff=cp, K=1, n=ns, offset=0, out=up):
        return wf.lib.rnnwf_pauli_step_complex(h or wf.h, flip, sign, coeff, K, None, n, 1, 0, offset, out, None, None, None, None)

    def last(h=None):
        return wf.lib.rnnwf_last_error(h or wf.h).decode()

    wf.timing_enable(True)
    wf.timing_reset()
    for kwargs, word in [(dict(K=0), "nterms"), (dict(n=0), "ns must"), (dict(flip=None), "non-null"), (dict(sign=None), "non-null"),
                         (dict(coeff=None), "non-null"), (dict(out=None), "non-null"), (dict(offset=-1), "sample_offset")]:
        assert call(**kwargs) == -1, kwargs
        assert word in last() and "rnnwf_pauli_step_complex" in last(), (kwargs, last())
    bad = x01.copy()
    bad[0, 4] = 2
    assert call(flip=bad.ctypes.data_as(I32P)) == -1 and "flip[0][4] = 2" in last()
    assert call(sign=bad.ctypes.data_as(I32P)) == -1 and "sign[0][4] = 2" in last()
    with pytest.raises(ValueError, match="0 or 1"):
        wf.pauli_step_complex(bad, one, [1.0], ns)
    # a caller-supplied sample outside the zero-magnetisation sector
    outside = np.array([[0, 1, 0, 1, 0, 1], [1, 1, 0, 1, 0, 1]], dtype=np.int32)
    with pytest.raises(ValueError, match=r"samples\[1\] has 4 up spins, the zero-magnetisation sector has 3"):
        wf.pauli_step_complex(x01, one, [1.0], 2, samples=outside)
    # the grid of the term kernel: nterms x ceil(ns / 256) beyond 2^31 - 1 (refused before the samples are touched)
    rep = np.ascontiguousarray(np.repeat(x01, 65536, axis=0))
    zer, cof = np.zeros_like(rep), np.ones(2 * 65536)
    assert call(flip=rep.ctypes.data_as(I32P), sign=zer.ctypes.data_as(I32P), coeff=cof.ctypes.data_as(F64P), K=65536, n=1 << 23) == -1
    assert "exceeds the grid" in last()
    # more than 65 535 distinct non-empty masks (N = 18 sites)
    w18 = make_wf(18, H, CR.weights(H, seed=1))
    k = np.arange(1, 65537)
    many = np.ascontiguousarray(((k[:, None] >> np.arange(18)[None, :]) & 1).astype(np.int32))
    w18.timing_enable(True)
    w18.timing_reset()
    with pytest.raises(ValueError, match="more than 65535 distinct flip masks"):
        w18.pauli_step_complex(many, np.zeros_like(many), np.ones(len(many)), 16, seed=1)
    assert sum(w18.timing_get(i)["launches"] for i in range(3)) == 0
    # uncommitted parameters
    raw = _lib.NativeWavefunction(_lib.MODEL_CRNN_U1, N, 1, (H,))
    assert call(h=raw.h) == -3 and "not committed" in last(raw.h)
    # stacked layers
    st = make_wf(N, H, P.init_gru_params([H, H], seed=1, heads=CR.HEADS), layers=2)
    st.timing_enable(True)
    with pytest.raises(ValueError, match="one GRU layer only"):
        st.pauli_step_complex(x01, one, [1.0], ns)
    assert sum(st.timing_get(i)["launches"] for i in range(3)) == 0
    # the refused calls launched nothing and left the resident batch usable
    assert sum(wf.timing_get(i)["launches"] for i in range(3)) == 0
    g1 = wf.vmc_gradient(mean, ns, shapes)["wf_dense_ampl/kernel"]
    assert np.array_equal(g0, g1)
    # every other model is refused by name, with a pointer to its own entry point
    for model, nx, ny, name in [(_lib.MODEL_GRU1D, N, 1, "GRU1D"), (_lib.MODEL_GRU1D_F64, 3, 2, "GRU1D_F64"), (_lib.MODEL_GRU1D_PARITY, N, 1, "GRU1D_PARITY"),
                                (_lib.MODEL_MDRNN2D, 3, 2, "MDRNN2D"), (_lib.MODEL_LSTM1D_F64, 3, 2, "LSTM1D_F64")]:
        w = _lib.NativeWavefunction(model, nx, ny, (H,))
        w.timing_enable(True)
        with pytest.raises(ValueError, match=r"model is %s; rnnwf_pauli_step serves the GRU models, rnnwf_pauli_step_2d the 2D RNN" % name):
            w.pauli_step_complex(x01, one, [1.0], ns)
        with pytest.raises(ValueError, match="CRNN_U1"):
            OC.pauli_expectations(w, ["XXIIII"], ns)
        assert sum(w.timing_get(i)["launches"] for i in range(3)) == 0
    # the existing entry points still refuse the complex RNN
    with pytest.raises(ValueError, match="not implemented for the complex RNN"):
        wf.pauli_step(x01, one, [1.0], ns)
    with pytest.raises(ValueError, match="complex RNN"):
        O.pauli_expectations(wf, ["XXIIII"], ns)
    with pytest.raises(ValueError, match="CRNN_U1"):
        wf.pauli_step_2d(x01, one, [1.0], ns)
