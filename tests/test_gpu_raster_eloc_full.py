"""The local-energy (flip) pass of the two float64 raster models - the LSTM (lstm_flip_kernel) and the float64 GRU, one layer and
stacks (the f64 instantiations of the GRU flip kernels that eloc_on_device of prnn.hip launches) - at real lattice sizes: 32 to 144
sites, two to five 32-bit spin words, every NFULL, ragged last blocks, more tiles than waves, several passes under a state budget.

Every case draws its samples with sample(ns, seed=111, step=0) on sharpened weights (kernels x 3, every bias randomised:
sampler_reference.build_params), takes random bonds Jz (so that a transposed bond index shows), Bx = 3, and hands the whole
log-probability queue of tfim_eloc(..., log_probs=lp) - row 0 log P(s), row k + 1 log P(s with site k flipped) - and the energies
to raster_eloc_reference.judge:

  every queue entry   |lp - lp_ref| <= 1e-11 N                      (the log P tolerance of test_gpu_lstm.py / test_gpu_prnn.py)
  row 0               bit for bit wf.log_prob(s)                    (the same base kernel)
  E_loc per sample    |e - e_ref| <= Bx sum_k r_k 1e-11 N + 1e-13 (|diag| + Bx sum_k r_k),  r_k from the reference alone

against chains scored from site 0 in float64 by the oracle's estimator.  The rows are judged one by one because with sharp weights
the ratios span many orders of magnitude: a wrong small ratio is invisible in E_loc and obvious in its row
(test_raster_eloc_reference.py shows both, that the float64 reference stays below a tenth of the row bound against numpy.longdouble
on every case, and that `judge` refuses the defects these cases are for: spins of sites >= 32 read from word 0, a checkpoint one
site early, a ragged block that takes its last chain, a grid stride that runs once, bonds on the transposed reshape).

A failing row names its tile: row - 1 is the flipped site, chain // 16 the block.

Measured on an MI355X (profiles/raster_eloc_full_size.txt), as fractions of the bounds: LSTM rows <= 2.0e-3 (9x11, 53 units), E_loc
<= 3.7e-5; one-layer float64 GRU rows <= 9.3e-3 (12x12, 100 units), E_loc <= 7.7e-5; stacks rows <= 1.9e-2 (12x12, (50, 50)), E_loc
<= 3.9e-4; the module takes 9 s, the largest reference (544 chains on 5x13) 2.1 s.
"""
import numpy as np
import pytest

import raster_eloc_reference as Q
import sampler_reference as R
from test_gpu_sampler_full import make_wf

pytestmark = pytest.mark.gpu


def eloc_with_queue(wf, s, Jz, Bx=Q.BX):
    lp = np.full((s.shape[1] + 1) * len(s), np.nan)
    e = wf.tfim_eloc(s, Jz, Bx, log_probs=lp)
    return e, lp.reshape(s.shape[1] + 1, len(s))


@pytest.mark.parametrize("cid,family,units,Nx,Ny,ns,sharp,what", Q.CASES, ids=Q.CASE_IDS)
def test_queue_rows_and_energies_against_float64(cid, family, units, Nx, Ny, ns, sharp, what):
    N = Nx * Ny
    prm = R.build_params(family, units, seed=111, sharp=sharp)
    wf = make_wf(family, (Nx, Ny), units, prm)
    if ns is None:
        cus = wf.device_info()["cu_count"]
        ns = Q.grid_stride_ns(cus)
        tiles = (N - 1) * ((ns + Q.CHAINS - 1) // Q.CHAINS)
        print("[%s] %d CUs: %d chains, %d tiles for at most %d waves" % (cid, cus, ns, tiles, 8 * cus))
        assert tiles > 8 * cus
    s = wf.sample(ns, seed=111, step=0).reshape(ns, N)
    Jz = Q.couplings(Nx, Ny)
    e, lp = eloc_with_queue(wf, s, Jz)
    e_ref, lp_ref, seconds = Q.timed_reference(family, prm, s, Jz, Q.BX, Nx, Ny)
    print(Q.line("[%s]" % cid, Q.measure(lp, e, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny), seconds))
    Q.judge(lp, e, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny, log_prob=wf.log_prob(s), label="[%s: %s]" % (cid, what))


# chains of one 16-chain block's checkpoints: (N - 1) sites x k-steps x 64 lanes x 8 bytes, k-steps = 4 NFULL + 1 per hidden vector;
# the LSTM keeps h and c (lstm.hip: hck_bytes_per_block), the one-layer GRU h (prnn.hip)
@pytest.mark.parametrize("family,vectors", [("lstm", 2), ("gru64", 1)])
def test_several_passes_on_several_words_are_bit_identical(family, vectors, monkeypatch):
    Nx, Ny, units, ns = 5, 13, (50,), 80
    N = Nx * Ny
    prm = R.build_params(family, units, seed=111, sharp=3.0)
    one = make_wf(family, (Nx, Ny), units, prm)
    many = make_wf(family, (Nx, Ny), units, prm, monkeypatch, {"RNNWF_STATE_BUDGET_MB": "1"})
    per_block = (N - 1) * vectors * 13 * 64 * 8
    chains = max(1, (1 << 20) // per_block) * Q.CHAINS
    passes = -(-ns // chains)
    print("[passes %s] %d bytes of checkpoints per block: %d chains per pass, %d passes" % (family, per_block, chains, passes))
    assert passes == (5 if family == "lstm" else 3)
    s = one.sample(ns, seed=111, step=0).reshape(ns, N)
    Jz = Q.couplings(Nx, Ny)
    e1, lp1 = eloc_with_queue(one, s, Jz)
    e2, lp2 = eloc_with_queue(many, s, Jz)
    assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)
    e_ref, lp_ref, seconds = Q.timed_reference(family, prm, s, Jz, Q.BX, Nx, Ny)
    m = Q.judge(lp2, e2, lp_ref, e_ref, s, Jz, Q.BX, Nx, Ny, log_prob=many.log_prob(s), label="[passes %s]" % family)
    print(Q.line("[passes %s]" % family, m, seconds))


@pytest.mark.parametrize("Nx,Ny", [(5, 13), (12, 12)])
@pytest.mark.parametrize("family,units", [("lstm", (50,)), ("gru64", (50,)), ("gru64", (20, 20))], ids=["lstm", "gru64", "gru64-stack"])
def test_copies_of_one_configuration_give_identical_rows(family, units, Nx, Ny):
    """40 copies span two full 16-chain blocks and the ragged third: every lane, clamped ones included, computes the same."""
    N = Nx * Ny
    prm = R.build_params(family, units, seed=111, sharp=3.0)
    wf = make_wf(family, (Nx, Ny), units, prm)
    s = np.repeat(wf.sample(3, seed=111, step=0).reshape(3, N)[2:], 40, axis=0)
    e, lp = eloc_with_queue(wf, s, Q.couplings(Nx, Ny))
    assert np.all(np.isfinite(lp)) and np.all(lp == lp[:, :1]) and np.all(e == e[0])


@pytest.mark.parametrize("family", ["lstm", "gru64"])
def test_fused_step_equals_sample_and_eloc(family):
    Nx, Ny, units, ns = 10, 10, (50,), 64
    N = Nx * Ny
    prm = R.build_params(family, units, seed=111, sharp=3.0)
    wf = make_wf(family, (Nx, Ny), units, prm)
    Jz = Q.couplings(Nx, Ny)
    out = wf.vmc_step(ns, seed=111, step=0, couplings=np.append(Jz.ravel(), Q.BX), want_samples=True, want_eloc=True)
    s = wf.sample(ns, seed=111, step=0)
    assert np.array_equal(out["samples"], s)
    e = wf.tfim_eloc(s, Jz, Q.BX)
    assert np.array_equal(out["eloc"], e)
    m = out["moments"]
    assert m[2] == ns and np.isclose(m[0], e.sum(), rtol=1e-13, atol=0) and np.isclose(m[1], (e * e).sum(), rtol=1e-13, atol=0)
