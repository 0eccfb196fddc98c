"""The local-energy (flip) pass of the 2D RNN - mdrnn_flip_kernel (csrc/mdrnn_kernels.h) driven by eloc_on_device (csrc/mdrnn.hip),
benchmark config 4 - row by row against float64 at real sizes: 35 to 256 sites, two to eight spin words, non-square lattices either
way round, every width class and remainder, ragged last blocks, tiles beyond the first lap of the persistent grid, several passes.

Every case draws its chains with sample(ns, seed=111, step=0) on sharpened weights (kernels x the case's scale, every bias randomised:
sampler_reference.build_params), takes random bonds Jz and Bx = 3, runs tfim_eloc(s, Jz, Bx, log_probs=lp) ONCE on the whole batch
and hands the queue rows and energies of whole 16-chain blocks - the first, the last (ragged where the case is) and fixed positions
between, never chosen by outcome; every flipped site of each - to mdrnn_flip_reference.judge:

  every queue entry   |lp - lp_ref| <= 1e-11 N         the family's bound; licensed by test_mdrnn_flip_reference.py: on these very
                                                       chains two float64 realisations stay within 1/16 of it of numpy.longdouble
  E_loc per chain     |e - e_ref| <= Bx sum_k r_k 1e-11 N + 1e-13 (|diag| + Bx sum_k r_k), r_k from the reference alone
  no row excused      the float64 reference is finite on every checked row
  sharp               the checked ratios spread, std > 0.2 mean
  row 0               within the row bound of wf.log_prob(s); whether it is bit-equal is printed

What the older tests of this kernel do not reach.  test_gpu_mdrnn.py checks every row on at most 36 sites (two words, first lap of
the grid) and 512 energies of config 4 on glorot weights, where every ratio is about 1.  test_gpu_sharpened.py::test_config4_sharpened
(left as it is) does not exercise the flip pass: measured on the CPU oracle with its exact parameters (init_mdrnn_params(50, seed=111),
kernels x 3, biases randomised with seed 115) the unbounded elu cell saturates - 16 oracle draws held 2 distinct configurations, 94 % of
the flip rows of four of them were -inf (ratios exactly 0), and none of the 16 draws had log P below -4.6.  Here at x 1.25 the checked
chains of config 4 are all distinct, log r spans -32 .. 4.8 and no row is -inf.  test_gpu_pauli_2d_full.py compares this kernel with
the masked-tail kernel, one kernel with another.  test_mdrnn_flip_reference.py shows which bookkeeping defect each case is for.

Measured on an MI355X (profiles/mdrnn_flip_full_size.txt), worst fractions of the row bound / of the E_loc bound: config 4 7.9e-4 /
4.1e-5; the non-square lattices 1.2e-2 (9x11, 17 units) / 3.7e-4 (7x9, 84 units); 16x16 1.3e-3 / 5.2e-5; 1x40 and 40x1 7.4e-4 / 5.1e-5;
on 7x5 the widths at or below 16 4.9e-4 / 2.0e-5, one full tile (17..20) 3.7e-4 / 3.8e-5, two (33..36) 8.5e-4 / 1.2e-4, three (49..52)
5.6e-4 / 6.8e-5, four (65..68) 7.9e-4 / 6.6e-5, five (81..84) 4.1e-4 / 4.6e-5.  Row 0 equalled log_prob(s) bit for bit everywhere.  The
module's 42 tests take 4.4 s; the largest reference (48 chains of 16x16) 0.6 s.
"""
import numpy as np
import pytest

import mdrnn_flip_reference as T
from test_gpu_sampler_full import make_wf

pytestmark = pytest.mark.gpu


def handle(Nx, Ny, H, scale, monkeypatch=None, env=None):
    prm = T.build_params(H, scale)
    return make_wf("mdrnn", (Nx, Ny), (H,), prm, monkeypatch, env), prm


def eloc_with_queue(wf, s, Jz, Bx=T.BX):
    ns, N = len(s), s.shape[1] * s.shape[2]
    lp = np.full((N + 1) * ns, np.nan)
    e = wf.tfim_eloc(s, Jz, Bx, log_probs=lp)
    return e, lp.reshape(N + 1, ns)


def run_and_judge(label, wf, prm, Nx, Ny, ns, blocks):
    """One tfim_eloc on the model's own draws; the checked blocks judged.  Returns (figures, samples, energies, queue)."""
    s = wf.sample(ns, seed=T.SEED, step=0)
    assert s.shape == (ns, Nx, Ny)
    Jz = T.couplings(Nx, Ny)
    e, lp = eloc_with_queue(wf, s, Jz)
    chains = T.checked_chains(ns, blocks)
    ref = T.Reference(prm, s[chains], Jz, chains=chains, ns=ns)
    log_prob = wf.log_prob(s[chains].astype(np.int32))
    print(T.line("MDRNN_FLIP_FULL %s" % label, T.measure(lp[:, chains], e[chains], ref, log_prob), ref.seconds))
    m = T.judge(lp[:, chains], e[chains], ref, log_prob, label=label)
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(lp))
    return m, s, e, lp


@pytest.mark.parametrize("cid,Nx,Ny,H,ns,scale,blocks,why", T.CASES, ids=T.CASE_IDS)
def test_every_row_of_the_checked_blocks_against_float64(cid, Nx, Ny, H, ns, scale, blocks, why):
    wf, prm = handle(Nx, Ny, H, scale)
    N = Nx * Ny
    label = "[%s x%.2f: %s]" % (cid, scale, why)
    if cid.startswith("cfg4"):
        # A wave's first tile is its own index, every later one a multiple of the grid's waves further on, and the grid holds at most
        # 8 waves on a CU at up to 3 full tiles (two workgroups of 4 waves): a tile index >= 8 CUs is a second or later tile of its
        # wave.  Tile (i, block) has index i nsb + block: every checked block's tile of the last flipped site, (N - 2) nsb + block, and
        # all of its tiles from site 8 CUs / nsb on, lie beyond the first lap.
        cus = wf.device_info()["cu_count"]
        nsb = (ns + T.CHAINS - 1) // T.CHAINS
        blocks_checked = sorted(set((T.checked_chains(ns, blocks) // T.CHAINS).tolist()))
        print("MDRNN_FLIP_FULL %s %d CUs: %d tiles for at most %d waves; checked blocks %s: beyond the first lap from site %d on" %
              (label, cus, (N - 1) * nsb, 8 * cus, blocks_checked, -(-8 * cus // nsb)))
        assert (N - 1) * nsb == 143 * (625 if ns == 10000 else 626) and blocks_checked[0] == 0 and blocks_checked[-1] == nsb - 1
        assert (N - 2) * nsb + blocks_checked[0] >= 8 * cus
    run_and_judge(label, wf, prm, Nx, Ny, ns, blocks)


@pytest.mark.parametrize("H", T.WIDTHS)
def test_every_width_on_7x5(H):
    """16 f + r for f = 1..5, r = 1..4 and the narrow widths 6, 9, 10, 16: 40 chains, two full blocks and a ragged one, all judged."""
    Nx, Ny = T.WIDTH_LATTICE
    scale = T.width_scale(H)
    wf, prm = handle(Nx, Ny, H, scale)
    nfull = max(1, -(-(H - 4) // 16))                              # rnnwf_api.hip: pick_nfull - the first layout with 16 NFULL + 4 >= H
    rem = "rem %d" % (H - 16 * nfull) if H > 16 * nfull else "no remainder unit"
    run_and_judge("[7x5-%d x%.2f: %d full tile%s, %s]" % (H, scale, nfull, "s" * (nfull > 1), rem), wf, prm, Nx, Ny, T.WIDTH_NS, None)


def test_the_largest_lattice_is_256_sites():
    """16x16 is the largest lattice (eight spin words); 16x17 is refused when its parameters are first committed."""
    with pytest.raises(ValueError, match="above 256 sites"):
        wf, _ = handle(16, 17, 50, 1.0)
        wf.log_prob(np.zeros((1, 16, 17), dtype=np.int32))


def test_85_units_are_refused():
    from rnnwavefunctions_amd import _lib
    with pytest.raises(ValueError, match="2D RNN: <= 84|> 84"):
        _lib.NativeWavefunction(_lib.MODEL_MDRNN2D, 4, 4, (85,))


def test_several_passes_equal_one_pass_bit_for_bit(monkeypatch):
    """12x12, 50 units: a block's states are 144 sites x 7 k-step pairs x 1 KB = 1 032 192 bytes, so an 8 MB budget holds 8 blocks =
    128 chains per pass and 330 chains take three passes, the last one ragged (74 chains: 4 blocks and one of 10)."""
    Nx, Ny, H, ns, scale = 12, 12, 50, 330, 1.25
    one, prm = handle(Nx, Ny, H, scale)
    many, _ = handle(Nx, Ny, H, scale, monkeypatch, {"RNNWF_STATE_BUDGET_MB": "8"})
    m, s, e1, lp1 = run_and_judge("[passes: one]", one, prm, Nx, Ny, ns, 3)
    many.timing_enable(True)
    many.timing_reset()
    e2, lp2 = eloc_with_queue(many, s, T.couplings(Nx, Ny))
    passes = many.timing_get(1)["launches"]                        # one flip launch per pass
    per_block = 144 * 7 * 1024
    print("MDRNN_FLIP_FULL [passes] %d bytes of states per block, %d chains per pass: %d passes" %
          (per_block, (8 << 20) // per_block * T.CHAINS, passes))
    assert passes == 3 == -(-ns // ((8 << 20) // per_block * T.CHAINS))
    assert np.array_equal(e1, e2) and np.array_equal(lp1, lp2)


def test_fused_step_equals_sample_and_eloc():
    Nx, Ny, H, ns, scale = 12, 12, 50, 1000, 1.25
    wf, prm = handle(Nx, Ny, H, scale)
    Jz = T.couplings(Nx, Ny)
    out = wf.vmc_step(ns, seed=T.SEED, step=0, couplings=np.append(Jz.ravel(), T.BX), want_samples=True, want_eloc=True)
    s = wf.sample(ns, seed=T.SEED, step=0)
    assert np.array_equal(out["samples"], s)
    e = wf.tfim_eloc(s, Jz, T.BX)
    assert np.array_equal(out["eloc"], e)
    m = out["moments"]
    assert m[2] == ns and np.isclose(m[0], e.sum(), rtol=1e-13, atol=0) and np.isclose(m[1], (e * e).sum(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("Nx,Ny,H", [(12, 12, 50), (5, 13, 68)])
def test_copies_of_one_configuration_give_identical_rows(Nx, Ny, H):
    """70 copies span four full 16-chain blocks and a ragged one of 6: every lane, clamped ones included, computes the same."""
    wf, prm = handle(Nx, Ny, H, 1.25)
    one = wf.sample(3, seed=T.SEED, step=0)[2:]
    s = np.repeat(one, 70, axis=0)
    Jz = T.couplings(Nx, Ny)
    e, lp = eloc_with_queue(wf, s, Jz)
    assert np.all(np.isfinite(lp)) and np.all(lp == lp[:, :1]) and np.all(e == e[0])
    ref = T.Reference(prm, one, Jz)
    err = np.abs(lp[:, :1] - ref.lp).max()
    print("MDRNN_FLIP_FULL [copies %dx%d] 70 identical lanes; max row error / bound %.3e" % (Nx, Ny, err / (T.ROW_TOL * Nx * Ny)))
    assert np.all(np.isfinite(ref.lp)) and err <= T.ROW_TOL * Nx * Ny
