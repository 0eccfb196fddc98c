"""The ping-pong kernels' MFMA segment (split_mfma_asm.h) reads each weight fragment once and issues all its products from the same
registers: set (weight part, quad) x state parts x tiles.  A wrong fragment offset, a product paired with the wrong state quad, a
tile fed another tile's fragment or a ring slot refilled too early changes whole pre-activations, so it shows on every row.  This
module compares the bf16x3 engine with float64 at the smallest shapes that reach every instantiation of the generated block:

  one layer, positive GRU   37, 44, 50 units (ends and middle of the K-packed class: RJ and the mixed-tile slots differ), N = 33 (one
                            spin word and one site), 40 samples (one full 32-chain tile and a ragged one of 8): prnn_flip_pp_kernel.
                            Every row of the queue, E_loc and row 0, judged by flip_rows_reference.judge.
  layer pipeline            units (50, 50) and (44, 37), N = 33, 40 samples: prnn_flip_pp_kernel below, prnn_flip_pp_upper_kernel on
                            top - the block twice per step (X block from zero, H block continuing three tiles).  Same judge.
  complex RNN               50 units, one layer and (50, 50), N = 34, 40 samples: crnn_swap_pp_kernel and crnn_swap_pp_upper_kernel
                            (three head rows).  Every amplitude ratio of the periodic chain's 2 N bonds through the one-hot probe of
                            test_gpu_crnn_swap_full.py, judged by crnn_swap_reference.judge_probes.

Bounds: the references' own (16 x the per-chain deviation of four float32 restatements from float64 on the same inputs; module
docstrings of flip_rows_reference and crnn_swap_reference), nothing taken from a kernel.  The batches are far below the size at which
the positive GRU chooses bf16x3 by itself, so every handle is created under RNNWF_ENGINE=bf16x3 - the library reads the switch once
per handle, in rnnwf_create (rnnwf_api.hip: read_knobs), so it is set around the creation alone (make_wf), as in
test_gpu_flip_rows_full.py - and the engine that ran is asserted.

On the CPU, with the oracle's own sampler on the same seeds (profiles/pp_fragment_order.txt): every float32 realisation is finite,
and an honest float32 evaluation in a fifth summation order lies at most 0.11 of the row bound; of the ratio bound 0.24 (one layer)
and 0.83 (two layers), both at entries whose bound is the rounding of the complex64 output, not the ratio term.
Measured on an MI355X (same file), worst deviation / bound: rows 0.08 (37 units), 0.07 (44), 0.08 (50), pipeline 0.08 (50, 50) and
0.10 (44, 37), E_loc <= 0.02, row 0 equals log_prob(s); ratios 0.24 (one layer), 0.83 (two layers) - the same output-rounding
entries as on the CPU.  The module takes 3 s.
"""
import numpy as np
import pytest

import crnn_swap_reference as C
import flip_rows_reference as F
from test_gpu_sampler_full import make_wf

pytestmark = pytest.mark.gpu

NS = 40
PIN = {"RNNWF_ENGINE": "bf16x3"}


@pytest.mark.parametrize("units", [(37,), (44,), (50,), (50, 50), (44, 37)], ids=["w37", "w44", "w50", "l2-50-50", "l2-44-37"])
def test_flip_queue_rows_against_float64(units, monkeypatch):
    N = 33
    prm = F.build_params("gru", units)
    wf = make_wf("gru", (N, 1), units, prm, monkeypatch, PIN)
    s = wf.sample(NS, seed=F.SEED, step=0).reshape(NS, N)
    Jz = F.couplings(N)
    lp = np.full((N + 1) * NS, np.nan)
    e = wf.tfim_eloc(s, Jz, F.BX, log_probs=lp)
    lp = lp.reshape(N + 1, NS)
    assert wf.engine_name() == "bf16x3", "%s ran on %s" % (units, wf.engine_name())
    ref = F.Reference("gru", prm, s, Jz, F.BX, None, np.arange(NS), NS, 32)
    log_prob = wf.log_prob(s)
    label = "[pp fragment order, gru %s]" % (units,)
    # the figures first, so that a failing case still prints them
    print(F.line(label, F.measure(lp, e, ref, log_prob), ref.seconds))
    F.judge(lp, e, ref, log_prob, None, label)


@pytest.mark.parametrize("units", [(50,), (50, 50)], ids=["w50", "l2-50-50"])
def test_swap_amplitude_ratios_against_float64(units, monkeypatch):
    N = 34
    prm = C.build_params(units)
    wf = make_wf("crnn", (N, 1), units, prm, monkeypatch, PIN)
    s = wf.sample(NS, seed=C.SEED, step=0).reshape(NS, N)
    assert np.all(s.sum(axis=1) == N // 2)
    ref = C.Reference(prm, s, np.arange(NS), NS, 32)
    slots = np.arange(2 * N)
    anti = s[:, ref.lo].T != s[:, ref.hi].T
    E = np.empty((2 * N, NS), dtype=np.complex128)
    for slot in slots:
        J1, J2, Bz = C.one_hot_couplings(N, slot)
        e, ncon = wf.j1j2_eloc(s, J1, J2, Bz, periodic=True, marshall=False)
        assert ncon == NS + int(anti[slot].sum())
        E[slot] = e
    assert wf.engine_name() == "bf16x3", "%s ran on %s" % (units, wf.engine_name())
    label = "[pp fragment order, crnn %s]" % (units,)
    print(C.probe_line(label, C.measure_probes(E, ref, slots), ref.seconds))
    C.judge_probes(E, ref, slots, label)
    C.assert_sharp(ref, label)
