"""rnnwf_renyi2_regions_stack on every shape of tests/test_gpu_shape_dispatch.py's matrix (4 sites, 8 pairs): the stacks of the positive
GRU models - one case per (layers, width class) with kernels - return finite sums; every one-layer shape and every other family is
refused with ValueError.  Nothing here checks a value: tests/test_gpu_renyi_stack.py does."""
import numpy as np
import pytest

import test_gpu_shape_dispatch as D

pytestmark = pytest.mark.gpu
NPAIRS = 8
REGION = np.array([1, 1, 0, 0], dtype=np.int32)


def served(family, units):
    return family in ("gru", "gru64") and len(units) > 1


def test_the_matrix_has_every_stack_row():
    stacks = {(f, len(u), D.nfull(f, u)) for f, u in D.CASES if served(f, u)}
    assert stacks == {(f, nl, nf) for f in ("gru", "gru64") for nl in (2, 3, 4) for nf in D.STACKS[f]}


@pytest.mark.parametrize("family,units", D.CASES, ids=[D.ident(*c) for c in D.CASES])
def test_the_stack_entry_is_served_or_refused(family, units):
    wf = D.handle(family, units)
    try:
        wf.init_params(D.SEED)
        assert wf.N == 4
        if served(family, units):
            out = wf.renyi2_regions_stack(REGION, NPAIRS, seed=D.SEED, log_ratio=True)
            assert out["sums"].shape == (1, 2) and D.finite(out) and np.all(out["sums"] > 0.0)
        else:
            with pytest.raises(ValueError, match="rnnwf_renyi2_regions_stack: "):
                wf.renyi2_regions_stack(REGION, NPAIRS, seed=D.SEED)
    finally:
        wf.close()
