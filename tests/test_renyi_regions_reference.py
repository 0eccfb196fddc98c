"""The float64 reference of tests/test_gpu_renyi_regions_full.py (tests/renyi_regions_reference.py), validated on its own - no GPU:

1. summed over every pair of configurations, the brute force gives Tr rho_A^2 from the dense vector of all 2^N amplitudes for
   non-prefix subsets (N = 4..6) and on 2x3 / 3x2 rasters (a column cut among them), relative 1e-12; r_A = r_complement; r = 1 for the
   empty and the full region; prefix regions equal tests/renyi_reference.py's cuts; the site-resolved form of the kernels agrees;
2. the bound has teeth at N = 80, 50 units, sharpened weights, model-drawn chains: the reference's own log r with one defect applied
   in NumPy is REJECTED at the bound test_gpu_renyi_regions_full.py enforces for float32 (16 x the float32 oracle's deviation from
   float64, capped at 2 (2e-6 N + 2e-6)), and a float32 evaluation summed in another order is ACCEPTED.

Measured (ratios max |d log r| / bound; 128 pairs x 14 regions, bound 6.36e-5 = 16 x dev32, dev32 = 3.97e-6, the cap 3.24e-4 not reached):
    mask shifted by one site 5.2e4, own spins on A 1.4e5, partner's spins everywhere after f 1.2e5, mask word 0 for sites >= 32
    2.5e4, restart from the partner's checkpoint 2.2e4; float32 in another order 0.054.  (The comparator's "cut" is the region's index.)
"""
import numpy as np
import pytest

import renyi_reference as R
import renyi_regions_reference as G
from conftest import all_configs
from oracle import models as M
from rnnwavefunctions_amd import params as P


def sharpened(H, seed, dtype, scale=3.0):
    return P.randomize_biases(P.scale_kernels(P.init_gru_params([H], seed=seed, dtype=dtype), scale), seed + 1)


def all_pairs(N):
    c = all_configs(N)
    i, j = np.meshgrid(np.arange(2 ** N), np.arange(2 ** N), indexing="ij")
    pairs = np.empty((2 * i.size, N), dtype=np.int32)
    pairs[0::2], pairs[1::2] = c[i.ravel()], c[j.ravel()]
    return c, i.ravel(), j.ravel(), pairs


def mask_of(N, sites):
    m = np.zeros(N, dtype=np.int32)
    m[list(sites)] = 1
    return m


def exact_check(prm, N, masks):
    c, i, j, pairs = all_pairs(N)
    lp = M.prnn_log_probability(prm, c, dtype=np.float64)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    lr = G.log_ratio(prm, pairs, masks)
    w = np.exp(lp[i] + lp[j])
    purity = (w[None, :] * np.exp(lr)).sum(axis=1)
    exact = np.array([G.purity_of_region(np.exp(0.5 * lp), N, m) for m in masks])
    return lr, purity, exact


# ---- 1. the brute force is the estimator ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H", [(4, 6), (5, 20), (6, 10)])
def test_brute_force_over_all_pairs_gives_the_exact_purity_of_non_prefix_subsets(N, H):
    prm = sharpened(H, N + H, np.float64)
    subsets = [[1], [N - 1], [1, 2], [0, 2], [1, N - 1], [0, N - 1], list(range(1, N - 1)), list(range(0, N, 2)), [2, 3], [0, 1, 3]]
    masks = np.stack([mask_of(N, s) for s in subsets])
    lr, purity, exact = exact_check(prm, N, masks)
    rel = np.abs(purity / exact - 1.0)
    print("N=%d H=%d: Tr rho_A^2 = %s, max rel %.2e" % (N, H, np.round(exact, 4), rel.max()))
    assert -np.log(exact.min()) > 0.05                             # entangled: the identity is not trivially 1 = 1
    assert rel.max() <= 1e-12
    # the dense-vector helper itself: a prefix region is the SVD across the cut
    from test_renyi_host import exact_renyi2
    lp = M.prnn_log_probability(prm, all_configs(N), dtype=np.float64)
    S = exact_renyi2(np.exp(0.5 * lp), N)
    for l in range(N + 1):
        assert abs(G.purity_of_region(np.exp(0.5 * lp), N, mask_of(N, range(l))) - np.exp(-S[l])) <= 1e-13


@pytest.mark.parametrize("Nx,Ny", [(2, 3), (3, 2)])
def test_raster_regions_count_raster_sites(Nx, Ny):
    """Site (nx, ny) is raster site ny Nx + nx.  A column cut, a single column, a corner block and a row, by explicit site lists."""
    N, H = Nx * Ny, 10
    prm = sharpened(H, 3, np.float64)
    col0 = [ny * Nx for ny in range(Ny)]
    last = [ny * Nx + Nx - 1 for ny in range(Ny)]
    corner = [0, 1, Nx, Nx + 1]
    row1 = [Nx + nx for nx in range(Nx)]
    masks = np.stack([mask_of(N, s) for s in (col0, last, corner, row1, [Nx + 1])])
    lr, purity, exact = exact_check(prm, N, masks)
    assert np.abs(purity / exact - 1.0).max() <= 1e-12
    # and NOT the other convention: column 0 read as "the first Ny sites" is another number
    psi = np.exp(0.5 * M.prnn_log_probability(prm, all_configs(N), dtype=np.float64))
    assert abs(purity[0] - G.purity_of_region(psi, N, mask_of(N, range(Ny)))) > 1e-4


def test_complement_empty_full_and_prefix_regions():
    N, H = 37, 20
    prm = sharpened(H, 5, np.float32)
    s = np.random.RandomState(3).randint(0, 2, size=(2 * 24, N)).astype(np.int32)
    masks = np.stack([m for _, m in G.region_set(N, 1)])
    lr = G.log_ratio(prm, s, masks)
    assert np.abs(lr).max() > 0.1
    assert np.abs(lr - G.log_ratio(prm, s, 1 - masks)).max() <= 1e-12           # r_A = r_complement
    ends = G.log_ratio(prm, s, np.stack([np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)]))
    assert np.abs(ends).max() <= 1e-12                                          # nothing swapped / everything swapped: r = 1
    cuts = np.array([1, 2, 31, 32, 33, 36])
    prefix = (np.arange(N)[None, :] < cuts[:, None]).astype(np.int32)
    assert np.abs(G.log_ratio(prm, s, prefix) - R.log_ratio_f64(prm, s, cuts)).max() <= 1e-12
    # the site-resolved form of the kernels (normalised mask, first site, mixed chain) is the same number
    assert np.abs(G.mixed_chain_form(prm, s, masks) - lr).max() <= 1e-12
    assert np.abs(G.mixed_chain_form(prm, s, prefix) - R.log_ratio_f64(prm, s, cuts)).max() <= 1e-12


def test_region_set_and_subset_choice_meet_their_conditions():
    for npairs, (Nx, Ny) in [(5000, (80, 1)), (5003, (80, 1)), (500, (33, 1)), (500, (64, 1)), (500, (65, 1)), (203, (40, 1)),
                             (301, (100, 1)), (1003, (6, 6)), (301, (4, 8)), (301, (8, 8))]:
        N = Nx * Ny
        names, masks = zip(*G.region_set(Nx, Ny))
        masks = np.stack(masks)
        assert masks.shape[1] == N and masks.dtype == np.int32 and len(set(names)) == len(names)
        assert all(0 < m.sum() < N for m in masks)
        idx = G.choose_pairs(npairs)
        G.check_subset(npairs, N, idx, masks)
        if Ny > 1:
            for c in range(1, Nx):                                 # every column cut is there
                col = (np.arange(N) % Nx < c).astype(np.int32)
                assert any(np.array_equal(col, m) for m in masks)
    with pytest.raises(AssertionError):                           # a subset without the ragged block's pairs is refused
        G.check_subset(5003, 80, G.choose_pairs(5000), np.stack([m for _, m in G.region_set(80, 1)]))
    with pytest.raises(AssertionError):                           # and one without the last full block
        G.check_subset(5000, 80, G.choose_pairs(5000)[:-8], np.stack([m for _, m in G.region_set(80, 1)]))
    with pytest.raises(AssertionError):                           # and a region set that misses a word boundary
        G.check_subset(5000, 80, G.choose_pairs(5000), np.stack([m for n, m in G.region_set(80, 1) if "64" not in n]))


# ---- 2. the bound rejects what it must -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def config2():
    """N = 80, 50 units, the sharpened weights of the full-size GPU tests (seeds 111 / 112), 128 pairs drawn by the oracle from the
    wave function itself, the full-size region set.  The reference, the float32 oracle's deviation from it and the bound."""
    N, H, npairs = 80, 50, 128
    prm = sharpened(H, 111, np.float32)
    u = np.random.RandomState(1).random_sample((2 * npairs, N))
    s = M.prnn_sample(prm, N, u)[0].astype(np.int32)
    masks = np.stack([m for _, m in G.region_set(N, 1)])
    ref = G.log_ratio(prm, s, masks)
    dev32 = np.abs(G.log_ratio(prm, s, masks, dtype=np.float32) - ref).max()
    bound, capped = R.f32_bound(dev32, N)
    mx, share = R.nontrivial(ref)
    print("config 2, %d pairs x %d regions: max |log r| = %.2f, %.0f %% of the entries above 0.01; dev32 = %.2e, bound %.2e (%s; cap %.2e)"
          % (npairs, len(masks), mx, 100 * share, dev32, bound, "capped" if capped else "16 x dev32", R.f32_ceiling(N)))
    assert mx > 0.1 and share >= 0.25
    pi, ri = np.meshgrid(np.arange(npairs), np.arange(len(masks)), indexing="xy")
    return dict(N=N, prm=prm, s=s, masks=masks, ref=ref, bound=bound, pi=pi.ravel(), ri=ri.ravel())


def _ratio(c, name, got):
    return R.compare("config 2, %s:" % name, np.ravel(got), c["ref"].ravel(), c["pi"], c["ri"], c["bound"])["ratio"]


# log r is O(0.1 - 1) at these weights and the bound O(1e-4): a defect that changes which spins are scored moves SOME entry by a large
# part of its log r.  Required: 100 x the bound (measured: above 1e4, see the module docstring).
WIDE = 100.0


def test_the_site_resolved_form_is_within_the_bound(config2):
    c = config2
    assert _ratio(c, "the site-resolved form itself", G.mixed_chain_form(c["prm"], c["s"], c["masks"])) < 1e-6


def test_bound_rejects_a_mask_shifted_by_one_site(config2):
    c = config2
    shifted = np.concatenate([np.zeros((len(c["masks"]), 1), dtype=np.int32), c["masks"][:, :-1]], axis=1)
    assert _ratio(c, "mask shifted by one site", G.log_ratio(c["prm"], c["s"], shifted)) > WIDE


@pytest.mark.parametrize("defect,what", [("own_on_A", "own instead of the partner's spins on A"),
                                         ("partner_after_f", "the partner's spins everywhere after f"),
                                         ("mask_word_0", "mask words of sites >= 32 read from word 0"),
                                         ("partner_checkpoint", "restart from the partner's checkpoint")])
def test_bound_rejects_a_defect_of_the_mixed_chain(config2, defect, what):
    c = config2
    assert _ratio(c, what, G.mixed_chain_form(c["prm"], c["s"], c["masks"], defect=defect)) > WIDE


def test_bound_accepts_a_float32_evaluation_in_another_order(config2):
    c = config2
    other = G.log_ratio_regions(lambda x: R.log_prob_other_order(c["prm"], x, dtype=np.float32), c["s"], c["masks"])
    assert _ratio(c, "float32, sums in another order", other) <= 1.0
