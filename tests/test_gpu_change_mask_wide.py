"""The change mask's compaction beyond 1024 walkers.  GPU only.

like_compact_kernel (sampler.hip) is one 1024-thread block per sparse
likelihood; thread t scans the flags of walkers [t chunk, min(W, (t + 1) chunk))
with chunk = ceil(W / 1024).  Every other masked test has W <= 1024, where
chunk is 1: here W = 1025 (chunk 2: the last busy thread holds one walker, half
the threads none) and W = 2500 (chunk 3, a clipped last range, threads past
the end), in the set-up of test_gpu_sampler.py's test_change_mask_matches_dense:
plik_lite on calPlanck and BICEP/Keck/Planck (3 maps) on six foreground
parameters in separate fast blocks, wide bounds, T = 1, so each step every
walker re-evaluates only the likelihood its own trial moved and each sparse
likelihood runs on a compacted subset.  One walker group (masked, sparse) and
two groups (dense: every likelihood for every walker) must make the same
decisions and end on the same bits, and the terms at the final points are the
oracles'.

The walkers start at points of their own (the existing test starts them all
at one point), so at every step each walker's terms differ from every other's
and a wrong slot -> walker map cannot give a walker a right value by accident;
the masked run alone is checked for that, and for an accepted walker at or
beyond 1024, before the comparison.
"""
import os

import numpy as np
import pytest

import cmblikes_oracle as co
import pyoracle as po
from cosmomc_amd import synthetic as syn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 8
VARY = [2, 3, 4, 5, 6, 8, 9]             # calPlanck, Adust, Async, alphadust, betadust, alphasync, betasync
WIDTH = [0.1, 2.0, 1.0, 0.5, 0.5, 1.0, 1.0]
SIGMA = np.array([0.002, 0.1, 0.05, 0.02, 0.02, 0.05, 0.05])


def _run_pair(cmbl_golden, refdata, path, W, th):
    """The masked (one group) and the dense (two groups) run of STEPS fast
    steps on theory th ([1, ...]: shared, ld_walker = 0; [W, ...]: per walker):
    ((P, CurLike, mult, num_accept, history terms) of each, the start point)."""
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    from cosmomc_amd.sampler import BatchedMCMC
    bc = cmbl_golden["cases"]["bkplanck_3map_bins1to5"]
    plik = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(path))
    bk = NativeCMBLikelihood(bc["tag"], os.path.join(refdata, bc["dataset"]), bc["overrides"])
    plik.nuisance_indices = [2]
    bk.nuisance_indices = list(range(3, 19))
    dl = torch.tensor(th, device="cuda")
    if th.shape[0] == 1:
        dl = dl.expand(W, -1, -1)
    bk0 = np.array(bc["nuis"][0])
    bk0[1] = 0.5                                      # Async > 0
    P0 = np.concatenate([[0.0222, 1.0], bk0])
    pmin, pmax = P0.copy(), P0.copy()
    for i, wdt in zip(VARY, WIDTH):
        pmin[i - 1], pmax[i - 1] = P0[i - 1] - wdt, P0[i - 1] + wdt
    pm, ps = np.zeros(18), np.zeros(18)
    pm[1], ps[1] = 1.0, 0.0025
    start = np.tile(P0, (W, 1))                       # each walker half a proposal sigma round P0
    start[:, [i - 1 for i in VARY]] += 0.5 * SIGMA * syn.gaussians(1025, W * len(VARY)).reshape(W, -1)
    runs = []
    for g in (1, 2):
        s = BatchedMCMC(W, 18, VARY, [[1], [2, 3, 4, 5, 6, 7]], 0, pmin, pmax, pm, ps, temperature=1.0,
                        seed_ij=41, seed_kl=42)
        s.set_covariance(np.diag(SIGMA ** 2))
        s.set_groups(g)
        s.add_likelihood(plik, dl)
        s.add_likelihood(bk, dl)
        s.enable_history(STEPS)
        s.set_start(start)
        s.step(STEPS, fast_only=True)
        P, lk, mult, nacc = s.state()
        runs.append((P.copy(), lk.copy(), mult.copy(), nacc.copy(), s.history_terms(0, STEPS)))
        s.close()
    return runs, start


def _check(cmbl_golden, refdata, runs, start, W, th):
    a, b = runs
    P, lk, mult, nacc, terms = a
    # the masked run alone: walkers beyond the first 1024 moved, and no two walkers share a term
    assert np.any(nacc[1024:] > 0), "no walker at or beyond 1024 accepted a trial"
    assert np.any(P[:1024] != start[:1024]) and np.all(np.isfinite(terms))
    n_unique = len(np.unique(terms[-1, 0]))
    print(f"W = {W}: {int(np.sum(nacc[1024:] > 0))} of {W - 1024} walkers >= 1024 accepted, "
          f"{n_unique} distinct final plik terms, {len(np.unique(terms[-1, 1]))} distinct BK terms")
    assert n_unique > W // 2
    for x, y in zip(a[3::-1], b[3::-1]):              # num_accept, mult, CurLike, P
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(terms, b[4])
    bc = cmbl_golden["cases"]["bkplanck_3map_bins1to5"]
    ob = co.CMBLikesOracle(os.path.join(refdata, bc["dataset"]), bc["overrides"], bc["tag"])
    op = po.PlikLite(syn.make_plik_lite(12345))
    for w in (0, 1023, 1024, W - 1):
        t = th[0 if th.shape[0] == 1 else w]
        assert terms[-1, 0, w] == pytest.approx(op.loglike(t, P[w, 1]), rel=1e-9)
        assert terms[-1, 1, w] == pytest.approx(ob.loglike(t, P[w, 2:]), rel=1e-9)


@pytest.mark.parametrize("W", [1025, 2500])
def test_change_mask_beyond_1024_walkers_shared_theory(cmbl_golden, refdata, tmp_path, W):
    th = syn.walker_theory(1, seed=8, n_fields=10, ld_field=2512)
    runs, start = _run_pair(cmbl_golden, refdata, str(tmp_path), W, th)
    _check(cmbl_golden, refdata, runs, start, W, th)


def test_change_mask_beyond_1024_walkers_per_walker_theory(cmbl_golden, refdata, tmp_path):
    """W = 1025 with a theory row per walker (130 theories tiled, w % 130):
    gather_theory_kernel reads a slot -> walker map that reaches walker 1024."""
    W = 1025
    th = syn.walker_theory(130, seed=8, n_fields=10, ld_field=2512)[np.arange(W) % 130]
    runs, start = _run_pair(cmbl_golden, refdata, str(tmp_path), W, th)
    _check(cmbl_golden, refdata, runs, start, W, th)
