"""The unified step launch's raw bin sums are stored bin-major, S[Np][Wp]
(steptail.h): the pass's RAW store and the quadratic form's readers
(qfs_body.h) must agree on it for every walker count and matrix size.  The
general schedule (cmamd_debug_pipeline mode 0) never touches that buffer -- its
pass stores calibrated Delta rows walker-major -- so the unified schedule's
state must equal it bit for bit.  GPU only."""
import os

import numpy as np
import pytest

from cosmomc_amd import synthetic as syn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 4
WMAX = 130


@pytest.fixture(scope="module")
def plik_data():
    return syn.make_plik_lite(12345)


@pytest.fixture(scope="module")
def theory():
    return syn.walker_theory(WMAX, seed=11, n_fields=10, ld_field=2512)


def _run(cmbl_golden, refdata, plik_data, tmp_path, th, W, mode, cache=False, plik_over=None):
    """4 fast-only steps of plik_lite + Planck lensing from calPlanck = 1:
    (history rows, history terms, the state image with its RNG rows, state)."""
    from cosmomc_amd import _native as N
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    from cosmomc_amd.sampler import BatchedMCMC
    c = cmbl_golden["cases"]["lensing_consext8"]
    dl = torch.tensor(np.ascontiguousarray(th[:W]), device="cuda")
    plik = NativeCMBLikelihood("PLIK_LITE", plik_data.write(str(tmp_path)), plik_over or {})
    lens = NativeCMBLikelihood(c["tag"], os.path.join(refdata, c["dataset"]), c["overrides"])
    plik.nuisance_indices = [2]
    lens.nuisance_indices = [2]
    s = BatchedMCMC(W, 3, [2], [[1]], 0, [0.0222, 0.9, 3.05], [0.0222, 1.1, 3.05], [0.0, 1.0, 0.0],
                    [0.0, 0.0025, 0.0], seed_ij=61, seed_kl=72)
    s.set_covariance(np.array([[0.002 ** 2]]))
    s.add_likelihood(plik, dl)
    s.add_likelihood(lens, dl)
    assert N.lib().cmamd_debug_fused(s._h) > 0
    if cache:
        s.set_binned_cache(True)
    assert N.lib().cmamd_debug_pipeline(s._h, mode) == 0
    s.enable_history(STEPS)
    s.set_start(np.tile([0.0222, 1.0, 3.05], (W, 1)))
    s.step(STEPS, fast_only=True)
    if mode == 3:
        assert N.lib().cmamd_debug_tail(s._h) == W            # the unified launch ran
    out = (s.history_host(0, STEPS), s.history_terms(0, STEPS), s.save_state(), *s.state())
    assert plik.status() == 0 and lens.status() == 0             # no hand-off gave up
    s.close()
    return out


def _assert_same(a, b):
    assert a[2] == b[2]                                           # P, CurLike, mult, accepts, RANMAR, proposer
    for x, y in ((a[0], b[0]), (a[1], b[1]), *zip(a[3:], b[3:])):
        np.testing.assert_array_equal(x, y)
    assert np.all(np.isfinite(a[1])) and np.any(a[6] > 0)        # real terms, and some walker moved


# one walker; a quarter tile; a tile short of one walker; a whole tile; a second tile of one
# walker (63 of padding); two tiles on different XCDs plus a third of two walkers
@pytest.mark.parametrize("W", [1, 16, 63, 64, 65, 130])
def test_unified_equals_general_schedule(cmbl_golden, refdata, plik_data, theory, tmp_path, W):
    uni = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, W, 3)
    gen = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, W, 0)
    if W == 1:                                                    # (a single walker may well reject 4 trials)
        assert uni[2] == gen[2]
        for x, y in ((uni[0], gen[0]), (uni[1], gen[1])):
            np.testing.assert_array_equal(x, y)
    else:
        _assert_same(uni, gen)


def test_binned_cache_equals_general_schedule(cmbl_golden, refdata, plik_data, theory, tmp_path):
    """The binned-cache steps (mh_tail_kernel) read the sums the call's first
    launch stored."""
    uni = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, WMAX, 3, cache=True)
    gen = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, WMAX, 0)
    _assert_same(uni, gen)


# Other matrix sizes than the full TTTEEE's Np = 640 (ten 64-bin column blocks, items of two):
# TT alone (215 bins, Np = 256, items of one block) and the TTTEEE bins inside L = 100 .. 1500.
# QuadForm::choose_kb gives items of three column blocks only from eleven blocks up, which no
# plik_lite selection reaches (613 bins at most), so no selection runs qfs_body_loop.
@pytest.mark.parametrize("over", [{"use_cl": "TT"}, {"bins_for_L_range": "100 1500"}],
                         ids=["TT_alone", "TTTEEE_L100_1500"])
def test_bin_selection_equals_general_schedule(cmbl_golden, refdata, plik_data, theory, tmp_path, over):
    uni = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, WMAX, 3, plik_over=over)
    gen = _run(cmbl_golden, refdata, plik_data, tmp_path, theory, WMAX, 0, plik_over=over)
    _assert_same(uni, gen)
