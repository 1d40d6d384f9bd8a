"""CMBlikes / BK foreground HIP kernels vs the compiled reference (golden
fixtures on the reference's own datasets) and the numpy oracle.  GPU only.

Tolerances (fp64): gaussian likelihoods rtol 1e-10; HL likelihoods rtol 1e-9
-- the GPU eigensolver (wave-parallel Jacobi) and DSYEV round differently
and the HL map g(x) = sqrt(2 (x - ln x - 1)) amplifies rounding near x = 1.
Both are far inside the north star's |d lnL| < 1e-6.
"""
import os

import numpy as np
import pytest

import cmblikes_oracle as co
from cosmomc_amd import synthetic as syn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = ["lensing_consext8", "bkplanck_3map_bins1to5", "bkplanck_all_maps", "bkplanck_decorr_lin_quad",
         "bkplanck_EB_4map", "sptsz_aberration_calprior", "bk15_B_12maps", "bk15_B_decorr_bandcentre",
         "bkplanck_calparam_prior"]
HL = {"bkplanck_3map_bins1to5", "bkplanck_all_maps", "bkplanck_decorr_lin_quad", "bkplanck_EB_4map",
      "bk15_B_12maps", "bk15_B_decorr_bandcentre", "bkplanck_calparam_prior"}


def _open(refdata, c):
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    return NativeCMBLikelihood(c["tag"], os.path.join(refdata, c["dataset"]), c["overrides"])


def _tol(case):
    return (1e-9, 1e-8) if case in HL else (1e-10, 1e-9)


@pytest.mark.parametrize("case", CASES)
def test_cmblikes_vs_reference_golden(cmbl_golden, refdata, case):
    c = cmbl_golden["cases"][case]
    like = _open(refdata, c)
    th = torch.tensor(syn.walker_theory(c["walkers"], seed=c["theory_seed"], lmax=c["lmax"]), device="cuda")
    nu = torch.tensor(c["nuis"], dtype=torch.float64, device="cuda")
    got = like.loglike_batch(th, nu).cpu().numpy()
    rtol, atol = _tol(case)
    np.testing.assert_allclose(got, c["minus_lnL"], rtol=rtol, atol=atol)
    assert like.status() == 0          # every HL eigensolve converged within the sweep cap


@pytest.mark.parametrize("case", ["lensing_consext8", "bkplanck_3map_bins1to5", "sptsz_aberration_calprior",
                                  "bk15_B_12maps", "bkplanck_calparam_prior"])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 130])
def test_cmblikes_walker_counts_vs_oracle(cmbl_golden, refdata, case, W):
    c = cmbl_golden["cases"][case]
    like = _open(refdata, c)
    o = co.CMBLikesOracle(os.path.join(refdata, c["dataset"]), c["overrides"], c["tag"])
    th = syn.walker_theory(W, seed=99 + W, lmax=c["lmax"])
    base = np.array(c["nuis"])
    nu = base[np.arange(W) % len(base)]
    got = like.loglike_batch(torch.tensor(th, device="cuda"), torch.tensor(nu, device="cuda")).cpu().numpy()
    idx = sorted(set([0, W - 1, W // 2, min(W - 1, 64)]))
    ref = np.array([o.loglike(th[w], nu[w]) for w in idx])
    rtol, atol = _tol(case)
    np.testing.assert_allclose(got[idx], ref, rtol=rtol, atol=atol)


def test_cmblikes_strided_theory(cmbl_golden, refdata):
    """Padded rows (ld_field > lmax+1) and a strided nuisance column."""
    c = cmbl_golden["cases"]["lensing_consext8"]
    like = _open(refdata, c)
    W = 9
    th = syn.walker_theory(W, seed=c["theory_seed"], lmax=c["lmax"])
    big = np.zeros((W, 10, 2600))
    big[:, :, :c["lmax"] + 1] = th
    nu = np.zeros((W, 3))
    nu[:, 2] = 1.0 + 0.002 * np.arange(W)
    got = like.loglike_batch(torch.tensor(big, device="cuda"), torch.tensor(nu, device="cuda")[:, 2:3]).cpu().numpy()
    o = co.CMBLikesOracle(os.path.join(refdata, c["dataset"]), c["overrides"], c["tag"])
    ref = [o.loglike(th[w], nu[w, 2:3]) for w in range(W)]
    np.testing.assert_allclose(got, ref, rtol=1e-10)


def test_cmblikes_metadata(cmbl_golden, refdata):
    lens = _open(refdata, cmbl_golden["cases"]["lensing_consext8"])
    assert lens.nuisance_names == ["calPlanck"]
    # T, E, P required: TT EE PP, plus TE (CMBlikes.f90:661-668)
    assert lens.cl_lmax[0][0] == lens.cl_lmax[1][1] == lens.cl_lmax[3][3] == lens.cl_lmax[1][0] == 2500
    bk = _open(refdata, cmbl_golden["cases"]["bkplanck_all_maps"])
    assert bk.nuisance_names[:2] == ["BBdust", "BBsync"] and len(bk.nuisance_names) == 16
    assert bk.cl_lmax[1][1] == bk.cl_lmax[2][2] == 600


def test_cmblikes_many_walkers_sampled(cmbl_golden, refdata):
    """W = 1024 BK (HL, all maps): spot-check walkers against the oracle."""
    c = cmbl_golden["cases"]["bkplanck_all_maps"]
    like = _open(refdata, c)
    W = 1024
    th = syn.walker_theory(W, seed=5, lmax=600)
    base = np.array(c["nuis"])
    nu = base[np.arange(W) % len(base)]
    got = like.loglike_batch(torch.tensor(th, device="cuda"), torch.tensor(nu, device="cuda")).cpu().numpy()
    o = co.CMBLikesOracle(os.path.join(refdata, c["dataset"]), c["overrides"], c["tag"])
    for w in (0, 333, 1023):
        assert got[w] == pytest.approx(o.loglike(th[w], nu[w]), rel=1e-9)


BK15_NAMES = ("BK15_95_E BK15_95_B BK15_150_E BK15_150_B BK15_220_E BK15_220_B W023_E W023_B P030_E P030_B "
              "W033_E W033_B P044_E P044_B P070_E P070_B P100_E P100_B P143_E P143_B P217_E P217_B "
              "P353_E P353_B").split()


@pytest.mark.parametrize("nmaps", [1, 2, 5, 7, 9, 13, 16])
def test_hl_every_kernel_width(cmbl_golden, refdata, nmaps):
    """The HL kernel at every packed width (M = 2, 6, 8, 10, 14, 16 lanes per
    matrix; 12 is the BK15 golden case): BK15 map subsets, E and B mixed,
    against the numpy oracle."""
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    c = cmbl_golden["cases"]["bk15_B_12maps"]
    ov = {"maps_use": " ".join(BK15_NAMES[:nmaps]), "use_min": "1", "use_max": "9"}
    like = NativeCMBLikelihood(c["tag"], os.path.join(refdata, c["dataset"]), ov)
    o = co.CMBLikesOracle(os.path.join(refdata, c["dataset"]), ov, c["tag"])
    W = 7
    th = syn.walker_theory(W, seed=500 + nmaps, lmax=c["lmax"])
    base = np.array(c["nuis"])
    nu = base[np.arange(W) % len(base)]
    got = like.loglike_batch(torch.tensor(th, device="cuda"), torch.tensor(nu, device="cuda")).cpu().numpy()
    ref = np.array([o.loglike(th[w], nu[w]) for w in range(W)])
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-8)


@pytest.mark.parametrize("case", ["bkplanck_3map_bins1to5", "bk15_B_12maps"])
def test_hl_non_positive_definite_theory_is_nan(cmbl_golden, refdata, case):
    """A trial theory whose binned C is not positive definite (here a strongly
    negative BB spectrum): the reference's CMBLikes_Transform takes sqrt / log
    of DSYEV's negative eigenvalues (CMBlikes.f90:877-894) and the point gets
    NaN, which the Metropolis test rejects.  The V-free eigensolver recovers the
    eigenvalues' signs, so such walkers give NaN too, and the walkers beside
    them in the launch keep the oracle's value."""
    c = cmbl_golden["cases"][case]
    like = _open(refdata, c)
    o = co.CMBLikesOracle(os.path.join(refdata, c["dataset"]), c["overrides"], c["tag"])
    W = 6
    th = syn.walker_theory(W, seed=77, lmax=c["lmax"])
    bad = [0, 3, 4]
    for w in bad:
        th[w, 5, :] = -1000.0 * np.abs(th[w, 5, :]) - 1.0      # BB << 0: C has a negative eigenvalue
    base = np.array(c["nuis"])
    nu = base[np.arange(W) % len(base)]
    got = like.loglike_batch(torch.tensor(th, device="cuda"), torch.tensor(nu, device="cuda")).cpu().numpy()
    assert np.all(np.isnan(got[bad])), got
    good = [w for w in range(W) if w not in bad]
    ref = np.array([o.loglike(th[w], nu[w]) for w in good])
    np.testing.assert_allclose(got[good], ref, rtol=1e-9, atol=1e-8)


@pytest.mark.parametrize("case", ["bkplanck_all_maps", "bk15_B_12maps"])
def test_hl_result_independent_of_walker_order(cmbl_golden, refdata, case):
    """A walker's HL -lnL depends on its own theory and nuisances only: the
    Jacobi sweep stop is per problem (cmblhl.h hl_ojacobi), so which
    walkers share its wave does not change its bits.  The same 192 walkers in
    their order, reversed, and in a random permutation give the same values
    bit for bit, against one another and against each walker evaluated alone."""
    c = cmbl_golden["cases"][case]
    like = _open(refdata, c)
    W = 192
    th = syn.walker_theory(W, seed=5, lmax=c["lmax"])
    base = np.array(c["nuis"])
    nu = base[np.arange(W) % len(base)] * (1.0 + 1e-3 * np.sin(np.arange(W)))[:, None]
    th[W // 2:] *= 1.0 + 0.05 * np.cos(np.arange(W - W // 2))[:, None, None]   # walkers far from the fiducial too

    def run(order):
        t = torch.tensor(np.ascontiguousarray(th[order]), device="cuda")
        n = torch.tensor(np.ascontiguousarray(nu[order]), device="cuda")
        out = np.empty(W)
        out[order] = like.loglike_batch(t, n).cpu().numpy()
        return out

    ref = run(np.arange(W))
    assert np.all(np.isfinite(ref))
    for order in (np.arange(W)[::-1], np.random.default_rng(3).permutation(W)):
        np.testing.assert_array_equal(run(order), ref)
    for w in (0, 17, W - 1):
        one = like.loglike_batch(torch.tensor(th[w:w + 1], device="cuda"), torch.tensor(nu[w:w + 1], device="cuda"))
        assert one.cpu().numpy()[0] == ref[w]
    assert like.status() == 0
