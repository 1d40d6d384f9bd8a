"""The galaxy power-spectrum kernels (mpk.hip) at the smallest shapes at which
their 16 x 16 MFMA tiles can go wrong, on seeded data sets made in the test
(mpk_fixture.make_mpk / make_wigglez), against the long-double restatement
(cosmomc_amd.mpk) under the bound of test_gpu_mpk.py (mpk_fixture.GPU_ATOL):

    (np, nk) = (1, 1)    the least size
               (16, 4)   exact tiles (one row tile, one MFMA step in k)
               (17, 5)   one past a tile in both directions
               (33, 67)  several tiles with a ragged edge

with one region ("MPK") and seven ("WIGGLEZ"), in every Q mode the shape
allows (Q_flat needs two points), the 13-vector Q grid at np = 17 among them,
with and without a covariance; and one data set of the real WiggleZ shape,
7 regions x 18 points x 100 kbands with the GiggleZ factor.  A value the
restatement gives as logZero must be logZero."""
import os

import numpy as np
import pytest

import mpk_fixture as mf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
CASES = [(1.0, 14.5, 1.0), (0.87, 14.8, 0.93), (1.13, 14.3, 1.04)]      # a_scl, amp, tilt


@pytest.fixture(scope="module")
def gigglez_src(tmp_path_factory):
    """The four GiggleZ fiducial files: those of a golden."""
    return mf.extract(tmp_path_factory.mktemp("mpk_edges"), names=["wigglez_a"])["wigglez_a"].gigglez_dir


def _check(like, host, W=19):
    from cosmomc_amd import mpk as M
    ds = like.ds
    rows = []
    for i, (a, amp, tilt) in enumerate(CASES):
        DV = ds.DV_fid / (mf.H0 * a) if ds.use_scaling else 1.0
        kh_min = 1e-4 if i < 2 else 1.2 * a * ds.k[0]                  # the last case clamps the first k
        rows.append(M.mpk_theory_row(ds, mf.H0, DV, mf.analytic_pk(ds.redshift, amp, tilt, ds.nonlinear), kh_min))
    rows = np.array(rows)
    want = np.array([float(host(ds, r, np.longdouble)) for r in rows])
    pick = np.arange(W) % len(rows)
    buf = torch.full((W, 1, rows.shape[1] + 3), -3.0, dtype=torch.float64, device="cuda")
    buf[:, 0, :rows.shape[1]] = torch.tensor(rows[pick], device="cuda")
    got = like.loglike_batch(buf[:, :, :rows.shape[1]]).cpu().numpy()
    tag = "WIGGLEZ" if ds.wigglez else "MPK"
    zero = want[pick] == LOGZERO
    print(tag, (ds.np, ds.nk, ds.nr), "q mode", ds.q_mode, "-lnL", want, "max |gpu - long double|:",
          np.abs(got - want[pick])[~zero].max() if np.any(~zero) else None)
    assert np.array_equal(got == LOGZERO, zero)
    np.testing.assert_allclose(got[~zero], want[pick][~zero], rtol=0, atol=mf.GPU_ATOL[tag])
    for i in range(len(rows)):                                          # and every copy of a row has the same bits
        assert len({x.tobytes() for x in got[pick == i]}) == 1
    assert like.workspace_bytes(32) == 2 * like.workspace_bytes(16)


@pytest.mark.parametrize("npts,nk,q,cov", [(1, 1, "none", False), (1, 1, "sigma0", True), (16, 4, "flat", True),
                                           (16, 4, "gauss", False), (17, 5, "flat", False), (17, 5, "gauss", True),
                                           (17, 5, "gauss", False), (33, 67, "flat", True), (33, 67, "gauss", True),
                                           (33, 67, "none", False)])
def test_mpk_shapes(tmp_path, npts, nk, q, cov):
    from cosmomc_amd import mpk as M
    ds = mf.make_mpk(str(tmp_path / "edge"), seed=100 + 7 * npts + nk, npf=npts, nkf=nk, cov=cov, q=q)
    like = M.MPKLikelihood(ds, nonlinear=True)
    assert (like.n_points, like.n_kbands, like.n_regions) == (npts, nk, 1)
    _check(like, M.mpk_loglike_host)


@pytest.mark.parametrize("npts,nk,q", [(1, 1, "none"), (16, 4, "flat"), (17, 5, "gauss"), (17, 5, "flat"),
                                       (33, 67, "gauss"), (33, 67, "none")])
def test_wigglez_shapes_seven_regions(tmp_path, gigglez_src, npts, nk, q):
    from cosmomc_amd import mpk as M
    d = str(tmp_path / "edge")
    ds = mf.make_wigglez(d, seed=200 + 7 * npts + nk, nkf=nk, q=q, regions=(1, 2, 3, 4, 5, 6, 7), z=0.41,
                         sel=(3, 2 + npts, 1, nk), gigglez_src=gigglez_src)
    like = M.WiggleZLikelihood(ds, os.path.join(d, "common.dataset"), use_gigglez=True, nonlinear=True,
                               gigglez_dir=os.path.join(d, "data"))
    assert (like.n_points, like.n_kbands, like.n_regions, like.zbin) == (npts, nk, 7, 2)
    _check(like, M.wigglez_loglike_host)


def test_wigglez_real_shape(tmp_path, gigglez_src):
    """7 regions x 18 of 50 points x 100 kbands, Q_marge = F, GiggleZ: the shape of the real bins."""
    from cosmomc_amd import mpk as M
    d = str(tmp_path / "full")
    ds = mf.make_wigglez(d, seed=301, nkf=100, q="none", regions=(1, 2, 3, 4, 5, 6, 7), z=0.78, sel=(3, 20, 1, 100),
                         gigglez_src=gigglez_src)
    like = M.WiggleZLikelihood(ds, os.path.join(d, "common.dataset"), use_gigglez=True, nonlinear=True,
                               gigglez_dir=os.path.join(d, "data"))
    assert (like.n_points, like.n_kbands, like.n_regions, like.zbin) == (18, 100, 7, 4)
    _check(like, M.wigglez_loglike_host, W=33)
