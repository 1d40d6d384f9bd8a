"""The weak-lensing kernels on in-test datasets (wl_fixture.make_synthetic) whose
sizes reach the edges of their tiles, against the long-double restatement
(wl_loglike_host with np.longdouble): nz in {5, 16, 17, 67} (the MFMA's k in
chunks of 16, a lane 4 consecutive k), nl made small and odd by lmax in {150,
1000}, 1, 15, 17 and 35 Limber columns (16 to a tile), one theta bin used,
first_theta_bin_used = num_theta_bins, a source bin shifted wholly off the
table, sparse evaluation at live counts 0, 1, W - 1 and W, W = 1025 (the
per-walker kernels run 1024 walkers a launch), and one synthetic dataset of
the DES Y1 shape (nz = 353: 22 full k chunks and a tail of one; nl = 75: five
row tiles; 35 columns; 810 points used of a 900-row covariance).

Tolerance: as test_gpu_wl.py, 10 x the larger of (a) = 5.1e-11 measured on the
goldens and (b), f64 against long double, formed here on the host as the
largest difference over the dataset's points; absolute on -lnL.  (a) was
measured on -lnL up to 4.9e4, so the datasets stay near that range: the
covariance of nz5 (a three-row n(z), where the shifted points are far from the
data) is scaled by 100."""
import os

import numpy as np
import pytest

import wl_fixture as wf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A_GOLDEN = 5.1e-11
#        name          make_synthetic arguments                                   nz, Limber columns (None: any)
EDGES = {"nz5": (dict(seed=201, nrows=3, lmax=1000, cov_scale=100.0), 5, None),
         "nz16": (dict(seed=202, nrows=14, lmax=1000), 16, None),
         "nz17": (dict(seed=203, nrows=15, lmax=1000), 17, None),
         "nz67": (dict(seed=204, nrows=65, lmax=1000), 67, None),
         "lmax150": (dict(seed=205, lmax=150), 31, None),
         "pairs1": (dict(seed=206, nsrc=1, ngal=0, data_types="xip xim", lmax=1000), 31, 1),
         "pairs15": (dict(seed=207, nsrc=5, ngal=0, data_types="xip xim", lmax=1000), 31, 15),
         "pairs17": (dict(seed=208, nsrc=3, ngal=3, drop_gammat=1, lmax=1000), 31, 17),
         "pairs35": (dict(seed=209, nsrc=4, ngal=5, lmax=1000), 31, 35),
         "one_theta": (dict(seed=210, select="one", lmax=1000), 31, None),
         "last_theta": (dict(seed=211, select="last", lmax=1000), 31, None)}
_made = {}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("wl_edges")


def _edge(root, name):
    """(synthetic dataset, its likelihood, long-double -lnL of its points, f64 host -lnL), made once."""
    if name not in _made:
        from cosmomc_amd import weaklensing as wl
        s = wf.make_synthetic(os.path.join(str(root), name), **EDGES[name][0])
        ld = np.array([wl.wl_loglike_host(s["ds"], s["row"], p, np.longdouble) for p in s["points"]])
        f64 = np.array([wl.wl_loglike_host(s["ds"], s["row"], p) for p in s["points"]])
        _made[name] = (s, wl.WLLikelihood(s["dataset"]), ld, f64)
    return _made[name]


def _eval(like, row, points):
    W = len(points)
    dl = torch.tensor(np.tile(row, (W, 1))[:, None, :].copy(), device="cuda")
    return like.loglike_batch(dl, torch.tensor(np.ascontiguousarray(points), device="cuda")).cpu().numpy()


def _bound(ld, f64):
    return 10 * max(A_GOLDEN, float(np.abs(f64 - ld).max()))


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_dataset(root, name):
    s, like, ld, f64 = _edge(root, name)
    _, nz, ncol = EDGES[name]
    assert like.nz == nz and (ncol is None or like.n_columns == ncol)
    if name == "lmax150":
        assert like.nl == 29
    if name == "one_theta":
        assert {it[3] for it in s["ds"].used_items} == {3} and like.first_theta_bin_used == 3
    if name == "last_theta":
        assert like.first_theta_bin_used == s["ds"].ntheta == 7
    got = _eval(like, s["row"], s["points"])
    err = np.abs(got - ld).astype(np.float64)
    print(name, "nl", like.nl, "columns", like.n_columns, "n_used", like.n_used, "max |gpu - long double|:", err.max(),
          "bound:", _bound(ld, f64), "-lnL up to", float(ld.max()))
    assert np.all(err <= _bound(ld, f64)), (err, _bound(ld, f64))


def test_source_bin_off_the_table(root):
    """DzS of the first source bin beyond the table's length: n_chi = 0 for it,
    so xi+- of its pairs are 0 and their residuals are minus the data."""
    from cosmomc_amd import weaklensing as wl
    s, like, _, _ = _edge(root, "nz17")
    ds = s["ds"]
    p = s["points"][0].copy()
    p[2 * ds.ngal + ds.nzb + 3] = 5.0
    vec = wl.wl_theory_vector(ds, s["row"], p)
    first = [i for i, it in enumerate(ds.used_items) if ds.data_types[it[0] - 1] in (0, 1) and 1 in it[1:3]]
    assert first and np.all(vec[first] == 0) and np.any(vec != 0)
    ld = np.array([wl.wl_loglike_host(ds, s["row"], p, np.longdouble)])
    f64 = np.array([wl.wl_loglike_host(ds, s["row"], p)])
    got = _eval(like, s["row"], p[None, :])
    assert np.all(np.abs(got - ld).astype(np.float64) <= _bound(ld, f64))


def test_sparse_live_counts(root):
    """loglike_batch_sparse over W = 70 slots with 0, 1, W - 1 and W live: the
    live slots get the dense bits, the others keep what they held."""
    s, like, _, _ = _edge(root, "pairs17")
    W = 70
    rng = np.random.RandomState(9)
    pts = s["points"][rng.randint(0, len(s["points"]), W)]
    dl = torch.tensor(np.tile(s["row"], (W, 1))[:, None, :].copy(), device="cuda")
    nu = torch.tensor(pts, device="cuda")
    dense = like.loglike_batch(dl, nu).cpu().numpy()
    for live in (0, 1, W - 1, W):
        out = torch.full((W,), -7.0, dtype=torch.float64, device="cuda")
        like.loglike_batch_sparse(dl, nu, out, torch.tensor([live], dtype=torch.int32, device="cuda"))
        got = out.cpu().numpy()
        assert np.array_equal(got[:live], dense[:live]) and np.all(got[live:] == -7.0), live


def test_w1025_crosses_the_walker_chunk(root):
    s, like, ld, f64 = _edge(root, "nz16")
    W = 1025
    idx = np.arange(W) % len(s["points"])
    got = _eval(like, s["row"], s["points"][idx])
    small = _eval(like, s["row"], s["points"])
    assert np.array_equal(got, small[idx])
    assert np.all(np.abs(small - ld).astype(np.float64) <= _bound(ld, f64))


def test_des_shape(root):
    """A synthetic dataset of the DES Y1 shape (the one tools/wl_profile.py
    times) at two nuisance points, all shifts zero and a generic one."""
    from cosmomc_amd import weaklensing as wl
    s = wf.make_synthetic(os.path.join(str(root), "des_shape"), seed=900, nsrc=4, ngal=5, ntheta=20, nrows=351,
                          lmax=50000)
    like = wl.WLLikelihood(s["dataset"])
    assert (like.nz, like.nl, like.n_columns, like.n_used) == (353, 75, 35, 810)
    pts = s["points"][[0, 5]]
    ld = np.array([wl.wl_loglike_host(s["ds"], s["row"], p, np.longdouble) for p in pts])
    f64 = np.array([wl.wl_loglike_host(s["ds"], s["row"], p) for p in pts])
    got = _eval(like, s["row"], pts)
    err = np.abs(got - ld).astype(np.float64)
    print("des_shape max |gpu - long double|:", err.max(), "bound:", _bound(ld, f64), "-lnL", ld.astype(np.float64))
    assert np.all(err <= _bound(ld, f64)), (err, _bound(ld, f64))
