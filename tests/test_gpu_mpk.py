"""The galaxy power-spectrum kernels (mpk.hip, tags MPK and WIGGLEZ) against the
recorded MPK_LnLike / WiggleZ_LnLike of the compiled reference on every golden
(the real LRG DR4 set and the four real WiggleZ bins among them), the library's
loader against the numpy loader, walker independence bit for bit, failure
rows, and the sparse entry.

Tolerance: the project's rule, absolute on -lnL (values up to 400), per tag:
10 x the larger of (a) the numpy restatement in f64 against the goldens and
(b) f64 against long double, both measured without a GPU (test_mpk.py prints
them per data set):
    MPK      (a) 1.2e-12  (b) 2.7e-12   ->  bound 2.7e-11
    WIGGLEZ  (a) 5.5e-12  (b) 7.3e-11   ->  bound 7.3e-10
The kernels sum in another order than the reference (MFMA tiles, a lane's rows,
then the four lane groups), which is the kind of difference (b) measures.

One caveat: WiggleZ's normV is rounded to single precision, so a device normV
that differs from the reference's in its last bits can round to the
neighbouring float; -lnL then moves by about 1e-6.  The chance is about 1e-8
per point; no golden point shows it, and none is excluded.
"""
import numpy as np
import pytest

import mpk_fixture as mf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GPU_ATOL = mf.GPU_ATOL              # {"MPK": 2.7e-11, "WIGGLEZ": 7.3e-10}
LOGZERO = 1e30


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return mf.extract(tmp_path_factory.mktemp("mpk"))


def make_like(g):
    """The library's likelihood of a golden, through the ini helpers."""
    from cosmomc_amd import mpk as M
    from cosmomc_amd.ini import IniFile
    from cosmomc_amd.likelihood import LikelihoodList
    lst, ini = LikelihoodList(), IniFile(g.ini)
    likes = M.mpk_likelihood_add(lst, ini) + M.wigglez_likelihood_add(lst, ini, gigglez_dir=g.gigglez_dir)
    assert len(likes) == 1
    return likes[0]


@pytest.fixture(scope="module")
def likes(goldens):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make_like(goldens[name])
        return cache[name]
    return get


def rows_on_device(rows, pad=0):
    """[W, 1, n] theory rows on the device, each walker's row pad doubles longer than n (ld_walker > n)."""
    rows = np.atleast_2d(rows)
    buf = torch.full((rows.shape[0], 1, rows.shape[1] + pad), -3.0, dtype=torch.float64, device="cuda")
    buf[:, 0, :rows.shape[1]] = torch.tensor(rows, device="cuda")
    return buf[:, :, :rows.shape[1]]


def tag_of(like):
    return "WIGGLEZ" if like.zbin else "MPK"


@pytest.mark.parametrize("name", mf.NAMES)
def test_matches_reference(goldens, likes, name):
    g, like = goldens[name], likes(name)
    assert like.n_theory == g.rows.shape[1] and like.nuisance_names == []
    got = like.loglike_batch(rows_on_device(g.rows)).cpu().numpy()
    assert np.all(np.abs(g.ref) < 1e29)
    print(name, tag_of(like), "max |gpu - golden|:", np.abs(got - g.ref).max(), "of", g.ref.max())
    np.testing.assert_allclose(got, g.ref, rtol=0, atol=GPU_ATOL[tag_of(like)])


@pytest.mark.parametrize("name", mf.NAMES)
def test_loader_matches_the_numpy_loader(goldens, likes, name):
    like = likes(name)
    ds = like.ds
    assert (like.n_points, like.n_kbands, like.n_regions, like.zbin) == (ds.np, ds.nk, ds.nr, ds.zbin)
    assert (like.q_mode, bool(like.has_cov), bool(like.use_scaling), bool(like.use_gigglez)) == \
        (ds.q_mode, ds.cov is not None, ds.use_scaling, ds.use_gigglez)
    assert like.name == ds.name
    k, P, inv = like.loader_arrays()
    assert np.array_equal(k, ds.k) and np.array_equal(P, ds.P)
    if ds.cov is not None:
        # the library's inverse (sums in extended precision, rounded once) against the long-double one: within
        # n eps cond(C) of it, the bound of an f64 Cholesky inverse, region by region
        ld = ds.invcov_as(np.longdouble)
        for r in range(ds.nr):
            err = float(np.abs(inv[r] - ld[r]).max() / np.abs(ld[r]).max())
            bound = ds.np * np.finfo(np.float64).eps * np.linalg.cond(ds.cov[r])
            assert err <= bound, (name, r, err, bound)
    else:
        assert np.array_equal(inv[0], np.diag(1 / ds.sdev ** 2))


@pytest.mark.parametrize("name", ["lrg_dr4", "mpk_grid", "mpk_grid_cov", "mpk_nomarge", "mpk_qsigma0_cov", "wigglez_a",
                                  "wz_flat_r25", "wz_grid"])
def test_walker_independence_bitwise(goldens, likes, name):
    """The same row in slots 0, 1 and W - 1 of batches of W in {1, 2, 15, 16, 17,
    63, 65, 129}, theory rows strided wider than a row, the other slots holding
    other rows: the same bits everywhere.  One data set of each Q mode, with
    and without a covariance, one region and several."""
    g, like = goldens[name], likes(name)
    rng = np.random.RandomState(7)
    seen = set()
    for W in (1, 2, 15, 16, 17, 63, 65, 129):
        pick = rng.randint(1, len(g.rows), W)
        slots = sorted({0, min(1, W - 1), W - 1})
        pick[slots] = 0
        got = like.loglike_batch(rows_on_device(g.rows[pick], pad=1 + W % 5)).cpu().numpy()
        seen |= {got[s].tobytes() for s in slots}
        np.testing.assert_allclose(got, g.ref[pick], rtol=0, atol=GPU_ATOL[tag_of(like)])
    assert len(seen) == 1


@pytest.mark.parametrize("name", ["mpk_grid", "wigglez_b"])
def test_chunk_edge_bitwise(goldens, likes, name):
    """Batches above 1024 walkers run in chunks: the same row at slots 0, 1023, 1024 has the same bits."""
    g, like = goldens[name], likes(name)
    W = 1025
    pick = np.arange(W) % len(g.rows)
    pick[[0, 1023, 1024]] = 2
    got = like.loglike_batch(rows_on_device(g.rows[pick], pad=2)).cpu().numpy()
    assert got[0].tobytes() == got[1023].tobytes() == got[1024].tobytes()
    small = like.loglike_batch(rows_on_device(g.rows[[2]])).cpu().numpy()
    assert small[0].tobytes() == got[0].tobytes()
    np.testing.assert_allclose(got, g.ref[pick], rtol=0, atol=GPU_ATOL[tag_of(like)])


def _failure_rows(g, like):
    nk = like.n_kbands
    base = g.rows[0]
    out = {}
    for what, at, v in (("nan entry", 2 + nk // 2, float("nan")), ("nan a_scl", 0, float("nan")),
                        ("inf entry", 2 + nk - 1, float("inf")), ("inf kh_min", 1, float("inf")),
                        ("a_scl = 0", 0, 0.0), ("a_scl < 0", 0, -0.9)):
        r = base.copy()
        r[at] = v
        out[what] = r
    r = base.copy()
    r[2:] = 0.0
    out["all-zero P"] = r
    # every chisq of the Q grid non-finite (with a finite chisq the grid's sum cannot be exactly 0: the
    # minimum's term is its calweight): the window products overflow
    r = base.copy()
    r[2:] = 1e200
    out["overflowing P"] = r
    if like.use_gigglez:
        r = base.copy()
        r[1] = 20.0                                   # k_scaled = kh_min above the last GiggleZ knot (15.87)
        out["k above the GiggleZ knots"] = r
        r = base.copy()
        r[1] = 1e-6                                   # and below the first (1e-4) through a_scl k_1
        r[0] = 1e-3
        out["k below the GiggleZ knots"] = r
    return out


@pytest.mark.parametrize("name", ["lrg_dr4", "mpk_grid", "mpk_grid_cov", "wigglez_c", "wz_grid"])
def test_failure_rows_are_logzero_for_that_walker_alone(goldens, likes, name):
    from cosmomc_amd import mpk as M
    g, like = goldens[name], likes(name)
    host = M.wigglez_loglike_host if like.zbin else M.mpk_loglike_host
    W = 19
    clean_rows = g.rows[np.arange(W) % len(g.rows)]
    clean = like.loglike_batch(rows_on_device(clean_rows, pad=1)).cpu().numpy()
    for what, bad_row in _failure_rows(g, like).items():
        assert host(like.ds, bad_row, np.longdouble) == LOGZERO or what == "overflowing P", what
        for slot in (0, 15, 16, W - 1):
            rows = clean_rows.copy()
            rows[slot] = bad_row
            got = like.loglike_batch(rows_on_device(rows, pad=1)).cpu().numpy()
            assert got[slot] == LOGZERO, (what, slot, got[slot])
            keep = np.arange(W) != slot
            assert np.array_equal(got[keep], clean[keep]), (what, slot)


@pytest.mark.parametrize("name", ["lrg_dr4", "mpk_grid", "wigglez_d"])
def test_sparse_evaluation_touches_the_live_slots_only(goldens, likes, name):
    g, like = goldens[name], likes(name)
    W = 21
    rows = rows_on_device(g.rows[np.arange(W) % len(g.rows)])
    dense = like.loglike_batch(rows).cpu().numpy()
    for live in (0, 1, W - 1, W):
        out = torch.full((W,), -7.0, dtype=torch.float64, device="cuda")
        like.loglike_batch_sparse(rows, None, out, torch.tensor([live], dtype=torch.int32, device="cuda"))
        got = out.cpu().numpy()
        assert np.array_equal(got[:live], dense[:live]) and np.all(got[live:] == -7.0), live


def test_workspace_grows_linearly_in_w(likes):
    like = likes("wz_grid")
    b16, b32, b1024 = like.workspace_bytes(16), like.workspace_bytes(32), like.workspace_bytes(1024)
    assert b32 == 2 * b16 and b1024 == 64 * b16 and like.workspace_bytes(5000) == b1024


def test_refusals(goldens, tmp_path):
    from cosmomc_amd import _native as N
    from cosmomc_amd import mpk as M
    g = goldens["mpk_cov_flat"]
    ds = g.dir + "/syn.dataset"
    for over, code in (({"name": "twodf"}, -6), ({"name": "lrg_2009"}, -6),
                       ({"no_such_key": "1"}, -6), ({"DV_fid": "-1.0"}, -3),
                       ({"max_mpk_points_use": "99"}, -3)):
        with pytest.raises(N.NativeError) as e:
            M.MPKLikelihood(ds, True, over)
        assert e.value.code == code, over
    w = goldens["wz_flat_r25"]
    for over, code in (({"Use_gigglez": "T", "nonlinear_wigglez": "F"}, -3),
                       ({"Use_11-hr_region": "F", "Use_1-hr_region": "F"}, -3),
                       ({"redshift": "0.5"}, -3), ({"no_such_key": "1"}, -6)):
        with pytest.raises(N.NativeError) as e:
            M.WiggleZLikelihood(w.dir + "/wz.dataset", w.dir + "/common.dataset", True, True, w.gigglez_dir, over)
        assert e.value.code == code, over
