"""The galaxy power-spectrum likelihoods on the host (cosmomc_amd/mpk.py) against
the goldens of the compiled reference: the numpy loaders, the theory row, the
restatement of MPK_LnLike and WiggleZ_LnLike in f64 and in long double, the ini
helpers, the conflict with the WiggleZ BAO likelihood, and the refusals.

What the GPU bound of test_gpu_mpk.py rests on is measured here and printed
per data set (pytest -s): (a) max |host f64 - golden| and (b) max |host f64 -
host long double|; mpk_fixture.GPU_ATOL is asserted to be the project's rule
on them, 10 x the larger, per tag.  Measured: MPK (a) 1.2e-12 (b) 2.7e-12,
WIGGLEZ (a) 5.5e-12 (b) 7.3e-11, at -lnL up to 400.
"""
import ctypes as C
import os

import numpy as np
import pytest

import mpk_fixture as mf
from cosmomc_amd import _native as N
from cosmomc_amd import mpk as M
from cosmomc_amd.derivedlike import _DerivedLike
from cosmomc_amd.ini import IniFile
from cosmomc_amd.likelihood import LikelihoodList

FORMAT, UNSUPPORTED = -3, -6           # CMBL_ERR_* of cosmomc_amd.h
EPS = np.finfo(np.float64).eps
LOGZERO = 1e30


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return mf.extract(tmp_path_factory.mktemp("mpk"))


@pytest.fixture(scope="module")
def datasets(goldens):
    out = {}
    for n, g in goldens.items():
        out[n], = M.datasets_from_ini(IniFile(g.ini), g.gigglez_dir)
    return out


def _host(ds):
    return M.wigglez_loglike_host if ds.wigglez else M.mpk_loglike_host


@pytest.fixture(scope="module")
def measured(goldens, datasets):
    """{name: (host f64, host long double)} over every golden's cases: computed once, shared."""
    return {n: (np.array([_host(datasets[n])(datasets[n], r) for r in g.rows]),
                np.array([_host(datasets[n])(datasets[n], r, np.longdouble) for r in g.rows]))
            for n, g in goldens.items()}


@pytest.mark.parametrize("name", mf.NAMES)
def test_host_loader_matches_harness(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    assert ds.nk == g.nk and np.array_equal(ds.k, g.case_k)      # MPK: the harness stops unless these are the reference's k
    if g.is_wigglez:
        # the reference keeps WiggleZLikelihood private: its parent's components (a wrong selection shows in -lnL)
        assert ds.DV_fid == g.DV_fid and ds.redshift == g.redshift and g.kmax == (1.2 if ds.nonlinear else 0.8)
        assert ds.zbin == 1 + int(np.argmin(np.abs(np.array(mf.ZBINS) - ds.redshift)))
        return
    assert (ds.np, ds.nr, ds.zbin) == (g.np, 1, 0) and (ds.cov is not None) == bool(g.has_cov)
    assert np.array_equal(ds.k, g.k) and np.array_equal(ds.P[0], g.P) and np.array_equal(ds.sdev, g.sdev)
    if g.has_cov:
        # two f64 Cholesky inverses of one matrix: each is within about n eps cond(C) of the inverse
        n, cond = ds.np, np.linalg.cond(ds.cov[0])
        err = np.abs(ds.invcov_as(np.float64)[0] - g.invcov).max() / np.abs(g.invcov).max()
        print(name, "inverse covariance against the reference's:", err, "n eps cond:", n * EPS * cond)
        assert err <= 2 * n * EPS * cond


def test_selections_and_modes(datasets):
    d = datasets
    assert (d["lrg_dr4"].np, d["lrg_dr4"].nk, d["lrg_dr4"].q_mode, d["lrg_dr4"].cov) == (20, 65, M.Q_FLAT, None)
    assert d["lrg_dr4"].nonlinear and d["lrg_dr4"].use_scaling and d["lrg_dr4"].name == "SDSS_lrgDR4"
    for i, c in enumerate("abcd"):
        w = d["wigglez_" + c]
        assert (w.np, w.nk, w.nr, w.zbin, w.q_mode) == (18, 100, 7, i + 1, M.Q_NONE) and w.use_gigglez
        assert w.name == "WiggleZ_nov11" + c and w.minp == 3 and len(w.gk) == 500
    assert (d["mpk_select"].np, d["mpk_select"].nk) == (17, 34)
    assert d["wz_flat_r25"].regions == [2, 5] and d["wz_region7"].regions == [7] and d["wz_grid"].nr == 7
    assert [d[n].q_mode for n in ("mpk_grid", "mpk_qsigma0", "mpk_nomarge", "wz_grid", "wz_flat_r25")] == \
        [M.Q_GAUSS, M.Q_POINT, M.Q_NONE, M.Q_GAUSS, M.Q_FLAT]
    assert not d["mpk_noscale"].use_scaling and not d["wz_linear"].use_gigglez and not d["wz_linear"].nonlinear
    # Read_Real: single-precision values widened
    assert d["mpk_grid"].Ag == float(np.float32(1.3)) and d["mpk_grid"].Q_sigma == 1.5 and d["lrg_dr4"].Ag == float(np.float32(1.4))


def test_region_key_order(goldens, datasets):
    """Regions 5-7 are asked for as 1-hr, 3-hr, 0-hr (wigglez.f90:243-248): wz_region7 sets Use_0-hr_region alone
    and the reference reads the seventh block (its golden would not match another block's data)."""
    ds = datasets["wz_region7"]
    common = IniFile(os.path.join(goldens["wz_region7"].dir, "common.dataset"))
    assert [k for k in M.REGION_KEYS if common.read_bool(k)] == ["Use_0-hr_region"] and ds.regions == [7]
    assert M.REGION_KEYS[4:] == ["Use_1-hr_region", "Use_3-hr_region", "Use_0-hr_region"]


@pytest.mark.parametrize("name", mf.NAMES)
def test_theory_row_matches_harness(goldens, datasets, name):
    """a_scl and kh_min exactly; P to what the reference's interpolation of its (ln k, z) grid leaves: the row's P
    is the interpolant, pk here the function it interpolates.  The grid's step in ln k is h = ln(2e4) / 159 =
    0.062; a cubic interpolant of ln P is off by about h^4 |(ln P)''''| / 384 inside (ln P's fourth derivative is
    below 20 around the turn at k = 0.02: 8e-7) and by about h^3 |(ln P)'''| / 10 in the end intervals (below
    1e-4 there, where ln P is nearly a line: 2e-9); rtol 5e-6 covers both."""
    g, ds = goldens[name], datasets[name]
    worst = 0.0
    for (H0, DV, amp, tilt, lkmin), ref in zip(g.cases, g.rows):
        row = M.mpk_theory_row(ds, H0, DV, mf.analytic_pk(ds.redshift, amp, tilt, ds.nonlinear), mf.grid_kh_min(lkmin))
        assert row[0] == ref[0] and row[1] == ref[1]
        worst = max(worst, np.abs(row[2:] / ref[2:] - 1).max())
        np.testing.assert_allclose(row[2:], ref[2:], rtol=5e-6, atol=0)
    print(name, "theory row P against the harness's interpolant: max relative difference", worst)


def test_clamp_is_active_in_the_goldens(goldens, datasets):
    for name in ("lrg_dr4", "wigglez_a", "mpk_grid"):
        g, ds = goldens[name], datasets[name]
        active = [np.sum(r[0] * ds.k < r[1]) for r in g.rows]
        assert max(active) > 0 and min(active) == 0, (name, active)
    a = np.array([r[0] for r in goldens["lrg_dr4"].rows])
    assert a.min() < 0.86 and a.max() > 1.14
    assert np.all(goldens["mpk_noscale"].rows[:, 0] == 1.0)


@pytest.mark.parametrize("name", mf.NAMES)
def test_host_restatement_matches_reference(goldens, measured, name):
    g = goldens[name]
    h64, hld = measured[name]
    assert np.all(np.isfinite(g.ref)) and np.all(np.abs(g.ref) < 1e29)         # no golden is logZero
    a, b = np.abs(h64 - g.ref).max(), np.abs(h64 - hld.astype(np.float64)).max()
    print("%-16s (a) max |host - golden| = %.3g   (b) max |f64 - long double| = %.3g   of -lnL up to %.1f"
          % (name, a, b, g.ref.max()))
    tag = "WIGGLEZ" if g.is_wigglez else "MPK"
    assert a <= mf.GPU_ATOL[tag] / 10 and b <= mf.GPU_ATOL[tag] / 10


def test_gpu_bound_is_the_rule(goldens, measured):
    """mpk_fixture.GPU_ATOL, per tag, is 10 x the larger of (a) and (b) as measured here (stated to two digits)."""
    for tag in ("MPK", "WIGGLEZ"):
        names = [n for n, g in goldens.items() if bool(g.is_wigglez) == (tag == "WIGGLEZ")]
        a = max(np.abs(measured[n][0] - goldens[n].ref).max() for n in names)
        b = max(np.abs(measured[n][0] - measured[n][1].astype(np.float64)).max() for n in names)
        print(tag, "(a)", a, "(b)", b, "10 x the larger:", 10 * max(a, b), "stated:", mf.GPU_ATOL[tag])
        assert 10 * max(a, b) <= mf.GPU_ATOL[tag] <= 11 * max(a, b)


def test_wigglez_normv_rounding_is_exercised(goldens, datasets):
    """With normV kept in double the real WiggleZ bins differ from the goldens by far more than the GPU bound:
    the goldens pin the reference's single-precision normV."""
    for name in ("wigglez_a", "wigglez_b", "wigglez_c", "wigglez_d", "wz_grid"):
        g, ds = goldens[name], datasets[name]
        d = np.abs(np.array([M.wigglez_loglike_host(ds, r, normv_single=False) for r in g.rows]) - g.ref)
        print(name, "|normV in f64 - golden|:", d.min(), "..", d.max())
        assert d.max() > 100 * mf.GPU_ATOL["WIGGLEZ"]
        assert np.sum(d > mf.GPU_ATOL["WIGGLEZ"]) >= len(d) - 1


def test_running_normv_is_exercised(goldens, datasets):
    """wz_grid (Q_marge = T, Q_flat = F): point iQ divides by the sum of normV over the points so far.  With
    normV restarted at every point the value is far from the golden."""
    g, ds = goldens["wz_grid"], datasets["wz_grid"]
    assert ds.q_mode == M.Q_GAUSS
    d = np.abs(np.array([M.wigglez_loglike_host(ds, r, normv_running=False) for r in g.rows]) - g.ref)
    print("wz_grid |normV restarted - golden|:", d.min(), "..", d.max())
    assert d.min() > 1e-3


def test_failure_rows_on_the_host(goldens, datasets):
    for name in ("lrg_dr4", "mpk_grid", "wigglez_a", "wz_grid"):
        g, ds = goldens[name], datasets[name]
        for at, v in ((0, 0.0), (0, -1.0), (0, np.nan), (1, np.inf), (5, np.nan), (2 + ds.nk - 1, np.inf)):
            r = g.rows[0].copy()
            r[at] = v
            assert _host(ds)(ds, r) == LOGZERO and _host(ds)(ds, r, np.longdouble) == LOGZERO
        r = g.rows[0].copy()
        r[2:] = 0.0
        assert _host(ds)(ds, r) == LOGZERO
        if ds.use_gigglez:
            r = g.rows[0].copy()
            r[1] = 20.0
            assert _host(ds)(ds, r) == LOGZERO


# ---- the ini helpers

def test_datasets_from_batch_inis(goldens):
    """A run ini equivalent to batch2/MPK.ini and batch2/WiggleZ_MPK.ini (two bins of the four)."""
    lrg, wa, wb = goldens["lrg_dr4"], goldens["wigglez_a"], goldens["wigglez_b"]
    run = ("use_mpk = T\nmpk_numdatasets = 1\nmpk_dataset1 = %s/sdss_lrgDR4.dataset\nmpk_dataset_nonlinear1 = T\n"
           "use_wigglez_mpk = T\nnonlinear_wigglez = T\nUse_gigglez = T\n"
           "wigglez_common_dataset = %s/wigglez_nov11_common.dataset\nmpk_wigglez_numdatasets = 2\n"
           "wigglez_dataset1 = %s/wigglez_nov11a.dataset\nwigglez_dataset2 = %s/wigglez_nov11b.dataset\n"
           % (lrg.dir, wa.dir, wa.dir, wb.dir))
    d = M.datasets_from_ini(IniFile(text=run), wa.gigglez_dir)      # (every bin's data/ holds the four GiggleZ files)
    assert [x.name for x in d] == ["SDSS_lrgDR4", "WiggleZ_nov11a", "WiggleZ_nov11b"]
    assert [x.wigglez for x in d] == [False, True, True] and [x.zbin for x in d] == [0, 1, 2]
    assert d[0].nonlinear and d[1].nonlinear and d[1].use_gigglez and d[1].nr == d[2].nr == 7
    over = M.wigglez_overrides(os.path.join(wa.dir, "wigglez_nov11_common.dataset"), True, True, "/somewhere")
    assert over["min_mpk_points_use"] == "3" and over["max_mpk_points_use"] == "20" and over["Use_0-hr_region"] == "T"
    assert over["Use_gigglez"] == "T" and over["nonlinear_wigglez"] == "T" and over["gigglez_dir"] == "/somewhere"
    assert "name" not in over and over["name_conflict1"] == "WiggleZ"
    assert M.datasets_from_ini(IniFile(text="use_mpk = F\nuse_wigglez_mpk = F\n")) == []


def test_likelihood_add_off(goldens):
    lst = LikelihoodList()
    assert M.mpk_likelihood_add(lst, IniFile(text="use_mpk = F\nmpk_numdatasets = 1\nmpk_dataset1 = nowhere\n")) == []
    assert M.wigglez_likelihood_add(lst, IniFile(text="use_wigglez_mpk = F\nwigglez_common_dataset = nowhere\n")) == []
    assert M.mpk_likelihood_add(lst, IniFile(text="use_mpk = T\n")) == [] and len(lst) == 0


class _FakeBAO(_DerivedLike):
    def __init__(self, name):
        self.name = name


def test_wigglez_bao_conflict(goldens):
    """type_conflict1 = BAO, name_conflict1 = WiggleZ of the common file (likelihood.f90:54-60)."""
    g = goldens["wigglez_a"]
    lst = LikelihoodList()
    lst.add(_FakeBAO("DR11CMASS"))
    lst.add(_FakeBAO("WiggleZ"))
    with pytest.raises(ValueError, match="WiggleZ.*WiggleZ_nov11|WiggleZ_nov11.*WiggleZ") as e:
        M.wigglez_likelihood_add(lst, IniFile(g.ini), gigglez_dir=g.gigglez_dir)
    assert "BAO" in str(e.value) and len(lst) == 2


# ---- refusals: the numpy loaders and the library's loader (which refuses before it touches the device)

def _open(tag, dataset, override=""):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(tag.encode(), dataset.encode(), override.encode(), C.byref(h), err, 1024)
    if rc == 0:
        N.lib().cmbl_close(h)
    return rc, err.value.decode()


@pytest.mark.parametrize("override,code,exc,text", [
    ("name = twodf", UNSUPPORTED, NotImplementedError, "twodf"),
    ("name = lrg_2009", UNSUPPORTED, NotImplementedError, "lrg_2009"),
    ("Use_gigglez = T", UNSUPPORTED, NotImplementedError, "Use_gigglez"),
    ("no_such_key = 1", UNSUPPORTED, NotImplementedError, "no_such_key"),
    ("DV_fid = -1.0", FORMAT, M.MPKFormatError, "DV_fid"),
    ("max_mpk_points_use = 99", FORMAT, M.MPKFormatError, "selection"),
    ("num_mpk_points_full = 0", FORMAT, M.MPKFormatError, "num_mpk_points_full")])
def test_mpk_refusals(goldens, override, code, exc, text):
    ds = os.path.join(goldens["mpk_cov_flat"].dir, "syn.dataset")
    rc, msg = _open("MPK", ds, override)
    assert rc == code and text in msg, (rc, msg)
    k, v = (x.strip() for x in override.split("="))
    with pytest.raises(exc, match=text):
        M.MPKDataset(ds, {k: v})


def test_mpk_use_scaling_needs_dv_fid(goldens, tmp_path):
    src = os.path.join(goldens["mpk_cov_flat"].dir, "syn.dataset")
    text = "".join(ln for ln in open(src) if not ln.startswith("DV_fid"))
    text = text.replace("%DATASETDIR%", os.path.join(goldens["mpk_cov_flat"].dir, "data") + "/")
    (tmp_path / "nodv.dataset").write_text(text)
    rc, msg = _open("MPK", str(tmp_path / "nodv.dataset"))
    assert rc == FORMAT and "DV_fid" in msg, (rc, msg)
    with pytest.raises(M.MPKFormatError, match="DV_fid"):
        M.MPKDataset(str(tmp_path / "nodv.dataset"))


@pytest.mark.parametrize("override,code,exc,text", [
    ("Use_gigglez = T\nnonlinear_wigglez = F", FORMAT, M.MPKFormatError, "nonlinear_wigglez"),
    ("Use_11-hr_region = F\nUse_1-hr_region = F", FORMAT, M.MPKFormatError, "no regions"),
    ("redshift = 0.5", FORMAT, M.MPKFormatError, "redshift"),
    ("mpk_dataset_nonlinear = T", UNSUPPORTED, NotImplementedError, "mpk_dataset_nonlinear"),
    ("name = twodf", UNSUPPORTED, NotImplementedError, "twodf")])
def test_wigglez_refusals(goldens, override, code, exc, text):
    g = goldens["wz_flat_r25"]
    over = M.wigglez_overrides(os.path.join(g.dir, "common.dataset"), True, True, g.gigglez_dir)
    over.update(dict((x.strip() for x in ln.split("=")) for ln in override.split("\n")))
    rc, msg = _open("WIGGLEZ", os.path.join(g.dir, "wz.dataset"), "".join("%s = %s\n" % kv for kv in over.items()))
    assert rc == code and text in msg, (rc, msg)
    with pytest.raises(exc, match=text):
        M.WiggleZDataset(os.path.join(g.dir, "wz.dataset"), over)


def test_short_files_are_format_errors(goldens, tmp_path):
    g = goldens["mpk_cov_flat"]
    os.makedirs(tmp_path / "data")
    for f in os.listdir(os.path.join(g.dir, "data")):
        rows = open(os.path.join(g.dir, "data", f)).read().split("\n")
        (tmp_path / "data" / f).write_text("\n".join(rows[:-3] if f == "syn_windows.txt" else rows))
    (tmp_path / "syn.dataset").write_bytes(open(os.path.join(g.dir, "syn.dataset"), "rb").read())
    rc, msg = _open("MPK", str(tmp_path / "syn.dataset"))
    assert rc == FORMAT and "syn_windows.txt" in msg, (rc, msg)
    with pytest.raises(M.MPKFormatError, match="syn_windows.txt"):
        M.MPKDataset(str(tmp_path / "syn.dataset"))


@pytest.mark.gpu
def test_likelihood_add_on(goldens):
    """The keys of batch2/MPK.ini and batch2/WiggleZ_MPK.ini on the real data sets: the terms are named by their
    data sets (chi2_SDSS_lrgDR4, chi2_WiggleZ_nov11a), have no nuisance parameters and LikelihoodType MPK."""
    lrg, wa = goldens["lrg_dr4"], goldens["wigglez_a"]
    lst = LikelihoodList()
    a, = M.mpk_likelihood_add(lst, IniFile(lrg.ini))
    b, = M.wigglez_likelihood_add(lst, IniFile(wa.ini), gigglez_dir=wa.gigglez_dir)
    assert [x.get_tag() for x in lst] == ["SDSS_lrgDR4", "WiggleZ_nov11a"] and len(lst) == 2
    assert a.LikelihoodType == b.LikelihoodType == "MPK" and a.nuisance_names == b.nuisance_names == []
    assert a.nonlinear and b.nonlinear and (a.n_theory, b.n_theory) == (67, 102)
    assert (a.q_mode, b.q_mode, a.zbin, b.zbin, b.n_regions, b.use_gigglez) == (M.Q_FLAT, M.Q_NONE, 0, 1, 7, 1)
    assert all(v == 0 for r in a.cl_lmax + b.cl_lmax for v in r)
