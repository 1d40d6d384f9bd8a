"""SZ cluster counts without a GPU: the host loader (SZDataset) against the
quantities the harness printed, the host restatement (sz_loglike_host) against
the recorded SZCC_Cash of the compiled reference, sz_theory_row against the
harness's row, the refusals of cmbl_open("SZ") (they happen before anything
touches the device) and the ini front end; the library's own loader, which
forms its tables on the device, is compared with the same quantities in
test_gpu_sz.py.

Tolerance inputs of the GPU tests, measured here on the goldens (absolute, on
-lnL, values up to 2.0e4; both are printed):
(a) sz_loglike_host in f64 against the goldens: 0 on every golden.  The
    restatement keeps the reference's types, literals and summation order, and
    numpy's exp, log, pow and scipy's erf gave the compiled reference's bits.
    The bound below still allows a few ulp of the largest -lnL for another libm.
(b) f64 against long double, over every golden point of syn_inside,
    syn_contains, syn_cat, syn_lastrow, syn_prior_all and real: 2.7e-5 at
    syn_inside point 1 and 2.9e-9 at point 2 (alpha_SZ = 1, bias_SZ = 0.1: the
    masses are scaled down so far that the counts of the upper S/N bins come
    from 1 - erf in its cancellation range, where f64 keeps no relative
    accuracy, and those bins hold clusters), 1.5e-10 at most elsewhere.  The
    test below measures the two worst points, the centre and the largest -lnL.
(c) for test_gpu_sz_edges.py, per entry of the completeness table: f64 against
    long double, 7.1e-15 on syn_inside and syn_two, 5.7e-14 on syn_unsorted
    (test_completeness_f64_against_long_double says where).
"""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

import sz_fixture as sf
from cosmomc_amd import _native as N
from cosmomc_amd import szcounts as S
from cosmomc_amd.ini import IniFile
from cosmomc_amd.likelihood import LikelihoodList

HOST_ATOL = 1e-10
FORMAT, UNSUPPORTED = -3, -6           # CMBL_ERR_* of cosmomc_amd.h


@pytest.fixture(scope="module")
def extracted(tmp_path_factory):
    d = tmp_path_factory.mktemp("sz")
    return d, sf.extract(d)


@pytest.fixture(scope="module")
def goldens(extracted):
    return extracted[1]


@pytest.fixture(scope="module")
def datasets(goldens):
    return {n: S.SZDataset(g.ini) for n, g in goldens.items()}


_counts = {}


def _dn(goldens, datasets, name, i):
    """The predicted counts of point i: shared by the goldens whose data files and points are the same
    (the prior switches do not enter them)."""
    g = goldens[name]
    key = (tuple(g.points[i]),) + tuple(open(os.path.join(g.dir, "data", f), "rb").read()
                                        for f in ("SZ_cat.txt", "SZ_thetas.txt", "SZ_skyfracs.txt", "SZ_ylims.txt"))
    if key not in _counts:
        _counts[key] = S.sz_counts(datasets[name], g.row, g.points[i])
    return _counts[key]


@pytest.mark.parametrize("name", sf.NAMES)
def test_host_loader_matches_harness(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    assert (ds.nzs, ds.nm, ds.Nz, ds.nq) == (g.nzs, g.nm, g.nz, g.nq)
    assert np.array_equal(ds.steps_z, g.steps_z)
    assert np.array_equal(ds.DNcat, g.DNcat)
    assert ds.n_theory == len(g.row) and ds.param_names == sf.PARAM_NAMES
    assert {k for k, v in ds.priors.items() if v} == set(g.priors)


def test_fixed_grid_sizes(datasets):
    """The sizes the reference's constants give: Nz = DINT(1 / 0.1d0) + 1 = 11
    bins in z, 5 in S/N, 281 steps in z (1e-3 to 0.2, 1e-2 to 1, one of binz),
    120 in ln M, N = 21.5 / (double)0.05f = 429 nodes in ln Y; the last z bin
    collapses onto the last step and adds no counts."""
    ds = datasets["syn_inside"]
    assert (ds.Nz, ds.nq, ds.nzs, ds.nm, S.NLNY) == (11, 5, 281, 120, 429)
    assert ds.steps_z[0] > 0 and ds.j1[0] == 0 and ds.j2[-1] == ds.nzs - 1 and ds.j1[-1] == ds.j2[-1]
    assert np.all(ds.j1[1:] == ds.j2[:-1]) and np.all(ds.j2[:-1] > ds.j1[:-1])


@pytest.mark.parametrize("name", sf.NAMES)
def test_host_restatement_matches_reference(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    assert np.all(np.isfinite(g.ref)) and np.all(np.abs(g.ref) < 1e29)         # no golden is logZero
    got = np.array([S.sz_loglike_host(ds, g.row, p, DN=_dn(goldens, datasets, name, i)) for i, p in enumerate(g.points)])
    print(name, "(a) max |f64 - golden|:", np.abs(got - g.ref).max(), "of", g.ref.max())
    np.testing.assert_allclose(got, g.ref, rtol=0, atol=HOST_ATOL)


def test_prior_goldens_share_their_data(goldens):
    """What lets _dn share the counts: the prior goldens differ in their switches alone, and each switch moves -lnL."""
    base = goldens["syn_prior_all"]
    for p in sf.PRIORS:
        g = goldens["syn_" + p]
        for f in ("SZ_cat.txt", "SZ_thetas.txt", "SZ_skyfracs.txt", "SZ_ylims.txt"):
            assert filecmp.cmp(os.path.join(g.dir, "data", f), os.path.join(base.dir, "data", f), shallow=False)
        assert np.array_equal(g.points, base.points) and g.priors == [p]
    one = np.array([goldens["syn_" + p].ref for p in sf.PRIORS])
    assert len({tuple(r) for r in one}) == len(sf.PRIORS)


LD_CASES = [("syn_inside", 0), ("syn_inside", 1), ("syn_inside", 2), ("syn_contains", 4)]


def test_longdouble_restatement(goldens, datasets):
    worst = 0.0
    for name, i in LD_CASES:
        g, ds = goldens[name], datasets[name]
        ld = S.sz_loglike_host(ds, g.row, g.points[i], np.longdouble)
        f64 = S.sz_loglike_host(ds, g.row, g.points[i], DN=_dn(goldens, datasets, name, i))
        print(name, i, "(b) |f64 - long double|:", float(abs(np.longdouble(f64) - ld)), "of", g.ref[i])
        worst = max(worst, float(abs(np.longdouble(f64) - ld)))
        assert abs(float(ld) - g.ref[i]) <= 1e-4
    print("(b) max |f64 - long double|:", worst)
    assert worst <= 1e-4


def test_goldens_cover_the_branches(goldens, datasets):
    """Both extrapolating theta branches and the bracket run in syn_inside, in
    syn_two (two thetas, one patch: the least the loaders accept) and in
    syn_unsorted, the bracket alone in syn_contains; completeness clips at fsky at the least
    scatter; scatter_SZ = 0 and beta_SZ != 2/3 are there; the catalogue of
    syn_cat has a bin above 10, empty bins and rescaled (non-integer) columns."""
    for name, lo, hi in (("syn_inside", True, True), ("syn_contains", False, False), ("syn_two", True, True),
                         ("syn_unsorted", True, True)):
        g, ds = goldens[name], datasets[name]
        row = g.row
        E, dA = row[3:3 + ds.nzs], row[3 + ds.nzs:3 + 2 * ds.nzs]
        mfac = np.exp(ds.steps_m) * 0.8 / S.M_PIVOT * (100 / row[0])
        thp = S.THETASTAR * (row[0] / 70) ** S.M2_3 * mfac[None, :] ** S.ALPHA_THETA * (E ** S.M2_3)[:, None] \
            / (100 * dA / 500 / row[0])[:, None]
        assert bool(np.any(thp < ds.thetas.min())) == lo and bool(np.any(thp > ds.thetas.max())) == hi
        assert np.any((thp >= ds.thetas.min()) & (thp <= ds.thetas.max()))
        assert np.any(g.points[:, 3] == 0) and np.any(g.points[:, 4] != 2.0 / 3.0)
    g, ds = goldens["syn_inside"], datasets["syn_inside"]
    assert g.points[3, 3] == 0.022
    comp = S.sz_completeness(ds, g.row, g.points[3])
    fsky = np.float32(ds.skyfracs.sum())
    assert comp.max() == fsky and np.count_nonzero(comp == fsky) > 100
    d = datasets["syn_cat"].DNcat
    assert d.max() > 10 and np.count_nonzero(d == 0) > 5 and np.any(d != np.round(d))
    cat = np.loadtxt(os.path.join(goldens["syn_cat"].dir, "data", "SZ_cat.txt"))
    assert np.any(cat[:, 2] < 6) and np.any((cat[:, 0] == -1) & (cat[:, 2] > 40)) and np.any((cat[:, 0] == -1) & (cat[:, 2] < 8))
    last = np.loadtxt(os.path.join(goldens["syn_lastrow"].dir, "data", "SZ_cat.txt"))
    assert last[-1, 2] >= 6 and datasets["syn_lastrow"].DNcat.sum() == np.count_nonzero(last[:, 2] >= 6) + 1


def test_smallest_and_unsorted_goldens(goldens, datasets):
    """syn_two is the least the loaders accept; in syn_unsorted every theta is the nearest of some theta500
    inside the range, each inner one from either side, so the scan over unsorted thetas meets them all."""
    two, uns = datasets["syn_two"], datasets["syn_unsorted"]
    assert len(two.thetas) == 2 and len(two.skyfracs) == 1 and two.ylims.shape == (1, 2)
    assert len(uns.thetas) == 5 and len(uns.skyfracs) == 3
    for name in ("syn_two", "syn_unsorted"):
        assert [tuple(p) for p in goldens[name].points[[0, 2]]] == [sf.CENTRE, sf.ZERO_SCATTER]
    thp = sf.scaling(uns, goldens["syn_unsorted"].row, sf.CENTRE)[0]
    ins = (thp >= uns.thetas.min()) & (thp <= uns.thetas.max())
    near = np.argmin(np.abs(uns.thetas[None, None, :] - thp[:, :, None]), axis=2)
    for t in range(5):
        assert np.any(ins & (near == t))
    for t in (1, 2, 3):
        assert np.any(ins & (near == t) & (uns.thetas[t] > thp)) and np.any(ins & (near == t) & (uns.thetas[t] < thp))


def test_window_classes_of_the_edge_cases(goldens, datasets):
    """The six kinds of ln Y node window sz_compl_kernel can meet (sf.window_classes) all occur over the
    syn_inside cases of test_gpu_sz_edges.py, and the loop without a node does.  Counted: scatter_SZ = 0.075:
    7033 cut low, 26530 inside, 37 cut high, 120 above; 1e-3: 963 below (876 without a node), 72 cut low, 32565
    inside, 120 above; 0.5: 28658 wider, 4924 cut low, 112 cut high, 26 above; 3.0: all 33720 wider."""
    g, ds = goldens["syn_inside"], datasets["syn_inside"]
    total = dict.fromkeys(sf.WINDOW_CLASSES + ("empty",), 0)
    for nu in sf.EDGE_CASES["syn_inside"]:
        if nu[3] != 0:
            n = sf.window_classes(ds, g.row, nu)
            print(nu[3], n)
            for c in total:
                total[c] += n[c]
    assert all(v > 0 for v in total.values()), total
    assert sf.window_classes(ds, g.row, sf.EDGE_CASES["syn_inside"][3])["wider"] == ds.nzs * ds.nm


@pytest.mark.parametrize("name", sorted(sf.LD_TABLE_CASES))
def test_completeness_f64_against_long_double(goldens, datasets, name):
    """(c) The bound of test_gpu_sz_edges.py, entry by entry: sz_completeness in f64 against long double over
    sf.LD_TABLE_CASES, both rounded to single precision as the reference's table is.  Measured, the largest
    absolute difference: syn_inside 7.1e-15 (scatter_SZ = 1e-3 and the ill-conditioned golden; 8.9e-16 at the
    centre, 3.6e-15 at scatter_SZ = 0, 0 at 3.0; 2.2e-16 at 0.5, measured once and not repeated here), syn_two
    7.1e-15, syn_unsorted 5.7e-14 (its scatter_SZ = 0 table; 3.6e-15 at the centre).  Each of these is one
    single-precision ulp of a small entry (2^-47 for one of 7.9e-8, 2^-44 below 9.5e-7): the rounding to single
    tipped.  Thousands of smaller entries differ by more than an ulp and less than that absolutely: they are
    1 - erf in its cancellation range, where f64 keeps no relative accuracy.  No entry is non-finite, and on
    the host scatter_SZ = -0.075 gives +0.075's table."""
    g, ds = goldens[name], datasets[name]
    worst = 0.0
    for nu in sf.LD_TABLE_CASES[name]:
        f64 = S.sz_completeness(ds, g.row, nu)
        ld = S.sz_completeness(ds, g.row, nu, np.longdouble)
        assert np.all(np.isfinite(f64)) and np.all(np.isfinite(ld))
        diff = np.abs(f64.astype(np.longdouble) - ld).astype(np.float64)
        at = diff > 0
        i = np.unravel_index(np.argmax(diff), diff.shape)
        print(name, nu, "(c) max |f64 - long double| per entry:", diff.max(), "at an entry of", f64[i], "; entries that differ:",
              np.count_nonzero(at), "of them neighbouring floats:", np.count_nonzero(sf.ulp_apart(f64, ld.astype(np.float64))),
              "; the largest entry that differs:", f64[at].max() if at.any() else 0.0)
        worst = max(worst, float(diff.max()))
        if name == "syn_inside" and tuple(nu) == sf.CENTRE:
            assert np.array_equal(S.sz_completeness(ds, g.row, sf.EDGE_CASES["syn_inside"][4]), f64)
    print(name, "(c) max |f64 - long double| per entry:", worst)
    assert worst <= sf.COMP_LD_ABS[name]


def test_theory_row_matches_harness(extracted, goldens, datasets):
    """H0, ns, ombh2 exactly, E(z) to rounding; dA and the grid to the tolerance
    of the reference's own integrations: its r(z) is a Romberg integral to 1e-5
    (the grid carries r^2) and its growth factor an ODE to 1e-8, while
    sz_theory_row integrates both to 1e-12.  Measured: dA 1.5e-13, the Tinker
    grid 2.2e-6 (4.9e-7 where it is above 1e-6 of its maximum), the Watson grid
    2.3e-7."""
    g, ds = goldens["syn_inside"], datasets["syn_inside"]
    n = ds.nzs
    row = S.sz_theory_row(ds, *g.cosmo, sf.sigma_table())
    assert row.shape == g.row.shape and np.array_equal(row[:3], g.row[:3])
    np.testing.assert_allclose(row[3:3 + n], g.row[3:3 + n], rtol=4e-16, atol=0)
    print("dA:", np.abs(row[3 + n:3 + 2 * n] / g.row[3 + n:3 + 2 * n] - 1).max(),
          "grid:", np.abs(row[3 + 2 * n:] / g.row[3 + 2 * n:] - 1).max())
    np.testing.assert_allclose(row[3 + n:3 + 2 * n], g.row[3 + n:3 + 2 * n], rtol=1e-5, atol=0)
    np.testing.assert_allclose(row[3 + 2 * n:], g.row[3 + 2 * n:], rtol=2e-5, atol=0)
    wat = S.sz_theory_row(ds, *g.cosmo, sf.sigma_table(), use_watson=True)[::sf.WATSON_STRIDE]
    ref = sf.watson_sample(extracted[0])
    assert wat.shape == ref.shape and not np.allclose(ref[20:], g.row[::sf.WATSON_STRIDE][20:], rtol=1e-2)
    print("Watson grid:", np.abs(wat / ref - 1).max())
    np.testing.assert_allclose(wat, ref, rtol=2e-5, atol=0)


# ---- refusals of the library's loader: each names its key

def _open(ini, override=""):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(b"SZ", ini.encode(), override.encode(), C.byref(h), err, 1024)
    if rc == 0:
        N.lib().cmbl_close(h)
    return rc, err.value.decode()


@pytest.mark.parametrize("override,text", [("1D = T", "1D"), ("use_watson = T", "use_watson"), ("use_SZ = T", "use_SZ"),
                                           ("prior_clash = T", "prior_clash")])
def test_loader_refusals(goldens, override, text):
    rc, msg = _open(goldens["syn_cat"].ini, override)
    assert rc == UNSUPPORTED and text in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match=text):
        k, v = (x.strip() for x in override.split("="))
        S.SZDataset(goldens["syn_cat"].ini, {k: v})


def _copy(g, tmp_path):
    os.makedirs(tmp_path / "data")
    (tmp_path / "sz.ini").write_bytes(open(g.ini, "rb").read())
    for f in os.listdir(os.path.join(g.dir, "data")):
        (tmp_path / "data" / f).write_bytes(open(os.path.join(g.dir, "data", f), "rb").read())
    return str(tmp_path / "sz.ini")


def test_wrong_ylims_size_is_a_format_error(goldens, tmp_path):
    ini = _copy(goldens["syn_cat"], tmp_path)
    rows = open(tmp_path / "data" / "SZ_ylims.txt").read().split("\n")
    (tmp_path / "data" / "SZ_ylims.txt").write_text("\n".join(rows[:-2]) + "\n")
    rc, msg = _open(ini)
    assert rc == FORMAT and "ylims" in msg, (rc, msg)
    with pytest.raises(S.SZFormatError, match="ylims"):
        S.SZDataset(ini)


def test_fewer_than_two_thetas_is_a_format_error(goldens, tmp_path):
    ini = _copy(goldens["syn_cat"], tmp_path)
    (tmp_path / "data" / "SZ_thetas.txt").write_text("3.0\n")
    rc, msg = _open(ini)
    assert rc == FORMAT and "thetas" in msg, (rc, msg)
    with pytest.raises(S.SZFormatError, match="thetas"):
        S.SZDataset(ini)


def _reorder_thetas(g, tmp_path, order):
    """A copy of a dataset with the thetas, and the ylims rows that go with them, in another order."""
    ini = _copy(g, tmp_path)
    th = open(tmp_path / "data" / "SZ_thetas.txt").read().split()
    yl = open(tmp_path / "data" / "SZ_ylims.txt").read().split()
    npatch = len(yl) // len(th)
    assert sorted(order) == list(range(len(th))) and npatch * len(th) == len(yl)
    (tmp_path / "data" / "SZ_thetas.txt").write_text("".join(th[k] + "\n" for k in order))
    (tmp_path / "data" / "SZ_ylims.txt").write_text("".join(y + "\n" for k in order for y in yl[k * npatch:(k + 1) * npatch]))
    return ini


@pytest.mark.parametrize("order", [(3, 2, 1, 0), (1, 0, 2, 3), (0, 1, 3, 2)],
                         ids=["descending", "first_not_least", "last_not_greatest"])
def test_thetas_that_leave_the_reference_table_are_refused(goldens, tmp_path, order):
    """The reference takes the bracket's second theta from outside its table when the nearest theta is the first
    entry and larger than theta500, or the last and smaller: no behaviour to follow, so neither loader opens it."""
    ini = _reorder_thetas(goldens["syn_cat"], tmp_path, order)
    rc, msg = _open(ini)
    assert rc == UNSUPPORTED and "thetas_file" in msg and "outside its table" in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match="thetas_file.*outside its table"):
        S.SZDataset(ini)


def test_unsorted_inner_thetas_open(goldens, datasets, tmp_path):
    """The order between the least theta, first, and the greatest, last, is free: syn_unsorted opens, and so
    does syn_cat in that kind of order.  (The library builds its tables on the device when it opens a data set:
    test_gpu_sz.py opens syn_unsorted there.)"""
    th = datasets["syn_unsorted"].thetas
    assert np.array_equal(np.argsort(th), np.argsort(sf.UNSORTED_ORDER)) and len(th) == 5
    assert th[0] == th.min() and th[-1] == th.max() and np.any(np.diff(th) < 0)
    ini = _reorder_thetas(goldens["syn_cat"], tmp_path, (0, 2, 1, 3))
    ds = S.SZDataset(ini)
    assert np.array_equal(ds.thetas[[0, 2, 1, 3]], datasets["syn_cat"].thetas)
    assert np.array_equal(ds.ylims[:, [0, 2, 1, 3]], datasets["syn_cat"].ylims)


# ---- the ini front end

def test_likelihood_add_off_and_errors(goldens):
    lst = LikelihoodList()
    assert S.sz_likelihood_add(lst, IniFile(text="use_SZ = F\nsz_dataset = nowhere.ini\n")) == []
    assert len(lst) == 0
    with pytest.raises(ValueError, match="1D and 2D"):
        S.sz_likelihood_add(lst, IniFile(text="use_SZ = T\n1D = T\n2D = T\nsz_dataset = %s\n" % goldens["syn_cat"].ini))
    with pytest.raises(ValueError, match="sz_dataset"):
        S.sz_likelihood_add(lst, IniFile(text="use_SZ = T\n"))


@pytest.mark.gpu
def test_likelihood_add_on(goldens):
    """The keys of batch2/SZ_plus_CMB.ini on a golden data set: the term is named
    SZ, the names come from SZ.paramnames, the run ini's switches reach the
    library (its -lnL moves by the priors they turn on)."""
    import torch
    g = goldens["syn_cat"]
    run = "use_SZ = T\nget_sigma8 = T\nprior_scatter_SZ = T\nprior_alpha_SZ = F\nprior_ystar_SZ = T\nprior_beta_SZ = F\n" \
          "2D = T\nsz_dataset = %s\n" % g.ini
    lst = LikelihoodList()
    like, = S.sz_likelihood_add(lst, IniFile(text=run))
    assert like.get_tag() == "SZ" and like.name == "SZ" and like.LikelihoodType == "SZ" and not like.use_watson
    assert like.description()[:3] == ("SZ", "SZ", "SZ")
    assert like.nuisance_names == sf.PARAM_NAMES and like.n_theory == len(g.row)
    names = lst.add_nuisance_parameters(["omegabh2"])
    assert names[1:] == sf.PARAM_NAMES and like.nuisance_indices == [2, 3, 4, 5, 6]
    assert like.ds.priors["prior_scatter_SZ"] and like.ds.priors["prior_ystar_SZ"] and not like.ds.priors["prior_alpha_SZ"]
    wat, = S.sz_likelihood_add(LikelihoodList(), IniFile(text=run + "use_watson = T\nsz_dataset_speed = 3\n"))
    assert wat.use_watson and wat.speed == 3
    p = np.array([[1.9, -0.15, 0.8, 0.09, 2.0 / 3.0]])
    rows = torch.tensor(g.row, device="cuda").reshape(1, 1, -1)
    plain = S.SZLikelihood(g.ini)
    with_pr = like.loglike_batch(rows, torch.tensor(p, device="cuda")).cpu().numpy()[0]
    without = plain.loglike_batch(rows, torch.tensor(p, device="cuda")).cpu().numpy()[0]
    want = sum((x - S.PRIOR_TABLE[k][0]) ** 2 / S.PRIOR_TABLE[k][1]
               for k, x in (("prior_ystar_SZ", p[0, 1]), ("prior_scatter_SZ", p[0, 3])))
    assert with_pr - without == pytest.approx(want, rel=1e-9)
