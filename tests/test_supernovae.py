"""JLA supernova likelihood without a GPU: the numpy restatement
(cosmomc_amd.supernovae.jla_loglike_host) against the compiled reference's
recorded JLA_alpha_beta_like, the loader's refusals through cmbl_open (they
come before any device call, as in test_cpu_cmblikes_loader.py) and
jla_likelihood_add's reading of the run's ini."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import jla_fixture as jf
from cosmomc_amd import _native as N
from cosmomc_amd import supernovae as sn
from cosmomc_amd.ini import IniFile
from cosmomc_amd.likelihood import LikelihoodList

IO, FORMAT, UNSUPPORTED = -2, -3, -6


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return jf.extract(tmp_path_factory.mktemp("jla"))


@pytest.mark.parametrize("name", jf.NAMES)
def test_host_restatement_matches_reference(goldens, name):
    """rtol 1e-12: the restatement sits at <= 4e-16 of the compiled reference
    where both were measured, three orders of margin for BLAS differences."""
    g = goldens[name]
    D = sn.JLADataset(g.dataset)
    got = np.array([sn.jla_loglike_host(D, a, b, mu) for (a, b), mu in zip(g.ab, g.mu)])
    print(name, np.abs(got / g.ref - 1).max())
    zero = g.ref == jf.LOGZERO
    assert np.array_equal(got[zero], g.ref[zero])
    np.testing.assert_allclose(got[~zero], g.ref[~zero], rtol=1e-12, atol=0)


def test_indefinite_case_is_logzero_exactly(goldens):
    g = goldens["syn5_indef"]
    assert list(g.ref == jf.LOGZERO) == [False, False, True, False, False]
    assert sn.jla_loglike_host(g.dataset, g.ab[2, 0], g.ab[2, 1], g.mu[2]) == 1e30


def _longdouble(D, ab, mu):
    r = [jf.jla_loglike_longdouble(D, a, b, m) for (a, b), m in zip(ab, mu)]
    return np.array([v for v, _ in r]), np.array([p for _, p in r])


def _host(D, ab, mu):
    return np.array([sn.jla_loglike_host(D, a, b, m) for (a, b), m in zip(ab, mu)])


@pytest.mark.parametrize("name", jf.NAMES)
def test_longdouble_restatement_matches_reference(goldens, name):
    """The long-double restatement (the reference of test_gpu_jla_edges.py)
    against the compiled reference and against the float64 restatement: 1e-13,
    LOGZERO exactly where ref.txt has it.  ref.txt itself is a float64 result."""
    g = goldens[name]
    D = sn.JLADataset(g.dataset)
    ld, bad = _longdouble(D, g.ab, g.mu)
    host = _host(D, g.ab, g.mu)
    zero = g.ref == jf.LOGZERO
    assert np.array_equal(ld == jf.LOGZERO, zero) and np.array_equal(bad >= 0, zero)
    assert np.array_equal(host == jf.LOGZERO, zero)
    print(name, jf.rel_distance(g.ref[~zero], ld[~zero]), jf.rel_distance(host[~zero], ld[~zero]))
    assert jf.rel_distance(g.ref[~zero], ld[~zero]) < 1e-13
    assert jf.rel_distance(host[~zero], ld[~zero]) < 1e-13


def test_longdouble_first_bad_pivot_of_golden(goldens):
    """syn5_indef: one block column, so any row of it may be the first to fail; the pivot before it is positive."""
    g = goldens["syn5_indef"]
    v, p = jf.jla_loglike_longdouble(sn.JLADataset(g.dataset), g.ab[2, 0], g.ab[2, 1], g.mu[2])
    assert v == jf.LOGZERO and 0 <= p < 5
    assert jf.jla_loglike_longdouble(sn.JLADataset(g.dataset), np.nan, 0.0, g.mu[0]) == (jf.LOGZERO, 0)


def test_write_dataset_round_trip(tmp_path):
    """write_dataset on what make_synthetic wrote gives the same dataset, and places single entries as given."""
    ds, mu, ab = jf.make_synthetic(str(tmp_path / "a"), 7, ("mag", "stretch_colour"), True, 77)
    names, rows = jf.read_lc(str(tmp_path / "a"))
    mats = {k: jf.read_matrix(str(tmp_path / "a" / (k + ".dat"))) for k in ("mag", "stretch_colour")}
    ds2 = jf.write_dataset(str(tmp_path / "b"), names, rows, mats, True)
    for f in ("lc.txt", "jla.dataset", "mag.dat", "stretch_colour.dat"):
        assert open(tmp_path / "a" / f).read() == open(tmp_path / "b" / f).read(), f
    mats["mag"][5, 2] += 1.0                    # strict lower triangle: not read
    mats["mag"][2, 5] -= 0.25
    D = sn.JLADataset(jf.write_dataset(str(tmp_path / "c"), names, rows, mats, True))
    E = sn.JLADataset(ds2)
    assert D.comp["mag"][5, 2] == D.comp["mag"][2, 5] == E.comp["mag"][2, 5] - 0.25
    assert (D.comp["mag"] != E.comp["mag"]).sum() == 2


# ---- input conditions of the datasets of test_gpu_jla_edges.py: a generator that drifts fails here

@pytest.mark.parametrize("nsn,p", jf.PIVOT)
def test_edge_pivot_inputs(nsn, p):
    """V(0.2, 1) fails first at pivot p exactly, the two other cases are positive definite."""
    e = jf.edge("pivot_%d_%d" % (nsn, p))
    assert e.D.nsn == nsn and sorted(e.D.comp) == ["mag", "stretch"] and e.D.twoscriptmfit
    assert list(e.bad) == [p, -1, -1]
    assert list(e.ref == jf.LOGZERO) == [True, False, False]
    host = _host(e.D, e.ab, e.mu)
    assert host[0] == jf.LOGZERO and jf.rel_distance(host[1:], e.ref[1:]) < 1e-13
    # the pivots before p do not depend on S[p, p]: without it the case is positive definite
    S = e.D.comp["stretch"]
    assert S[p, p] == -jf.PIVOT_S and np.count_nonzero(S) == 1
    assert np.linalg.eigvalsh(jf.jla_V(e.D, *e.ab[0]) - e.ab[0, 0] ** 2 * S).min() > 0


@pytest.mark.parametrize("name", [n for n in jf.EDGE_NAMES if n.split("_")[0] in ("slabs", "subset", "diag300")])
def test_edge_finite_inputs(name):
    """No case is LOGZERO in the long-double reference, and the float64 restatement sits at 1e-13 of it."""
    e = jf.edge(name)
    kind, _, arg = name.partition("_")
    if kind == "slabs":
        assert e.D.nsn == int(arg.split("_")[0]) and sorted(e.D.comp) == sorted(jf.COMPONENTS)
        assert e.D.twoscriptmfit == bool(int(arg.split("_")[1]))
        T = (e.D.nsn + 15) // 16
        assert ((T + 3) // 4 > 4) == (e.D.nsn == 257)         # slabs of block column 0: a second lap at 257 only
    elif kind == "subset":
        assert e.D.nsn == 33 and sorted(e.D.comp) == sorted(jf.SUBSETS[arg]) and e.D.twoscriptmfit
    else:
        assert e.D.nsn == 300 and e.D.diag_errors and e.D.twoscriptmfit == bool(int(arg))
    assert len(e.ref) == 3 and np.all(e.bad == -1)
    assert np.all(np.isfinite(e.ref.astype(np.float64))) and np.all(e.ref < 1e4)
    d = jf.rel_distance(_host(e.D, e.ab, e.mu), e.ref)
    print(name, [float(x) for x in e.ref], d)
    assert d < 1e-13


def test_edge_subsets_share_the_zero_case():
    """alpha = beta = 0 leaves only mag of V's components: the datasets without it agree there exactly."""
    assert list(jf.edge("subset_mag").ab[1]) == [0.0, 0.0]
    ref = [jf.edge("subset_" + k).ref[1] for k in jf.SUBSETS if k != "mag"]
    assert len(ref) == 6 and all(r == ref[0] for r in ref) and ref[0] != jf.edge("subset_mag").ref[1]


def test_edge_illcond_inputs():
    e = jf.edge("illcond")
    assert e.D.nsn == 230 and sorted(e.D.comp) == ["mag"] and not e.D.cov_ms.any()
    cond = [np.linalg.cond(jf.jla_V(e.D, a, b)) for a, b in e.ab]
    d = jf.rel_distance(_host(e.D, e.ab, e.mu), e.ref)
    print(cond, [float(x) for x in e.ref], d)
    assert min(cond) >= 1e6 and np.all(e.bad == -1)
    assert d < 1e-11


@pytest.fixture(scope="module")
def upper(tmp_path_factory):
    return jf.extract(tmp_path_factory.mktemp("jla_upper"), jf.GOLDEN_UPPER, jf.NAMES_UPPER)["syn21_upper"]


def test_upper_triangle_is_the_one_read(upper):
    """syn21_upper: matrix files whose strict lower triangles are noise, one of
    them a number a line.  Both restatements (np.triu) match the compiled
    reference; the same files read by their lower triangle do not."""
    d = os.path.dirname(upper.dataset)
    files = {k: jf.read_matrix(os.path.join(d, k + ".dat")) for k in ("mag", "stretch", "mag_colour")}
    assert all(not np.allclose(m, m.T) for m in files.values())
    assert len(open(os.path.join(d, "stretch.dat")).read().split("\n")) == 21 * 21 + 2
    D = sn.JLADataset(upper.dataset)
    assert D.nsn == 21 and sorted(D.comp) == ["mag", "mag_colour", "stretch"] and not D.twoscriptmfit
    for k, m in files.items():
        assert np.array_equal(D.comp[k], np.triu(m) + np.triu(m, 1).T)
    assert np.all(upper.ref < 1e4)
    host = _host(D, upper.ab, upper.mu)
    ld, bad = _longdouble(D, upper.ab, upper.mu)
    print(jf.rel_distance(upper.ref, ld), jf.rel_distance(host, ld))
    np.testing.assert_allclose(host, upper.ref, rtol=1e-13, atol=0)
    assert np.all(bad == -1) and jf.rel_distance(upper.ref, ld) < 1e-13
    for k, m in files.items():
        D.comp[k] = np.tril(m) + np.tril(m, -1).T
    lower = _host(D, upper.ab, upper.mu)
    print(lower)
    assert np.all(np.abs(lower / upper.ref - 1) > 1e-6)


def test_dataset_tables(goldens):
    D = sn.JLADataset(goldens["syn131"].dataset)
    assert D.nsn == 131 and D.twoscriptmfit and not D.diag_errors
    assert sorted(D.comp) == ["mag", "mag_colour", "stretch"]
    assert np.array_equal(D.one + D.A2, np.ones(131)) and 0 < D.A2.sum() < 131
    assert sn.JLADataset(goldens["syn37_diag"].dataset).diag_errors
    # a cut above every third variable empties the second set: one scriptm (:950-956)
    E = sn.JLADataset(goldens["syn37"].dataset, {"scriptmcut": "100"})
    assert not E.twoscriptmfit and np.array_equal(E.one, np.ones(37)) and not E.A2.any()


def test_distance_moduli():
    z, zh = np.array([0.1, 0.5]), np.array([0.101, 0.499])
    DA = np.array([[400.0, 1200.0], [410.0, 1250.0]])
    mu = sn.jla_distance_moduli(z, zh, DA)
    assert mu.shape == (2, 2)
    np.testing.assert_allclose(mu[1, 0], 5 * np.log10(1.101 * 1.1 * 410.0), rtol=1e-15)


def _open(dataset, override=""):
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(b"JLA", dataset.encode(), override.encode(), C.byref(h), err, 1024)
    if h:
        N.lib().cmbl_close(h)
    return rc, err.value.decode()


@pytest.fixture(scope="module")
def broken(goldens, tmp_path_factory):
    """Variants of syn5_indef the loader refuses."""
    src = os.path.dirname(goldens["syn5_indef"].dataset)
    d = str(tmp_path_factory.mktemp("jla_broken"))
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), d)
    rows = [l for l in open(os.path.join(d, "lc.txt")) if not l.startswith("#")]
    with open(os.path.join(d, "lc15.txt"), "w") as f:          # legacy layout: no set number
        f.write("".join(" ".join(r.split()[:15]) + "\n" for r in rows))
    with open(os.path.join(d, "lcset.txt"), "w") as f:
        f.write("".join(" ".join(r.split()[:15] + ["11"]) + "\n" for r in rows))
    m = open(os.path.join(d, "mag.dat")).read().split("\n", 1)
    open(os.path.join(d, "mag4.dat"), "w").write("4\n" + m[1])
    open(os.path.join(d, "magshort.dat"), "w").write(m[0] + "\n" + " ".join(m[1].split()[:-1]) + "\n")
    return os.path.join(d, "jla.dataset")


@pytest.mark.parametrize("override,code,text", [
    ("JLA_marginalize = T\n", UNSUPPORTED, "JLA_marginalize"),
    ("absdist_file = T\n", UNSUPPORTED, "absdist_file"),
    ("data_file = lc15.txt\n", UNSUPPORTED, "15 columns"),
    ("data_file = lcset.txt\n", FORMAT, "dataset number 11"),
    ("mag_covmat_file = mag4.dat\n", FORMAT, "expected size 5 got 4"),
    ("mag_covmat_file = magshort.dat\n", FORMAT, "wrong size"),
    ("mag_covmat_file = nowhere.dat\n", IO, "nowhere.dat"),
], ids=["marginalize", "absdist", "legacy_columns", "set_number", "matrix_n", "matrix_short", "matrix_missing"])
def test_loader_refusals(broken, override, code, text):
    rc, msg = _open(broken, override)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_theory_len_of_null_handle():
    assert N.lib().cmbl_theory_len(None) == 0


def test_likelihood_add_off_and_marginalize(goldens):
    ll = LikelihoodList()
    assert sn.jla_likelihood_add(ll, IniFile(text="use_JLA = F\n")) is None
    assert sn.jla_likelihood_add(ll, IniFile(text="jla_dataset = x\n")) is None
    assert len(ll) == 0
    with pytest.raises(NotImplementedError, match="JLA_marginalize"):
        sn.jla_likelihood_add(ll, IniFile(text=f"use_JLA = T\nJLA_marginalize = T\n"
                                               f"jla_dataset = {goldens['syn37'].dataset}\n"))
    assert len(ll) == 0


@pytest.mark.gpu
def test_likelihood_add_on(goldens):
    ll = LikelihoodList()
    like = sn.jla_likelihood_add(ll, IniFile(text=f"use_JLA = T\njla_dataset = {goldens['syn37'].dataset}\n"))
    assert list(ll) == [like]
    assert like.description() == ("JLA", "SN", "JLA", "December_2013")
    assert like.nuisance_names == ["alpha_JLA", "beta_JLA"] and like.n_theory == 37 and like.speed == 0
    assert like.lmax_needed() == 0
    names = ll.add_nuisance_parameters(["omegabh2"])
    assert names == ["omegabh2", "alpha_JLA", "beta_JLA"] and like.nuisance_indices == [2, 3]
    np.testing.assert_array_equal(like.lc.zcmb, sn.JLADataset(goldens["syn37"].dataset).zcmb)
