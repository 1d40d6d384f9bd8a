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
