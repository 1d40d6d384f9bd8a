"""The alpha, beta-marginalised JLA likelihood without a GPU: the grid, the
numpy restatement (cosmomc_amd.supernovae.jla_marge_loglike_host) against the
compiled reference's recorded jla_LnLike with JLA_marginalize = T, the refusals
of cmbl_open("JLA_MARGE") that come before any device call, and
jla_likelihood_add's keyword."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import jla_marge_fixture as mf
from cosmomc_amd import _native as N
from cosmomc_amd import supernovae as sn
from cosmomc_amd.ini import IniFile
from cosmomc_amd.likelihood import LikelihoodList

ARG, FORMAT, UNSUPPORTED = -1, -3, -6


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return mf.extract(tmp_path_factory.mktemp("jla_marge"))


@pytest.mark.parametrize("steps,count", [(0, 1), (1, 5), (2, 13), (3, 29), (7, 149)])
def test_grid_counts(steps, count):
    al, be = sn.jla_marge_grid(steps, 0.003, 0.04)
    assert len(al) == len(be) == count


def test_grid_order_and_centres():
    """alpha_i outer, beta_i inner (:243-251); the centres are the reference's
    single-precision literals promoted to double (:119-120), not 0.14 and 3.123."""
    al, be = sn.jla_marge_grid(1, 0.003, 0.04)
    ca, cb = float(np.float32(0.14)), float(np.float32(3.123))
    assert ca != 0.14 and cb != 3.123
    assert list(al) == [ca - 0.003, ca, ca, ca, ca + 1 * 0.003]
    assert list(be) == [cb, cb - 0.04, cb, cb + 1 * 0.04, cb]
    al, be = sn.jla_marge_grid(2, 0.01, 0.1)
    ij = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if a * a + b * b <= 4]
    assert list(al) == [ca + a * 0.01 for a, _ in ij] and list(be) == [cb + b * 0.1 for _, b in ij]
    al, be = sn.jla_marge_grid(0, 0.003, 0.04, center=(0.2, 2.5))
    assert list(al) == [0.2] and list(be) == [2.5]


@pytest.mark.parametrize("case", mf.CASES)
def test_host_restatement_matches_reference(cases, case):
    c = cases[case]
    D = sn.JLADataset(c.dataset)
    assert len(sn.jla_marge_grid(**c.options)[0]) == c.n_points
    got = np.array([sn.jla_marge_loglike_host(D, mu, **c.options) for mu in c.mu])
    print(case, got, np.abs(got / c.ref - 1).max())
    assert np.all(np.isfinite(c.ref)) and np.all(c.ref < 1e29)
    np.testing.assert_allclose(got, c.ref, rtol=mf.RTOL, atol=0)


def test_indefinite_case_drops_points(cases):
    c = cases["syn5_indef_s2"]
    assert 0 < c.n_kept < c.n_points == 13
    L = sn.jla_marge_points_host(c.dataset, c.mu[0], **c.options)
    assert (L != sn.LOGZERO).sum() == c.n_kept


def _open(dataset, override=""):
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(b"JLA_MARGE", dataset.encode(), override.encode(), C.byref(h), err, 1024)
    if h:
        N.lib().cmbl_close(h)
    return rc, err.value.decode()


@pytest.mark.parametrize("override,code,text", [
    ("JLA_marge_steps = -1\n", ARG, "JLA_marge_steps"),
    ("JLA_marge_steps = 17\n", ARG, "JLA_marge_steps"),
    ("JLA_step_width_alpha = 0\n", ARG, "JLA_step_width_alpha"),
    ("JLA_step_width_beta = 0\n", ARG, "JLA_step_width_beta"),
    ("JLA_step_width_beta = -0.04\n", ARG, "JLA_step_width_beta"),
    ("absdist_file = T\n", UNSUPPORTED, "absdist_file"),
    ("JLA_marginalize = T\nabsdist_file = T\n", UNSUPPORTED, "absdist_file"),
], ids=["steps_negative", "steps_17", "width_alpha_0", "width_beta_0", "width_beta_negative", "absdist",
        "absdist_with_key"])
def test_loader_refusals(cases, override, code, text):
    rc, msg = _open(cases["syn5_indef_s2"].dataset, override)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_legacy_columns_refused(cases, tmp_path):
    src = os.path.dirname(cases["syn5_indef_s2"].dataset)
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), str(tmp_path))
    rows = [l for l in open(os.path.join(src, "lc.txt")) if not l.startswith("#")]
    with open(os.path.join(str(tmp_path), "lc15.txt"), "w") as f:
        f.write("".join(" ".join(r.split()[:15]) + "\n" for r in rows))
    rc, msg = _open(os.path.join(str(tmp_path), "jla.dataset"), "data_file = lc15.txt\n")
    assert rc == UNSUPPORTED and "15 columns" in msg, (rc, msg)


@pytest.mark.gpu
def test_no_point_left_is_a_format_error(cases):
    """Which points the reference drops is decided where V is factored, on the
    device: syn5_indef is indefinite at (0.2, 2.5), the only point of this grid."""
    rc, msg = _open(cases["syn5_indef_s2"].dataset,
                    "JLA_marge_steps = 0\nJLA_alpha_center = 0.2\nJLA_beta_center = 2.5\n")
    assert rc == FORMAT, (rc, msg)
    assert "not positive definite" in msg, msg
    with pytest.raises(ValueError):
        sn.jla_marge_loglike_host(cases["syn5_indef_s2"].dataset, cases["syn5_indef_s2"].mu[0], steps=0,
                                  center=(0.2, 2.5))


def test_the_jla_tag_points_to_the_new_one(cases):
    h, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(b"JLA", cases["syn37_s7"].dataset.encode(), b"JLA_marginalize = T\n", C.byref(h), err, 1024)
    assert rc == UNSUPPORTED and "JLA_marginalize" in err.value.decode() and "JLA_MARGE" in err.value.decode()


def test_dataset_class_still_refuses_the_key(cases):
    with pytest.raises(NotImplementedError, match="JLA_marginalize"):
        sn.JLADataset(cases["syn37_s7"].dataset, {"JLA_marginalize": "T"})


def test_likelihood_add_keyword(cases):
    ll = LikelihoodList()
    ini = f"use_JLA = T\nJLA_marginalize = T\njla_dataset = {cases['syn37_s7'].dataset}\n"
    with pytest.raises(NotImplementedError, match="JLA_marginalize"):
        sn.jla_likelihood_add(ll, IniFile(text=ini))
    assert sn.jla_likelihood_add(ll, IniFile(text="use_JLA = F\nJLA_marginalize = T\n"), allow_marginalize=True) is None
    assert len(ll) == 0


@pytest.mark.gpu
def test_likelihood_add_marginalised(cases):
    ll = LikelihoodList()
    like = sn.jla_likelihood_add(ll, IniFile(text=f"use_JLA = T\nJLA_marginalize = T\nJLA_marge_steps = 2\n"
                                                  f"JLA_step_width_beta = 0.05\n"
                                                  f"jla_dataset = {cases['syn37_s7'].dataset}\n"),
                                 allow_marginalize=True)
    assert list(ll) == [like] and isinstance(like, sn.JLAMargeLikelihood)
    assert like.description() == ("JLA", "SN", "JLA", "December_2013")
    assert like.nuisance_names == [] and like.n_theory == 37 and like.speed == 0 and like.lmax_needed() == 0
    assert (like.steps, like.width_alpha, like.width_beta, like.n_grid) == (2, 0.003, 0.05, 13)
    assert ll.add_nuisance_parameters(["omegabh2"]) == ["omegabh2"] and like.nuisance_indices == []
    assert len(like.lc.zcmb) == 37
