"""Weak lensing without a GPU: the host restatement (wl_loglike_host) against the
recorded WL_LnLike of the compiled reference, the host loader against the
quantities the harness printed (used_items, first_theta_bin_used; ls_cl and
ls_bessel are private in the reference, so they are checked through -lnL, which
the reference forms with its own: syn_acc has another ls_cl and Bessel binning
than the rest), wl_theory_row against the harness's row, the
refusals of cmbl_open("WL") (they happen before anything touches the device)
and wl_likelihood_add; the library's own loader, which uploads its tables, is
compared with the same quantities in the tests marked gpu.

Tolerance inputs of the GPU tests, measured here on the goldens (absolute, on
-lnL, values up to 4.9e4): (a) wl_loglike_host in f64 against the goldens
5.1e-11, (b) f64 against long double 3.7e-11.  The bound below is for (a): the
restatement keeps the reference's summation order, so it differs from the
compiled reference by the rounding of a few library calls (pow, exp, the
Bessel functions, the inverse covariance), a few ulp of a -lnL of 5e4: 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest

import wl_fixture as wf
from cosmomc_amd import _native as N
from cosmomc_amd import weaklensing as wl
from cosmomc_amd.ini import IniFile
from cosmomc_amd.likelihood import LikelihoodList

HOST_ATOL = 1e-9
FORMAT, UNSUPPORTED = -3, -6           # CMBL_ERR_* of cosmomc_amd.h


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return wf.extract(tmp_path_factory.mktemp("wl"))


@pytest.fixture(scope="module")
def datasets(goldens):
    return {n: wl.WLDataset(g.dataset, use_weyl=g.weyl) for n, g in goldens.items()}


@pytest.mark.parametrize("name", wf.NAMES)
def test_host_restatement_matches_reference(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    assert len(g.points) >= 5
    got = np.array([wl.wl_loglike_host(ds, g.row, p) for p in g.points])
    print(name, "max |f64 - golden|:", np.abs(got - g.ref).max())
    np.testing.assert_allclose(got, g.ref, rtol=0, atol=HOST_ATOL)


@pytest.mark.parametrize("name", ["syn_all", "syn_lens_weyl", "syn_acc"])
def test_longdouble_restatement_matches_reference(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    got = np.array([wl.wl_loglike_host(ds, g.row, p, np.longdouble) for p in g.points])
    f64 = np.array([wl.wl_loglike_host(ds, g.row, p) for p in g.points])
    print(name, "max |f64 - long double|:", float(np.abs(f64 - got).max()))
    np.testing.assert_allclose(got.astype(np.float64), g.ref, rtol=0, atol=HOST_ATOL)


@pytest.mark.parametrize("name", wf.NAMES)
def test_host_loader_matches_reference(goldens, datasets, name):
    g, ds = goldens[name], datasets[name]
    assert np.array_equal(ds.ls_cl, g.ls_row)        # the harness formed the row at the l it was given: these
    assert ds.used_items == g.used_items
    assert ds.first_theta_bin_used == g.first_theta_bin_used
    assert ds.n_theory == len(g.row)


def test_l_sampling_sizes():
    """The sizes wl.f90 is known to give at its defaults (acc = 1, lmax =
    50000): 75 l for the Limber sums, linear to 96 then log; the Bessel bins
    start at l = 2, tile the l range without gaps and end below lmax."""
    ls = wl.make_ls_cl(1.0, 50000)
    assert len(ls) == 75 and ls[0] == 2 and ls[23] == 94 and ls[24] == 100 and ls[-1] >= 50000 > ls[-2]
    lb, lo, hi = wl.make_bessel_bins(1.0, 50000)
    assert lo[0] == 2 and np.all(lo[1:] == hi[:-1] + 1) and hi[-1] <= 50000 and 360 <= len(lb) <= 375
    assert np.array_equal(lb, (lo + hi) / 2)


def test_golden_cases_cover_the_edges(goldens, datasets):
    """The conditions the goldens are there for: P entries outside the kh range,
    a shift of one knot spacing, shifted z off the table at both ends, A_IA = 0,
    negative alphaIA, and the selections of syn_cut."""
    for name, g in goldens.items():
        ds = datasets[name]
        P = g.row[2 + 3 * ds.nz:]
        assert 0 < np.count_nonzero(P == 0) < P.size
        s0 = ds.ngal + ds.nzb + 3
        assert np.all(g.points[0][s0:] == 0)
        assert np.all(g.points[1][s0:] == ds.z_p[1] - ds.z_p[0])
        assert g.points[2][s0:].max() > ds.z_p[1] - ds.z_p[0] and np.any(ds.z_p - g.points[2][s0:].max() < ds.z_p[0])
        assert np.any(ds.z_p - g.points[2][s0:].min() > ds.z_p[-1])
        assert g.points[3][ds.ngal + ds.nzb] == 0 and g.points[4][ds.ngal + ds.nzb + 1] < 0
    cut = datasets["syn_cut"]
    assert (1, 1, 1) not in {it[:3] for it in cut.used_items}                 # a row that keeps no point
    assert (4, 2, 2) not in {it[:3] for it in cut.used_items}                 # measurements without a row
    assert datasets["syn_noxim"].xim_index == 0 and not datasets["syn_noxim"].ia_des1yr
    assert datasets["syn_nogal"].ngal == 0
    assert datasets["syn_acc"].nl != datasets["syn_all"].nl


@pytest.mark.parametrize("name", ["syn_all", "syn_lens_weyl"])
def test_theory_row_matches_harness(goldens, datasets, name):
    """h, omm, chis, Hs and the zero pattern of P exactly; P itself to the error
    of the reference's bicubic interpolation of the harness's 60 x 12 grid of the
    analytic ln P (6.4e-4 measured; d ln k = 0.14, dz = 0.15)."""
    g, ds = goldens[name], datasets[name]
    nz = ds.nz
    which = wf.pk_which(g.weyl)
    row = wl.wl_theory_row(ds, g.h0 / 100, g.omdm, g.chis, g.Hs, g.row[2 + 2 * nz:2 + 3 * nz],
                           lambda kh, z: np.exp(wf.analytic_lnpk(which, np.log(kh), z)), g.kh_min, g.kh_max)
    assert row.shape == g.row.shape
    assert np.array_equal(row[:2 + 3 * nz], g.row[:2 + 3 * nz])
    P0, P1 = row[2 + 3 * nz:], g.row[2 + 3 * nz:]
    assert np.array_equal(P0 == 0, P1 == 0)
    np.testing.assert_allclose(P0[P1 != 0], P1[P1 != 0], rtol=2e-3, atol=0)
    _, _, Dg = wf.cosmology(ds.z_p)
    np.testing.assert_allclose(Dg, g.row[2 + 2 * nz:2 + 3 * nz], rtol=1e-4, atol=0)


# ---- refusals of the library's loader: each names its key

def _open(dataset, override=""):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = N.lib().cmbl_open(b"WL", dataset.encode(), override.encode(), C.byref(h), err, 1024)
    if rc == 0:
        N.lib().cmbl_close(h)
    return rc, err.value.decode()


REFUSALS = [("measurements_format = CFHTLENS", UNSUPPORTED, "measurements_format"),
            ("intrinsic_alignment_model = linear", UNSUPPORTED, "intrinsic_alignment_model"),
            ("wl_use_weyl = T", UNSUPPORTED, "wl_use_weyl"),
            ("use_photoz_marge = T", UNSUPPORTED, "use_photoz_marge"),
            ("cut_theta = 3", UNSUPPORTED, "cut_theta")]


@pytest.mark.parametrize("override,code,text", REFUSALS)
def test_loader_refusals(goldens, override, code, text):
    rc, msg = _open(goldens["syn_all"].dataset, override)
    assert rc == code and text in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match=text):
        k, v = (x.strip() for x in override.split("="))
        wl.WLDataset(goldens["syn_all"].dataset, {k: v})


def test_weyl_is_refused_with_galaxy_data_only(goldens):
    """wl_use_weyl with gammat or wtheta wanted is refused (wl.f90:201-203);
    with xip and xim alone the refusal is gone (the open then needs the device)."""
    rc, msg = _open(goldens["syn_gg"].dataset, "wl_use_weyl = T")
    assert rc == UNSUPPORTED and "wl_use_weyl" in msg
    assert wl.WLDataset(goldens["syn_lens_weyl"].dataset, use_weyl=True).use_weyl


@pytest.mark.parametrize("key", ["lmax", "num_z_bins", "num_theta_bins", "acc"])
def test_malformed_number_is_a_format_error_naming_the_key(goldens, key):
    rc, msg = _open(goldens["syn_all"].dataset, key + " = 3x")
    assert rc == FORMAT and key in msg, (rc, msg)


def test_wrong_covariance_size_is_a_format_error(goldens, tmp_path):
    g = goldens["syn_nogal"]
    for f in os.listdir(g.dir):
        (tmp_path / f).write_bytes(open(os.path.join(g.dir, f), "rb").read())
    cov = open(os.path.join(g.dir, "cov.dat")).read().split("\n")
    (tmp_path / "cov.dat").write_text("\n".join(cov[:-2]) + "\n")
    rc, msg = _open(str(tmp_path / "wl.dataset"))
    assert rc == FORMAT and "cov size" in msg, (rc, msg)


def test_likelihood_add_off(goldens):
    lst = LikelihoodList()
    assert wl.wl_likelihood_add(lst, IniFile(text="use_WL = F\nwl_dataset[DES] = nowhere.dataset\n")) == []
    assert len(lst) == 0


def _des_ini(g, extra=""):
    """The keys of batch3/DES.ini (with DES_lensing.ini's used_data_types in extra), on a golden dataset."""
    return IniFile(text="use_WL = T\nwl_use_non_linear = T\nwl_dataset[DES] = %s\nwl_dataset_speed[DES] = 8\n%s"
                   % (g.dataset, extra))


@pytest.mark.gpu
def test_likelihood_add_on(goldens):
    lst = LikelihoodList()
    like, = wl.wl_likelihood_add(lst, _des_ini(goldens["syn_all"]))
    assert like.get_tag() == "DES" and like.speed == 8 and like.LikelihoodType == "WL"
    assert like.use_non_linear and not like.use_weyl
    assert like.nuisance_names == wf.param_names(3, 2)
    assert like.n_theory == len(goldens["syn_all"].row) and like.n_used == 100
    lens, = wl.wl_likelihood_add(LikelihoodList(), _des_ini(goldens["syn_all"],
                                                            "wl_dataset[DES,used_data_types] = xip xim\n"))
    assert lens.n_used == 60 and lens.n_columns == 6
    names = lst.add_nuisance_parameters(["omegabh2"])
    assert names[1:] == like.nuisance_names and like.nuisance_indices == list(range(2, 2 + len(like.nuisance_names)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", wf.NAMES)
def test_library_loader_matches_reference(goldens, name):
    g = goldens[name]
    like = wl.WLLikelihood(g.dataset, use_weyl=g.weyl)
    ls_cl, ls_b, items = like.loader_arrays()
    assert np.array_equal(ls_cl, like.ds.ls_cl) and np.array_equal(ls_b, like.ds.ls_bessel)      # the two loaders agree
    assert [tuple(r) for r in items] == g.used_items
    assert like.first_theta_bin_used == g.first_theta_bin_used
    assert like.n_theory == len(g.row)
