"""The SPTpol HIP kernels on window geometries that reach their edges
(cosmomc_amd.synthetic.make_sptpol_geom; test_sptpol_geometry.py shows on the
CPU that every reached l weighs at least 1e4 tolerances).  Reference: the
long-double restatement of sptpol_fixture.py for all 67 walkers, and the
compiled reference (tests/golden/sptpol_geom_ref.json) for the first three.
GPU only, through the C ABI; tolerance as test_gpu_sptpol.py (rtol 1e-10,
atol 1e-8).

Measured on an MI355X over every case, both switch settings and all call
layouts (232 comparisons): the kernel lies at most 6.7e-5 tolerances, that is
6.7e-5 * (1e-10 |lnL| + 1e-8), from long double.  The module runs in 7 s.  A
build whose upper derivative halo stops one l early (``lb + LPL < lcap``)
fails 18 of these tests and none of test_gpu_sptpol.py.
"""
import numpy as np
import pytest

import sptpol_fixture as sf
from conftest import load_golden
from sptpol_fixture import geom  # noqa: F401  (session fixture)

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, sf.needs_longdouble]

GOLDEN = load_golden("sptpol_geom_ref.json")
SWITCH = [False, True]
LAYOUT_CASES = ["odd_lmin_17", "edge_sweep_31_200", "bb_odd"]
NAN_CASES = ["odd_lmin_17", "lmin2", "edge_sweep_31_200", "bb_odd", "bb_17", "zero_group"]


def _call(like, W, dl, ld_field, ld_walker, nuis, ld_nuis):
    """cmbl_loglike_batch on device tensors with explicit strides -> numpy [W]."""
    from cosmomc_amd import _native as N
    out = torch.full((W,), float("nan"), dtype=torch.float64, device="cuda")
    rc = N.lib().cmbl_loglike_batch(like.handle, W, dl.data_ptr(), ld_field, ld_walker, nuis.data_ptr(), ld_nuis,
                                    out.data_ptr(), None, None)
    N.check(rc, like.handle)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _tight(geom, case, th=None, W=None):
    """The contiguous [W, nf, lmax + 2] device tensor and its strides: nothing behind lmax + 1."""
    th = geom.theory(case) if th is None else th
    th = th[:W] if W else th
    nf, n = th.shape[1], th.shape[2]
    assert n == geom.data(case).lmax + 2
    return torch.tensor(np.ascontiguousarray(th), device="cuda"), n, nf * n


def _nuis(geom, case, W=None):
    P = geom.nuis(case)[:W] if W else geom.nuis(case)
    return torch.tensor(np.ascontiguousarray(P), device="cuda"), P.shape[1]


def _check(got, ref, what):
    ref = np.asarray(ref)
    err = float(np.max(np.abs(got - ref.astype(np.float64)) / (sf.RTOL * np.abs(ref) + sf.ATOL).astype(np.float64)))
    print(f"{what}: max |kernel - reference| = {err:.3g} tolerances")
    np.testing.assert_allclose(got, ref.astype(np.float64), rtol=sf.RTOL, atol=sf.ATOL, err_msg=what)


@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", sf.ALL_CASES)
def test_every_case_tight_buffer(geom, case, on):
    """W = 67 (two walker tiles, the second partial) on a contiguous
    [W, nf, lmax + 2] tensor, ld_field = lmax + 2 exactly: all walkers against
    long double, the golden walkers against the compiled reference."""
    like = geom.open_native(case, on)
    dl, ldf, ldw = _tight(geom, case)
    nu, nn = _nuis(geom, case)
    got = _call(like, sf.W_ALL, dl, ldf, ldw, nu, nn)
    _check(got, geom.longdouble(case, on), f"{case} on={on} vs long double")
    if case in GOLDEN["cases"]:
        Wg = GOLDEN["walkers"]
        _check(got[:Wg], GOLDEN["cases"][case]["on" if on else "off"], f"{case} on={on} vs compiled reference")


@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", sf.ALL_CASES)
def test_every_case_padded_even_rows(geom, case, on):
    """The same through rows padded to an even length (the 16-byte theory loads
    where the tight rows are odd), NaN behind lmax + 1."""
    like = geom.open_native(case, on)
    th = geom.theory(case)
    W, nf, n = th.shape
    ldf = n + 6 + (n % 2)
    big = np.full((W, nf, ldf), np.nan)
    big[:, :, :n] = th
    nu, nn = _nuis(geom, case)
    got = _call(like, W, torch.tensor(big, device="cuda"), ldf, nf * ldf, nu, nn)
    _check(got, geom.longdouble(case, on), f"{case} on={on} padded rows vs long double")


@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", LAYOUT_CASES)
def test_call_layouts(geom, case, on):
    like = geom.open_native(case, on)
    th, P = geom.theory(case), geom.nuis(case)
    W, nf, n = th.shape
    ref = geom.longdouble(case, on)
    # W = 1
    dl, ldf, ldw = _tight(geom, case, W=1)
    nu, nn = _nuis(geom, case, W=1)
    _check(_call(like, 1, dl, ldf, ldw, nu, nn), ref[:1], f"{case} on={on} W=1")
    # odd ld_field (scalar theory loads) and padded nuisance rows
    ldo = n + 5 + (n % 2)
    assert ldo % 2 == 1
    big = np.full((W, nf, ldo), np.nan)
    big[:, :, :n] = th
    Pp = np.full((W, nn + 3), np.nan)
    Pp[:, :nn] = P
    dlo, nup = torch.tensor(big, device="cuda"), torch.tensor(Pp, device="cuda")
    _check(_call(like, W, dlo, ldo, nf * ldo, nup, nn + 3), ref, f"{case} on={on} odd ld_field, padded nuisances")
    # ld_walker = 0: walker 0's theory for everybody
    shared = geom.longdouble(case, on, dl=np.repeat(th[:1], W, axis=0))
    _check(_call(like, W, dlo, ldo, 0, nup, nn + 3), shared, f"{case} on={on} ld_walker=0")
    # a base pointer 8 bytes off 16-byte alignment with even strides: the scalar
    # path (theory_vec16) must give what the aligned call gives
    lde = n + 6 + (n % 2)
    flat = torch.full((W * nf * lde + 1,), float("nan"), dtype=torch.float64, device="cuda")
    view = flat[1:].view(W, nf, lde)                    # one double into a larger tensor
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and lde % 2 == 0
    view[:, :, :n] = torch.tensor(th, device="cuda")
    off8 = _call(like, W, view, lde, nf * lde, nup, nn + 3)
    _check(off8, ref, f"{case} on={on} theory pointer off by 8 bytes")
    al = view.clone()
    assert al.data_ptr() % 16 == 0
    _check(_call(like, W, al, lde, nf * lde, nup, nn + 3), ref, f"{case} on={on} aligned twin")


@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", NAN_CASES)
def test_theory_below_the_range_is_ignored(geom, case, on):
    """NaN at every l the likelihood does not read below its range: l <= lmin - 2
    for TE/EE (lmin - 1 is the derivative's halo and stays), l <= lmin - 1 for BB.
    The lower-side twin of test_sptpol_theory_beyond_lmax_is_ignored."""
    like = geom.open_native(case, on)
    lmin = geom.data(case).lmin
    first = lmin - 1 if sf.tag_of(case) == "SPTPOL_TEEE" else lmin
    th = geom.theory(case).copy()
    th[:, :, :first] = np.nan
    assert first >= 1 and np.isnan(th[:, :, 0]).all() and np.isfinite(th[:, :, first:]).all()
    nu, nn = _nuis(geom, case)
    for pad in (0, 7, 8):                               # tight, odd and even padded rows
        W, nf, n = th.shape
        big = np.full((W, nf, n + pad), np.nan)
        big[:, :, :n] = th
        got = _call(like, W, torch.tensor(big, device="cuda"), n + pad, nf * (n + pad), nu, nn)
        _check(got, geom.longdouble(case, on), f"{case} on={on} NaN below l = {first}, pad {pad}")


@pytest.mark.parametrize("case", ["odd_lmin_17", "nine_rows", "all_zero", "bb_zero_band"])
def test_same_handle_twice(geom, case):
    """The delta kernel zeroes the quadratic form's tickets for the next call: W = 67
    then W = 5 then W = 67 on one handle give identical bits for the shared walkers."""
    like = geom.open_native(case, True)
    dl, ldf, ldw = _tight(geom, case)
    nu, nn = _nuis(geom, case)
    a = _call(like, sf.W_ALL, dl, ldf, ldw, nu, nn)
    b = _call(like, 5, dl, ldf, ldw, nu, nn)
    c = _call(like, sf.W_ALL, dl, ldf, ldw, nu, nn)
    assert np.array_equal(a[:5], b) and np.array_equal(a, c)
    _check(a, geom.longdouble(case, True), f"{case} first of three calls")
