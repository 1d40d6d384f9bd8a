"""The CMBlikes window kernels (cmbl_window_direct, cmbl_window_kernel<ABER, FG>,
cmbl_window_group<LDEC>) on window geometries that reach their edges:
cosmomc_amd.synthetic.make_cmbl_geom for the direct and the staged kernel, and
bin / map / lform selections of the reference's own BKPlanck and BK15 datasets
for the grouped one (cmbl_geom_fixture.BK_SELECTIONS).  test_cmbl_geom.py shows
on the CPU that every edge weight and every aberration end-point rule weighs at
least 100 tolerances.  References: the long-double restatement of
cmbl_geom_fixture.py (gaussian) or CMBLikesOracle (HL, BK) for all 67 walkers,
and the compiled reference (tests/golden/cmbl_geom_ref.json) for the first three.
GPU only, through the C ABI with explicit strides; tolerances as
test_gpu_cmblikes.py (gaussian rtol 1e-10 / atol 1e-9, HL and BK 1e-9 / 1e-8).

Measured on an MI355X over all 108 tests (195 comparisons): the kernels lie at
most 7.4e-4 tolerances from their reference.  The module runs in 13 s, no test
longer than 0.7 s.

What the module found.  With the parent's cmblwindow.h 13 of these tests fail,
all with NaN for every walker, and no older test does:
* cmbl_window_kernel (staged), 9 tests: a 16-byte theory load at l == the item's
  last l also brings l + 1, and the staging loop left it in the spectrum tile
  against a zero weight.  Where that l is an even lmax the entry is the caller's
  row padding, and 0 * NaN is NaN in the MFMA: the six aberration and SMICA cases
  with an even lmax on padded rows, two of them again with NaN outside the range,
  and the aligned padded call of test_call_layouts.  The slot is now set to 0.
* cmbl_window_group, 4 tests: an item whose first l is odd starts at the even l
  below it; with cl_lmin = 3 that is lmin - 1, read against zero weights.  The
  four lmin3 selections fail with NaN below lmin.  The entry is now taken as 0.
The direct kernel passed everything as it was.

Builds with one arithmetic mutation each fail this many tests of this module /
of test_gpu_cmblikes.py (48 tests):
  staged  nk = clen / 4                                   17 / 6
  staged  second column block stored for c1 < ncol - 1     4 / 6
  staged  aberration at lmax through l - 1 (not l - 2)    22 / 6
  direct  partial step takes the item's last l as 0       33 / 7
  direct  second column block stored for c1 < ncol - 1     6 / 0
  group   decorrelation evaluated at l + 1                25 / 2
"""
import numpy as np
import pytest

import cmbl_geom_fixture as cf
from cmbl_geom_fixture import bksel, cgeom  # noqa: F401  (session fixtures)
from conftest import load_golden
from cosmomc_amd import synthetic as syn

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, cf.needs_longdouble]

GOLDEN = load_golden("cmbl_geom_ref.json")
NAN_CASES = ["odd_lmin_17", "aber_odd_lmin_17", "seg_edges", "three_pairs", "aber_full_even", "aber_full_odd",
             "smica_even_top_aber", "hl_seg_edges_two_maps"] + cf.BK_CASES
LAYOUT_CASES = ["odd_lmin_17", "seg_edges", "aber_full_even", "bkp_all_bins-lin_quad"]
TWICE_CASES = ["full_even", "cols_32_33", "aber_seg_edges", "smica_even_top", "hl_full_even", "bk15_all_bins-flat"]
# cols_32_33 is not here: its 8-l windows and plik's 9-l bins put more than the pass's 64 columns into
# 352 l, and the sampler then keeps the two window stages apart, as it is meant to
FUSED_CASES = ["full_even", "odd_lmin_17", "seg_edges", "cols_1_16_17"]


def _src(case, cgeom, bksel):
    """The fixture object that knows ``case``: its theory, nuisances, reference and native handle."""
    return bksel if case in cf.BK_CASES else cgeom


def _call(like, W, dl, ld_field, ld_walker, nuis, ld_nuis):
    """cmbl_loglike_batch on device tensors with explicit strides -> numpy [W]."""
    from cosmomc_amd import _native as N
    out = torch.full((W,), float("nan"), dtype=torch.float64, device="cuda")
    rc = N.lib().cmbl_loglike_batch(like.handle, W, dl.data_ptr(), ld_field, ld_walker, nuis.data_ptr(), ld_nuis,
                                    out.data_ptr(), None, None)
    N.check(rc, like.handle)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _padded(th, pad, fill=np.nan):
    """[W, nf, n + pad] on the device with ``fill`` behind the n theory entries, and its strides."""
    W, nf, n = th.shape
    big = np.full((W, nf, n + pad), fill)
    big[:, :, :n] = th
    return torch.tensor(big, device="cuda"), n + pad, nf * (n + pad)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _check(case, got, ref, what):
    ref = np.asarray(ref).astype(np.float64)
    rtol, atol = cf.tol(case)
    with np.errstate(invalid="ignore"):
        err = float(np.max(np.nan_to_num(np.abs(got - ref), nan=np.inf) / (rtol * np.abs(ref) + atol)))
    print(f"{case} {what}: max |kernel - reference| = {err:.3g} tolerances")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=f"{case} {what}")


@pytest.mark.parametrize("case", cf.ALL_CASES + cf.BK_CASES)
def test_every_case_tight_buffer(cgeom, bksel, case):
    """W = 67 (two walker tiles, the second partial) on a contiguous [W, nf, lmax + 1]
    tensor, ld_field = lmax + 1 and nothing behind it: all walkers against long
    double or the oracle, the golden walkers against the compiled reference."""
    g = _src(case, cgeom, bksel)
    like = g.open_native(case)
    th, P = g.theory(case), g.nuis(case)
    dl, ldf, ldw = _padded(th, 0)
    got = _call(like, cf.W_ALL, dl, ldf, ldw, _dev(P), P.shape[1])
    _check(case, got, g.reference(case), "tight buffer")
    assert like.status() == 0
    if case in GOLDEN["cases"]:
        _check(case, got[:cf.W_GOLDEN], GOLDEN["cases"][case]["minus_lnL"], "tight buffer vs compiled reference")


@pytest.mark.parametrize("case", cf.ALL_CASES + cf.BK_CASES)
def test_every_case_padded_rows_nan_behind(cgeom, bksel, case):
    """Rows padded to the smallest even ld_field >= lmax + 2 (the 16-byte theory
    loads also where lmax is even) with NaN in every entry behind lmax: a weight
    of 0 does not silence a NaN that reaches an MFMA operand."""
    g = _src(case, cgeom, bksel)
    like = g.open_native(case)
    th, P = g.theory(case), g.nuis(case)
    n = th.shape[2]
    dl, ldf, ldw = _padded(th, 1 + (n + 1) % 2)
    assert ldf % 2 == 0 and ldf >= n + 1 and dl.data_ptr() % 16 == 0
    got = _call(like, cf.W_ALL, dl, ldf, ldw, _dev(P), P.shape[1])
    _check(case, got, g.reference(case), f"ld_field {ldf}, NaN behind lmax")


def _lmin(g, case):
    return g.oracle(case).lmin


@pytest.mark.parametrize("case", NAN_CASES)
def test_theory_outside_the_range_is_ignored(cgeom, bksel, case):
    """NaN at every l < lmin (the reference reads none of them: AddAberration's
    derivative at lmin is the one at lmin + 1) and behind lmax, with rows that are
    tight, padded by an odd and by an even count."""
    g = _src(case, cgeom, bksel)
    like = g.open_native(case)
    lmin = _lmin(g, case)
    th, P = g.theory(case).copy(), g.nuis(case)
    th[:, :, :lmin] = np.nan
    assert lmin >= 2 and np.isfinite(th[:, :, lmin:]).all()
    nu = _dev(P)
    for pad in (0, 7, 8):
        dl, ldf, ldw = _padded(th, pad)
        got = _call(like, cf.W_ALL, dl, ldf, ldw, nu, P.shape[1])
        _check(case, got, g.reference(case), f"NaN below l = {lmin} and behind lmax, pad {pad}")


@pytest.mark.parametrize("case", LAYOUT_CASES)
def test_call_layouts(cgeom, bksel, case):
    g = _src(case, cgeom, bksel)
    like = g.open_native(case)
    th, P = g.theory(case), g.nuis(case)
    W, nf, n = th.shape
    nn = P.shape[1]
    ref = g.reference(case)
    # W = 1
    dl, ldf, ldw = _padded(th[:1], 0)
    _check(case, _call(like, 1, dl, ldf, ldw, _dev(P[:1]), nn), ref[:1], "W=1")
    # odd ld_field (scalar theory loads) and padded nuisance rows
    pad = 5 + n % 2
    dlo, ldo, ldwo = _padded(th, pad)
    assert ldo % 2 == 1
    Pp = np.full((W, nn + 3), np.nan)
    Pp[:, :nn] = P
    nup = _dev(Pp)
    _check(case, _call(like, W, dlo, ldo, ldwo, nup, nn + 3), ref, "odd ld_field, padded nuisances")
    # ld_walker = 0: walker 0's theory for everybody
    shared = g.reference(case, dl=np.repeat(th[:1], W, axis=0))
    _check(case, _call(like, W, dlo, ldo, 0, nup, nn + 3), shared, "ld_walker=0")
    # a base pointer 8 bytes off 16-byte alignment with even strides: the scalar
    # path (theory_vec16) must give what the aligned call gives
    lde = n + 6 + (n % 2)
    flat = torch.full((W * nf * lde + 1,), float("nan"), dtype=torch.float64, device="cuda")
    view = flat[1:].view(W, nf, lde)                    # one double into a larger tensor
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and lde % 2 == 0
    view[:, :, :n] = torch.tensor(th, device="cuda")
    _check(case, _call(like, W, view, lde, nf * lde, nup, nn + 3), ref, "theory pointer off by 8 bytes")
    al = view.clone()
    assert al.data_ptr() % 16 == 0
    _check(case, _call(like, W, al, lde, nf * lde, nup, nn + 3), ref, "aligned twin")


@pytest.mark.parametrize("case", TWICE_CASES)
def test_same_handle_twice(cgeom, bksel, case):
    """W = 67, then W = 5, then W = 67 on one handle: identical bits for the shared
    walkers (the workspace, the quadratic form's tickets and the T_dust table carry
    nothing from one call into the next)."""
    g = _src(case, cgeom, bksel)
    like = g.open_native(case)
    th, P = g.theory(case), g.nuis(case)
    dl, ldf, ldw = _padded(th, 0)
    nu = _dev(P)
    a = _call(like, cf.W_ALL, dl, ldf, ldw, nu, P.shape[1])
    b = _call(like, 5, dl, ldf, ldw, nu, P.shape[1])
    c = _call(like, cf.W_ALL, dl, ldf, ldw, nu, P.shape[1])
    assert np.array_equal(a[:5], b) and np.array_equal(a, c)
    _check(case, a, g.reference(case), "first of three calls")


@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_window_pass_geometry(cgeom, tmp_path, case):
    """test_fused_window_pass (test_gpu_sampler.py) with a direct-window geometry
    dataset in the lensing likelihood's place: plik_lite and the dataset on one
    theory buffer run their window stages as one pass (theorypass.hip), the
    dataset's work items rebuilt on segment starts that plik's bins dictate
    (window_resegment).  The per-likelihood terms of the recorded points equal
    each likelihood's own loglike_batch (rtol 1e-12: only the summation split
    differs) and, for every walker, the long-double reference."""
    import pyoracle as po
    from cosmomc_amd import _native as N
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    from cosmomc_amd.sampler import BatchedMCMC
    W, steps = cf.W_ALL, 4
    data = syn.make_plik_lite(12345)
    plik = NativeCMBLikelihood("PLIK_LITE", data.write(str(tmp_path)))
    like = cgeom.open_native(case)
    plik.nuisance_indices = [2]
    like.nuisance_indices = [2]
    th = syn.walker_theory(W, seed=7, n_fields=10, ld_field=2512)
    dl = torch.tensor(th, device="cuda")
    s = BatchedMCMC(W, 3, [2], [[1]], 0, [0.0222, 0.9, 3.05], [0.0222, 1.1, 3.05], [0.0, 1.0, 0.0],
                    [0.0, 0.0025, 0.0], seed_ij=58, seed_kl=69)
    s.set_covariance(np.array([[0.002 ** 2]]))
    s.add_likelihood(plik, dl)
    s.add_likelihood(like, dl)
    assert N.lib().cmamd_debug_fused(s._h) > 0, N.lib().cmamd_debug_fused(s._h)
    s.enable_history(steps)
    s.set_start(np.tile([0.0222, 1.0, 3.05], (W, 1)))
    s.step(steps, fast_only=True)
    hist = s.history_host(0, steps)
    terms = s.history_terms(0, steps)
    s.close()
    po_plik = po.PlikLite(data)
    for k in (0, steps - 1):
        cal = hist[k, 0, :].copy()
        nu = torch.tensor(cal, device="cuda").reshape(-1, 1)
        np.testing.assert_allclose(terms[k, 0], plik.loglike_batch(dl, nu).cpu().numpy(), rtol=1e-12)
        np.testing.assert_allclose(terms[k, 1], like.loglike_batch(dl, nu).cpu().numpy(), rtol=1e-12)
        _check(case, terms[k, 1], cgeom.reference(case, dl=th, P=cal[:, None]), f"fused pass, step {k}")
        for w in (0, W // 2, W - 1):
            assert terms[k, 0, w] == pytest.approx(po_plik.loglike(th[w, :3], cal[w]), rel=1e-9)
