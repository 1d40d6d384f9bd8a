"""The SZ cluster-counts kernels (sz.hip) against the recorded SZCC_Cash of the
compiled reference, the library's loader against the harness's printed
quantities, walker independence bit for bit, NaN rows, batches that mix
scatter_SZ == 0 with scatter_SZ != 0, and the sparse entry.

Tolerance, measured on the goldens without a GPU (test_szcounts.py prints
both; absolute, on -lnL, values up to 2.0e4): (a) sz_loglike_host in f64
against the goldens: 0 on every golden; (b) f64 against long double: 2.7e-5.
The GPU bound is 10 x the larger, the project's rule: 2.7e-4.

(b) is that large at two points only, syn_inside 1 and 2 (alpha_SZ = 1,
bias_SZ = 0.1: 2.7e-5 and 2.9e-9), where the counts of S/N bins that hold
clusters come from 1 - erf in its cancellation range and f64 keeps no relative
accuracy; over every other golden point (b) is 1.5e-10 at most.  So every
other point is also held to 10 x that, 1.5e-9: the reference rounds each
completeness to single precision and the kernels round there too, which
leaves the rounding of the f64 sums (the ln Y trapezoid summed by nodes in a
16-lane tree, DN in a 64-lane tree) and of the device's exp, pow, log and erf.
"""
import numpy as np
import pytest

import sz_fixture as sf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GPU_ATOL = 10 * 2.7e-5
WELL_ATOL = 10 * 1.5e-10                               # every point but ILL
ILL = {"syn_inside": [1, 2]}
LOGZERO = 1e30


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return sf.extract(tmp_path_factory.mktemp("sz"))


@pytest.fixture(scope="module")
def inside(goldens):
    from cosmomc_amd.szcounts import SZLikelihood
    return goldens["syn_inside"], SZLikelihood(goldens["syn_inside"].ini)


def _rows(row, W, pad=0):
    """[W, 1, n] theory rows on the device, each walker's row pad doubles longer than n (ld_walker > n)."""
    buf = torch.zeros((W, 1, len(row) + pad), dtype=torch.float64, device="cuda")
    buf[:, 0, :len(row)] = torch.tensor(row, device="cuda")
    return buf[:, :, :len(row)]


def _eval(like, rows, nu):
    return like.loglike_batch(rows, torch.tensor(np.ascontiguousarray(nu), device="cuda")).cpu().numpy()


@pytest.mark.parametrize("name", sf.NAMES)
def test_matches_reference(goldens, name):
    from cosmomc_amd.szcounts import SZLikelihood
    g = goldens[name]
    like = SZLikelihood(g.ini)
    assert like.n_theory == len(g.row) and like.nuisance_names == sf.PARAM_NAMES
    sz, dn, j1, j2 = like.loader_arrays()
    assert (like.nzs, like.nm, like.Nz, like.nq) == (g.nzs, g.nm, g.nz, g.nq)
    assert np.array_equal(sz, g.steps_z) and np.array_equal(dn, g.DNcat)
    assert np.all(j2 >= j1) and np.all(j1[1:] == j2[:-1]) and j1[0] == 0 and j2[-1] == like.nzs - 1
    got = _eval(like, _rows(g.row, len(g.points)), g.points)
    assert np.all(np.abs(g.ref) < 1e29)
    well = np.setdiff1d(np.arange(len(g.ref)), ILL.get(name, []))
    print(name, "max |gpu - golden|:", np.abs(got - g.ref).max(), "of", g.ref.max(), "; without the ill-conditioned points:",
          np.abs(got - g.ref)[well].max())
    np.testing.assert_allclose(got, g.ref, rtol=0, atol=GPU_ATOL)
    np.testing.assert_allclose(got[well], g.ref[well], rtol=0, atol=WELL_ATOL)


def test_walker_independence_bitwise(inside):
    """The same point in slots 0, 1 and W - 1 of batches of W in {1, 2, 63, 65,
    129}, theory rows strided wider than a row, the other slots holding other
    points (with and without scatter): the same bits everywhere."""
    g, like = inside
    rng = np.random.RandomState(5)
    seen = set()
    for W in (1, 2, 63, 65, 129):
        nu = g.points[rng.randint(1, len(g.points), W)]
        slots = sorted({0, min(1, W - 1), W - 1})
        nu[slots] = g.points[0]
        got = _eval(like, _rows(g.row, W, pad=3 + W % 5), nu)
        seen |= {got[s].tobytes() for s in slots}
        ref = {tuple(p): r for p, r in zip(g.points, g.ref)}
        np.testing.assert_allclose(got, [ref[tuple(p)] for p in nu], rtol=0, atol=GPU_ATOL)
    assert len(seen) == 1


@pytest.mark.parametrize("where", ["H0", "E", "dA", "grid"])
def test_nan_is_logzero_for_that_walker_alone(inside, where):
    g, like = inside
    W = 5
    nu = g.points[[0, 9, 3, 10, 12]]                       # two of them with scatter_SZ == 0
    assert nu[1, 3] == 0 and nu[3, 3] == 0
    rows = _rows(g.row, W, pad=1).clone()
    clean = _eval(like, rows, nu)
    nzs = g.nzs
    at = {"H0": 0, "E": 3 + 40, "dA": 3 + nzs + 120, "grid": 3 + 2 * nzs + 150 * g.nm + 60}[where]
    for bad in (1, 2):                                     # a walker of either branch
        r = rows.clone()
        r[bad, 0, at] = float("nan")
        got = _eval(like, r, nu)
        assert got[bad] == LOGZERO
        keep = np.arange(W) != bad
        assert np.array_equal(got[keep], clean[keep])


def test_mixed_scatter_batch_equals_the_two_apart(inside):
    g, like = inside
    nu = g.points[[9, 0, 10, 1, 12, 9, 2]]
    zero = nu[:, 3] == 0
    assert 0 < zero.sum() < len(nu)
    both = _eval(like, _rows(g.row, len(nu)), nu)
    a = _eval(like, _rows(g.row, int(zero.sum())), nu[zero])
    b = _eval(like, _rows(g.row, int((~zero).sum())), nu[~zero])
    assert np.array_equal(both[zero], a) and np.array_equal(both[~zero], b)


def test_sparse_evaluation_touches_the_live_slots_only(inside):
    g, like = inside
    W = 6
    nu = torch.tensor(g.points[:W], device="cuda")
    rows = _rows(g.row, W)
    dense = like.loglike_batch(rows, nu).cpu().numpy()
    out = torch.full((W,), -7.0, dtype=torch.float64, device="cuda")
    like.loglike_batch_sparse(rows, nu, out, torch.tensor([4], dtype=torch.int32, device="cuda"))
    got = out.cpu().numpy()
    assert np.array_equal(got[:4], dense[:4]) and np.all(got[4:] == -7.0)
