"""The weak-lensing kernels (wl.hip) against the recorded WL_LnLike of the
compiled reference, walker independence bit for bit, and a NaN row.

Tolerance, measured on the goldens without a GPU (test_weaklensing.py prints
both; absolute, on -lnL, values up to 4.9e4): (a) wl_loglike_host in f64
against the goldens 5.1e-11, (b) f64 against long double 3.7e-11.  The GPU
bound is 10 x the larger: 5.1e-10, below the 1e-6 the sampler needs; it leaves
room for the re-associated sums (the l-spline and Bessel operator formed at
open, the MFMA's order in the Limber sums, the quadratic form's tiles)."""
import numpy as np
import pytest

import wl_fixture as wf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GPU_ATOL = 10 * 5.1e-11
LOGZERO = 1e30


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return wf.extract(tmp_path_factory.mktemp("wl"))


def _like(g):
    from cosmomc_amd.weaklensing import WLLikelihood
    return WLLikelihood(g.dataset, use_weyl=g.weyl)


def _rows(row, W, pad=0):
    """[W, 1, n] theory rows on the device, each walker's row pad doubles longer than n (ld_walker > n)."""
    buf = torch.zeros((W, 1, len(row) + pad), dtype=torch.float64, device="cuda")
    buf[:, 0, :len(row)] = torch.tensor(row, device="cuda")
    return buf[:, :, :len(row)]


@pytest.mark.parametrize("name", wf.NAMES)
def test_matches_reference(goldens, name):
    g = goldens[name]
    like = _like(g)
    W = len(g.points)
    got = like.loglike_batch(_rows(g.row, W), torch.tensor(g.points, device="cuda")).cpu().numpy()
    print(name, "max |gpu - golden|:", np.abs(got - g.ref).max(), "of", g.ref.max())
    np.testing.assert_allclose(got, g.ref, rtol=0, atol=GPU_ATOL)


def test_walker_independence_bitwise(goldens):
    """The same point in slots 0, 1 and W - 1 of batches of W in {1, 2, 63, 65,
    129}, theory rows strided wider than a row, the other slots holding other
    points: the same bits everywhere."""
    g = goldens["syn_all"]
    like = _like(g)
    rng = np.random.RandomState(5)
    seen = set()
    for W in (1, 2, 63, 65, 129):
        nu = g.points[rng.randint(1, len(g.points), W)]
        slots = sorted({0, min(1, W - 1), W - 1})
        nu[slots] = g.points[0]
        rows = _rows(g.row, W, pad=3 + W % 2)
        rows[:, 0, 2 + 3 * like.nz:] *= torch.tensor(1 + 0.01 * rng.standard_normal(W), device="cuda")[:, None]
        rows[slots] = torch.tensor(g.row, device="cuda")
        got = like.loglike_batch(rows, torch.tensor(nu, device="cuda")).cpu().numpy()
        seen |= {got[s].tobytes() for s in slots}
        assert np.all(np.isfinite(got)) and np.all(got < 1e29)
    assert len(seen) == 1
    assert abs(np.frombuffer(seen.pop())[0] - g.ref[0]) <= GPU_ATOL


@pytest.mark.parametrize("where", ["h", "chis", "P"])
def test_nan_row_is_logzero_for_that_walker_alone(goldens, where):
    g = goldens["syn_all"]
    like = _like(g)
    W, bad = 70, 33
    nu = torch.tensor(np.tile(g.points[5], (W, 1)), device="cuda")
    rows = _rows(g.row, W)
    clean = like.loglike_batch(rows, nu).cpu().numpy()
    at = {"h": 0, "chis": 2 + 7, "P": 2 + 3 * like.nz + 5 * like.nz + 11}[where]
    rows[bad, 0, at] = float("nan")
    got = like.loglike_batch(rows, nu).cpu().numpy()
    assert got[bad] == LOGZERO
    keep = np.arange(W) != bad
    assert np.array_equal(got[keep], clean[keep]) and np.all(clean == clean[0])
