"""fit_derived and dl_columns (cosmomc_amd.theory): pure numpy, no GPU."""
import numpy as np
import pytest

from cosmomc_amd import theory as th


def test_fit_derived_recovers_an_exact_polynomial():
    """Three scalar surfaces that are exact degree-3 polynomials in 3 inputs:
    the fit returns their coefficients to 1e-12 relative (of the largest
    coefficient of each surface) and a residual at rounding level."""
    rng = np.random.default_rng(5)
    ex = th.monomials(3, 3)
    center, scale = np.array([0.3, -1.0, 2.0]), np.array([0.5, 2.0, -0.25])
    true = rng.normal(size=(len(ex), 3)) * np.array([70.0, 0.3, 0.8])
    pts = center + np.abs(scale) * rng.uniform(-2.0, 2.0, size=(4 * len(ex), 3))
    vals = th.basis(pts, ex, center, scale) @ true
    coef, resid = th.fit_derived(pts, vals, ex, center, scale)
    assert coef.shape == true.shape and coef.flags.c_contiguous
    rel = np.max(np.abs(coef - true), axis=0) / np.max(np.abs(true), axis=0)
    assert np.all(rel <= 1e-12), rel
    assert resid <= 1e-10 * np.max(np.abs(vals))


def test_fit_derived_refuses_bad_shapes():
    ex = th.monomials(2, 2)
    pts = np.zeros((10, 2))
    with pytest.raises(ValueError):
        th.fit_derived(pts, np.zeros(10), ex, [0, 0], [1, 1])
    with pytest.raises(ValueError):
        th.fit_derived(pts, np.zeros((9, 2)), ex, [0, 0], [1, 1])


def test_dl_columns_picks_the_right_columns():
    K, nf, L = 6, 3, 41
    coef = np.arange(K * nf * L, dtype=np.float64).reshape(K, nf, L)
    pos, ells = [0, 2, 2, 1], [40, 0, 7, 39]
    got = th.dl_columns(coef, pos, ells)
    assert got.shape == (K, 4) and got.flags.c_contiguous
    for i, (p, l) in enumerate(zip(pos, ells)):
        assert np.array_equal(got[:, i], coef[:, p, l])
    assert np.array_equal(th.dl_columns(coef, 1, [3, 5]), coef[:, 1, [3, 5]])   # one field for every l
    for bad_pos, bad_l in (([3], [0]), ([0], [41]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(ValueError):
            th.dl_columns(coef, bad_pos, bad_l)
