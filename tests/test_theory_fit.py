"""cosmomc_amd.theory's host side: the monomial table and the least-squares
fit of a polynomial theory surface (pure numpy, no GPU)."""
import numpy as np
import pytest

from cosmomc_amd import theory as th


def test_monomials_graded_lexicographic():
    m = th.monomials(3, 2)
    assert m.dtype == np.int32
    assert m.tolist() == [[0, 0, 0],
                          [1, 0, 0], [0, 1, 0], [0, 0, 1],
                          [2, 0, 0], [1, 1, 0], [1, 0, 1], [0, 2, 0], [0, 1, 1], [0, 0, 2]]


def test_monomials_quartic_in_six():
    m = th.monomials(6, 4)
    assert m.shape == (210, 6)                       # C(10, 4)
    assert m[0].tolist() == [0] * 6
    assert m.sum(axis=1).max() == 4 and np.all(np.diff(m.sum(axis=1)) >= 0)
    assert len({tuple(r) for r in m.tolist()}) == 210


def test_monomials_degree_above_four_refused():
    with pytest.raises(ValueError):
        th.monomials(3, 5)


def test_fit_recovers_known_quadratic():
    rng = np.random.default_rng(5)
    ex = th.monomials(3, 2)
    center, scale = np.array([0.02, 0.12, 1.0]), np.array([0.002, 0.01, 0.05])
    true = rng.normal(size=(10, 2, 7))
    pts = center + scale * rng.uniform(-1.0, 1.0, size=(40, 3))
    theory = np.einsum("mk,kfl->mfl", th.basis(pts, ex, center, scale), true)
    coef, resid = th.fit_coefficients(pts, theory, ex, center, scale)
    assert coef.shape == (10, 2, 7)
    assert np.max(np.abs(coef - true)) < 1e-10
    assert resid < 1e-10
