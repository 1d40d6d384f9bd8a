"""The alpha, beta-marginalised JLA likelihood on the GPU (cmbl_open tag
JLA_MARGE: jla_marge_chol_kernel / jla_marge_inv_kernel at open,
jla_marge_pro_kernel / jla_marge_qf_kernel / jla_marge_chi_kernel /
jla_marge_fin_kernel per evaluation): the compiled reference's goldens, tile, grid, walker and chunk
edges against the long-double restatement, bit independence of a walker's
result from the batch, dropped grid points, a non-finite row and the host
entry."""

import numpy as np
import pytest

import jla_fixture as jf
import jla_marge_fixture as mf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = mf.RTOL


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return mf.extract(tmp_path_factory.mktemp("jla_marge"))


def _dl(mu):
    return torch.tensor(np.ascontiguousarray(mu)[:, None, :], device="cuda")


def _eval(like, mu):
    return like.loglike_batch(_dl(mu), None).cpu().numpy()


def _singles(like, mu):
    return np.array([_eval(like, mu[i:i + 1])[0] for i in range(len(mu))])


@pytest.mark.parametrize("case", mf.CASES)
def test_goldens(cases, case):
    from cosmomc_amd.supernovae import JLAMargeLikelihood
    c = cases[case]
    like = JLAMargeLikelihood(c.dataset, **c.options)
    assert like.n_theory == c.mu.shape[1] and like.nuisance_names == [] and like.speed == 0
    assert like.name == "JLA" and like.LikelihoodType == "SN" and like.lmax_needed() == 0
    assert (like.n_points, like.n_grid) == (c.n_points, c.n_kept)
    got = _eval(like, c.mu)
    print(case, got, np.abs(got / c.ref - 1).max())
    np.testing.assert_allclose(got, c.ref, rtol=RTOL, atol=0)
    if case == "syn5_indef_s2":
        assert like.n_grid < like.n_points


@pytest.mark.parametrize("two", [False, True], ids=["one_scriptm", "two_scriptm"])
@pytest.mark.parametrize("nsn", [1, 2, 16, 17, 33, 64, 65])
def test_tile_edges(tmp_path, nsn, two):
    from cosmomc_amd.supernovae import JLADataset, JLAMargeLikelihood
    ds, mu, _ = jf.make_synthetic(str(tmp_path), nsn, jf.COMPONENTS, two, 1000 + nsn)
    D = JLADataset(ds)
    assert D.twoscriptmfit == (two and nsn > 1)
    ref, kept = mf.marge_longdouble_rows(D, mu, 1, 0.003, 0.04)
    like = JLAMargeLikelihood(ds, steps=1)
    assert like.n_grid == kept == 5
    got = _eval(like, mu)
    print(nsn, two, jf.rel_distance(got, ref))
    assert jf.rel_distance(got, ref) <= RTOL


def test_bits_independent_of_batch(tmp_path):
    """nsn = 257 (Np = 272: a last 16-row tile with one real row, a last row
    block with one tile), 13 grid points: five rows one at a time, at W = 17, at
    W = 67 in permuted order with ld_walker = 288, and through the sparse entry
    with 5 live of 67 slots."""
    from cosmomc_amd.supernovae import JLADataset, JLAMargeLikelihood, jla_marge_loglike_host
    n = 257
    ds, mu3, _ = jf.make_synthetic(str(tmp_path), n, jf.COMPONENTS, True, 2570, fmt="%.9g")
    mu = np.concatenate([mu3, mu3[:2] + 0.01])
    like = JLAMargeLikelihood(ds, steps=2)
    assert like.n_grid == 13
    single = _singles(like, mu)
    ref = jla_marge_loglike_host(JLADataset(ds), mu[0], steps=2)
    print(single, single[0] / ref - 1)
    np.testing.assert_allclose(single[0], ref, rtol=RTOL, atol=0)
    assert np.array_equal(_eval(like, mu[np.arange(17) % 5]), single[np.arange(17) % 5])
    W, ldw = 67, 288
    perm = np.random.RandomState(5).permutation(W)
    case = perm % 5
    dl = torch.full((W, 1, ldw), 7.0, dtype=torch.float64, device="cuda")
    dl[:, 0, :n] = torch.tensor(mu[case], device="cuda")
    assert np.array_equal(like.loglike_batch(dl, None).cpu().numpy(), single[case])
    # the sparse entry: live slots [0, 5); the dead slots hold NaN moduli, which would show in a live
    # walker's tile if they were read, and their outputs stay as they were
    dl[5:] = float("nan")
    out = torch.full((W,), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.tensor([5], dtype=torch.int32, device="cuda")
    like.loglike_batch_sparse(dl, None, out, cnt)
    sp = out.cpu().numpy()
    assert np.array_equal(sp[:5], single[case[:5]])
    assert np.all(sp[5:] == -1.0)


def test_chunks(tmp_path):
    """W = 1030: a second launch of six walkers behind the 1024 of the first."""
    from cosmomc_amd.supernovae import JLAMargeLikelihood
    n, W = 17, 1030
    ds, mu3, _ = jf.make_synthetic(str(tmp_path), n, jf.COMPONENTS, True, 170)
    mu = mu3[0][None, :] + 0.03 * np.random.RandomState(17).standard_normal((W, n))
    like = JLAMargeLikelihood(ds, steps=1)
    assert like.workspace_bytes(W) == like.workspace_bytes(1024)
    got = _eval(like, mu)
    assert np.all(np.isfinite(got)) and np.all(got < 1e29)
    for w in (0, 127, 128, 1023, 1024, 1029):
        assert _eval(like, mu[w:w + 1])[0] == got[w], w


def test_odd_grid_count(cases):
    """149 grid points on syn37 at five other rows than the goldens'."""
    from cosmomc_amd.supernovae import JLADataset, JLAMargeLikelihood
    c = cases["syn37_s7"]
    mu = c.mu[::-1] + 0.02
    ref, kept = mf.marge_longdouble_rows(JLADataset(c.dataset), mu, 7, 0.003, 0.04)
    like = JLAMargeLikelihood(c.dataset)
    assert like.n_grid == kept == 149
    got = _eval(like, mu)
    print(jf.rel_distance(got, ref))
    assert jf.rel_distance(got, ref) <= RTOL


def test_full_size(tmp_path):
    """nsn = 740 as the JLA sample: any buffer sized by nsn, 12 row blocks."""
    from cosmomc_amd.supernovae import JLADataset, JLAMargeLikelihood, jla_marge_loglike_host
    ds, mu3, _ = jf.make_synthetic(str(tmp_path), 740, ("mag", "stretch"), True, 740, fmt="%.9g")
    mu = np.concatenate([mu3, mu3[:2] - 0.02])
    like = JLAMargeLikelihood(ds, steps=2)
    assert like.n_grid == 13 and like.grid_bytes == 13 * 752 * 752 * 8
    assert like.workspace_bytes(5000) == like.workspace_bytes(1024) == 1024 * like.workspace_bytes(1)
    D = JLADataset(ds)
    ref = np.array([jla_marge_loglike_host(D, m, steps=2) for m in mu[:2]])
    got = _eval(like, mu)
    print(got, np.abs(got[:2] / ref - 1).max())
    np.testing.assert_allclose(got[:2], ref, rtol=RTOL, atol=0)
    assert np.array_equal(got, _singles(like, mu))


@pytest.mark.parametrize("two", [0, 1], ids=["one_scriptm", "two_scriptm"])
def test_diag_errors(two):
    """No component matrix: V^-1 is the diagonal invvars and no matrix is stored."""
    from cosmomc_amd.supernovae import JLAMargeLikelihood
    e = jf.edge("diag300_%d" % two)
    ref, kept = mf.marge_longdouble_rows(e.D, e.mu, 2, 0.003, 0.04)
    like = JLAMargeLikelihood(e.dataset, steps=2)
    assert like.n_grid == kept == 13 and like.grid_bytes == 0
    got = _eval(like, e.mu)
    print(two, jf.rel_distance(got, ref))
    assert jf.rel_distance(got, ref) <= RTOL
    assert np.array_equal(got, _singles(like, e.mu))


def test_dropped_points(cases):
    """syn5_indef with a grid that reaches (0.2, 2.5): a batch around the golden
    rows stays finite and every walker equals its single evaluation."""
    from cosmomc_amd.supernovae import JLADataset, JLAMargeLikelihood
    c = cases["syn5_indef_s2"]
    like = JLAMargeLikelihood(c.dataset, **c.options)
    assert like.n_grid == c.n_kept < c.n_points
    mu = np.concatenate([c.mu - 0.05, c.mu, c.mu + 0.05])
    got = _eval(like, mu)
    assert np.all(np.isfinite(got)) and np.all(got < 1e29)
    np.testing.assert_allclose(got[5:10], c.ref, rtol=RTOL, atol=0)
    assert np.array_equal(got, _singles(like, mu))
    ref, kept = mf.marge_longdouble_rows(JLADataset(c.dataset), mu[:5], **c.options)
    assert kept == c.n_kept and jf.rel_distance(got[:5], ref) <= RTOL


def test_non_finite_row(cases):
    """One NaN modulus in walker 3 of 8: CMBL_LOGZERO there, no other walker's bits change."""
    from cosmomc_amd.supernovae import JLAMargeLikelihood
    c = cases["syn70_s2"]
    like = JLAMargeLikelihood(c.dataset, **c.options)
    mu = c.mu[np.arange(8) % 5].copy()
    clean = _eval(like, mu)
    mu[3, 41] = np.nan
    got = _eval(like, mu)
    assert got[3] == 1e30
    keep = np.arange(8) != 3
    assert np.array_equal(got[keep], clean[keep])


def test_host_entry(cases):
    from cosmomc_amd.supernovae import JLAMargeLikelihood
    c = cases["syn37_s7"]
    like = JLAMargeLikelihood(c.dataset)
    dev = _eval(like, c.mu)
    for i in range(5):
        h = like.loglike_host(c.mu[i][None, None, :])
        assert h.shape == (1,) and h[0] == dev[i]
