"""JLA supernova likelihood on the GPU (jla_chol_kernel): the compiled
reference's goldens, tile edges and the full 740-supernova size against the
numpy restatement, bit independence of a walker's result from the batch, and
the host entry."""

import numpy as np
import pytest

import jla_fixture as jf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-10      # the project's plik_lite golden tolerance; the restatement sits at 1e-15 of the reference


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return jf.extract(tmp_path_factory.mktemp("jla"))


def _eval(like, mu, ab):
    dl = torch.tensor(np.ascontiguousarray(mu)[:, None, :], device="cuda")
    return like.loglike_batch(dl, torch.tensor(np.ascontiguousarray(ab), device="cuda")).cpu().numpy()


@pytest.mark.parametrize("name", jf.NAMES)
def test_goldens(goldens, name):
    from cosmomc_amd.supernovae import JLALikelihood
    g = goldens[name]
    like = JLALikelihood(g.dataset)
    assert like.n_theory == g.mu.shape[1]
    got = _eval(like, g.mu, g.ab)
    zero = g.ref == jf.LOGZERO
    print(name, got, np.abs(got[~zero] / g.ref[~zero] - 1).max())
    assert np.array_equal(got[zero], g.ref[zero])          # == CMBL_LOGZERO, its batch neighbours below
    np.testing.assert_allclose(got[~zero], g.ref[~zero], rtol=RTOL, atol=0)
    if name == "syn5_indef":
        assert zero.sum() == 1


@pytest.mark.parametrize("two", [False, True], ids=["one_scriptm", "two_scriptm"])
@pytest.mark.parametrize("nsn", [1, 2, 16, 17, 33, 64, 65])
def test_tile_edges(tmp_path, nsn, two):
    from cosmomc_amd.supernovae import JLADataset, JLALikelihood, jla_loglike_host
    ds, mu, ab = jf.make_synthetic(str(tmp_path), nsn, jf.COMPONENTS, two, 1000 + nsn)
    D = JLADataset(ds)
    assert D.twoscriptmfit == (two and nsn > 1)
    ref = np.array([jla_loglike_host(D, a, b, m) for (a, b), m in zip(ab, mu)])
    got = _eval(JLALikelihood(ds), mu, ab)
    print(nsn, two, np.abs(got / ref - 1).max())
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


def test_full_size(tmp_path):
    """nsn = 740 as the JLA sample: any buffer sized by nsn."""
    from cosmomc_amd.supernovae import JLADataset, JLALikelihood, jla_loglike_host
    ds, mu, ab = jf.make_synthetic(str(tmp_path), 740, ("mag", "stretch"), True, 740, fmt="%.9g")
    D = JLADataset(ds)
    ref = np.array([jla_loglike_host(D, a, b, m) for (a, b), m in zip(ab[:2], mu[:2])])
    like = JLALikelihood(ds)
    assert like.workspace_bytes(5000) == like.workspace_bytes(1024) == 1024 * like.workspace_bytes(1)
    got = _eval(like, mu[:2], ab[:2])
    print(got, np.abs(got / ref - 1).max())
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)


def test_bits_independent_of_batch(goldens):
    """The 5 cases of syn70 one at a time, at W = 67 in permuted order with
    ld_walker > nsn, and through the sparse entry with 5 live of 67 slots."""
    from cosmomc_amd.supernovae import JLALikelihood
    g = goldens["syn70"]
    like = JLALikelihood(g.dataset)
    single = np.array([_eval(like, g.mu[i:i + 1], g.ab[i:i + 1])[0] for i in range(5)])
    W, ldw = 67, 96
    perm = np.random.RandomState(5).permutation(W)
    case = perm % 5
    dl = torch.zeros((W, 1, ldw), dtype=torch.float64, device="cuda")
    dl[:, 0, :70] = torch.tensor(g.mu[case], device="cuda")
    nuis = torch.full((W, 3), 7.0, dtype=torch.float64, device="cuda")
    nuis[:, :2] = torch.tensor(g.ab[case], device="cuda")
    big = like.loglike_batch(dl, nuis[:, :2]).cpu().numpy()
    assert np.array_equal(big, single[case])
    # the sparse entry: live slots [0, 5), the rest never read or written
    out = torch.full((W,), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.tensor([5], dtype=torch.int32, device="cuda")
    like.loglike_batch_sparse(dl, nuis[:, :2], out, cnt)
    sp = out.cpu().numpy()
    assert np.array_equal(sp[:5], single[case[:5]])
    assert np.all(sp[5:] == -1.0)


def test_host_entry(goldens):
    from cosmomc_amd.supernovae import JLALikelihood
    g = goldens["syn37"]
    like = JLALikelihood(g.dataset)
    dev = _eval(like, g.mu, g.ab)
    for i in range(5):
        h = like.loglike_host(g.mu[i][None, None, :], g.ab[i][None, :])
        assert h.shape == (1,) and h[0] == dev[i]
