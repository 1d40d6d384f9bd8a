"""Every path of jla_chol_kernel and its launcher against a long-double
restatement (jla_fixture.jla_loglike_longdouble): a non-positive pivot in a
chosen row, block columns of more than four slabs, each component matrix alone,
the diagonal-errors loops' second trip, batches beyond one launch's walkers,
theory strides, an ill-conditioned V, and matrix files whose triangles differ.
test_supernovae.py checks the input conditions of the datasets without a GPU."""

import numpy as np
import pytest

import jla_fixture as jf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-10      # as test_gpu_jla.py; measured on MI355X: 3e-15 at most of long double where V is well
                  # conditioned, 2.9e-12 at cond(V) = 4e6 (test_ill_conditioned); each figure is beside its test
ARG = -1          # CMBL_ERR_ARG


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return jf.extract(tmp_path_factory.mktemp("jla"))


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), device="cuda")


def _eval(like, mu, ab, workspace=None):
    return like.loglike_batch(_dev(np.asarray(mu)[:, None, :]), _dev(ab), workspace=workspace).cpu().numpy()


def _singles(like, mu, ab):
    return np.array([_eval(like, mu[i:i + 1], ab[i:i + 1])[0] for i in range(len(ab))])


def _against_longdouble(name):
    """The kernel on every case of an edge dataset, none of them LOGZERO in the reference."""
    from cosmomc_amd.supernovae import JLALikelihood, jla_loglike_host
    e = jf.edge(name)
    assert np.all(e.bad == -1) and np.all(e.ref < 1e29)
    got = _eval(JLALikelihood(e.dataset), e.mu, e.ab)
    host = np.array([jla_loglike_host(e.D, a, b, m) for (a, b), m in zip(e.ab, e.mu)])
    print(name, got, "kernel %.2e restatement %.2e of long double" % (jf.rel_distance(got, e.ref),
                                                                     jf.rel_distance(host, e.ref)))
    assert jf.rel_distance(got, e.ref) < RTOL
    return got


# ---- 1. the failure path

SLOTS = np.array([0, 1, 2, 0, 2, 1, 0, 1, 2])      # case 0 is not positive definite: bad, good, good, bad, ...
GOOD = np.array([1, 1, 2, 2, 2, 1, 1, 1, 2])


@pytest.mark.parametrize("nsn,p", jf.PIVOT)
def test_bad_pivot_at_row(nsn, p):
    """The first non-positive pivot is row p of block column p / 16: those
    walkers are CMBL_LOGZERO exactly, their batch neighbours keep the bits they
    have alone, and the same workspace then serves nine good walkers."""
    from cosmomc_amd.supernovae import JLALikelihood
    e = jf.edge("pivot_%d_%d" % (nsn, p))
    assert list(e.bad) == [p, -1, -1]
    like = JLALikelihood(e.dataset)
    single = _singles(like, e.mu, e.ab)
    print(nsn, p, single, jf.rel_distance(single[1:], e.ref[1:]))
    assert single[0] == jf.LOGZERO
    assert jf.rel_distance(single[1:], e.ref[1:]) < RTOL          # measured: <= 7.8e-16
    ws = torch.zeros(like.workspace_bytes(len(SLOTS)), dtype=torch.uint8, device="cuda")
    got = _eval(like, e.mu[SLOTS], e.ab[SLOTS], workspace=ws)
    assert np.all(got[SLOTS == 0] == jf.LOGZERO)
    assert np.array_equal(got, single[SLOTS])
    again = _eval(like, e.mu[GOOD], e.ab[GOOD], workspace=ws)
    assert np.array_equal(again, single[GOOD])


def test_nan_alpha_is_a_bad_pivot():
    """A NaN alpha makes every pivot NaN, which DPOTRF's disnan test counts as
    not positive: CMBL_LOGZERO.  With one scriptm nothing after the pivot test
    (the two-scriptm fit's tempG > 0) would turn the NaN into LOGZERO."""
    from cosmomc_amd.supernovae import JLALikelihood
    e = jf.edge("slabs_230_0")
    assert not e.D.twoscriptmfit and not e.D.diag_errors
    like = JLALikelihood(e.dataset)
    single = _singles(like, e.mu, e.ab)
    ws = torch.zeros(like.workspace_bytes(len(SLOTS)), dtype=torch.uint8, device="cuda")
    others = np.arange(len(SLOTS)) != 4
    ab = e.ab[SLOTS].copy()
    ab[4, 0] = np.nan
    assert jf.jla_loglike_longdouble(e.D, ab[4, 0], ab[4, 1], e.mu[SLOTS[4]]) == (jf.LOGZERO, 0)
    got = _eval(like, e.mu[SLOTS], ab, workspace=ws)
    assert got[4] == jf.LOGZERO and np.array_equal(got[others], single[SLOTS][others])
    assert np.array_equal(_eval(like, e.mu[SLOTS], e.ab[SLOTS], workspace=ws), single[SLOTS])


def test_nan_mu_is_nan():
    """A NaN in mu leaves V alone: that walker is NaN, not LOGZERO, and its neighbours keep their bits."""
    from cosmomc_amd.supernovae import JLALikelihood
    e = jf.edge("pivot_230_100")
    like = JLALikelihood(e.dataset)
    single = _singles(like, e.mu, e.ab)
    ws = torch.zeros(like.workspace_bytes(len(SLOTS)), dtype=torch.uint8, device="cuda")
    others = np.arange(len(SLOTS)) != 4
    mu = e.mu[GOOD].copy()
    mu[4, 117] = np.nan
    assert np.isnan(float(jf.jla_loglike_longdouble(e.D, *e.ab[GOOD[4]], mu[4])[0]))
    got = _eval(like, mu, e.ab[GOOD], workspace=ws)
    assert np.isnan(got[4]) and np.array_equal(got[others], single[GOOD][others])
    assert np.array_equal(_eval(like, e.mu[GOOD], e.ab[GOOD], workspace=ws), single[GOOD])


# ---- 2. more than four slabs a block column, all six components, a last tile of one real row

@pytest.mark.parametrize("two", [0, 1], ids=["one_scriptm", "two_scriptm"])
@pytest.mark.parametrize("nsn", jf.SLAB_NSN)
def test_many_slabs(nsn, two):
    _against_longdouble("slabs_%d_%d" % (nsn, two))     # measured: <= 1.1e-15 (the restatement: 1.5e-15)


# ---- 3. each component matrix alone, and V without mag

@pytest.fixture(scope="module")
def subset_result():
    memo = {}

    def get(key):
        if key not in memo:
            memo[key] = _against_longdouble("subset_" + key)
        return memo[key]
    return get


@pytest.mark.parametrize("key", list(jf.SUBSETS))
def test_component_subsets(subset_result, key):
    subset_result(key)                                  # measured: <= 3.0e-15 (the restatement: 3.2e-15)


def test_subsets_without_mag_share_the_zero_case(subset_result):
    """alpha = beta = 0: every component but mag has the coefficient 0, so these datasets give the same bits."""
    keys = [k for k in jf.SUBSETS if k != "mag"]
    assert len(keys) == 6 and all(subset_result(k)[1] == subset_result(keys[0])[1] for k in keys)
    assert subset_result("mag")[1] != subset_result(keys[0])[1]


# ---- 4. diagonal errors, a second trip of the workgroup's loops

@pytest.mark.parametrize("two", [0, 1], ids=["one_scriptm", "two_scriptm"])
def test_diagonal_errors_300(two):
    _against_longdouble("diag300_%d" % two)             # measured: <= 8.4e-16 (the restatement: 9.5e-16)


# ---- 5. batches beyond one launch's 1024 walkers

def test_chunks(goldens):
    """W = 1100 is two launches.  syn5_indef's five cases (one LOGZERO) in a
    seeded order, ld_walker = 8, ld_nuis = 3 with NaN wherever nothing may be
    read; the sparse entry for live counts around the chunk edge; a workspace of
    exactly workspace_bytes(W) with a guard behind it."""
    from cosmomc_amd.supernovae import JLALikelihood
    g = goldens["syn5_indef"]
    like = JLALikelihood(g.dataset)
    single = _singles(like, g.mu, g.ab)
    assert np.array_equal(single == jf.LOGZERO, g.ref == jf.LOGZERO) and (single == jf.LOGZERO).sum() == 1
    W = 1100
    case = np.random.RandomState(1100).permutation(W) % 5
    zero = single[case] == jf.LOGZERO
    assert zero[:1024].any() and zero[1024:].any()
    dl = torch.full((W, 1, 8), float("nan"), dtype=torch.float64, device="cuda")
    dl[:, 0, :5] = _dev(g.mu[case])
    nuis = torch.full((W, 3), float("nan"), dtype=torch.float64, device="cuda")
    nuis[:, :2] = _dev(g.ab[case])
    assert dl.stride(0) == 8 and nuis[:, :2].stride(0) == 3
    out = torch.full((W,), -2.0, dtype=torch.float64, device="cuda")
    big = like.loglike_batch(dl, nuis[:, :2], out=out).cpu().numpy()
    assert np.array_equal(big, single[case])

    def sparse(count, workspace=None):
        out = torch.full((W,), -1.0, dtype=torch.float64, device="cuda")
        like.loglike_batch_sparse(dl, nuis[:, :2], out, torch.tensor([count], dtype=torch.int32, device="cuda"),
                                  workspace=workspace)
        sp = out.cpu().numpy()
        assert np.array_equal(sp[:count], single[case[:count]]), count
        assert np.all(sp[count:] == -1.0), count
    for count in (0, 1, 1023, 1024, 1025, 1100):
        sparse(count)
    nb = like.workspace_bytes(W)
    assert nb == 1024 * like.workspace_bytes(1)
    buf = torch.zeros(nb + 4096, dtype=torch.uint8, device="cuda")
    buf[nb:] = 0xA5
    sparse(1025, workspace=buf)
    assert bool((buf[nb:] == 0xA5).all())


# ---- 6. strides of the theory rows

def test_strides_and_refusals(goldens):
    from cosmomc_amd import _native as N
    from cosmomc_amd.supernovae import JLALikelihood
    g = goldens["syn37"]
    like = JLALikelihood(g.dataset)
    W = 67
    case = np.random.RandomState(67).permutation(W) % 5
    ab = _dev(g.ab[case])
    # one theory row for every walker (ld_walker = 0)
    row = _dev(g.mu[0][None, None, :])
    dl = row.expand(W, 1, 37)
    assert dl.stride(0) == 0
    one_row = like.loglike_batch(dl, ab).cpu().numpy()
    assert np.array_equal(one_row, like.loglike_batch(dl.contiguous(), ab).cpu().numpy())
    assert np.array_equal(one_row[:5], _singles(like, g.mu[[0] * 5], g.ab[case[:5]]))
    # three fields of 96: field 0 is read, and no further than nsn
    want = _eval(like, g.mu[case], g.ab[case])
    dl3 = torch.full((W, 3, 96), float("nan"), dtype=torch.float64, device="cuda")
    dl3[:, 0, :37] = _dev(g.mu[case])
    assert np.array_equal(like.loglike_batch(dl3, ab).cpu().numpy(), want)
    # refusals, before anything is launched
    dl1 = _dev(g.mu[case][:, None, :])
    with pytest.raises(N.NativeError, match="ld_nuis") as ei:
        like.loglike_batch(dl1, ab[:, :1].contiguous())
    assert ei.value.code == ARG
    base = torch.zeros(W * 36 + 37, dtype=torch.float64, device="cuda")
    dl36 = base.as_strided((W, 1, 37), (36, 37, 1))
    with pytest.raises(N.NativeError, match="ld_walker") as ei:
        like.loglike_batch(dl36, ab)
    assert ei.value.code == ARG
    assert np.array_equal(like.loglike_batch(dl1, ab).cpu().numpy(), want)
    assert np.array_equal(want, _singles(like, g.mu, g.ab)[case])


# ---- 7. an ill-conditioned V: Y = L^-1 R where the reference forms V^-1 by DPOTRI

def test_ill_conditioned():
    """cond(V) ~ 4e6 and -lnL ~ 3e6: the float64 restatement sits within 1e-11
    of long double (test_supernovae.py); the kernel is held to RTOL."""
    _against_longdouble("illcond")                       # measured: 2.9e-12 (the restatement: 1.4e-12)


# ---- 8. the upper triangle is the one read

def test_upper_triangle_golden(tmp_path):
    """Matrix files whose lower triangles are noise, one written a number a line, against the compiled reference."""
    from cosmomc_amd.supernovae import JLALikelihood
    g = jf.extract(tmp_path, jf.GOLDEN_UPPER, jf.NAMES_UPPER)["syn21_upper"]
    got = _eval(JLALikelihood(g.dataset), g.mu, g.ab)
    print(got, np.abs(got / g.ref - 1).max())
    assert np.all(g.ref < 1e29)
    np.testing.assert_allclose(got, g.ref, rtol=RTOL, atol=0)
