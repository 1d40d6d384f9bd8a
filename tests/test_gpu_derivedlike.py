"""Gaussian likelihoods on calculator-derived quantities (cmbg_*,
cosmomc_amd.derivedlike.DerivedGaussian) on the GPU: the kernel against a
numpy longdouble restatement built on cmbt_derived_eval's own bits, its
determinism, the box rule, a scaling invariance and the argument errors.
GPU only."""
import ctypes as C
import os

import numpy as np
import pytest

from cosmomc_amd import theory as th
from cosmomc_amd.derivedlike import DerivedGaussian
from test_gpu_theory_calc import CENTER, HI, LO, NPAR, PIDX, SCALE, _points, _surface

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
BAO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bao")
CALCS = [(3, 2), (3, 4)]                                # n_in, degree: K = 10 and K = 35
NS = [1, 6, 32]
MS = [1, 63, 64, 65, 257]
MMAX = max(MS)


def _invcov(n):
    if n == 1:
        return np.array([[2.5]])
    if n == 6:                                          # the DR12 consensus set's
        inv = np.linalg.inv(np.loadtxt(os.path.join(BAO, "DR12", "BAO_consensus_covtot_dM_Hz.txt")))
        return (inv + inv.T) / 2
    g = np.random.default_rng(5).normal(size=(n, n))
    a = g @ g.T / n + np.eye(n)
    return (a + a.T) / 2


class _Case:
    """One calculator per (n_in, degree) and one object per n on it: n surfaces
    dcoef, obs near the surfaces' values, the points P [NPAR, 320], and at
    them cmbt_derived_eval's v [n, 257] for the same columns."""

    def __init__(self, n_in, degree, n):
        self.ex = th.monomials(n_in, degree)
        self.n = n
        self.coef = _surface(n_in, self.ex, 2, 5, 20 + n)
        self.dcoef = np.ascontiguousarray(_surface(n_in, self.ex, 1, n - 1, 60 + n)[:, 0, :])
        self.P = _points(n_in, NPAR, PIDX, CENTER, SCALE, MMAX, 500 + n)
        self.invcov = _invcov(n)
        self.calc = th.PolynomialTheory(PIDX, CENTER, SCALE, LO, HI, self.ex, [0, 2], self.coef)
        self.calc.set_derived([f"d{i}" for i in range(n)], self.dcoef)
        self.v = self.calc.derived(torch.tensor(self.P, device="cuda")[:, :MMAX]).cpu().numpy()
        rng = np.random.default_rng(70 + n)
        self.obs = self.v[:, 3] + rng.normal(size=n) * np.std(self.v, axis=1)
        self.g = DerivedGaussian(self.calc, self.dcoef, self.obs, invcov=self.invcov)

    def restate(self, M, obs=None, invcov=None):
        """(ref [M], sum_ij |r_i| |invcov_ij| |r_j| / 2 [M]) in longdouble from v's bits"""
        ld_ = np.longdouble
        r = self.v[:, :M].astype(ld_) - (self.obs if obs is None else obs).astype(ld_)[:, None]
        ic = (self.invcov if invcov is None else invcov).astype(ld_)
        ref = np.einsum("im,ij,jm->m", r, ic, r) / 2
        mag = np.einsum("im,ij,jm->m", np.abs(r), np.abs(ic), np.abs(r)) / 2
        return ref, mag


@pytest.fixture(scope="module")
def cases():
    c = {}
    yield c
    for v in c.values():
        v.g.close()
        v.calc.close()


def _case(cases, calc, n):
    key = (*calc, n)
    if key not in cases:
        cases[key] = _Case(*key)
    return cases[key]


def _eval(g, P, M, ld=None, pad=3):
    """g.eval at P[:, :M] (row stride ld) into the [M] corner of NaN-filled
    (out) and -7-filled (fail) buffers: (out, fail, the whole buffers)"""
    Pd = torch.tensor(np.ascontiguousarray(P[:, :ld if ld else P.shape[1]]), device="cuda")[:, :M]
    full = torch.full((M + pad,), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((M + pad,), -7, dtype=torch.int32, device="cuda")
    ret = g.eval(Pd, out=full[:M], fail=fl[:M])
    assert ret.data_ptr() == full.data_ptr()
    return full[:M].cpu().numpy(), fl[:M].cpu().numpy(), full.cpu().numpy(), fl.cpu().numpy()


# ---------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("calc", CALCS)
def test_matches_restatement(cases, calc, n, M):
    """|got - ref| <= (2n + 4) 2^-52 sum_ij |r_i| |invcov_ij| |r_j| / 2, ref the
    longdouble quadratic form of cmbt_derived_eval's own v for the same
    columns: one rounding for each residual, two chains of n fma, the halving
    exact.  The output is the [M] corner of a NaN-filled buffer and nothing
    else is written."""
    c = _case(cases, calc, n)
    got, fl, full, flfull = _eval(c.g, c.P, M)
    assert np.array_equal(fl, np.zeros(M, dtype=np.int32))
    ref, mag = c.restate(M)
    bound = (2 * n + 4) * 2.0 ** -52 * mag
    err = np.abs(got.astype(np.longdouble) - ref)
    print(f"{calc} n={n} M={M}: max |got - ref| / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.all(got > 0) and np.all(np.isfinite(got))
    assert np.all(np.isnan(full[M:])) and np.all(flfull[M:] == -7), "an element outside [0, M) was written"


# ---------------------------------------------------------------- 2. determinism
def test_deterministic_across_batch_and_strides(cases):
    """A point alone (M = 1), in a batch of 65 (ld 128) and in one of 257
    (ld 320) gives the same bits; so do host points [M, num_params]."""
    c = _case(cases, (3, 4), 32)
    big = _eval(c.g, c.P, 257, pad=5)[0]
    mid = _eval(c.g, c.P, 65, ld=128)[0]
    assert np.array_equal(mid, big[:65])
    for w in (0, 31, 63, 64, 255, 256):
        alone = _eval(c.g, np.ascontiguousarray(c.P[:, w:w + 1]), 1, pad=0)[0]
        assert alone[0] == big[w], w
    host = c.g.eval(np.ascontiguousarray(c.P[:, :257].T))
    assert host.shape == (257,)
    assert np.array_equal(host.cpu().numpy(), big)


# ---------------------------------------------------------------- 3. the box
def test_box_gives_logzero(cases):
    """At lo and at hi, and nextafter inside them, passes (a finite term, fail
    0); nextafter outside, far outside and NaN give exactly 1e30 and fail 1."""
    c = _case(cases, (3, 2), 6)
    inside = CENTER + 0.5 * np.abs(SCALE)
    pts = [(inside.copy(), 0)]
    for i in range(3):
        for edge, out_dir in ((LO[i], -np.inf), (HI[i], np.inf)):
            at = inside.copy()
            at[i] = edge
            pts.append((at, 0))
            just_in = at.copy()
            just_in[i] = np.nextafter(edge, -out_dir)
            pts.append((just_in, 0))
            off = at.copy()
            off[i] = np.nextafter(edge, out_dir)
            pts.append((off, 1))
        nan = inside.copy()
        nan[i] = np.nan
        pts.append((nan, 1))
    pts.append((np.array([LO[0] - 1e6, HI[1] + 1e6, np.nan]), 1))
    M = len(pts)
    P = _points(3, NPAR, PIDX, CENTER, SCALE, M, 1)
    for m, (raw, _) in enumerate(pts):
        for i, p in enumerate(PIDX):
            P[p - 1, m] = raw[i]
    got, fl, _, _ = _eval(c.g, P, M)
    want = np.array([p[1] for p in pts], dtype=np.int32)
    assert np.array_equal(fl, want)
    assert np.all(got[want == 1] == LOGZERO)
    assert np.all(np.isfinite(got[want == 0])) and np.all(got[want == 0] < 1e29)
    nofail = c.g.eval(torch.tensor(P, device="cuda")[:, :M]).cpu().numpy()      # fail = None
    assert np.array_equal(nofail, got)


# ---------------------------------------------------------------- 4. scaling invariance
@pytest.mark.parametrize("n", [6, 32])
def test_scaling_invariance(cases, n):
    """The surface 0.5 x column with obs / 2 and 4 x invcov: every scaling is a
    power of two, so v / 2, r / 2, 2 y and s are exact images and the term has
    the same bits.  A wrong column, obs entry or invcov entry breaks this."""
    c = _case(cases, (3, 4), n)
    h = DerivedGaussian(c.calc, 0.5 * c.dcoef, c.obs / 2, invcov=4 * c.invcov)
    a = _eval(c.g, c.P, 257)[0]
    b = _eval(h, c.P, 257)[0]
    h.close()
    assert np.array_equal(a, b)
    # and the columns do matter: obs permuted changes the result
    p = DerivedGaussian(c.calc, c.dcoef, np.roll(c.obs, 1), invcov=c.invcov)
    assert np.all(_eval(p, c.P, 65)[0] != a[:65])
    p.close()


def test_cov_is_inverted_and_prior(cases):
    """cov= gives numpy's symmetrised inverse; prior() is n = 1 with 1 / std^2:
    (v - mean)^2 / std^2 / 2 to the restatement's bound."""
    c = _case(cases, (3, 2), 6)
    cov = np.linalg.inv(c.invcov)
    g = DerivedGaussian(c.calc, c.dcoef, c.obs, cov=cov)
    inv = np.linalg.inv(cov)
    assert np.array_equal(g.invcov, (inv + inv.T) / 2) and np.array_equal(g.invcov, g.invcov.T)
    g.close()
    p = DerivedGaussian.prior(c.calc, c.dcoef[:, 2], c.obs[2], 0.75)
    assert p.n == 1 and p.invcov[0, 0] == 1.0 / (0.75 * 0.75)
    got = _eval(p, c.P, 65)[0]
    p.close()
    r = c.v[2, :65].astype(np.longdouble) - np.longdouble(c.obs[2])
    ref = r * r * np.longdouble(1.0 / (0.75 * 0.75)) / 2
    assert np.all(np.abs(got - ref) <= 6 * 2.0 ** -52 * ref)


# ---------------------------------------------------------------- 5. argument errors
def test_argument_errors(cases):
    """Every argument error of cmbg_create and cmbg_eval is code -1, never an
    abort, and the handle stays usable."""
    from cosmomc_amd import _native as N
    c = _case(cases, (3, 2), 6)
    K = len(c.ex)

    def bad(call):
        with pytest.raises(N.NativeError) as e:
            call()
        assert e.value.code == -1, e.value

    bad(lambda: DerivedGaussian(c.calc, np.zeros((K, 0)), [], invcov=np.zeros((0, 0))))       # n = 0
    bad(lambda: DerivedGaussian(c.calc, np.zeros((K, 33)), np.zeros(33), invcov=np.eye(33)))   # n = 33
    dp = C.POINTER(C.c_double)
    for null in ("coef", "obs", "invcov"):                                                    # a NULL table
        cfg = N.CmbgConfig()
        cfg.n = 6
        for name, a in (("coef", c.dcoef), ("obs", c.obs), ("invcov", c.invcov)):
            if name != null:
                setattr(cfg, name, np.ascontiguousarray(a).ctypes.data_as(dp))
        h, err = C.c_void_p(), C.create_string_buffer(256)
        assert N.lib().cmbg_create(c.calc.handle, C.byref(cfg), C.byref(h), err, 256) == -1, null
        assert not h.value and err.value
    obs = c.obs.copy()
    obs[4] = np.inf
    bad(lambda: DerivedGaussian(c.calc, c.dcoef, obs, invcov=c.invcov))                        # non-finite obs
    ic = c.invcov.copy()
    ic[2, 2] = np.nan
    bad(lambda: DerivedGaussian(c.calc, c.dcoef, c.obs, invcov=ic))                            # non-finite invcov
    ic = c.invcov.copy()
    ic[1, 4] = np.nextafter(ic[1, 4], np.inf)
    bad(lambda: DerivedGaussian(c.calc, c.dcoef, c.obs, invcov=ic))                            # not symmetric

    M = 8
    P = torch.tensor(c.P[:, :64], device="cuda")
    out = torch.zeros(64, dtype=torch.float64, device="cuda")

    def raw(M=M, ld=64, num_params=NPAR):
        N.check(N.lib().cmbg_eval(c.g.handle, M, P.data_ptr(), ld, num_params, out.data_ptr(), None,
                                  N.current_stream_ptr()), c.g.handle, "cmbg")

    bad(lambda: raw(ld=M - 1))                                                                 # ld < M
    bad(lambda: raw(num_params=3))                                                             # param_index 4 outside 1..3
    bad(lambda: c.g.eval(P[:3, :M]))
    bad(lambda: raw(M=0))
    raw()                                                                                      # and the handle still works
    torch.cuda.synchronize()
    ref, mag = c.restate(M)
    assert np.all(np.abs(out.cpu().numpy()[:M] - ref) <= 16 * 2.0 ** -52 * mag)
