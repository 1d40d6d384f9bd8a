"""Calculator-derived parameters (cmbt_set_derived / cmbt_derived_eval,
PolynomialTheory.set_derived / derived, chains.TheoryDerived) on the GPU:
the evaluation against the numpy longdouble restatement of
test_gpu_theory_calc, its bit identity with cmbt_eval's D_l, the failure
flags of box and hard ranges, the sampler's rejection of a trial that leaves
a range, and the derived columns of a chain.  GPU only."""
import ctypes as C

import numpy as np
import pytest

from cosmomc_amd import theory as th
from test_gpu_theory_calc import (CENTER, DRAG_COV, DRAG_SEEDS, DRAG_STEPS, DRAG_T, DRAG_W, FIELDS, FULL_COV,
                                  FULL_SEEDS, FULL_STEPS, FULL_W, HI, LMAX, LO, NPAR, PIDX, SCALE, TIGHT_A, WIDE,
                                  _assert_same, _eval, _points, _restate, _Run, _surface)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = [(3, 2, 1), (3, 2, 5), (3, 4, 32)]               # n_in, degree, n_derived; the last: K = 35, 5 chunks of 8 terms
MS = [1, 63, 64, 65, 257]
MMAX = max(MS)


class _Case:
    """One calculator per (n_in, degree, n_derived) with a small D_l table of
    its own, its points P [NPAR, 320] and their restatement, computed once."""

    def __init__(self, n_in, degree, nd):
        self.ex = th.monomials(n_in, degree)
        self.K, self.nd = len(self.ex), nd
        self.coef = _surface(n_in, self.ex, 2, 5, 20 + nd)
        self.dcoef = np.ascontiguousarray(_surface(n_in, self.ex, 1, nd - 1, 40 + nd)[:, 0, :])
        self.P = _points(n_in, NPAR, PIDX, CENTER, SCALE, MMAX, 300 + nd)
        self.val, self.mag = self.restate(self.P, MMAX)[:2]

    def calc(self, lo=None, hi=None):
        c = th.PolynomialTheory(PIDX, CENTER, SCALE, LO, HI, self.ex, [0, 2], self.coef)
        c.set_derived([f"d{i}" for i in range(self.nd)], self.dcoef, lo, hi)
        return c

    def restate(self, P, M):
        """(values [M, nd], sum_k |basis_k coef_k| [M, nd], box failure [M])"""
        val, mag, bad = _restate(P, M, PIDX, CENTER, SCALE, LO, HI, self.ex, self.dcoef[:, None, :])
        return val[:, 0, :], mag[:, 0, :], bad

    def bound(self, mag):
        return (self.K + 2 * 4 + 4) * 2.0 ** -52 * mag


@pytest.fixture(scope="module")
def cases():
    return {c: _Case(*c) for c in CASES}


def _derived(calc, P, M, nd, pad=(2, 3), ld=None):
    """calc.derived at P[:, :M] (row stride ld) into the [nd, M] corner of a
    NaN-filled buffer [nd + pad[0], M + pad[1]]: (out, fail, the whole buffer)"""
    Pd = torch.tensor(np.ascontiguousarray(P[:, :ld if ld else P.shape[1]]), device="cuda")[:, :M]
    full = torch.full((nd + pad[0], M + pad[1]), float("nan"), dtype=torch.float64, device="cuda")
    out = full[:nd, :M]
    fl = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    ret = calc.derived(Pd, out=out, fail=fl)
    assert ret is out
    return out.cpu().numpy(), fl.cpu().numpy(), full.cpu().numpy()


# ---------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("case", CASES)
def test_derived_matches_restatement(cases, case, M):
    """|got - ref| <= (K + 2 x 4 + 4) 2^-52 sum_k |basis_k coef_k| against the
    longdouble restatement (the bound of test_eval_matches_restatement); the
    output is the [n_derived, M] corner of a NaN-filled buffer with ld_out =
    M + 3 and two more rows, and nothing outside the corner is written."""
    c = cases[case]
    calc = c.calc()
    got, fl, full = _derived(calc, c.P, M, c.nd)
    calc.close()
    assert np.array_equal(fl, np.zeros(M, dtype=np.int32))
    err = np.abs(got.T.astype(np.longdouble) - c.val[:M])
    bound = c.bound(c.mag[:M])
    print(f"{case} M={M}: max |got - ref| / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    assert not np.any(np.isnan(got))
    assert np.all(np.isnan(full[c.nd:, :])) and np.all(np.isnan(full[:, M:])), "an element outside [n_derived, M] was written"


# ---------------------------------------------------------------- 2. bit identity with D_l
def test_dl_columns_give_cmbt_evals_bits():
    """Derived outputs whose coefficients are D_l coefficient columns (l = 0,
    1, 36 and lmax of the first and the third field) are cmbt_eval's D_l at
    those (field, l), bit for bit, for M = 65 (K = 10: six zero-padded terms)."""
    ex = th.monomials(3, 2)
    coef = _surface(3, ex, len(FIELDS), LMAX, 11)
    calc = th.PolynomialTheory(PIDX, CENTER, SCALE, LO, HI, ex, FIELDS, coef)
    pos, ells = [0] * 4 + [2] * 4, [0, 1, 36, LMAX] * 2
    calc.set_derived([f"DL{l}_{p}" for p, l in zip(pos, ells)], th.dl_columns(coef, pos, ells))
    M = 65
    P = _points(3, NPAR, PIDX, CENTER, SCALE, M, 9)
    dl, _, _ = _eval(calc, P, M)
    got, fl, _ = _derived(calc, P, M, 8)
    calc.close()
    assert not fl.any()
    for d, (p, l) in enumerate(zip(pos, ells)):
        assert np.array_equal(got[d], dl[:, FIELDS[p], l]), (p, l)
    assert np.any(got != 0.0)


# ---------------------------------------------------------------- 3. determinism
def test_derived_deterministic_across_batch_and_strides(cases):
    """A point's outputs alone (M = 1), in a batch of 65 (ld 128, ld_out 68)
    and in one of 257 (ld 320, ld_out 262, other padding rows) are the same
    bits; so are those of host points [M, num_params]."""
    c = cases[(3, 4, 32)]
    calc = c.calc()
    big, _, _ = _derived(calc, c.P, 257, c.nd, pad=(0, 5))
    mid, _, _ = _derived(calc, c.P, 65, c.nd, pad=(2, 3), ld=128)
    assert np.array_equal(mid, big[:, :65])
    for w in (0, 31, 63, 64, 255, 256):
        alone, _, _ = _derived(calc, np.ascontiguousarray(c.P[:, w:w + 1]), 1, c.nd, pad=(1, 0))
        assert np.array_equal(alone[:, 0], big[:, w]), w
    host = calc.derived(np.ascontiguousarray(c.P[:, :257].T))
    assert host.shape == (c.nd, 257)
    assert np.array_equal(host.cpu().numpy(), big)
    calc.close()


# ---------------------------------------------------------------- 4. flags
def test_box_flags_as_cmbt_eval(cases):
    """test_validity_box's cases with no range set: at lo and at hi passes,
    nextafter outside and NaN fail, and a failed point's outputs are those of
    its clamped inputs (NaN: the centre)."""
    c = cases[(3, 2, 5)]
    calc = c.calc()
    inside = CENTER + 0.5 * np.abs(SCALE)
    pts = []                                            # (inputs, fails, clamped inputs)
    for i in range(3):
        for edge, out_dir in ((LO[i], -np.inf), (HI[i], np.inf)):
            at = inside.copy()
            at[i] = edge
            pts.append((at, 0, at))
            off = at.copy()
            off[i] = np.nextafter(edge, out_dir)
            pts.append((off, 1, at))
        nan = inside.copy()
        nan[i] = np.nan
        cl = inside.copy()
        cl[i] = CENTER[i]
        pts.append((nan, 1, cl))
    pts.append((np.array([LO[0] - 1e6, HI[1] + 1e6, np.nan]), 1, np.array([LO[0], HI[1], CENTER[2]])))
    M = len(pts)
    P = _points(3, NPAR, PIDX, CENTER, SCALE, M, 1)
    Pc = P.copy()
    for m, (raw, _, cl) in enumerate(pts):
        for i, p in enumerate(PIDX):
            P[p - 1, m], Pc[p - 1, m] = raw[i], cl[i]
    got, fl, _ = _derived(calc, P, M, c.nd)
    ref, flc, _ = _derived(calc, Pc, M, c.nd)
    calc.close()
    assert fl.tolist() == [p[1] for p in pts]
    assert not flc.any()
    assert np.array_equal(got, ref)
    assert np.array_equal(fl, c.restate(P, M)[2])


def _limits(val, bound):
    """lo, hi [nd] from restated values [M, nd]: output d has a lower limit
    only (d % 4 == 0), an upper only (1), both (2) or none (3), each at the
    midpoint of two adjacent sorted values a few places in from the end whose
    gap is asserted >= 1e3 x the evaluation bound of either, so the GPU's
    rounding cannot move a value across a limit."""
    M, nd = val.shape
    lo, hi = np.full(nd, -np.inf), np.full(nd, np.inf)
    for d in range(nd):
        order = np.argsort(val[:, d])
        s, b = val[order, d], bound[order, d]

        def mid(j0):
            j = max(range(j0, j0 + 3), key=lambda j: s[j + 1] - s[j])
            assert s[j + 1] - s[j] >= 1e3 * max(b[j], b[j + 1]), (d, j, float(s[j + 1] - s[j]))
            return float((s[j] + s[j + 1]) / 2)
        if d % 4 in (0, 2):
            lo[d] = mid(1)
        if d % 4 in (1, 2):
            hi[d] = mid(M - 5)
    return lo, hi


def _range_fail(val, lo, hi):
    return np.any(~((val >= lo) & (val <= hi)), axis=1).astype(np.int32)


@pytest.mark.parametrize("case", CASES)
def test_range_flags(cases, case):
    """M = 65 points inside the box: fail is exactly the range test of the
    restated values (limits by _limits), with flagged and unflagged points in
    every case, and the outputs do not depend on the limits."""
    c = cases[case]
    M = 65
    lo, hi = _limits(c.val[:M], c.bound(c.mag[:M]))
    want = _range_fail(c.val[:M], lo, hi)
    assert 0 < want.sum() < M, want.sum()
    plain = c.calc()
    ranged = c.calc(lo, hi)
    got0, fl0, _ = _derived(plain, c.P, M, c.nd)
    got, fl, _ = _derived(ranged, c.P, M, c.nd)
    plain.close()
    ranged.close()
    assert not fl0.any()
    assert np.array_equal(fl, want)
    assert np.array_equal(got, got0)


def test_range_equality_passes_and_nan_fails(cases):
    """lo = hi = a value the GPU returned for point 7: point 7 passes (and
    points with another value fail).  A coefficient of +inf on the monomial
    x_0 gives NaN (0 x inf) at a point with x_0 = 0 and +-inf elsewhere:
    against infinite limits only the NaN fails; with no range set nothing is
    flagged."""
    c = cases[(3, 2, 5)]
    M = 65
    calc = c.calc()
    got, _, _ = _derived(calc, c.P, M, c.nd)
    lo, hi = np.full(c.nd, -np.inf), np.full(c.nd, np.inf)
    lo[3] = hi[3] = got[3, 7]
    calc.set_derived([f"d{i}" for i in range(c.nd)], c.dcoef, lo, hi)
    _, fl, _ = _derived(calc, c.P, M, c.nd)
    assert fl[7] == 0
    assert np.array_equal(fl, (got[3] != got[3, 7]).astype(np.int32)) and fl.sum() >= M - 2

    k = [tuple(r) for r in c.ex.tolist()].index((1, 0, 0))
    dc = c.dcoef.copy()
    dc[k, 2] = np.inf
    P = c.P.copy()
    P[PIDX[0] - 1, 11] = CENTER[0]
    names = [f"d{i}" for i in range(c.nd)]
    calc.set_derived(names, dc, np.full(c.nd, -np.inf), np.full(c.nd, np.inf))
    v, fl, _ = _derived(calc, P, M, c.nd)
    want = np.zeros(M, dtype=np.int32)
    want[11] = 1
    assert np.isnan(v[2, 11]) and np.all(np.isinf(np.delete(v[2], 11)))
    assert np.array_equal(fl, want)
    calc.set_derived(names, dc)                          # no range: the box alone
    _, fl, _ = _derived(calc, P, M, c.nd)
    assert not fl.any()
    calc.close()


# ---------------------------------------------------------------- 5. cmbt_eval with ranges
def test_cmbt_eval_flags_include_ranges(cases):
    """cmbt_eval of a calculator with ranges: its D_l is that of a twin
    without derived outputs in every bit, and fail is box-or-range (M = 65,
    five points moved outside the box, whose range test is on the outputs at
    the clamped inputs).  A twin with derived outputs but no range flags the
    box alone."""
    c = cases[(3, 2, 5)]
    M = 65
    P = c.P.copy()
    for m, (i, x) in zip((3, 20, 40, 63, 64), ((0, HI[0] + 1.0), (1, LO[1] - 2.0), (2, np.nan), (0, np.nan),
                                                  (2, np.nextafter(HI[2], np.inf)))):
        P[PIDX[i] - 1, m] = x
    val, mag, box = c.restate(P, M)
    assert box.sum() == 5
    lo, hi = _limits(val, c.bound(mag))
    rng = _range_fail(val, lo, hi)
    want = box | rng
    assert np.any(box & ~rng) and np.any(rng & ~box) and np.any(want == 0)
    twin = th.PolynomialTheory(PIDX, CENTER, SCALE, LO, HI, c.ex, [0, 2], c.coef)
    unranged, ranged = c.calc(), c.calc(lo, hi)
    dl0, fl0, _ = _eval(twin, P, M, shape=(3, 9))
    dl1, fl1, _ = _eval(unranged, P, M, shape=(3, 9))
    dl2, fl2, full = _eval(ranged, P, M, shape=(3, 9), pad=(1, 2))
    _, fld, _ = _derived(ranged, P, M, c.nd)
    for calc in (twin, unranged, ranged):
        calc.close()
    assert np.array_equal(fl0, box) and np.array_equal(fl1, box)
    assert np.array_equal(fl2, want) and np.array_equal(fld, want)
    for dl in (dl1, dl2):
        assert np.array_equal(dl[:, [0, 2], :6], dl0[:, [0, 2], :6])
    assert np.all(np.isnan(dl2[:, 1, :])) and np.all(np.isnan(dl2[:, :, 6:])) and np.all(np.isnan(full[:, 3:, :]))


# ---------------------------------------------------------------- 6. the sampler
def _cut_on_a(r):
    """One derived output equal to A (coefficient 1 on the only monomial, A
    itself: fma(A, 1, +0) = A) with the hard range TIGHT_A."""
    r.calc.set_derived(["A"], [[1.0]], lo=[TIGHT_A[0]], hi=[TIGHT_A[1]])


def _runs(tmp_path, W, oversample, T, seeds, cov, n_calls, step):
    """Run (a): the calculator's box is TIGHT_A.  Run (b): box WIDE and the
    derived cut.  Both have the sampler's own A bounds at WIDE, centre 0 and
    scale 1, so the theory bits agree.  Outputs after every call."""
    outs = []
    for tag, box, cut in (("a", TIGHT_A, False), ("b", WIDE, True)):
        r = _Run(tmp_path, tag, W, "native", WIDE, box, oversample, T, seeds, cov, n_calls)
        if cut:
            _cut_on_a(r)
        r.start()
        o = []
        for _ in range(n_calls):
            step(r.s)
            o.append(r.outputs())
        r.close()
        outs.append(o)
    return outs


@pytest.mark.parametrize("oversample", [1, 3])
def test_range_cut_equals_box_cut_in_full_steps(tmp_path, oversample):
    """test_calculator_failure_equals_out_of_bounds' run B (which that test
    pins to the callback run with A's bounds at TIGHT_A, at least 5 of every
    walker's 40 trials having only A outside) against the same run with a wide
    box and the range TIGHT_A on a derived output equal to A: state and
    history are the same bits after every step."""
    a, b = _runs(tmp_path, FULL_W, oversample, 2.5, FULL_SEEDS, FULL_COV, FULL_STEPS, lambda s: s.step_theory(1))
    for k, (x, y) in enumerate(zip(a, b)):
        _assert_same(x, y, f"step {k}")
    assert np.any(a[-1][2][:, 0] != 1.0), "no slow move was accepted"
    hist_a = b[-1][0][:, 0, :]
    assert hist_a.min() >= TIGHT_A[0] and hist_a.max() <= TIGHT_A[1]


def test_range_cut_equals_box_cut_in_drags(tmp_path):
    """The same comparison for test_dragging_native_equals_callback's run c
    (W = 130, 24 step_drag(1) calls, oversample_fast 2, Temperature 2)."""
    a, b = _runs(tmp_path, DRAG_W, 2, DRAG_T, DRAG_SEEDS, DRAG_COV, DRAG_STEPS, lambda s: s.step_drag(1))
    for k, (x, y) in enumerate(zip(a, b)):
        _assert_same(x, y, f"call {k}")
    assert np.any(a[-1][2][:, 0] != 1.0), "no drag was accepted"


def test_refresh_theory_refuses_a_point_outside_a_range(tmp_path):
    """After slow moves, with the range [1.2, 1.3] on the derived A every
    current point violates it: refresh_theory(None) fails with code -4 and
    leaves the walker theory rows; with the derived outputs removed it
    reproduces them."""
    from cosmomc_amd._native import NativeError
    r = _Run(tmp_path, "a", FULL_W, "native", WIDE, (0.5, 1.5), 1, 1.0, FULL_SEEDS, FULL_COV, 16)
    r.start()
    r.s.step_theory(12)
    assert np.sum(r.s.state()[0][:, 0] != 1.0) > FULL_W // 4, "few slow moves were accepted"
    rows = r.theory[0].cpu().numpy()
    r.calc.set_derived(["A"], [[1.0]], lo=[1.2], hi=[1.3])
    r.theory[0].fill_(-3.0)
    with pytest.raises(NativeError) as e:
        r.s.refresh_theory(None)
    assert e.value.code == -4, e.value
    assert torch.all(r.theory[0] == -3.0), "a failed refresh changed the walker theory rows"
    r.calc.set_derived(None, None)
    r.s.refresh_theory(None)
    assert np.array_equal(r.theory[0].cpu().numpy(), rows)
    r.close()


# ---------------------------------------------------------------- 7. end to end
def test_chain_rows_carry_the_derived_columns(tmp_path):
    """A calculator-driven run (W = 80, 40 full steps) written by
    ChainWriter(theory_derived=TheoryDerived(...)): outputs H0 = 70 A (hard
    range 60 .. 80) and DL40 = the TT coefficient column at l = 40.  In every
    written row the two derived fields, which follow the parameters and
    precede chi2_*, are fortran_e(calc.derived(the row's point), 16), and the
    DL40 field is that of the trial theory's own D_40."""
    from cosmomc_amd.chains import ChainWriter, TheoryDerived, fortran_e
    r = _Run(tmp_path, "a", FULL_W, "native", WIDE, (0.5, 1.5), 1, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS,
             cal_bounds=WIDE)
    dcoef = np.concatenate([[[70.0]], th.dl_columns(r.bh[None], 0, [40])], axis=1)
    r.calc.set_derived(["H0", "DL40"], dcoef, lo=[60.0, None], hi=[80.0, None], labels=["H_0", "D_{40}"])
    td = TheoryDerived(r.calc, [1, 2], [1.0, 1.0])
    assert td.names == [("H0", "H_0"), ("DL40", "D_{40}")] and td.ranges == [("H0", 60.0, 80.0)]
    root = str(tmp_path / "chain")
    walkers = [0, 1, 41, 79]
    cw = ChainWriter(root, ["A", "cal"], ranges=[WIDE, WIDE], walkers=walkers, burn_in=0,
                     likelihoods=[("plik", "CMB", "plik_lite", "v")], theory_derived=td)
    r.start()
    r.s.step_theory(FULL_STEPS)
    cw.append(r.s)
    hist = r.s.history_host(0, FULL_STEPS)
    with open(root + ".paramnames") as f:
        assert [l.split("\t")[0] for l in f.read().splitlines()] == ["A", "cal", "H0*", "DL40*", "chi2_plik*",
                                                                     "chi2_prior*"]
    with open(root + ".ranges") as f:
        assert f.read().splitlines()[2] == f"{'H0':<22}{fortran_e(60.0)}{fortran_e(80.0)}"
    n_rows = 0
    for w in walkers:
        starts = [t for t in range(FULL_STEPS) if t == 0 or not np.array_equal(hist[t, :, w], hist[t - 1, :, w])]
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        assert len(lines) == len(starts) - 2 and len(lines) >= 3, (w, len(lines), len(starts))
        pts = hist[starts[1:-1], :2, w]                                  # [rows, 2]
        d = r.calc.derived(pts).cpu().numpy()                            # [2, rows]
        for i, line in enumerate(lines):
            f16 = [line[j:j + 16] for j in range(0, len(line), 16)]
            assert len(f16) == 8
            assert f16[2:4] == [fortran_e(v, 16) for v in pts[i]]
            assert f16[4:6] == [fortran_e(v, 16) for v in d[:, i]]
            assert d[0, i] == 70.0 * pts[i, 0] and d[1, i] == pts[i, 0] * r.bh[0, 40]
        n_rows += len(lines)
    print(f"{n_rows} rows checked")
    r.close()


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors(cases):
    """Every argument error of cmbt_set_derived and cmbt_derived_eval is code
    -1, never an abort, and leaves the handle usable."""
    from cosmomc_amd import _native as N
    c = cases[(3, 2, 5)]
    calc = th.PolynomialTheory(PIDX, CENTER, SCALE, LO, HI, c.ex, [0, 2], c.coef)
    M = 8
    P = torch.tensor(c.P[:, :64], device="cuda")
    out = torch.zeros((c.nd, 64), dtype=torch.float64, device="cuda")

    def bad(call):
        with pytest.raises(N.NativeError) as e:
            call()
        assert e.value.code == -1, e.value

    def raw(M=M, ld=64, num_params=NPAR, ld_out=64):
        N.check(N.lib().cmbt_derived_eval(calc.handle, M, P.data_ptr(), ld, num_params, out.data_ptr(), ld_out, None,
                                          N.current_stream_ptr()), calc.handle, "cmbt")

    assert N.lib().cmbt_derived_count(calc.handle) == 0
    bad(raw)                                                               # nothing set
    bad(lambda: calc.derived(P[:, :M]))
    bad(lambda: calc.set_derived([], np.zeros((c.K, 0))))                  # n_derived = 0
    bad(lambda: calc.set_derived([f"d{i}" for i in range(33)], np.zeros((c.K, 33))))
    cfg = N.CmbtDerivedConfig()
    cfg.n_derived = 2                                                      # NULL coef
    bad(lambda: N.check(N.lib().cmbt_set_derived(calc.handle, C.byref(cfg)), calc.handle, "cmbt"))
    names = [f"d{i}" for i in range(c.nd)]
    lo, hi = np.zeros(c.nd), np.ones(c.nd)
    lo[4] = 2.0
    bad(lambda: calc.set_derived(names, c.dcoef, lo, hi))                  # lo > hi
    assert N.lib().cmbt_derived_count(calc.handle) == 0
    calc.set_derived(names, c.dcoef)
    assert N.lib().cmbt_derived_count(calc.handle) == c.nd
    bad(lambda: raw(ld=M - 1))
    bad(lambda: raw(ld_out=M - 1))
    bad(lambda: raw(num_params=3))                                         # param_index 4 outside 1..3
    bad(lambda: calc.derived(P[:3, :M]))
    raw()                                                                  # and the handle still works
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:, :M]
    assert np.all(np.abs(got.T - c.val[:M]) <= c.bound(c.mag[:M]))
    calc.set_derived(None, None)
    assert N.lib().cmbt_derived_count(calc.handle) == 0
    bad(raw)
    calc.close()
