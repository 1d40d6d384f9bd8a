"""The polynomial theory calculator (cmbt_*, cosmomc_amd.theory) on the GPU:
its evaluation against a numpy longdouble restatement, and the sampler's slow
steps with the calculator as their theory source against the same steps with
the theory callback (bit for bit).  GPU only."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
from cosmomc_amd import synthetic as syn
from cosmomc_amd import theory as th

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
TIGHT_CAL = (0.997, 1.004)          # as test_gpu_sampler: calPlanck bounds
TIGHT_A = (0.998, 1.003)            # bounds of the slow amplitude A, here also the calculator's box
WIDE = (0.9, 1.1)
PM, PS = np.array([0.0, 1.0]), np.array([0.0, 0.0025])

# ---------------------------------------------------------------- evaluation
PIDX, NPAR, FIELDS, LMAX = [4, 1, 3], 5, [0, 1, 2, 9], 37
CENTER, SCALE = np.array([0.3, -1.0, 2.0]), np.array([0.5, 2.0, -0.25])
LO, HI = CENTER - 3.0 * np.abs(SCALE), CENTER + 3.0 * np.abs(SCALE)


def _surface(n_in, ex, n_fields, lmax, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(len(ex), n_fields, lmax + 1)) * 10.0 ** rng.uniform(-2, 2, size=(len(ex), 1, 1))


def _points(n_in, num_params, pidx, center, scale, W, seed):
    """P [num_params, ld] (ld = W rounded up to 64) with the inputs inside
    center +- 2 |scale| and the other rows junk the calculator must not read."""
    rng = np.random.default_rng(seed)
    ld = (W + 63) // 64 * 64
    P = rng.normal(size=(num_params, ld)) * 1e3
    for i, p in enumerate(pidx):
        P[p - 1] = center[i] + np.abs(scale[i]) * rng.uniform(-2.0, 2.0, size=ld)
    return P


def _restate(P, W, pidx, center, scale, lo, hi, ex, coef):
    """cmbt_eval restated in numpy longdouble: (values [W, n_fields, L],
    sum_k |basis_k coef_k| [W, n_fields, L], fail [W])."""
    ld_ = np.longdouble
    n_in = len(pidx)
    raw = np.stack([P[p - 1, :W] for p in pidx], axis=1)                 # [W, n_in]
    ok = np.all((raw >= lo) & (raw <= hi), axis=1)
    q = np.where(np.isnan(raw), center, raw)
    q = np.minimum(np.maximum(q, lo), hi)
    x = (q.astype(ld_) - center.astype(ld_)) / scale.astype(ld_)
    B = np.ones((W, len(ex)), dtype=ld_)
    for k, row in enumerate(ex):
        for i in range(n_in):
            for _ in range(int(row[i])):
                B[:, k] = B[:, k] * x[:, i]
    c = coef.astype(ld_)
    val = np.einsum("wk,kfl->wfl", B, c)
    mag = np.einsum("wk,kfl->wfl", np.abs(B), np.abs(c))
    return val, mag, (~ok).astype(np.int32)


def _eval(calc, P, W, shape=(10, 45), pad=(0, 0), fail=True):
    """calc at P[:, :W] into a NaN-filled buffer [W, shape] cut out of one
    with `pad` more fields and l, so that the strides differ."""
    Pd = torch.tensor(P, device="cuda")[:, :W]
    full = torch.full((W, shape[0] + pad[0], shape[1] + pad[1]), float("nan"), dtype=torch.float64, device="cuda")
    out = full[:, :shape[0], :shape[1]]
    fl = torch.full((W,), -7, dtype=torch.int32, device="cuda") if fail else None
    calc.eval(Pd, out, fl)
    return out.cpu().numpy(), (fl.cpu().numpy() if fail else None), full.cpu().numpy()


def _check_against_restatement(got, P, W, pidx, center, scale, lo, hi, ex, coef, fields, lmax):
    val, mag, _ = _restate(P, W, pidx, center, scale, lo, hi, ex, coef)
    K = len(ex)
    bound = (K + 2 * 4 + 4) * 2.0 ** -52 * mag
    err = np.abs(got[:, fields, :lmax + 1].astype(np.longdouble) - val)
    print(f"W={W} K={K}: max |got - ref| / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    rest = np.ones(got.shape, dtype=bool)
    rest[:, fields, :lmax + 1] = False
    assert np.all(np.isnan(got[rest])), "an element outside the calculator's fields or beyond lmax was written"
    assert not np.any(np.isnan(got[~rest]))


@pytest.fixture(scope="module")
def quad():
    ex = th.monomials(3, 2)
    coef = _surface(3, ex, len(FIELDS), LMAX, 11)
    return ex, coef


def _calc3(ex, coef, lo=LO, hi=HI):
    return th.PolynomialTheory(PIDX, CENTER, SCALE, lo, hi, ex, FIELDS, coef)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("K", [10, 7])
def test_eval_matches_restatement(quad, W, K):
    """n_in = 3 out of 5 parameter rows (param_index 4, 1, 3), degree 2 (K = 10)
    and a 7-row subset (K no multiple of the 8-term chunk nor of 4), fields TT
    TE EE PP to lmax 37 in a NaN-filled [W, 10, 45] buffer (odd ld_field: every
    other row only 8-byte aligned).  |got - ref| <= (K + 2 x 4 + 4) 2^-52
    sum_k |basis_k coef_k| against the longdouble restatement: K roundings of
    the sum, at most 4 multiplications of inputs that carry 2 roundings each
    (subtraction and division), 4 spare; untouched elements stay NaN."""
    ex, coef = quad
    if K == 7:
        keep = [0, 2, 3, 5, 6, 8, 9]
        ex, coef = ex[keep], coef[keep]
    calc = _calc3(ex, coef)
    P = _points(3, NPAR, PIDX, CENTER, SCALE, W, 100 + W)
    got, fl, _ = _eval(calc, P, W)
    assert np.array_equal(fl, np.zeros(W, dtype=np.int32))
    _check_against_restatement(got, P, W, PIDX, CENTER, SCALE, LO, HI, ex, coef, FIELDS, LMAX)
    calc.close()


def test_eval_quartic_in_six_chunks_k():
    """n_in = 6, degree 4: K = 210 terms go through the LDS in 27 chunks; W = 65
    (three walker tiles, the last with one walker), lmax 300 (two l tiles)."""
    ex = th.monomials(6, 4)
    pidx, fields, lmax, W = [2, 7, 1, 5, 4, 8], [1, 4], 300, 65
    rng = np.random.default_rng(3)
    center, scale = rng.normal(size=6), rng.uniform(0.5, 2.0, size=6)
    lo, hi = center - 3 * scale, center + 3 * scale
    coef = _surface(6, ex, 2, lmax, 12)
    calc = th.PolynomialTheory(pidx, center, scale, lo, hi, ex, fields, coef)
    P = _points(6, 8, pidx, center, scale, W, 7)
    got, fl, _ = _eval(calc, P, W, shape=(5, 303))
    assert not fl.any()
    _check_against_restatement(got, P, W, pidx, center, scale, lo, hi, ex, coef, fields, lmax)
    calc.close()


def test_eval_deterministic_across_batch_and_strides(quad):
    """Walker w's rows from the W = 257 batch equal, bit for bit, the same
    walker evaluated alone and evaluated into a buffer with other ld_walker
    and ld_field (even ld_field: every row 16-byte aligned)."""
    ex, coef = quad
    calc = _calc3(ex, coef)
    W = 257
    P = _points(3, NPAR, PIDX, CENTER, SCALE, W, 100 + W)
    got, _, _ = _eval(calc, P, W)
    other, _, full = _eval(calc, P, W, pad=(2, 3))
    sel = got[:, FIELDS, :LMAX + 1]
    assert np.array_equal(other[:, FIELDS, :LMAX + 1], sel)
    assert np.all(np.isnan(full[:, 10:, :])) and np.all(np.isnan(full[:, :, 45:]))
    for w in (0, 31, 32, 63, 64, 255, 256):
        alone, _, _ = _eval(calc, np.ascontiguousarray(P[:, w:w + 1]), 1)
        assert np.array_equal(alone[0, FIELDS, :LMAX + 1], sel[w]), w
    host = torch.full((W, 10, 45), float("nan"), dtype=torch.float64, device="cuda")
    calc.eval(np.ascontiguousarray(P[:, :W].T), host)   # host points [W, num_params], as importance sampling passes them
    assert np.array_equal(host.cpu().numpy()[:, FIELDS, :LMAX + 1], sel)
    calc.close()


def test_validity_box(quad):
    """Inputs exactly at lo and at hi pass; nextafter outside either fails, NaN
    fails; a failed walker's rows are those of its clamped input (NaN: the
    centre) evaluated directly; fail holds only 0 or 1."""
    ex, coef = quad
    calc = _calc3(ex, coef)
    inside = CENTER + 0.5 * np.abs(SCALE)
    cases = []                                          # (inputs, fails, clamped inputs)
    for i in range(3):
        for edge, out_dir in ((LO[i], -np.inf), (HI[i], np.inf)):
            at = inside.copy()
            at[i] = edge
            cases.append((at, 0, at))
            off = at.copy()
            off[i] = np.nextafter(edge, out_dir)
            cases.append((off, 1, at))
        nan = inside.copy()
        nan[i] = np.nan
        cl = inside.copy()
        cl[i] = CENTER[i]
        cases.append((nan, 1, cl))
    far = np.array([LO[0] - 1e6, HI[1] + 1e6, np.nan])
    cases.append((far, 1, np.array([LO[0], HI[1], CENTER[2]])))
    W = len(cases)
    P = _points(3, NPAR, PIDX, CENTER, SCALE, W, 1)
    Pc = P.copy()
    for w, (raw, _, cl) in enumerate(cases):
        for i, p in enumerate(PIDX):
            P[p - 1, w], Pc[p - 1, w] = raw[i], cl[i]
    got, fl, _ = _eval(calc, P, W)
    ref, flc, _ = _eval(calc, Pc, W)
    assert fl.tolist() == [c[1] for c in cases]
    assert not flc.any()
    assert np.array_equal(got[:, FIELDS, :LMAX + 1], ref[:, FIELDS, :LMAX + 1])
    _, _, ref_fail = _restate(P, W, PIDX, CENTER, SCALE, LO, HI, ex, coef)
    assert np.array_equal(fl, ref_fail)
    calc.close()


def test_argument_errors(quad):
    """Every argument error of cmbt_create and cmbt_eval is code -1 (a
    NativeError), never an abort."""
    from cosmomc_amd._native import NativeError
    ex, coef = quad

    def create(pidx=PIDX, center=CENTER, scale=SCALE, lo=LO, hi=HI, ex=ex, fields=FIELDS, coef=coef):
        with pytest.raises(NativeError) as e:
            th.PolynomialTheory(pidx, center, scale, lo, hi, ex, fields, coef)
        assert e.value.code == -1, e.value

    z = np.zeros
    create(pidx=[], center=[], scale=[], lo=[], hi=[], ex=z((10, 0)))                       # n_in = 0
    create(pidx=list(range(1, 18)), center=z(17), scale=np.ones(17), lo=-np.ones(17), hi=np.ones(17),
           ex=z((10, 17)))                                                                     # n_in = 17
    create(ex=z((0, 3)), coef=z((0, 4, LMAX + 1)))                                             # n_terms = 0
    create(ex=z((257, 3)), coef=z((257, 4, LMAX + 1)))                                         # n_terms = 257
    create(fields=[], coef=z((10, 0, LMAX + 1)))                                               # n_fields = 0
    create(fields=list(range(11)), coef=z((10, 11, LMAX + 1)))                                 # n_fields = 11
    bad = ex.copy()
    bad[4] = [2, 2, 1]
    create(ex=bad)                                                                             # order 5
    create(scale=[0.5, 0.0, -0.25])
    create(lo=[LO[0], HI[1] + 1.0, LO[2]])                                                     # lo > hi
    create(fields=[0, 1, 2, 10])
    create(fields=[0, 1, -1, 9])
    create(fields=[0, 1, 1, 9])                                                                # repeated
    create(pidx=[4, 0, 3])

    calc = _calc3(ex, coef)
    W = 8
    P = torch.tensor(_points(3, NPAR, PIDX, CENTER, SCALE, W, 2), device="cuda")[:, :W]
    out = torch.zeros((W, 10, 45), dtype=torch.float64, device="cuda")

    def ev(P=P, out=out):
        with pytest.raises(NativeError) as e:
            calc.eval(P, out)
        assert e.value.code == -1, e.value

    ev(P=P[:3])                                                  # param_index 4 outside 1..3
    ev(out=out[:1].expand(W, 10, 45))                            # ld_walker == 0
    ev(out=torch.zeros((W, 10, 20), dtype=torch.float64, device="cuda"))   # ld_field < lmax + 1
    calc.eval(P, out)                                            # and the handle still works
    assert torch.isfinite(out).all()
    calc.close()


# ---------------------------------------------------------------- the sampler
def _one_term(base, box, fields=(0, 1, 2)):
    """theory = A x base as a one-term surface in A = P(1): exponents [[1]],
    centre 0, scale 1, so the basis is A itself and every D_l one rounding,
    as the callback's product."""
    return th.PolynomialTheory([1], [0.0], [1.0], [box[0]], [box[1]], [[1]], list(fields), base[None])


class _Run:
    """Full-step / dragging runs of test_gpu_sampler's A x base problem
    (synthetic plik_lite, A = P(1) slow, calPlanck = P(2) fast): mode "callback"
    fills the trial theory with torch, mode "native" sets a calculator."""

    def __init__(self, tmp_path, tag, W, mode, a_bounds, box, oversample, T, seeds, cov, capacity, n_like=1,
                 share_trial=False, cal_bounds=TIGHT_CAL):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        from cosmomc_amd.sampler import BatchedMCMC
        data = syn.make_plik_lite(12345)
        self.bh = np.ascontiguousarray(syn.base_theory(2508)[:3])
        self.base = torch.tensor(self.bh, device="cuda")
        self.W, self.mode = W, mode
        pmin, pmax = np.array([a_bounds[0], cal_bounds[0]]), np.array([a_bounds[1], cal_bounds[1]])
        self.s = BatchedMCMC(W, 2, [1, 2], [[1], [2]], 1, pmin, pmax, PM, PS, oversample_fast=oversample,
                             propose_scale=2.4, temperature=T, seed_ij=seeds[0], seed_kl=seeds[1])
        self.s.set_covariance(cov)
        self.likes, self.theory, self.trial = [], [], []
        for i in range(n_like):
            like = NativeCMBLikelihood("PLIK_LITE", data.write(str(tmp_path / f"{tag}{i}")))
            like.nuisance_indices = [2]
            self.likes.append(like)
            self.theory.append(self.base.unsqueeze(0).repeat(W, 1, 1).contiguous())
            self.trial.append(self.trial[0] if share_trial and i else torch.empty_like(self.theory[0]))
            self.s.add_likelihood(like, self.theory[i])
            self.s.set_trial_theory(i, self.trial[i])
        self.s.enable_history(capacity)
        self.calc = None
        if mode == "native":
            self.calc = _one_term(self.bh, box)
            self.s.set_theory_calculator(self.calc)

    def start(self):
        self.s.set_start(np.tile([1.0, 1.0], (self.W, 1)))

    def theory_fn(self, P):
        for t in ({id(t): t for t in self.trial}).values():
            t.copy_(self.base.unsqueeze(0) * P[0].reshape(-1, 1, 1))

    @property
    def fn(self):
        return self.theory_fn if self.mode == "callback" else None

    def outputs(self):
        """history_host, history_terms, state() and the walker theory rows"""
        n = self.s.history_count()
        return (self.s.history_host(0, n), self.s.history_terms(0, n), *self.s.state(),
                *[t.cpu().numpy() for t in self.theory])

    def close(self):
        self.s.close()
        if self.calc is not None:
            self.calc.close()


def _assert_same(a, b, what):
    names = ["history_host", "history_terms", "P", "CurLike", "mult", "num_accept"]
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        n = names[i] if i < len(names) else f"theory rows of likelihood {i - len(names)}"
        assert np.array_equal(x, y), f"{what}: {n} differ"


FULL_COV = np.diag([0.002 ** 2, 0.0025 ** 2])
FULL_W, FULL_STEPS, FULL_SEEDS = 80, 40, (71, 72)


def _full_run(tmp_path, tag, mode, a_bounds, box, oversample, T, per_call, **kw):
    r = _Run(tmp_path, tag, FULL_W, mode, a_bounds, box, oversample, T, FULL_SEEDS, FULL_COV, FULL_STEPS, **kw)
    r.start()
    outs = []
    for _ in range(FULL_STEPS // per_call):
        r.s.step_theory(per_call, theory_fn=r.fn)
        outs.append(r.outputs())
    r.close()
    return outs


@pytest.mark.parametrize("oversample", [1, 3])
def test_full_steps_native_equals_callback(tmp_path, oversample):
    """test_full_steps_with_theory_callback's run (not tight: W = 80, 40 steps
    in one call, seeds 71/72), whose chain that test pins to the C oracle,
    against the same run with the one-term calculator and no callback:
    history, terms, state and the walker theory rows are the same bits."""
    a = _full_run(tmp_path, "a", "callback", WIDE, None, oversample, 1.0, FULL_STEPS, cal_bounds=WIDE)
    b = _full_run(tmp_path, "b", "native", WIDE, (0.5, 1.5), oversample, 1.0, FULL_STEPS, cal_bounds=WIDE)
    assert np.any(np.abs(a[0][2][:, 0] - 1.0) > 1e-6), "no slow move was accepted"
    _assert_same(a[0], b[0], f"oversample_fast {oversample}")


def _a_only_out_of_box(oversample, T, walkers):
    """Of each walker's 40 orc_mh_step trials in the callback run (bounds
    TIGHT_A, TIGHT_CAL), how many have A outside TIGHT_A while calPlanck is
    inside its bounds.  The oracle reports no trial point, so step k is found
    by replaying k steps on that target and making step k + 1 on a target with
    A's bounds at 0.9 .. 1.1 and a probe likelihood (returning 0.0), which is
    called with the trial point whenever that is inside those bounds."""
    from cosmomc_amd.sampler import walker_seed
    from test_gpu_sampler import _scaled_plik_target
    orc = po.PlikLite(syn.make_plik_lite(12345))
    bh = np.ascontiguousarray(syn.base_theory(2508)[:3])
    seen = []

    def probe(user, Pp):
        seen.append(Pp[0])
        return 0.0
    tt, k1 = _scaled_plik_target(orc, bh, np.array([TIGHT_A[0], TIGHT_CAL[0]]), np.array([TIGHT_A[1], TIGHT_CAL[1]]),
                                 PM, PS, T)
    tw, k2 = _scaled_plik_target(orc, bh, np.array([WIDE[0], TIGHT_CAL[0]]), np.array([WIDE[1], TIGHT_CAL[1]]),
                                 PM, PS, T, extra_like=probe)
    counts = []
    for w in walkers:
        ij, kl = walker_seed(*FULL_SEEDS, w)
        n = 0
        for k in range(FULL_STEPS):
            h = po.lib().orc_proposer_create(2, np.array([1, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32),
                                             1, oversample, 2.4, 2, np.array([1, 2], dtype=np.int32))
            po.lib().orc_proposer_set_covariance(h, np.ascontiguousarray(FULL_COV))
            r = po.Ranmar(ij, kl)
            Q = np.array([1.0, 1.0])
            cur = C.c_double(po.lib().orc_target_loglike(C.byref(tt), Q))
            tl = C.c_double(0.0)
            for _ in range(k):
                po.lib().orc_mh_step(h, C.byref(r.s), C.byref(tt), Q, C.byref(cur), 0, C.byref(tl))
            del seen[:]
            po.lib().orc_mh_step(h, C.byref(r.s), C.byref(tw), Q, C.byref(cur), 0, C.byref(tl))
            po.lib().orc_proposer_free(h)
            n += bool(seen) and not TIGHT_A[0] <= seen[-1] <= TIGHT_A[1]
        counts.append(n)
    return counts


@pytest.mark.parametrize("oversample", [1, 3])
def test_calculator_failure_equals_out_of_bounds(tmp_path, oversample):
    """Temperature 2.5, one step per call.  Run A: the callback, sampler bounds
    A in [0.998, 1.003], calPlanck in [0.997, 1.004].  Run B: the calculator
    with box A in [0.998, 1.003] and the sampler's A bounds at 0.9 .. 1.1, so
    only the calculator's flag rejects those trials.  All outputs are the same
    bits after every step.

    Of the 40 trials of the oracle chains of walkers 0, 1, 41 and 79 (seeds
    71/72), 11, 12, 12 and 12 (oversample_fast 1) / 6, 7, 7 and 7 (3) have A
    outside the box while calPlanck is inside its bounds; at least 5 each are
    asserted."""
    counts = _a_only_out_of_box(oversample, 2.5, (0, 1, 41, 79))
    print(f"oversample_fast {oversample}: trials with only A outside the box: {counts}")
    assert min(counts) >= 5, counts
    a = _full_run(tmp_path, "a", "callback", TIGHT_A, None, oversample, 2.5, 1)
    b = _full_run(tmp_path, "b", "native", WIDE, TIGHT_A, oversample, 2.5, 1)
    for k, (x, y) in enumerate(zip(a, b)):
        _assert_same(x, y, f"step {k}")
    assert np.any(a[-1][2][:, 0] != 1.0), "no slow move was accepted"


DRAG_W, DRAG_STEPS, DRAG_T, DRAG_SEEDS = 130, 24, 2.0, (95, 96)
DRAG_COV = np.diag([0.003 ** 2, 0.0025 ** 2])


def test_dragging_native_equals_callback(tmp_path):
    """test_dragging_plik_follows_oracle_at_bounds' run (W = 130, 24
    step_drag(1) calls, oversample_fast 2, Temperature 2, seeds 95/96; that
    test pins the callback run to orc_drag_step, with 31 drags aborted at their
    end point) against the calculator with identical bounds, and against the
    calculator with A's bounds moved into its box: the same bits after every
    call."""
    def run(tag, mode, a_bounds, box):
        r = _Run(tmp_path, tag, DRAG_W, mode, a_bounds, box, 2, DRAG_T, DRAG_SEEDS, DRAG_COV, DRAG_STEPS)
        r.start()
        outs = []
        for _ in range(DRAG_STEPS):
            r.s.step_drag(1, theory_fn=r.fn)
            outs.append(r.outputs())
        r.close()
        return outs
    a = run("a", "callback", TIGHT_A, None)
    assert np.any(a[-1][2][:, 0] != 1.0), "no drag was accepted"
    for tag, a_bounds, box in (("b", TIGHT_A, (0.5, 1.5)), ("c", WIDE, TIGHT_A)):
        b = run(tag, "native", a_bounds, box)
        for k, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, f"run {tag} call {k}")


def test_refresh_theory_from_calculator(tmp_path):
    """After slow moves: save_state, a new sampler, load_state,
    set_theory_calculator, refresh_theory(None) -- the walker theory rows are
    the original run's bits.  With a box that excludes the points the call
    fails with code -4 and leaves the rows as they are."""
    from cosmomc_amd._native import NativeError
    r = _Run(tmp_path, "a", FULL_W, "native", WIDE, (0.5, 1.5), 1, 1.0, FULL_SEEDS, FULL_COV, 16)
    r.start()
    r.s.step_theory(12)
    P = r.s.state()[0]
    assert np.sum(P[:, 0] != 1.0) > FULL_W // 4, "few slow moves were accepted"
    image, rows = r.s.save_state(), r.theory[0].cpu().numpy()
    r.close()
    n = _Run(tmp_path, "b", FULL_W, "callback", WIDE, None, 1, 1.0, FULL_SEEDS, FULL_COV, 16)
    n.s.load_state(image)
    n.theory[0].fill_(-3.0)
    off = _one_term(n.bh, (1.2, 1.3))
    n.s.set_theory_calculator(off)
    with pytest.raises(NativeError) as e:
        n.s.refresh_theory(None)
    assert e.value.code == -4, e.value
    assert torch.all(n.theory[0] == -3.0), "a failed refresh changed the walker theory rows"
    good = _one_term(n.bh, (0.5, 1.5))
    n.s.set_theory_calculator(good)
    n.s.refresh_theory(None)
    assert np.array_equal(n.theory[0].cpu().numpy(), rows)
    n.s.step_theory(2)                                  # and the run goes on natively
    n.close()
    off.close()
    good.close()


def test_no_calculator_and_no_callback_still_refused(tmp_path):
    from cosmomc_amd._native import NativeError
    r = _Run(tmp_path, "a", 64, "callback", WIDE, None, 1, 1.0, FULL_SEEDS, FULL_COV, 4)
    r.start()
    for call in (lambda: r.s.step_theory(1, theory_fn=None), lambda: r.s.step_drag(1, theory_fn=None),
                 lambda: r.s.refresh_theory(None)):
        with pytest.raises(NativeError) as e:
            call()
        assert e.value.code == -1, e.value
    calc = _one_term(r.bh, (0.5, 1.5))
    r.s.set_theory_calculator(calc)
    r.s.set_theory_calculator(None)                     # removed again: refused as before
    with pytest.raises(NativeError) as e:
        r.s.step_theory(1, theory_fn=None)
    assert e.value.code == -1, e.value
    r.close()
    calc.close()


def test_callback_steps_ignore_the_calculators_flags(tmp_path):
    """A theory function passed to step_theory / step_drag is the theory
    source even when a calculator is set, and the out-of-box flags of the
    calculator's last call stay out of its steps: after a refresh_theory(None)
    that flagged every walker (box A in [1.2, 1.3]; code -4, rows untouched),
    callback steps give the bits of a run that never had a calculator."""
    from cosmomc_amd._native import NativeError
    outs = []
    for tag in ("plain", "flagged"):
        r = _Run(tmp_path, tag, FULL_W, "callback", WIDE, None, 1, 1.0, FULL_SEEDS, FULL_COV, 8, cal_bounds=WIDE)
        r.start()
        off = None
        if tag == "flagged":
            off = _one_term(r.bh, (1.2, 1.3))
            r.s.set_theory_calculator(off)
            with pytest.raises(NativeError) as e:
                r.s.refresh_theory(None)
            assert e.value.code == -4, e.value
        r.s.step_theory(4, theory_fn=r.fn)
        r.s.step_drag(2, theory_fn=r.fn)
        outs.append(r.outputs())
        r.close()
        if off is not None:
            off.close()
    assert np.any(outs[0][2][:, 0] != 1.0), "no slow move was accepted"
    _assert_same(outs[0], outs[1], "calculator set and flagged")


@pytest.mark.parametrize("share_trial", [False, True])
def test_two_trial_buffers(tmp_path, share_trial):
    """Two likelihood handles on the same dataset with theory buffers of their
    own: the native run fills both trial buffers (one launch each) and equals
    the callback run that fills both; with one trial buffer shared by both
    handles it is evaluated once per step (counted by the library's profiler)."""
    from cosmomc_amd import _native as N
    steps = 12
    outs = {}
    for mode in ("callback", "native"):
        r = _Run(tmp_path, mode[0], FULL_W, mode, TIGHT_A if mode == "callback" else WIDE, TIGHT_A, 1, 2.5,
                 FULL_SEEDS, FULL_COV, steps, n_like=2, share_trial=share_trial)
        r.start()
        N.profile_reset()
        N.profile_enable(True)
        try:
            r.s.step_theory(steps, theory_fn=r.fn)
            outs[mode] = r.outputs()
        finally:
            N.profile_enable(False)
        launches = N.profile_read("theory_calc_kernel")[1]
        assert launches == (0 if mode == "callback" else steps * (1 if share_trial else 2)), launches
        r.close()
    assert np.any(outs["callback"][2][:, 0] != 1.0), "no slow move was accepted"
    _assert_same(outs["callback"], outs["native"], f"share_trial {share_trial}")
