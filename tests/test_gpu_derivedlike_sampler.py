"""Derived likelihoods as term rows of the sampler (cmbs_add_derived_likelihood,
BatchedMCMC.add_derived_likelihood) on the GPU: a derived Gaussian on A against
the sampler's own Gaussian prior on A (bit for bit, which pins the accept
logic to paths the C oracle pins), a zero-weight row that must change
nothing, the rows against DerivedGaussian.eval, the calculator's box, the
checkpoint image, the chain file and the refusals.  GPU only."""
import os

import numpy as np
import pytest

from cosmomc_amd import synthetic as syn
from cosmomc_amd import theory as th
from cosmomc_amd.derivedlike import DerivedGaussian
from test_gpu_theory_calc import (DRAG_COV, DRAG_SEEDS, DRAG_STEPS, DRAG_W, FULL_COV, FULL_SEEDS, FULL_STEPS, FULL_W,
                                  TIGHT_A, TIGHT_CAL, WIDE, _one_term)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
BAO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bao")
OBS_A, STD_A = 1.0 + 2.0 ** -10, 2.0 ** -9             # the constraint on A: std a power of two
FAST_TAIL = 8                                          # fast-only steps after the full-step runs


def _on_a(calc, kind):
    """Derived likelihoods on the one-term calculator (basis A itself).
    "a": the surface A (coef [[1.0]]) with obs 1 + 2^-10 and invcov 2^18, the
    twin of a Gaussian prior on A with std 2^-9.  "zero": the same with
    invcov 0.  "dr12": six surfaces linear in A, obs_i x A, with the DR12
    consensus set's obs and inverse covariance."""
    if kind == "a":
        return DerivedGaussian(calc, [[1.0]], [OBS_A], invcov=[[2.0 ** 18]], name="a")
    if kind == "zero":
        return DerivedGaussian(calc, [[1.0]], [OBS_A], invcov=[[0.0]], name="zero")
    obs = np.loadtxt(os.path.join(BAO, "DR12", "sdss_DR12Consensus_bao.dat"), usecols=(1,))
    cov = np.loadtxt(os.path.join(BAO, "DR12", "BAO_consensus_covtot_dM_Hz.txt"))
    return DerivedGaussian(calc, obs[None, :], obs, cov=cov, name="dr12")


class _DRun:
    """test_gpu_theory_calc._Run's A x base problem (synthetic plik_lite, A =
    P(1) slow, calPlanck = P(2) fast, the one-term calculator as the theory
    source) with the priors and derived likelihoods of its arguments: prior_a
    puts the sampler's Gaussian prior (OBS_A, STD_A) on A; no other prior is
    set.  n_like = 0: no data likelihood at all."""

    def __init__(self, tmp_path, tag, W, oversample, T, seeds, cov, capacity, derived=(), prior_a=False, n_like=1,
                 a_bounds=WIDE, box=(0.5, 1.5), cal_bounds=TIGHT_CAL, calc=True):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        from cosmomc_amd.sampler import BatchedMCMC
        self.bh = np.ascontiguousarray(syn.base_theory(2508)[:3])
        self.base = torch.tensor(self.bh, device="cuda")
        self.W = W
        pmin, pmax = np.array([a_bounds[0], cal_bounds[0]]), np.array([a_bounds[1], cal_bounds[1]])
        pm = np.array([OBS_A if prior_a else 0.0, 0.0])
        ps = np.array([STD_A if prior_a else 0.0, 0.0])
        self.s = BatchedMCMC(W, 2, [1, 2], [[1], [2]], 1, pmin, pmax, pm, ps, oversample_fast=oversample,
                             propose_scale=2.4, temperature=T, seed_ij=seeds[0], seed_kl=seeds[1])
        self.s.set_covariance(cov)
        self.likes, self.theory, self.trial = [], [], []
        for i in range(n_like):
            like = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(str(tmp_path / f"{tag}{i}")))
            like.nuisance_indices = [2]
            self.likes.append(like)
            self.theory.append(self.base.unsqueeze(0).repeat(W, 1, 1).contiguous())
            self.trial.append(torch.empty_like(self.theory[0]))
            self.s.add_likelihood(like, self.theory[i])
            self.s.set_trial_theory(i, self.trial[i])
        self.s.enable_history(capacity)
        self.calc = _one_term(self.bh, box)
        if calc:
            self.s.set_theory_calculator(self.calc)
        self.derived = [_on_a(self.calc, k) for k in derived]
        for g in self.derived:
            self.s.add_derived_likelihood(g)

    def start(self):
        self.s.set_start(np.tile([1.0, 1.0], (self.W, 1)))

    def outputs(self):
        """history_host, history_terms, P, CurLike, mult, num_accept"""
        n = self.s.history_count()
        return (self.s.history_host(0, n), self.s.history_terms(0, n), *self.s.state())

    def close(self):
        self.s.close()
        for g in self.derived:
            g.close()
        self.calc.close()


# The runs of tests 6 and 7: W 80 full steps (oversample_fast 1 and 3, then 8 fast-only
# steps), W 130 drags (oversample_fast 2), and a sampler with no data likelihood
CASES = {"full1": dict(W=FULL_W, oversample=1, seeds=FULL_SEEDS, cov=FULL_COV, calls=FULL_STEPS, kind="full"),
         "full3": dict(W=FULL_W, oversample=3, seeds=FULL_SEEDS, cov=FULL_COV, calls=FULL_STEPS, kind="full"),
         "drag": dict(W=DRAG_W, oversample=2, seeds=DRAG_SEEDS, cov=DRAG_COV, calls=DRAG_STEPS, kind="drag"),
         "only": dict(W=FULL_W, oversample=1, seeds=FULL_SEEDS, cov=FULL_COV, calls=FULL_STEPS, kind="only")}
_cache = {}


def _outs(factory, case, derived=(), prior_a=False):
    """The outputs after every call of a case's run with these derived
    likelihoods / this prior (Temperature 1), computed once per module."""
    key = (case, tuple(derived), prior_a)
    if key in _cache:
        return _cache[key]
    c = CASES[case]
    tmp = factory.mktemp(f"{case}_{'_'.join(derived) or 'none'}_{int(prior_a)}")
    r = _DRun(tmp, "r", c["W"], c["oversample"], 1.0, c["seeds"], c["cov"], c["calls"] + FAST_TAIL, derived, prior_a,
              n_like=0 if c["kind"] == "only" else 1)
    r.start()
    outs = []
    for _ in range(c["calls"]):
        if c["kind"] == "drag":
            r.s.step_drag(1)
        elif c["kind"] == "only" and not derived:
            r.s.step(1, fast_only=False)               # no term needs a theory: plain Metropolis
        else:
            r.s.step_theory(1)
        outs.append(r.outputs())
    if c["kind"] == "full":
        r.s.step(FAST_TAIL, fast_only=True)
        outs.append(r.outputs())
    r.close()
    _cache[key] = outs
    return outs


def _same_chain(a, b, what, terms=False):
    names = ["history_host", "history_terms", "P", "CurLike", "mult", "num_accept"]
    for i, (x, y) in enumerate(zip(a, b)):
        if i == 1 and not terms:
            continue
        assert np.array_equal(x, y), f"{what}: {names[i]} differ"


# ---------------------------------------------------------------- 6. equals a Gaussian prior
@pytest.mark.parametrize("case", list(CASES))
def test_derived_row_equals_gaussian_prior(tmp_path_factory, case):
    """Run a: the sampler's Gaussian prior on A, mean 1 + 2^-10, std 2^-9.
    Run b: no prior, the surface A with obs 1 + 2^-10 and invcov 2^18 as a
    derived likelihood.  With Temperature 1, z = r 2^9 is exact, z^2 = 2^18
    round(r^2) = r (2^18 r), so pri / 2 and the derived term are the same
    double and target_like returns the same bits: history rows, P, CurLike,
    mult and num_accept agree after every call (the terms differ by design).
    full1 / full3: plik_lite, 40 step_theory(1) calls, then step(8,
    fast_only=True); drag: 24 step_drag(1) calls; only: no data likelihood,
    run a plain cmbs_step(fast_only = 0), run b step_theory(None).  And the
    constraint matters: the chain without it differs."""
    a = _outs(tmp_path_factory, case, prior_a=True)
    b = _outs(tmp_path_factory, case, derived=("a",))
    free = _outs(tmp_path_factory, case)
    assert len(a) == len(b) == CASES[case]["calls"] + (CASES[case]["kind"] == "full")
    for k, (x, y) in enumerate(zip(a, b)):
        _same_chain(x, y, f"{case} call {k}")
    assert np.any(b[-1][2][:, 0] != 1.0), "no slow move was accepted"
    assert not np.array_equal(b[-1][0], free[-1][0]), "the derived likelihood changed nothing"
    # the derived row is the last one, and it is the prior's term
    t = b[-1][1][:, -1, :]
    A = b[-1][0][:, 0, :]
    assert np.array_equal(t, ((A - OBS_A) * (2.0 ** 18 * (A - OBS_A))) / 2)


# ---------------------------------------------------------------- 7. zero weight changes nothing
@pytest.mark.parametrize("prior_a,derived", [(True, ()), (False, ("a",))], ids=["on_prior_run", "on_derived_run"])
@pytest.mark.parametrize("case", list(CASES))
def test_zero_weight_row_changes_nothing(tmp_path_factory, case, prior_a, derived):
    """A further derived likelihood with invcov = 0 on each run of test 6:
    state, history and the other term rows are the same bits, and its own row
    is +0.0 everywhere.  (The prior run with no data likelihood steps with
    cmbs_step; with the row it steps with step_theory.)"""
    base = _outs(tmp_path_factory, case, derived=derived, prior_a=prior_a)
    zero =_outs(tmp_path_factory, case, derived=(*derived, "zero"), prior_a=prior_a)
    for k, (x, y) in enumerate(zip(base, zero)):
        _same_chain(x, y, f"{case} call {k}")
        assert np.array_equal(x[1], y[1][:, :-1, :]), f"{case} call {k}: the other term rows differ"
        assert np.all(y[1][:, -1, :] == 0.0) and not np.any(np.signbit(y[1][:, -1, :]))


def _headline(cmbl_golden, refdata, tmp_path, th_rows, W, zero):
    """test_gpu_raw_sums_layout's headline pair (plik_lite + Planck lensing,
    calPlanck the only varying parameter), 4 fast-only steps, in whichever
    fast-step schedule the sampler picks."""
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    from cosmomc_amd.sampler import BatchedMCMC
    c = cmbl_golden["cases"]["lensing_consext8"]
    dl = torch.tensor(np.ascontiguousarray(th_rows[:W]), device="cuda")
    plik = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(str(tmp_path)))
    lens = NativeCMBLikelihood(c["tag"], os.path.join(refdata, c["dataset"]), c["overrides"])
    plik.nuisance_indices = [2]
    lens.nuisance_indices = [2]
    s = BatchedMCMC(W, 3, [2], [[1]], 0, [0.0222, 0.9, 3.05], [0.0222, 1.1, 3.05], [0.0, 1.0, 0.0],
                    [0.0, 0.0025, 0.0], seed_ij=61, seed_kl=72)
    s.set_covariance(np.array([[0.002 ** 2]]))
    s.add_likelihood(plik, dl)
    s.add_likelihood(lens, dl)
    calc = th.PolynomialTheory([3], [0.0], [1.0], [3.0], [3.1], [[1]], [0], np.ones((1, 1, 1)))
    g = DerivedGaussian(calc, [[1.0]], [3.0], invcov=[[0.0]])
    if zero:
        s.set_theory_calculator(calc)
        s.add_derived_likelihood(g)
    s.enable_history(4)
    s.set_start(np.tile([0.0222, 1.0, 3.05], (W, 1)))
    s.step(4, fast_only=True)
    out = (s.history_host(0, 4), s.history_terms(0, 4), *s.state())
    assert plik.status() == 0 and lens.status() == 0
    s.close()
    g.close()
    calc.close()
    return out


def test_zero_weight_row_on_the_headline_pair(cmbl_golden, refdata, tmp_path):
    """The headline pair with W = 130 and 4 fast steps, with and without a
    zero-weight derived row: the same bits (the run without takes the
    pipelined schedule, the run with it the general one)."""
    W = 130
    rows = syn.walker_theory(W, seed=11, n_fields=10, ld_field=2512)
    a = _headline(cmbl_golden, refdata, tmp_path, rows, W, False)
    b = _headline(cmbl_golden, refdata, tmp_path, rows, W, True)
    _same_chain(a, b, "headline pair")
    assert a[1].shape[1] == 2 and b[1].shape[1] == 3
    assert np.array_equal(a[1], b[1][:, :2, :])
    assert np.all(b[1][:, 2, :] == 0.0) and not np.any(np.signbit(b[1][:, 2, :]))
    assert np.all(np.isfinite(a[1])) and np.any(a[5] > 0)


# ---------------------------------------------------------------- 8. row consistency
def test_rows_equal_eval_at_the_rows_points(tmp_path):
    """full3's run at Temperature 2.5 with the DR12-sized 6-vector (surfaces
    obs_i x A): in every history row the derived term is DerivedGaussian.eval
    at that row's point, bit for bit; it is constant while A stays; and
    CurLike is (sum of the terms) / T in target_like's order."""
    T = 2.5
    r = _DRun(tmp_path, "r", FULL_W, 3, T, FULL_SEEDS, FULL_COV, FULL_STEPS + FAST_TAIL, derived=("dr12",))
    r.start()
    for _ in range(FULL_STEPS):
        r.s.step_theory(1)
    r.s.step(FAST_TAIL, fast_only=True)
    n = r.s.history_count()
    hist, terms = r.s.history_host(0, n), r.s.history_terms(0, n)
    assert n == FULL_STEPS + FAST_TAIL and terms.shape[1] == 2
    pts = np.ascontiguousarray(hist[:, :2, :].transpose(0, 2, 1).reshape(-1, 2))        # [n x W, 2]
    want = r.derived[0].eval(pts).cpu().numpy().reshape(n, FULL_W)
    assert np.array_equal(terms[:, 1, :], want)
    stay = hist[1:, 0, :] == hist[:-1, 0, :]
    assert np.any(stay) and np.any(~stay)
    assert np.array_equal(terms[1:, 1, :][stay], terms[:-1, 1, :][stay])
    assert np.any(hist[1:, 1, :][stay] != hist[:-1, 1, :][stay]), "no fast move between slow moves"
    assert np.array_equal(hist[:, 2, :], ((0.0 + terms[:, 0, :]) + terms[:, 1, :]) / T)
    assert np.all(want >= 0) and np.ptp(want) > 0        # (exactly 0 at the start point A = 1)
    r.close()


# ---------------------------------------------------------------- 9. calculator failure
@pytest.mark.parametrize("oversample", [1, 3])
def test_trial_outside_the_box_is_rejected(tmp_path, oversample):
    """test_calculator_failure_equals_out_of_bounds' configuration
    (Temperature 2.5, one step per call) with the DR12-sized derived row: the
    calculator's box TIGHT_A under wide sampler bounds against the sampler's
    bounds at TIGHT_A under a wide box.  A trial outside the box gets every
    row logZero and is rejected, so both runs have the same bits after every
    step, terms included, and A never leaves the box."""
    outs = []
    for tag, a_bounds, box in (("a", TIGHT_A, (0.5, 1.5)), ("b", WIDE, TIGHT_A)):
        r = _DRun(tmp_path, tag, FULL_W, oversample, 2.5, FULL_SEEDS, FULL_COV, FULL_STEPS, derived=("dr12",),
                  a_bounds=a_bounds, box=box)
        r.start()
        o = []
        for _ in range(FULL_STEPS):
            r.s.step_theory(1)
            o.append(r.outputs())
        r.close()
        outs.append(o)
    for k, (x, y) in enumerate(zip(*outs)):
        _same_chain(x, y, f"step {k}", terms=True)
    A = outs[1][-1][0][:, 0, :]
    assert A.min() >= TIGHT_A[0] and A.max() <= TIGHT_A[1]
    assert np.any(outs[1][-1][2][:, 0] != 1.0), "no slow move was accepted"
    assert np.all(outs[1][-1][1] < 1e29)


def test_derived_only_trial_outside_the_box(tmp_path):
    """No data likelihood: the box TIGHT_A alone keeps A inside it (the flags
    come from the derived row's own launch), as the sampler's bounds do."""
    outs = []
    for tag, a_bounds, box in (("a", TIGHT_A, (0.5, 1.5)), ("b", WIDE, TIGHT_A)):
        r = _DRun(tmp_path, tag, FULL_W, 1, 2.5, FULL_SEEDS, FULL_COV, FULL_STEPS, derived=("a", "dr12"), n_like=0,
                  a_bounds=a_bounds, box=box)
        r.start()
        r.s.step_theory(FULL_STEPS)
        outs.append(r.outputs())
        r.close()
    _same_chain(outs[0], outs[1], "derived only", terms=True)
    assert outs[1][1].shape[1] == 2 and np.any(outs[1][2][:, 0] != 1.0)


# ---------------------------------------------------------------- 10. checkpoint
def test_checkpoint_carries_the_rows(tmp_path):
    """20 steps, save_state, a new sampler of the same configuration,
    load_state (+ history_restore, refresh_theory from the calculator), 20
    steps: the bits of 40 steps straight, history_terms included.  An image
    from a sampler without derived rows is refused by one with them with the
    shape-mismatch error, and the other way round."""
    from cosmomc_amd._native import NativeError
    half = FULL_STEPS // 2
    kw = dict(derived=("a", "dr12"))
    full = _DRun(tmp_path, "f", FULL_W, 3, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS, **kw)
    full.start()
    full.s.step_theory(FULL_STEPS)
    want = full.outputs()
    full.close()
    a = _DRun(tmp_path, "a", FULL_W, 3, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS, **kw)
    a.start()
    a.s.step_theory(half)
    image, hist, terms = a.s.save_state(), a.s.history_host(0, half), a.s.history_terms(0, half)
    assert terms.shape[1] == 3
    a.close()
    b = _DRun(tmp_path, "b", FULL_W, 3, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS, **kw)
    b.s.load_state(image)
    b.s.history_restore(0, hist, terms)
    b.s.refresh_theory(None)
    b.s.step_theory(FULL_STEPS - half)
    got = b.outputs()
    _same_chain(want, got, "resumed", terms=True)
    assert np.any(want[2][:, 0] != 1.0)
    plain = _DRun(tmp_path, "p", FULL_W, 3, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS)
    plain.start()
    for s, img in ((plain.s, image), (b.s, plain.s.save_state())):
        with pytest.raises(NativeError, match="different sampler") as e:
            s.load_state(img)
        assert e.value.code == -1
    plain.close()
    b.close()


# ---------------------------------------------------------------- 11. chain file
def test_chain_file_has_the_chi2_columns(tmp_path):
    """ChainWriter with one (tag, "BAO", name, version) entry per derived row:
    in every written row chi2_<tag> is fortran_e(2 x term), chi2_prior is 2 x
    (like - sum of terms) and chi2_BAO the sum of the two BAO rows."""
    from cosmomc_amd.chains import ChainWriter, fortran_e
    r = _DRun(tmp_path, "r", FULL_W, 1, 1.0, FULL_SEEDS, FULL_COV, FULL_STEPS, derived=("a", "dr12"), prior_a=True)
    root = str(tmp_path / "chain")
    walkers = [0, 1, 41, 79]
    cw = ChainWriter(root, ["A", "cal"], ranges=[WIDE, TIGHT_CAL], walkers=walkers, burn_in=0,
                     likelihoods=[("plik", "CMB", "plik_lite", "v"), ("a", "BAO", "on A", "v"),
                                  ("dr12", "BAO", "DR12BAO", "v")])
    r.start()
    r.s.step_theory(FULL_STEPS)
    cw.append(r.s)
    hist, terms = r.s.history_host(0, FULL_STEPS), r.s.history_terms(0, FULL_STEPS)
    with open(root + ".paramnames") as f:
        assert [l.split("\t")[0] for l in f.read().splitlines()] == ["A", "cal", "chi2_plik*", "chi2_a*", "chi2_dr12*",
                                                                     "chi2_prior*", "chi2_BAO*"]
    n_rows = 0
    for w in walkers:
        starts = [t for t in range(FULL_STEPS) if t == 0 or not np.array_equal(hist[t, :, w], hist[t - 1, :, w])]
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        assert len(lines) == len(starts) - 2 and len(lines) >= 3, (w, len(lines), len(starts))
        for line, t in zip(lines, starts[1:]):
            f16 = [line[j:j + 16] for j in range(0, len(line), 16)]
            tr, like = terms[t, :, w], hist[t, 2, w]
            assert f16[4:7] == [fortran_e(2.0 * v, 16) for v in tr]
            assert f16[7] == fortran_e(2.0 * (like - tr.sum()), 16)
            assert f16[8] == fortran_e(2.0 * (tr[1] + tr[2]), 16)
            assert tr[1] > 0 and tr[2] >= 0 and 2.0 * (like - tr.sum()) > 0      # the prior on A is still a prior
        n_rows += len(lines)
    print(f"{n_rows} rows checked")
    r.close()


# ---------------------------------------------------------------- 12. refusals
def test_refusals(tmp_path):
    from cosmomc_amd._native import NativeError

    def bad(call, match):
        with pytest.raises(NativeError, match=match) as e:
            call()
        assert e.value.code == -1, e.value

    # no calculator set
    r = _DRun(tmp_path, "a", 64, 1, 1.0, FULL_SEEDS, FULL_COV, 4, derived=("a",), calc=False)
    bad(r.start, "calculator")
    r.s.set_theory_calculator(r.calc)
    r.start()
    r.s.set_theory_calculator(None)
    for call in (lambda: r.s.step_theory(1), lambda: r.s.step_drag(1), lambda: r.s.step(1, fast_only=True)):
        bad(call, "calculator")
    # another calculator than the object's
    other = _one_term(r.bh, (0.5, 1.5))
    r.s.set_theory_calculator(other)
    for call in (r.start, lambda: r.s.step_theory(1), lambda: r.s.step_drag(1), lambda: r.s.step(1, fast_only=True)):
        bad(call, "another calculator")
    r.s.set_theory_calculator(r.calc)
    r.s.step_theory(1)                                   # and with its own the run goes on
    # add_likelihood after add_derived_likelihood
    bad(lambda: r.s.add_likelihood(r.likes[0], r.theory[0]), "before derived")
    # a ninth row: one data likelihood and seven derived rows are there
    extra = [_on_a(r.calc, "zero") for _ in range(7)]
    for g in extra[:6]:
        r.s.add_derived_likelihood(g)
    bad(lambda: r.s.add_derived_likelihood(extra[6]), "at most 8")
    # slow proposals still need cmbs_step_theory
    bad(lambda: r.s.step(1, fast_only=False), "cmbs_step_theory")
    r.close()
    other.close()
    for g in extra:
        g.close()
