"""A tabulated derived likelihood (DerivedTable) as a term row of the sampler,
W = 64: beside a data likelihood and a Gaussian derived row, alone, against
DerivedTable.eval at the walkers' points, with a grid edge that rejects
trials, through the chain file, the checkpoint image and GPUEvaluator, and
the objects an ini equivalent to batch3/BAO.ini yields.  GPU only."""
import os

import numpy as np
import pytest

import bao_fixture as bf
from cosmomc_amd import synthetic as syn
from cosmomc_amd.derivedlike import DerivedGaussian, DerivedTable, derived_likelihoods_from_ini
from test_gpu_theory_calc import DRAG_COV, DRAG_SEEDS, FULL_COV, FULL_SEEDS, TIGHT_CAL, WIDE, _one_term

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
BAO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bao")
W, STEPS, FAST_TAIL = 64, 24, 6
# the table on the surface A: a chi^2 parabola about A = 1 in cells of 2^-12 on [0.997, 1.002]; proposals in A
# have a standard deviation near 0.005, so a good part of the slow trials leaves the grid
X_MIN, X_MAX, STEP = 0.997, 1.002, 2.0 ** -12
TABLE = ((X_MIN + STEP * np.arange(22) - 1.0) / 0.002) ** 2
OBS_A = 1.0 + 2.0 ** -10


def _table(calc, name="MGS"):
    return DerivedTable.table1d(calc, [[1.0]], TABLE, 1.0, X_MIN, X_MAX, STEP, name=name)


def _gauss(calc):
    return DerivedGaussian(calc, [[1.0]], [OBS_A], invcov=[[2.0 ** 16]], name="a")


class _Run:
    """test_gpu_derivedlike_sampler's A x base problem (synthetic plik_lite, A =
    P(1) slow, calPlanck = P(2) fast, the one-term calculator whose basis is A)
    with the derived rows `make` builds on the calculator; n_like = 0: no data
    likelihood."""

    def __init__(self, tmp_path, tag, make, n_like=1, oversample=3, T=1.0, seeds=FULL_SEEDS, cov=FULL_COV,
                 a_bounds=WIDE, capacity=STEPS + FAST_TAIL):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        from cosmomc_amd.sampler import BatchedMCMC
        self.bh = np.ascontiguousarray(syn.base_theory(2508)[:3])
        base = torch.tensor(self.bh, device="cuda")
        pmin, pmax = np.array([a_bounds[0], TIGHT_CAL[0]]), np.array([a_bounds[1], TIGHT_CAL[1]])
        self.s = BatchedMCMC(W, 2, [1, 2], [[1], [2]], 1, pmin, pmax, np.zeros(2), np.zeros(2),
                             oversample_fast=oversample, propose_scale=2.4, temperature=T, seed_ij=seeds[0],
                             seed_kl=seeds[1])
        self.s.set_covariance(cov)
        self.likes, self.theory, self.trial = [], [], []
        for i in range(n_like):
            like = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(str(tmp_path / f"{tag}{i}")))
            like.nuisance_indices = [2]
            self.likes.append(like)
            self.theory.append(base.unsqueeze(0).repeat(W, 1, 1).contiguous())
            self.trial.append(torch.empty_like(self.theory[0]))
            self.s.add_likelihood(like, self.theory[i])
            self.s.set_trial_theory(i, self.trial[i])
        self.s.enable_history(capacity)
        self.calc = _one_term(self.bh, (0.5, 1.5))
        self.s.set_theory_calculator(self.calc)
        self.derived = make(self.calc)
        for g in self.derived:
            self.s.add_derived_likelihood(g)

    def start(self):
        self.s.set_start(np.tile([1.0, 1.0], (W, 1)))

    def outputs(self):
        n = self.s.history_count()
        return (self.s.history_host(0, n), self.s.history_terms(0, n), *self.s.state())

    def close(self):
        self.s.close()
        for g in self.derived:
            g.close()
        self.calc.close()


def _points(hist):
    """history rows [n, n_used + 1, W] -> points [n W, 2]"""
    return np.ascontiguousarray(hist[:, :2, :].transpose(0, 2, 1).reshape(-1, 2))


# ---------------------------------------------------------------- 1. the row is eval at the row's point
@pytest.mark.parametrize("kind", ["theory", "drag"])
def test_table_row_beside_data_and_gaussian(tmp_path, kind):
    """Rows: plik_lite, a Gaussian on A, the table on A.  At the start point
    and in every history row of cmbs_step_theory / cmbs_step_drag the table's
    term is DerivedTable.eval at that row's point, bit for bit, and so is the
    Gaussian's; fast-only steps keep both; CurLike is the sum in target_like's
    order; no accepted point has a logZero term."""
    drag = kind == "drag"
    r = _Run(tmp_path, "r", lambda c: [_gauss(c), _table(c)], oversample=2 if drag else 3,
             seeds=DRAG_SEEDS if drag else FULL_SEEDS, cov=DRAG_COV if drag else FULL_COV)
    r.start()
    P0 = r.s.state()[0]
    assert np.all(P0[:, 0] == 1.0)
    start_term = r.derived[1].eval(np.ascontiguousarray(P0)).cpu().numpy()
    assert np.all(start_term == (TABLE[12] + TABLE[13]) / 2 / 2)         # A = 1: cell floor(0.003 / 2^-12) = 12
    for _ in range(STEPS):
        (r.s.step_drag if drag else r.s.step_theory)(1)
    r.s.step(FAST_TAIL, fast_only=True)
    hist, terms = r.outputs()[:2]
    n = STEPS + FAST_TAIL
    assert hist.shape[0] == n and terms.shape[1] == 3
    pts = _points(hist)
    for row, g in ((1, r.derived[0]), (2, r.derived[1])):
        want = g.eval(pts).cpu().numpy().reshape(n, W)
        assert np.array_equal(terms[:, row, :], want), row
    stayed = hist[0, 0, :] == 1.0                                        # not moved in the first step: the start term
    assert np.any(stayed) and np.all(terms[0, 2, stayed] == start_term[stayed])
    assert np.all(terms < 1e29) and np.ptp(terms[:, 2, :]) > 0
    assert hist[:, 0, :].min() >= X_MIN and hist[:, 0, :].max() <= X_MAX
    moved = np.any(hist[:, 0, :] != 1.0, axis=0)
    assert moved.sum() > W // 2, "few slow moves were accepted"
    assert np.array_equal(hist[:, 2, :], ((0.0 + terms[:, 0, :]) + terms[:, 1, :]) + terms[:, 2, :])
    # fast-only steps keep the derived terms while calPlanck moves
    tail = slice(STEPS - 1, n)
    assert np.all(terms[tail, 1:, :] == terms[STEPS - 1, 1:, :][None])
    assert np.any(hist[STEPS:, 1, :] != hist[STEPS - 1, 1, :][None])
    r.close()


# ---------------------------------------------------------------- 2. the grid's edge rejects, walker by walker
def test_trial_off_the_grid_is_rejected_for_that_walker(tmp_path):
    """Run a: wide sampler bounds on A, the table's grid [0.997, 1.002].  Run
    b: the same table and the sampler's bounds on A at the grid's ends.  A
    trial off the grid has the table's row logZero, so target_like is logZero
    (Temperature 1: the data term vanishes in 1e30) and the walker stays, as for
    a trial outside the bounds; a trial inside has the same terms in both.  So
    the runs have the same bits after every step, terms included, and the
    walkers' accept counts differ: each was judged alone."""
    outs = []
    for tag, a_bounds in (("a", WIDE), ("b", (X_MIN, X_MAX))):
        r = _Run(tmp_path, tag, lambda c: [_table(c)], a_bounds=a_bounds, capacity=STEPS)
        r.start()
        o = []
        for _ in range(STEPS):
            r.s.step_theory(1)
            o.append(r.outputs())
        r.close()
        outs.append(o)
    for k, (x, y) in enumerate(zip(*outs)):
        for name, u, v in zip(["history_host", "history_terms", "P", "CurLike", "mult", "num_accept"], x, y):
            assert np.array_equal(u, v), f"step {k}: {name} differ"
    hist, terms, P, _, _, nacc = outs[0][-1]
    assert hist[:, 0, :].min() >= X_MIN and hist[:, 0, :].max() <= X_MAX and np.all(terms < 1e29)
    assert np.any(P[:, 0] != 1.0) and len(set(nacc.tolist())) > 2
    # and the edge did bind: the free run (a table row with a grid that holds every trial) leaves [X_MIN, X_MAX]
    free = _Run(tmp_path, "f", lambda c: [DerivedTable.table1d(c, [[1.0]], np.zeros(1100), 1.0, 0.75, 1.25,
                                                               2.0 ** -11, name="flat")], capacity=STEPS)
    free.start()
    free.s.step_theory(STEPS)
    h = free.outputs()[0]
    free.close()
    assert h[:, 0, :].min() < X_MIN or h[:, 0, :].max() > X_MAX


# ---------------------------------------------------------------- 3. table rows alone
def test_sampler_with_table_rows_alone(tmp_path):
    """No data likelihood and no Gaussian: two table rows.  It steps
    (cmbs_step_theory and cmbs_step_drag), and the rows are eval at the points."""
    r = _Run(tmp_path, "r", lambda c: [_table(c), _table(c, "second")], n_like=0)
    r.start()
    r.s.step_theory(STEPS // 2)
    r.s.step_drag(STEPS // 2)
    hist, terms = r.outputs()[:2]
    assert terms.shape == (STEPS, 2, W)
    want = r.derived[0].eval(_points(hist)).cpu().numpy().reshape(STEPS, W)
    assert np.array_equal(terms[:, 0, :], want) and np.array_equal(terms[:, 1, :], want)
    assert np.array_equal(hist[:, 2, :], (0.0 + terms[:, 0, :]) + terms[:, 1, :])
    assert np.any(hist[-1, 0, :] != 1.0) and np.all(terms < 1e29)
    r.close()


# ---------------------------------------------------------------- 4. chain file, checkpoint, GPUEvaluator
def test_chain_file_has_the_chi2_column(tmp_path):
    from cosmomc_amd.chains import ChainWriter, fortran_e
    r = _Run(tmp_path, "r", lambda c: [_gauss(c), _table(c)], capacity=STEPS)
    root = str(tmp_path / "chain")
    walkers = [0, 17, 63]
    cw = ChainWriter(root, ["A", "cal"], ranges=[WIDE, TIGHT_CAL], walkers=walkers, burn_in=0,
                     likelihoods=[("plik", "CMB", "plik_lite", "v"), ("a", "BAO", "on A", "v"),
                                  ("MGS", "BAO", "MGS", "v")])
    r.start()
    r.s.step_theory(STEPS)
    cw.append(r.s)
    hist, terms = r.outputs()[:2]
    with open(root + ".paramnames") as f:
        assert [l.split("\t")[0] for l in f.read().splitlines()] == ["A", "cal", "chi2_plik*", "chi2_a*", "chi2_MGS*",
                                                                     "chi2_prior*", "chi2_BAO*"]
    n_rows = 0
    for w in walkers:
        starts = [t for t in range(STEPS) if t == 0 or not np.array_equal(hist[t, :, w], hist[t - 1, :, w])]
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        assert len(lines) == len(starts) - 2
        for line, t in zip(lines, starts[1:]):
            f16 = [line[j:j + 16] for j in range(0, len(line), 16)]
            assert f16[6] == fortran_e(2.0 * terms[t, 2, w], 16)
            assert f16[8] == fortran_e(2.0 * (terms[t, 1, w] + terms[t, 2, w]), 16)
        n_rows += len(lines)
    assert n_rows >= 3
    r.close()


def test_checkpoint_carries_the_row(tmp_path):
    """Half the steps, save_state, a new sampler, load_state (+
    history_restore, refresh_theory), the other half: the bits of the run
    straight through, the table's term row included."""
    half = STEPS // 2
    make = lambda c: [_gauss(c), _table(c)]                              # noqa: E731
    full = _Run(tmp_path, "f", make, capacity=STEPS)
    full.start()
    full.s.step_theory(STEPS)
    want = full.outputs()
    full.close()
    a = _Run(tmp_path, "a", make, capacity=STEPS)
    a.start()
    a.s.step_theory(half)
    image, hist, terms = a.s.save_state(), a.s.history_host(0, half), a.s.history_terms(0, half)
    a.close()
    b = _Run(tmp_path, "b", make, capacity=STEPS)
    b.s.load_state(image)
    b.s.history_restore(0, hist, terms)
    b.s.refresh_theory(None)
    b.s.step_theory(STEPS - half)
    got = b.outputs()
    b.close()
    for name, u, v in zip(["history_host", "history_terms", "P", "CurLike", "mult", "num_accept"], want, got):
        assert np.array_equal(u, v), name
    assert np.any(want[2][:, 0] != 1.0) and want[1].shape[1] == 3


def test_gpu_evaluator_scores_the_row(tmp_path):
    """GPUEvaluator (importance sampling's GetLogLikePost) on a sampler with a
    Gaussian and a table row: -lnL at listed rows is the sum of the two evals in
    target_like's order, and logZero off the grid."""
    from cosmomc_amd.importance import GPUEvaluator
    r = _Run(tmp_path, "r", lambda c: [_gauss(c), _table(c)], n_like=0)
    rng = np.random.default_rng(3)
    P = np.column_stack([rng.uniform(0.9965, 1.0025, 100), rng.uniform(0.998, 1.003, 100)])
    got = GPUEvaluator(r.s)(P)
    tg, tt = (g.eval(np.ascontiguousarray(P)).cpu().numpy() for g in r.derived)
    off = (P[:, 0] < X_MIN) | (P[:, 0] > X_MAX)
    assert off.sum() >= 5 and (~off).sum() >= 50
    assert np.all(tt[off] == LOGZERO) and np.all(got[off] >= 1e29)
    assert np.array_equal(got[~off], (0.0 + tg[~off]) + tt[~off])
    r.close()


# ---------------------------------------------------------------- 5. the objects of a batch3 BAO ini
def test_batch3_bao_ini_runs_in_the_sampler(tmp_path, tmp_path_factory):
    """An ini equivalent to batch3/BAO.ini (the DR12 consensus set by DEFAULT,
    6DF, MGS) yields a Gaussian, the MGS table and a Gaussian, named by tag;
    with surfaces linear in A (each dataset's own measurement x A) a sampler
    with them alone steps and writes chi2_6DF, chi2_MGS and chi2_DR12BAO, and
    the MGS row is the host restatement of BAO_MGS_loglike at v = 4.465666824 A."""
    from cosmomc_amd.chains import ChainWriter
    fx = bf.extract(tmp_path_factory.mktemp("bao_table_sampler"))
    (tmp_path / "DR12_BAO_consensus.ini").write_text(
        "use_BAO=T\nbao_dataset[DR12BAO] = %s\n" % os.path.join(BAO, "DR12", "sdss_DR12Consensus_bao.dataset"))
    (tmp_path / "BAO.ini").write_text("use_BAO=T\nDEFAULT(DR12_BAO_consensus.ini)\nbao_dataset[6DF] = %s\n"
                                      "bao_dataset[MGS] = %s\n" % (os.path.join(BAO, "sdss_6DF_bao.dataset"),
                                                                   os.path.join(fx, "sdss_MGS_bao.dataset")))
    dr12 = np.loadtxt(os.path.join(BAO, "DR12", "sdss_DR12Consensus_bao.dat"), usecols=(1,))
    surfaces = {"6DF": [[0.336]], "MGS": [4.465666824], "DR12BAO": dr12[None, :]}
    made = []

    def make(calc):
        made.extend(derived_likelihoods_from_ini(str(tmp_path / "BAO.ini"), calc, surfaces))
        return made

    r = _Run(tmp_path, "r", make, n_like=0, capacity=STEPS)
    assert [(type(g).__name__, g.name) for g in made] == [("DerivedGaussian", "6DF"), ("DerivedTable", "MGS"),
                                                         ("DerivedGaussian", "DR12BAO")]
    root = str(tmp_path / "chain")
    cw = ChainWriter(root, ["A", "cal"], ranges=[WIDE, TIGHT_CAL], walkers=[0, 1], burn_in=0,
                     likelihoods=[(g.name, "BAO", g.name, "v") for g in made])
    r.start()
    r.s.step_theory(STEPS)
    cw.append(r.s)
    with open(root + ".paramnames") as f:
        names = [l.split("\t")[0] for l in f.read().splitlines()]
    assert names[2:5] == ["chi2_6DF*", "chi2_MGS*", "chi2_DR12BAO*"]
    hist, terms = r.outputs()[:2]
    assert np.all(terms < 1e29) and np.any(hist[-1, 0, :] != 1.0)
    mgs = bf.read_all(fx)["MGS"]
    A = hist[:, 0, :].reshape(-1)
    want = np.array([bf.bao_table_loglike_host(mgs, np.float64(4.465666824) * a) for a in A])
    assert np.array_equal(terms[:, 1, :].reshape(-1), want)
    r.close()
