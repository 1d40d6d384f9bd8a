"""SZ cluster counts in the batched sampler (W = 64, the golden data set
syn_inside): full steps with a calculator serving the theory row, the term row
and the chi2_SZ chain column against the likelihood re-evaluated at the stored
parameters, the checkpoint round trip, and fast steps beside a PLIK_LITE
likelihood whose calibration moves alone.

P = (A, the 5 SZ parameters, calPlanck): A scales every theory row (row = A x
base, D_l = A x base); beta_SZ stays fixed as in batch2/SZ_plus_CMB.ini."""
import numpy as np
import pytest

import sz_fixture as sf
from cosmomc_amd import synthetic as syn
from cosmomc_amd import theory as th

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W = 64
NN = 5
NP = NN + 2
P0 = np.concatenate([[1.0], sf.CENTRE, [1.0]])
#                  alpha  ystar  bias   scatter beta
SIG_SZ = np.array([0.02, 0.004, 0.02, 0.002, 0.0])
SIG = np.concatenate([[3e-4], SIG_SZ, [0.002]])
PMIN, PMAX = P0 - 20 * SIG, P0 + 20 * SIG
PMIN[0], PMAX[0] = 0.99, 1.01
SZ_USED = [i + 2 for i in range(NN) if SIG_SZ[i] > 0]      # 1-based into P: all but beta_SZ
CAL = NP
SLOW_USED = [1] + SZ_USED


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    return sf.extract(tmp_path_factory.mktemp("sz"), names=["syn_inside"])["syn_inside"]


@pytest.fixture(scope="module")
def rows(golden):
    """A theory row per walker [W, 1, n]: the golden's, its grid scaled a little per walker."""
    r = np.tile(golden.row, (W, 1))
    r[:, 3 + 2 * golden.nzs:] *= 1 + 0.01 * np.random.RandomState(3).standard_normal((W, 1))
    return np.ascontiguousarray(r[:, None, :])


def _sz(golden):
    from cosmomc_amd.szcounts import SZLikelihood
    like = SZLikelihood(golden.ini)
    like.nuisance_indices = list(range(2, 2 + NN))
    return like


def _plik(tmp_path):
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    like = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(str(tmp_path)))
    like.nuisance_indices = [CAL]
    return like


def _sampler(used, blocks, slow_max, seeds=(71, 72)):
    from cosmomc_amd.sampler import BatchedMCMC
    pm, ps = np.zeros(NP), np.zeros(NP)
    pm[CAL - 1], ps[CAL - 1] = 1.0, 0.0025
    s = BatchedMCMC(W, NP, used, blocks, slow_max, PMIN, PMAX, pm, ps, seed_ij=seeds[0], seed_kl=seeds[1])
    s.set_covariance(np.diag(SIG[np.array(used) - 1] ** 2))
    return s


def _row_calc(base, box):
    """row = A x base as a one-term surface in A = P(1): field 0, lmax = n - 1."""
    return th.PolynomialTheory([1], [0.0], [1.0], [box[0]], [box[1]], [[1]], [0], base[None, None, :])


def _slow_blocks():
    return [[1], list(range(2, 2 + len(SZ_USED)))]


def _make(golden):
    like = _sz(golden)
    calc = _row_calc(golden.row, (0.99, 1.01))
    theory = torch.tensor(golden.row, device="cuda").reshape(1, 1, -1).repeat(W, 1, 1).contiguous()
    trial = torch.empty_like(theory)
    s = _sampler(SLOW_USED, _slow_blocks(), 1)
    s.add_likelihood(like, theory)
    s.set_trial_theory(0, trial)
    s.set_like_calculator(0, calc)
    return s, theory, calc, (like, trial)


def test_term_row_and_chi2_column_are_the_likelihood_at_the_stored_point(golden, tmp_path):
    """Full steps on a calculator's row: the theory the sampler holds is the
    calculator's at the stored parameters, the term row is the likelihood
    evaluated directly on it, bit for bit, CurLike is that term, and the chain
    file's chi2_SZ column is fortran_e(2 x the term)."""
    from cosmomc_amd.chains import ChainWriter, fortran_e
    s, theory, calc, (like, _) = _make(golden)
    assert like.description()[:2] == ("SZ", "SZ")
    steps = 12
    s.enable_history(steps)
    s.set_start(np.tile(P0, (W, 1)))
    root = str(tmp_path / "chain")
    names = ["A"] + [like.nuisance_names[i - 2] for i in SZ_USED]
    cw = ChainWriter(root, names, walkers=[0, 63], burn_in=0, likelihoods=[like.description()])
    s.step_theory(steps)
    cw.append(s)
    P, lk, mult, nacc = s.state()
    assert nacc.sum() > 0 and np.any(P[:, 0] != 1.0) and np.any(P[:, 1:5] != P0[1:5])
    want = torch.zeros_like(theory)
    calc.eval(P, want)
    assert torch.equal(theory, want)
    nu = torch.tensor(np.ascontiguousarray(P[:, 1:1 + NN]), device="cuda")
    direct = like.loglike_batch(want, nu).cpu().numpy()
    terms = s.history_terms(0, steps)
    hist = s.history_host(0, steps)
    assert np.array_equal(terms[-1, 0], direct)
    np.testing.assert_allclose(lk, direct, rtol=1e-12, atol=0)
    with open(root + ".paramnames") as f:
        cols = [ln.split("\t")[0] for ln in f.read().splitlines()]
    assert cols == names + ["chi2_SZ*", "chi2_prior*"]
    n = len(names)
    checked = 0
    for w in (0, 63):
        starts = [t for t in range(steps) if t == 0 or not np.array_equal(hist[t, :, w], hist[t - 1, :, w])]
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        for line, t in zip(lines, starts[1:]):
            f16 = [line[j:j + 16] for j in range(0, len(line), 16)]
            assert f16[2 + n] == fortran_e(2.0 * terms[t, 0, w], 16)
            checked += 1
    assert checked >= 2
    s.close()


def test_checkpoint_round_trip(golden):
    """save_state / load_state / refresh_theory with SZ registered: the resumed
    run continues as the uninterrupted one."""
    a, ta, _, _ka = _make(golden)
    a.set_start(np.tile(P0, (W, 1)))
    a.step_theory(5)
    image = a.save_state()
    a.step_theory(5)
    want = (*a.state(), ta.cpu().numpy())
    b, tb, _, _kb = _make(golden)
    b.load_state(image)
    b.refresh_theory(None)
    b.step_theory(5)
    got = (*b.state(), tb.cpu().numpy())
    assert want[3].sum() > 0
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    a.close()
    b.close()


def _fast_run(golden, rows, tmp_path, groups, steps=20):
    szl, plik = _sz(golden), _plik(tmp_path)
    dl = torch.tensor(rows, device="cuda")
    cmb = torch.tensor(syn.walker_theory(1, n_fields=3), device="cuda").expand(W, -1, -1)
    used = SZ_USED + [CAL]
    n = len(SZ_USED)
    s = _sampler(used, [list(range(1, n + 1)), [n + 1]], 0)
    s.set_groups(groups)
    s.add_likelihood(szl, dl)
    s.add_likelihood(plik, cmb)
    s.enable_history(steps)
    s.set_start(np.tile(P0, (W, 1)))
    s.step(steps, fast_only=True)
    out = (s.history_host(0, steps), s.history_terms(0, steps), *s.state())
    s.close()
    return out, szl, dl


def test_fast_step_that_moves_no_sz_parameter_keeps_the_term(golden, rows, tmp_path):
    """The SZ block and calPlanck in two fast blocks: a walker re-evaluates only
    the likelihood whose block moved (SZ on the compacted slots).  Two walker
    groups take the dense path: the same chains and terms bit for bit; across a
    step that moved calPlanck alone the SZ term keeps its bits; and the last
    term row is the likelihood evaluated directly at the final points."""
    a, szl, dl = _fast_run(golden, rows, tmp_path / "a", 1)
    b, _, _ = _fast_run(golden, rows, tmp_path / "b", 2)
    assert a[5].sum() > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    hist, terms, P = a[0], a[1], a[2]
    direct = szl.loglike_batch(dl, torch.tensor(np.ascontiguousarray(P[:, 1:1 + NN]), device="cuda")).cpu().numpy()
    assert np.array_equal(terms[-1, 0], direct)
    n = len(SZ_USED)
    cal_only = sz_moved = 0
    for k in range(1, hist.shape[0]):
        same_sz = np.all(hist[k, :n] == hist[k - 1, :n], axis=0)
        moved_cal = hist[k, n] != hist[k - 1, n]
        sel = same_sz & moved_cal
        assert np.array_equal(terms[k, 0, sel], terms[k - 1, 0, sel])
        assert np.all(terms[k, 1, sel] != terms[k - 1, 1, sel])
        cal_only += int(sel.sum())
        sz_moved += int(np.sum(~same_sz))
        assert np.all(terms[k, 0, ~same_sz] != terms[k - 1, 0, ~same_sz])
    assert cal_only > 20 and sz_moved > 20
