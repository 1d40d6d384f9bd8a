"""Weak lensing in the batched sampler (W = 64, the golden dataset syn_all):
fast steps on the WL nuisance block beside a PLIK_LITE likelihood, followed
decision by decision by a host chain on wl_loglike_host; the per-likelihood
change mask; a calculator per likelihood as the source of the theory row; the
checkpoint round trip; the chi2_WL column of the chain files.

P = (A, the 13 WL parameters, calPlanck): A scales every theory row (row = A x
base, D_l = A x base); DES_z0AI's counterpart WL_z0AI stays fixed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import wl_fixture as wf
from cosmomc_amd import synthetic as syn
from cosmomc_amd import theory as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyoracle as po  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W = 64
NSRC, NGAL = 3, 2
NN = 2 * (NSRC + NGAL) + 3
NP = NN + 2
FID = wf.fiducial(NSRC, NGAL)
P0 = np.concatenate([[1.0], FID, [1.0]])
#                  b           m            A    alpha  z0    DzL          DzS
SIG_WL = np.array([0.008] * 2 + [0.003] * 3 + [0.03, 0.05, 0.0] + [0.001] * 2 + [0.002] * 3)
SIG = np.concatenate([[3e-4], SIG_WL, [0.002]])
PMIN, PMAX = P0 - 20 * SIG, P0 + 20 * SIG
PMIN[0], PMAX[0] = 0.99, 1.01
WL_USED = [i + 2 for i in range(NN) if SIG_WL[i] > 0]      # 1-based into P: all but WL_z0AI
CAL = NP


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    return wf.extract(tmp_path_factory.mktemp("wl"), names=["syn_all"])["syn_all"]


@pytest.fixture(scope="module")
def rows(golden):
    """A theory row per walker [W, 1, n]: the golden's, its P entries scaled a little per walker."""
    r = np.tile(golden.row, (W, 1))
    r[:, 2 + 3 * len(golden.chis):] *= 1 + 0.01 * np.random.RandomState(3).standard_normal((W, 1))
    return np.ascontiguousarray(r[:, None, :])


def _wl(golden):
    from cosmomc_amd.weaklensing import WLLikelihood
    like = WLLikelihood(golden.dataset)
    like.nuisance_indices = list(range(2, 2 + NN))
    return like


def _plik(tmp_path):
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    like = NativeCMBLikelihood("PLIK_LITE", syn.make_plik_lite(12345).write(str(tmp_path)))
    like.nuisance_indices = [CAL]
    return like


def _sampler(used, blocks, slow_max, seeds=(61, 62)):
    from cosmomc_amd.sampler import BatchedMCMC
    pm, ps = np.zeros(NP), np.zeros(NP)
    pm[CAL - 1], ps[CAL - 1] = 1.0, 0.0025
    s = BatchedMCMC(W, NP, used, blocks, slow_max, PMIN, PMAX, pm, ps, seed_ij=seeds[0], seed_kl=seeds[1])
    s.set_covariance(np.diag(SIG[np.array(used) - 1] ** 2))
    return s


def _last_terms(s):
    return s.history_terms(s.history_count() - 1, 1)[0]


def _fast_run(golden, rows, tmp_path, groups, steps=24):
    wlk, plik = _wl(golden), _plik(tmp_path)
    dl = torch.tensor(rows, device="cuda")
    cmb = torch.tensor(syn.walker_theory(1, n_fields=3), device="cuda").expand(W, -1, -1)
    used = WL_USED + [CAL]
    n = len(WL_USED)
    s = _sampler(used, [list(range(1, n + 1)), [n + 1]], 0)
    s.set_groups(groups)
    s.add_likelihood(wlk, dl)
    s.add_likelihood(plik, cmb)
    s.enable_history(steps)
    s.set_start(np.tile(P0, (W, 1)))
    s.step(steps, fast_only=True)
    out = (s.history_host(0, steps), s.history_terms(0, steps), *s.state())
    s.close()
    return out, wlk, dl


def test_fast_steps_follow_host_chain(golden, rows, tmp_path):
    """Walkers 0, 31 and 63 against the C oracle's FastParameterSample chain
    (orc_mh_step) on a target of pyoracle.PlikLite + wl_loglike_host + the
    calPlanck prior: every accept decision, the point (rtol 1e-11) and CurLike
    (rel 1e-9) after every step; the WL term row is the likelihood evaluated
    directly at the final points, bit for bit."""
    from cosmomc_amd import weaklensing as wl
    from cosmomc_amd.sampler import walker_seed
    steps = 24
    (hist, terms, P, lk, mult, nacc), wlk, dl = _fast_run(golden, rows, tmp_path, 1, steps)
    direct = wlk.loglike_batch(dl, torch.tensor(np.ascontiguousarray(P[:, 1:1 + NN]), device="cuda")).cpu().numpy()
    assert np.array_equal(terms[-1, 0], direct)
    ds = wl.WLDataset(golden.dataset)
    plik = po.PlikLite(syn.make_plik_lite(12345))
    dlw = np.ascontiguousarray(syn.walker_theory(1, n_fields=3)[0])
    used = np.array(WL_USED + [CAL], dtype=np.int32)
    n = len(used)
    pm, ps = np.zeros(NP), np.zeros(NP)
    pm[CAL - 1], ps[CAL - 1] = 1.0, 0.0025
    keep = [np.ascontiguousarray(a) for a in (PMIN, PMAX, pm, ps)]
    n_acc = 0
    for w in (0, 31, 63):
        def wl_term(user, Pp, row=rows[w, 0]):
            return float(wl.wl_loglike_host(ds, row, np.array(Pp[1:1 + NN])))
        cb = po.EXTRA_LIKE_FN(wl_term)
        t = po.Target()
        t.num_params = NP
        t.pmin, t.pmax, t.prior_mean, t.prior_std = [a.ctypes.data for a in keep]
        t.temperature = 1.0
        t.plik, t.plik_nuis_index, t.plik_dl, t.plik_ld_field = plik.h, CAL, dlw.ctypes.data, dlw.shape[1]
        t.extra_like = C.cast(cb, C.c_void_p)
        h = po.lib().orc_proposer_create(2, np.array([n - 1, 1], dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), 0,
                                         1, 2.4, n, used)
        po.lib().orc_proposer_set_covariance(h, np.ascontiguousarray(np.diag(SIG[used - 1] ** 2)))
        r = po.Ranmar(*walker_seed(61, 62, w))
        Q = P0.copy()
        cur = C.c_double(po.lib().orc_target_loglike(C.byref(t), Q))
        for k in range(steps):
            prev = hist[k - 1, :n, w] if k else P0[used - 1]
            acc = po.lib().orc_mh_step(h, C.byref(r.s), C.byref(t), Q, C.byref(cur), 1, None)
            assert bool(acc) == (not np.array_equal(hist[k, :n, w], prev)), (w, k)
            n_acc += acc
            np.testing.assert_allclose(hist[k, :n, w], Q[used - 1], rtol=1e-11, atol=0, err_msg=f"walker {w} step {k}")
            assert hist[k, n, w] == pytest.approx(cur.value, rel=1e-9), (w, k)
        po.lib().orc_proposer_free(h)
    print("accepts of the three host chains:", n_acc, "of", 3 * steps)
    assert 5 <= n_acc <= 3 * steps - 5


def test_change_mask_skips_wl_when_only_cal_moved(golden, rows, tmp_path):
    """The WL block and calPlanck in two fast blocks: a walker re-evaluates only
    the likelihood whose block moved (WL on the compacted slots).  Two walker
    groups take the dense path: the same chains and terms bit for bit; and
    across a step that moved calPlanck alone the WL term keeps its bits."""
    a, _, _ = _fast_run(golden, rows, tmp_path / "a", 1)
    b, _, _ = _fast_run(golden, rows, tmp_path / "b", 2)
    assert a[5].sum() > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    hist, terms = a[0], a[1]
    n = len(WL_USED)
    cal_only = wl_moved = 0
    for k in range(1, hist.shape[0]):
        same_wl = np.all(hist[k, :n] == hist[k - 1, :n], axis=0)
        moved_cal = hist[k, n] != hist[k - 1, n]
        sel = same_wl & moved_cal
        assert np.array_equal(terms[k, 0, sel], terms[k - 1, 0, sel])
        assert np.all(terms[k, 1, sel] != terms[k - 1, 1, sel])
        cal_only += int(sel.sum())
        wl_moved += int(np.sum(~same_wl))
        assert np.all(terms[k, 0, ~same_wl] != terms[k - 1, 0, ~same_wl])
    assert cal_only > 20 and wl_moved > 20


def _row_calc(base, box):
    """row = A x base as a one-term surface in A = P(1): field 0, lmax = n - 1."""
    return th.PolynomialTheory([1], [0.0], [1.0], [box[0]], [box[1]], [[1]], [0], base[None, None, :])


def _calc_theory(calc, P, shape):
    out = torch.zeros(shape, dtype=torch.float64, device="cuda")
    calc.eval(P, out)
    return out


SLOW_USED = [1] + WL_USED


def _slow_blocks():
    return [[1], list(range(2, 2 + len(WL_USED)))]


def _wl_run(golden, mode):
    """WL alone, full steps: 'default' set_theory_calculator, 'override'
    set_like_calculator only, 'callback' a theory function."""
    like = _wl(golden)
    calc = _row_calc(golden.row, (0.99, 1.01))
    base = torch.tensor(golden.row, device="cuda").reshape(1, 1, -1)
    theory = base.repeat(W, 1, 1).contiguous()
    trial = torch.empty_like(theory)
    s = _sampler(SLOW_USED, _slow_blocks(), 1)
    s.add_likelihood(like, theory)
    s.set_trial_theory(0, trial)
    if mode == "default":
        s.set_theory_calculator(calc)
    elif mode == "override":
        s.set_like_calculator(0, calc)
    s.enable_history(8)
    s.set_start(np.tile(P0, (W, 1)))
    fn = (lambda P: trial.copy_(base * P[0].reshape(-1, 1, 1))) if mode == "callback" else None
    s.step_theory(8, theory_fn=fn)
    out = (s.history_host(0, 8), s.history_terms(0, 8), *s.state(), theory.cpu().numpy())
    s.close()
    return out


def test_like_calculator_is_the_single_calculator_path(golden):
    a, b, c = (_wl_run(golden, m) for m in ("default", "callback", "override"))
    assert a[5].sum() > 0
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_two_calculators(golden, tmp_path):
    """WL on its own calculator beside plik_lite on the sampler's: each term row
    is its likelihood alone on its own calculator's theory."""
    bh = np.ascontiguousarray(syn.base_theory(2508)[:3])
    wlk, plik = _wl(golden), _plik(tmp_path)
    box_wl, box_cmb = (1 - 3e-4, 1 + 9e-4), (1 - 9e-4, 1 + 3e-4)
    c_wl = _row_calc(golden.row, box_wl)
    c_cmb = th.PolynomialTheory([1], [0.0], [1.0], [box_cmb[0]], [box_cmb[1]], [[1]], [0, 1, 2], bh[None])
    t_wl = torch.tensor(golden.row, device="cuda").reshape(1, 1, -1).repeat(W, 1, 1).contiguous()
    t_cmb = torch.tensor(bh, device="cuda").unsqueeze(0).repeat(W, 1, 1).contiguous()
    e_wl, e_cmb = torch.empty_like(t_wl), torch.empty_like(t_cmb)
    n = len(WL_USED)
    s = _sampler(SLOW_USED + [CAL], _slow_blocks() + [[n + 2]], 1)
    s.add_likelihood(wlk, t_wl)
    s.add_likelihood(plik, t_cmb)
    s.set_trial_theory(0, e_wl)
    s.set_trial_theory(1, e_cmb)
    s.set_theory_calculator(c_cmb)
    s.set_like_calculator(0, c_wl)
    s.enable_history(12)
    s.set_start(np.tile(P0, (W, 1)))
    s.step_theory(12)
    P, lk, mult, nacc = s.state()
    hist = s.history_host(0, 12)
    assert np.any(P[:, 0] != 1.0)
    assert np.all((hist[:, 0] >= box_wl[0]) & (hist[:, 0] <= box_cmb[1]))      # inside both boxes
    want_wl, want_cmb = _calc_theory(c_wl, P, t_wl.shape), _calc_theory(c_cmb, P, t_cmb.shape)
    assert torch.equal(t_wl, want_wl) and torch.equal(t_cmb, want_cmb)
    terms = _last_terms(s)
    nu = torch.tensor(np.ascontiguousarray(P[:, 1:1 + NN]), device="cuda")
    cal = torch.tensor(np.ascontiguousarray(P[:, CAL - 1:CAL]), device="cuda")
    assert np.array_equal(terms[0], wlk.loglike_batch(want_wl, nu).cpu().numpy())
    assert np.array_equal(terms[1], plik.loglike_batch(want_cmb, cal).cpu().numpy())
    np.testing.assert_allclose(lk, terms[0] + terms[1] + (P[:, CAL - 1] - 1.0) ** 2 / (2 * 0.0025 ** 2), rtol=1e-12, atol=0)
    s.close()


def test_checkpoint_round_trip(golden):
    """save_state / load_state / refresh_theory with WL registered: the resumed
    run continues as the uninterrupted one."""
    calc = _row_calc(golden.row, (0.99, 1.01))
    base = torch.tensor(golden.row, device="cuda").reshape(1, 1, -1)

    def make():
        like = _wl(golden)
        theory = base.repeat(W, 1, 1).contiguous()
        trial = torch.empty_like(theory)
        s = _sampler(SLOW_USED, _slow_blocks(), 1)
        s.add_likelihood(like, theory)
        s.set_trial_theory(0, trial)
        s.set_theory_calculator(calc)
        return s, theory, (like, trial)

    a, ta, _ka = make()
    a.set_start(np.tile(P0, (W, 1)))
    a.step_theory(6)
    image = a.save_state()
    a.step_theory(6)
    want = (*a.state(), ta.cpu().numpy())
    b, tb, _kb = make()
    b.load_state(image)
    b.refresh_theory(None)
    b.step_theory(6)
    got = (*b.state(), tb.cpu().numpy())
    assert want[3].sum() > 0
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    a.close()
    b.close()


def test_chain_file_has_the_chi2_wl_column(golden, rows, tmp_path):
    """ChainWriter with the likelihood's own description: a chi2_WL column whose
    entries are fortran_e(2 x the WL term)."""
    from cosmomc_amd.chains import ChainWriter, fortran_e
    like = _wl(golden)
    assert like.description()[:2] == ("WL", "WL")
    dl = torch.tensor(rows, device="cuda")
    n = len(WL_USED)
    s = _sampler(WL_USED, [list(range(1, n + 1))], 0)
    s.add_likelihood(like, dl)
    s.enable_history(16)
    s.set_start(np.tile(P0, (W, 1)))
    root = str(tmp_path / "chain")
    names = [like.nuisance_names[i - 2] for i in WL_USED]
    cw = ChainWriter(root, names, walkers=[0, 63], burn_in=0, likelihoods=[like.description()])
    s.step(16, fast_only=True)
    cw.append(s)
    hist, terms = s.history_host(0, 16), s.history_terms(0, 16)
    with open(root + ".paramnames") as f:
        cols = [l.split("\t")[0] for l in f.read().splitlines()]
    assert cols == names + ["chi2_WL*", "chi2_prior*"]
    checked = 0
    for w in (0, 63):
        starts = [t for t in range(16) if t == 0 or not np.array_equal(hist[t, :, w], hist[t - 1, :, w])]
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        for line, t in zip(lines, starts[1:]):
            f16 = [line[j:j + 16] for j in range(0, len(line), 16)]
            assert f16[2 + n] == fortran_e(2.0 * terms[t, 0, w], 16)
            checked += 1
    assert checked >= 3
    s.close()
