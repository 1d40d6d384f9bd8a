"""The SPTpol window-geometry datasets (cosmomc_amd.synthetic.make_sptpol_geom)
on the CPU: the conditions under which test_gpu_sptpol_geometry.py means
something.

* the numpy oracle against the long-double restatement of sptpol_fixture.py at
  1e-11 relative, a tenth of the GPU tolerance (measured maximum over every
  case, both switch settings and all 67 walkers: 1.3e-14);
* the oracle against the compiled reference (tests/golden/sptpol_geom_ref.json,
  oracle/gen_golden.py ``sptpol``) at the GPU tolerance;
* sensitivity: zeroing the theory at one of the l a case was built to reach
  moves the long-double -lnL of every walker by at least 1e4 GPU tolerances,
  so a kernel that misread that l could not pass (weakest: zero_group without
  aberration, l = lmax + 1, 1.4e4);
* the work items SPTpol::finish cuts the windows into, restated on the windows.
"""
import numpy as np
import pytest

import sptpol_fixture as sf
from conftest import load_golden
from cosmomc_amd import synthetic as syn
from sptpol_fixture import geom  # noqa: F401  (session fixture)

GOLDEN = load_golden("sptpol_geom_ref.json")
SWITCH = [False, True]


def _tol(ref):
    return sf.RTOL * np.abs(ref) + sf.ATOL


@sf.needs_longdouble
@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", sf.ALL_CASES)
def test_oracle_vs_longdouble(geom, case, on):
    ld = geom.longdouble(case, on)
    got = geom.oracle(case, on).loglike_batch(geom.theory(case), geom.nuis(case))
    rel = float(np.max(np.abs((got - ld) / ld)))
    print(f"{case} on={on}: max |oracle - long double| / |long double| = {rel:.2e}")
    assert rel <= 1e-11


@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", list(GOLDEN["cases"]))
def test_oracle_vs_reference_golden(geom, case, on):
    W = GOLDEN["walkers"]
    got = geom.oracle(case, on).loglike_batch(geom.theory(case)[:W], geom.nuis(case)[:W])
    np.testing.assert_allclose(got, GOLDEN["cases"][case]["on" if on else "off"], rtol=sf.RTOL, atol=sf.ATOL)


def test_reference_golden_covers_the_named_cases():
    named = ["lmin2", "odd_lmin_17", "len257", "zero_group", "nine_rows", "bb_odd", "bb_zero_band",
             "edge_sweep_31_200"]
    assert set(named) <= set(GOLDEN["cases"]) <= set(sf.ALL_CASES)


@sf.needs_longdouble
@pytest.mark.parametrize("on", SWITCH)
@pytest.mark.parametrize("case", [c for c in sf.ALL_CASES if c != "all_zero"])
def test_reached_entries_move_every_walker(geom, case, on):
    """Theory = 0 at one reached l (in TE and EE, or in BB) moves -lnL of every
    walker by >= 1e4 * (1e-10 |lnL| + 1e-8).  The BB walker with Abb == 0 has
    its theory multiplied by 0 and must not move at all."""
    ld = geom.longdouble(case, on)
    bb = sf.tag_of(case) == "SPTPOL_BB"
    fields = [5] if bb else [1, 2]
    entries = sf.reach(case)
    assert len(entries) == (2 if bb else 4)
    for l in entries:
        th = geom.theory(case).copy()
        assert np.all(th[:, fields, l] != 0)
        th[:, fields, l] = 0
        moved = np.abs(geom.longdouble(case, on, dl=th) - ld) / _tol(ld)
        if bb:
            assert geom.nuis(case)[1, 0] == 0 and moved[1] == 0
            moved = np.delete(moved, 1)
        print(f"{case} on={on} l={l}: moves by {float(moved.min()):.3g} .. {float(moved.max()):.3g} tolerances")
        assert moved.min() >= 1e4, (case, on, l, int(np.argmin(moved)))


@sf.needs_longdouble
@pytest.mark.parametrize("on", SWITCH)
def test_all_zero_ignores_the_theory(geom, on):
    """No window at all: -lnL = log det + spec . C^-1 spec / 2 + priors, whatever the theory."""
    case = "all_zero"
    ld = geom.longdouble(case, on)
    assert np.array_equal(ld, geom.longdouble(case, on, dl=np.zeros_like(geom.theory(case))))
    o, P = geom.oracle(case, on), geom.nuis(case).astype(sf.LD)
    spec = np.concatenate([o.spec[0], o.spec[1]]).astype(sf.LD)
    base = sf.gauss_loglike_ld(geom.chol(case), -spec[None, :])[0]
    pri = np.sum(P[:, 9:11] ** 2, axis=1) / 2
    pri = pri + (np.log(P[:, 7] / sf.LD(o.meanTcal)) / sf.LD(o.sigmaTcal)) ** 2 / 2
    pri = pri + (np.log(P[:, 8] / sf.LD(o.meanPcal)) / sf.LD(o.sigmaPcal)) ** 2 / 2
    pri = pri + ((P[:, 0] - sf.LD(o.meankappa)) / sf.LD(o.sigmakappa)) ** 2 / 2
    pri = pri + ((P[:, 4] - sf.LD(o.meanAlphaTE)) / sf.LD(o.sigmaAlphaTE)) ** 2 / 2
    pri = pri + ((P[:, 6] - sf.LD(o.meanAlphaEE)) / sf.LD(o.sigmaAlphaEE)) ** 2 / 2
    assert o.Tcal_prior and o.Pcal_prior and o.kappa_prior and o.aTE_prior and o.aEE_prior
    np.testing.assert_allclose((ld - (base + pri)).astype(float), 0, atol=1e-15 * float(np.max(np.abs(ld))))


def _items(case):
    d = syn.make_sptpol_geom(case)
    return sf.items(d.windows, d.lmin, 2 if sf.tag_of(case) == "SPTPOL_TEEE" else 3)


def test_item_layout():
    per_band = lambda case, k: [it for it in _items(case) if it[0] == k]       # noqa: E731
    for k in (0, 1):
        assert [it[2:] for it in per_band("len256", k)] == [(40, 256)]
        assert [it[2:] for it in per_band("len257", k)] == [(40, 256), (296, 1)]
        assert [it[2:] for it in per_band("nine_rows", k)] == [(4 + 256 * i, 256) for i in range(8)] + [(2052, 1)]
        assert per_band("odd_lmin_17", k)[0][2] == 50                 # lmin - 1: the item starts in the halo
        assert [it[1] for it in per_band("odd_lmin_17", k)] == [0, 0, 16]
        assert [it[2] for it in per_band("lmin2", k)] == [2, 258]
    assert [it[1] for it in per_band("zero_group", 0)] == [16, 32]    # no item for TE columns 0..15
    assert [it[1] for it in per_band("zero_group", 1)] == [0, 16, 32]
    assert _items("all_zero") == []
    assert {it[1] for it in _items("disjoint")} == {0, 16} and max(it[3] for it in _items("disjoint")) == 256
    assert [it[0] for it in _items("bb_zero_band")] == [0, 0, 2, 2]   # the 95x150 band has no item
    assert {it[1] for it in _items("bb_17")} == {0, 16}
    assert _items("bb_odd")[0][2] == 50
    # edge_sweep: l0 = 30 for both lmin, and every residue of (lmax + 1 - l0) mod 8
    sweep = [c for c in sf.TEEE_CASES if c.startswith("edge_sweep")]
    assert len(sweep) == 16 and all(_items(c)[0][2] == 30 for c in sweep)
    assert {(syn.make_sptpol_geom(c).lmax + 1 - 30) % 8 for c in sweep} == set(range(8))


@pytest.mark.parametrize("case", sf.ALL_CASES)
def test_windows_and_inputs(case):
    d = syn.make_sptpol_geom(case)
    nband = 2 if sf.tag_of(case) == "SPTPOL_TEEE" else 3
    nb = d.nbin
    win = d.windows
    for c in range(win.shape[1]):
        sup = np.nonzero(win[:, c])[0]
        if sup.size == 0:
            assert d.spec[c // nb, c % nb] != 0                       # a zero window still has data
            continue
        w = win[sup[0]:sup[-1] + 1, c]
        assert abs(w.sum() - 1) < 1e-14 and w.min() > 0
        assert 1 / 3 - 1e-12 <= w[0] / w.max() and 1 / 3 - 1e-12 <= w[-1] / w.max()   # (0.5 + u) / max: full weight at both ends
        assert np.unique(w).size == w.size                            # no two l weigh the same
    for a in range(nband):
        for b in range(a + 1, nband):
            wa, wb = win[:, a * nb:(a + 1) * nb], win[:, b * nb:(b + 1) * nb]
            assert not np.any((wa == wb) & (wa != 0) & (wa != 1))     # every band has weights of its own (a one-l bin: 1)
    P = syn.sptpol_geom_nuisance(case, sf.W_ALL)
    assert np.unique(P, axis=0).shape[0] == sf.W_ALL
    if nband == 2:
        assert np.all(np.abs(P[:, 0] - 0.02) < 0.01) and np.all(P[:, 7:9] != 1)
        assert np.all(P[:, [3, 5]] != 0) and np.all(P[:, 9:11] != 0)
    else:
        assert P[0, 0] == 1 and P[1, 0] == 0 and np.all(P[2:, 0] != 1) and np.all(P[2:, 0] != 0)
        assert np.all(P[:, 7:9] != 1) and np.all(P[:, 3] != 0) and np.all(P[:, 9:16] != 0)
        assert d.r_template[d.lmin] != 0 and d.r_template[d.lmax] != 0
        assert d.nbin >= 7
