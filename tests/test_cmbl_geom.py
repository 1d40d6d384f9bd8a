"""The CMBlikes window-geometry datasets (cosmomc_amd.synthetic.make_cmbl_geom)
on the CPU: the conditions under which test_gpu_cmbl_geom.py means something.

* the three references agree: CMBLikesOracle against the long-double
  restatement of cmbl_geom_fixture.py at a tenth of the GPU tolerance (all 67
  walkers of every gaussian case), and against the compiled reference
  (tests/golden/cmbl_geom_ref.json, oracle/gen_golden.py ``cmbl_geom``) at the
  GPU tolerance (every case, the first three walkers);
* every case has the property it is named for, read off the work items of
  cmblikes.hip build_items restated on the windows (cmbl_geom_fixture.items);
* every edge is visible: taking one window weight at an edge l as 0 -- the first
  and last l of every window, the l on either side of every segment boundary a
  window crosses -- or replacing the aberration end-point rule at l = lmin or at
  l = lmax by no derivative or by the central difference, moves the reference
  -lnL of every walker by at least 100 GPU tolerances.  A condition on the
  inputs, not on the kernel: a kernel that dropped that weight or that rule could
  not pass.  Weakest measured, as the least-moved of the 67 walkers: 871
  tolerances for a weight (smica_even_top) and 690 for an end-point rule
  (aber_full_even, no derivative at lmin); the HL cases use their first four
  walkers and CMBLikesOracle;
* the BK selections of test_gpu_cmbl_geom.py are what their names say.
"""
import numpy as np
import pytest

import cmbl_geom_fixture as cf
from cmbl_geom_fixture import cgeom  # noqa: F401  (session fixture)
from conftest import load_golden
from cosmomc_amd import synthetic as syn

GOLDEN = load_golden("cmbl_geom_ref.json")
W_HL_EDGES = 4                       # walkers of the HL edge test (each weight costs W oracle evaluations)


@cf.needs_longdouble
@pytest.mark.parametrize("case", cf.GAUSS_CASES)
def test_oracle_vs_longdouble(cgeom, case):
    ld = cgeom.reference(case)
    got = cgeom.oracle_batch(case)
    err = float(np.max(np.abs(got - ld.astype(np.float64)) / cf.tolerances(case, ld)))
    print(f"{case}: max |oracle - long double| = {err:.3g} tolerances")
    assert err <= 0.1


def test_reference_golden_covers_every_case():
    assert list(GOLDEN["cases"]) == cf.ALL_CASES and GOLDEN["walkers"] == cf.W_GOLDEN


@pytest.mark.parametrize("case", cf.ALL_CASES)
def test_oracle_vs_reference_golden(cgeom, case):
    W = GOLDEN["walkers"]
    got = cgeom.oracle_batch(case, cgeom.theory(case)[:W], cgeom.nuis(case)[:W])
    rtol, atol = cf.tol(case)
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, GOLDEN["cases"][case]["minus_lnL"], rtol=rtol, atol=atol)
    assert GOLDEN["cases"][case]["tag"] == syn.cmbl_geom_tag(case)


# ------------------------------------------------------------ named properties

def _items(name):
    return cf.items(syn.make_cmbl_geom(name))


def _rel_windows(d, p=0):
    return [(a - d.lmin, b - d.lmin) for a, b in d.bins[p]]


def test_full_range_cases():
    for name, lmax in (("full_even", 600), ("full_odd", 601), ("smica_even_top", 600), ("aber_full_odd", 601)):
        d, it = syn.make_cmbl_geom(name), _items(name)
        assert (d.lmin, d.lmax) == (2, lmax) and [i["seg"] for i in it] == [0, 1, 2]
        assert it[0]["l0"] == d.lmin and it[-1]["l1"] == d.lmax       # the first window starts at lmin, the last ends at lmax
        assert all(i["l0"] % 2 == 0 for i in it)                      # items_even: 16-byte theory loads
        assert d.windows[0].any() and d.windows[-1].any()
        assert d.bins[0][0][0] == d.lmin and d.bins[0][-1][1] == d.lmax
    # full_odd: a tight buffer (ld_field == lmax + 1) is even and keeps the vector path
    assert (601 + 1) % 2 == 0 and (600 + 1) % 2 == 1


def test_odd_lmin_17():
    d, it = syn.make_cmbl_geom("odd_lmin_17"), _items("odd_lmin_17")
    assert d.lmin == 17 and it[0]["l0"] == 17 and not it[0]["moved"]  # an odd first l that cannot move down: scalar loads
    assert len(it) == 2 and it[-1]["l1"] == d.lmax
    assert _items("aber_odd_lmin_17") == it


def test_seg_edges():
    d, it = syn.make_cmbl_geom("seg_edges"), _items("seg_edges")
    rel = _rel_windows(d)
    assert {255, 256, 257, 511, 512} <= {b for _, b in rel}                       # window ends around both boundaries
    assert (0, d.lmax - d.lmin) in rel                                            # one window over all three segments
    L = d.lmax - d.lmin
    assert {(0, 0), (255, 255), (256, 256), (511, 511), (512, 512), (L, L)} <= set(rel)   # one-l windows
    assert [i["seg"] for i in it] == [0, 1, 2] and [i["nch"] for i in it] == [4, 4, 1]
    # split dot products: windows that cross a boundary are columns of two or three items
    crossing = [sum(1 for c in range(0, L + 1, cf.SEG) if a <= min(L, c + cf.SEG - 1) and b >= c) for a, b in rel]
    assert sorted(set(crossing)) == [1, 2, 3] and [i["ncol"] for i in it] == [6, 7, 5]
    assert sum(i["ncol"] for i in it) == sum(crossing)
    for name in ("aber_seg_edges", "hl_seg_edges_two_maps"):
        assert [(i["l0"], i["l1"], i["ncol"]) for i in _items(name) if i["pair"] == 0] == \
            [(i["l0"], i["l1"], i["ncol"]) for i in it]
    assert len(_items("hl_seg_edges_two_maps")) == 9


def test_column_counts():
    assert [i["ncol"] for i in _items("cols_1_16_17")] == [1, 16, 17]             # one block, one full block, 16 + 1
    it = _items("cols_32_33")
    assert [(i["seg"], i["ncol"]) for i in it] == [(0, 32), (1, 32), (1, 1)]      # the 33rd column is an item of its own
    assert it[2]["l0"] < it[2]["l1"] == syn.make_cmbl_geom("cols_32_33").lmax
    assert syn.make_cmbl_geom("cols_32_33").nbin == 65                            # > 64 bandpowers: the quadratic-form path


def test_tails_mod4():
    it = _items("tails_mod4")
    assert sorted(i["len"] for i in it) == [1, 2, 3, 4, 31, 32, 65, 131, 222]
    assert {i["clen"] % 4 for i in it} == {0, 1, 2, 3}                            # nk = (clen + 3) / 4 on every residue
    assert {1, 31, 32} <= {i["sub"] for i in it}                                  # the direct kernel's last 32-l step
    assert {i["nch"] for i in it} == {1, 2, 3, 4} and 1 in {i["clen"] for i in it}
    assert all(i["l0"] % 2 == 0 and not i["moved"] for i in it)
    assert max(i["l1"] for i in it) == syn.make_cmbl_geom("tails_mod4").lmax == 644


def test_three_pairs():
    d, it = syn.make_cmbl_geom("three_pairs"), _items("three_pairs")
    assert d.pairs == ("TT", "TE", "EE") and [i["pair"] for i in it] == [0, 0, 1, 1, 2, 2]
    assert d.bins[0] != d.bins[1] != d.bins[2] != d.bins[0]
    first = {i["pair"]: i for i in reversed(it)}
    assert first[1]["moved"] and first[1]["l0"] == 4 and first[2]["moved"] and first[2]["l0"] == 2   # lo--
    assert all(i["l0"] % 2 == 0 for i in it)


def test_variants(cgeom):
    for case, (gname, approx, aber, smica) in syn.cmbl_geom_cases().items():
        o = cgeom.oracle(case)
        assert o.like_approx == {"HL": 1, "gaussian": 2}[approx] and o.smica == smica
        assert (o.aberration != 0) == aber and o.cal_index == (5 if smica else 0)
        assert (o.log_cal_prior > 0) == (not smica)
        assert o.nmaps == len(syn.cmbl_geom_geometries()[gname][2].split())
    assert cgeom.oracle("hl_full_even").nmaps == 1 and cgeom.oracle("hl_seg_edges_two_maps").nmaps == 2


@pytest.mark.parametrize("case", cf.ALL_CASES)
def test_windows_and_inputs(cgeom, case):
    d = cgeom.data(case)
    for p in range(len(d.pairs)):
        for b in range(d.nbin):
            w = d.windows[:, b, p]
            a, z = d.bins[p][b][0] - d.lmin, d.bins[p][b][1] - d.lmin
            assert not w[:a].any() and not w[z + 1:].any()
            w = w[a:z + 1]
            assert abs(w.sum() - 1) < 1e-14 and w.min() > 0 and w[0] >= w.max() / 3 - 1e-12 <= w[-1]
            assert np.unique(w).size == w.size                        # no two l weigh the same
    for p in range(len(d.pairs)):
        for q in range(p + 1, len(d.pairs)):
            wa, wb = d.windows[:, :, p], d.windows[:, :, q]
            assert not np.any((wa == wb) & (wa != 0) & (wa != 1))     # every spectrum has weights of its own
    np.linalg.cholesky(d.cov)
    P, th = cgeom.nuis(case), cgeom.theory(case)
    assert np.unique(P, axis=0).shape[0] == cf.W_ALL and np.all(P[:, -1] != 1)
    assert th.shape == (cf.W_ALL, 3, d.lmax + 1) and np.all(th[:, :, d.lmin:] != 0)
    ref = cgeom.reference(case) if (cf.HAVE_LONGDOUBLE or case in cf.HL_CASES) else cgeom.oracle_batch(case)
    assert np.all(np.isfinite(ref.astype(np.float64))) and np.unique(ref).size == cf.W_ALL


def test_bk_selections(refdata):
    """The bins each selection keeps, the lform switch, and for cl_lmin = 3 a first
    window that starts on the odd lmin: its grouped item starts at lmin - 1."""
    bk = cf.BKSelections(refdata)
    for name in cf.BK_CASES:
        o = bk.oracle(name)
        sel = name.split("-")[0]
        want = {"first_bin": [1], "last_bin": [9]}.get(sel.split("_", 1)[1], list(range(1, 10)))
        assert o.bins == want and o.like_approx == 1 and o.aberration == 0 and o.nmaps in (3, 4)
        assert (o.lform_dust, o.lform_sync) == (("lin", "quad") if name.endswith("lin_quad") else ("flat", "flat"))
        first = min(int(np.nonzero(o.W_main["W"][b].any(axis=0))[0][0]) for b in o.bins) + o.lmin
        assert o.lmin == (3 if "lmin3" in sel else 2)
        if "lmin3" in sel:
            assert first == 3 and (first & ~1) == o.lmin - 1
        th, P = cf.bk_inputs(name, 4)
        assert np.all(np.abs(P[:, 10:12] - 1) > 1e-5)                 # decorrelation is on
        assert np.all(np.isfinite([o.loglike(th[w], P[w]) for w in range(4)]))


# ------------------------------------------------------------ every edge is visible

@cf.needs_longdouble
@pytest.mark.parametrize("case", cf.GAUSS_CASES)
def test_every_edge_weight_moves_every_walker(cgeom, case):
    o, L, P = cgeom.oracle(case), cgeom.chol(case), cgeom.nuis(case)
    ref = cgeom.reference(case)
    mc = cf.map_cls_ld(o, cgeom.theory(case), P)
    worst = np.inf
    es = cf.edges(cgeom.data(case))
    assert len(es) >= 2 * cgeom.data(case).nbin
    for b, p, l in es:
        assert o.W_main["W"][b + 1][p][l - o.lmin] != 0
        moved = np.abs(cf.gauss_ld(o, L, mc, P, zero=(b + 1, p, l)) - ref).astype(np.float64) / cf.tolerances(case, ref)
        worst = min(worst, float(moved.min()))
        assert moved.min() >= 100, (case, b, p, l, int(np.argmin(moved)))
    print(f"{case}: {len(es)} edge weights, the weakest moves -lnL by {worst:.3g} tolerances")


@pytest.mark.parametrize("case", cf.HL_CASES)
def test_every_edge_weight_moves_every_walker_hl(cgeom, case):
    """The same against CMBLikesOracle, on the first W_HL_EDGES walkers."""
    o = cgeom.oracle(case)
    th, P = cgeom.theory(case)[:W_HL_EDGES], cgeom.nuis(case)[:W_HL_EDGES]
    ref = cgeom.oracle_batch(case, th, P)
    worst = np.inf
    es = cf.edges(cgeom.data(case))
    for b, p, l in es:
        row = o.W_main["W"][b + 1][p]
        keep = row[l - o.lmin]
        assert keep != 0
        row[l - o.lmin] = 0.0
        try:
            with np.errstate(invalid="ignore"):
                got = cgeom.oracle_batch(case, th, P)
        finally:
            row[l - o.lmin] = keep
        # a one-l TT or EE window without its weight leaves the bin's matrix indefinite: NaN, which no
        # finite kernel result matches
        moved = np.where(np.isnan(got), np.inf, np.abs(got - ref) / cf.tolerances(case, ref))
        worst = min(worst, float(moved.min()))
        assert moved.min() >= 100, (case, b, p, l)
    assert np.array_equal(cgeom.oracle_batch(case, th, P), ref)
    print(f"{case}: {len(es)} edge weights, the weakest moves -lnL by {worst:.3g} tolerances")


@cf.needs_longdouble
@pytest.mark.parametrize("case", cf.ABER_CASES)
def test_aberration_end_rules_move_every_walker(cgeom, case):
    o, L, P = cgeom.oracle(case), cgeom.chol(case), cgeom.nuis(case)
    d = cgeom.data(case)
    assert d.windows[0].any() and d.windows[-1].any()                 # lmin and lmax carry window weight
    ref = cgeom.reference(case)
    for ends in (("zero", "rule"), ("central", "rule"), ("rule", "zero"), ("rule", "central")):
        got = cf.gauss_ld(o, L, cf.map_cls_ld(o, cgeom.theory(case), P, ends=ends), P)
        moved = np.abs(got - ref).astype(np.float64) / cf.tolerances(case, ref)
        print(f"{case} ends={ends}: moves -lnL by {float(moved.min()):.3g} .. {float(moved.max()):.3g} tolerances")
        assert moved.min() >= 100, (case, ends, int(np.argmin(moved)))
