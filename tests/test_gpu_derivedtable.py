"""Tabulated likelihoods on calculator-derived quantities (cmbg_create_table,
cosmomc_amd.derivedlike.DerivedTable) on the GPU against the compiled
reference's -lnL (tests/golden/bao/bao_table.tar.xz): the MGS chi^2 table and
the probability grids at 3, 4, 40 and 280 knots at their edges, the batch
shapes and the argument errors.  GPU only.

The calculator has two inputs (centre 0, scale 1) and its surfaces are the
inputs themselves, so v equals the parameter bit for bit and a point names an
exact alpha.

Tolerance (the rule of the weak-lensing goldens): measured on the host per
dataset, (a) the f64 restatement against the goldens and (b) f64 against long
double; the device must meet the goldens to 10 x the larger, absolute on -lnL.
A logZero outcome must be the golden's, with no tolerance."""
import ctypes as C

import numpy as np
import pytest

import bao_fixture as bf
from cosmomc_amd import theory as th
from cosmomc_amd.derivedlike import DerivedTable

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOGZERO = 1e30
TD_TM = 256                                            # theory_table_kernel's points per workgroup
BOX = 1e6
NPAR = 3                                               # P(1), P(3) are the inputs; P(2) is not read
MGS_COL = np.array([1.0, 0.0])
GRID_COLS = np.array([[1.0, 0.0], [0.0, 1.0]])


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return bf.extract(tmp_path_factory.mktemp("bao_table_gpu"))


@pytest.fixture(scope="module")
def calc():
    c = th.PolynomialTheory([1, 3], [0.0, 0.0], [1.0, 1.0], [-BOX, -BOX], [BOX, BOX], [[1, 0], [0, 1]], [0],
                            np.zeros((2, 1, 1)))
    yield c
    c.close()


def _make(calc, d):
    if d["kind"] == "mgs":
        return DerivedTable.mgs(calc, MGS_COL, d["table"], name=d["name"])
    return DerivedTable.grid(calc, GRID_COLS, d["perp"], d["plel"], d["prob"], d["DA_rd_fid"], d["Hrd_fid"],
                             name=d["name"])


def _rows(v0, v1):
    """P [NPAR, M] with v0 in P(1) and v1 in P(3)"""
    P = np.full((NPAR, len(v0)), 0.25)
    P[0], P[2] = v0, v1
    return P


def _eval(g, P, M, ld=None, pad=3):
    """g.eval at P[:, :M] (row stride ld) into the [M] corner of NaN-filled
    (out) and -7-filled (fail) buffers: (out, fail, the whole buffers)"""
    Pd = torch.tensor(np.ascontiguousarray(P[:, :ld if ld else P.shape[1]]), device="cuda")[:, :M]
    full = torch.full((M + pad,), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((M + pad,), -7, dtype=torch.int32, device="cuda")
    ret = g.eval(Pd, out=full[:M], fail=fl[:M])
    assert ret.data_ptr() == full.data_ptr()
    return full[:M].cpu().numpy(), fl[:M].cpu().numpy(), full.cpu().numpy(), fl.cpu().numpy()


def _case_points(cases, kind):
    v = [bf.surfaces_of(c["DV"], c["DA"], c["H"], c["rd"], kind) for c in cases]
    return np.array([x[0] for x in v]), np.array([0.5 if x[1] is None else x[1] for x in v])


# ---------------------------------------------------------------- 1. the goldens
@pytest.mark.parametrize("ini,tag", [(i, t) for i in bf.INIS for t in bf.TAGS[i]])
def test_matches_the_compiled_reference(fx, calc, ini, tag):
    """Every golden case of the dataset, then a NaN in each input and a point
    outside the calculator's box in each input.  MGS: at x_min and x_max, the
    nearest doubles outside, cell edges, interior points.  Grids: the four
    corners of the valid rectangle, the second-to-last knot exactly and the
    nearest double beyond it, a zero cell, points where floor and a knot search
    name different cells, v1 negative and v1 = 0."""
    d = bf.read_all(fx, ini)[tag]
    cases = [c for c in bf.load_cases(fx, ini) if c["tag"] == tag]
    e = bf.host_errors(fx, ini)[tag]
    bound = 10 * max(e["a"], e["b"])
    v0, v1 = _case_points(cases, d["kind"])
    n = len(cases)
    inside0, inside1 = v0[[c["ref"] < 1e29 for c in cases]][0], v1[[c["ref"] < 1e29 for c in cases]][0]
    extra = [(np.nan, inside1, 1), (inside0, np.nan, 1), (2 * BOX, inside1, 1), (inside0, -2 * BOX, 1),
             (inside0, inside1, 0)]
    P = _rows(np.concatenate([v0, [x[0] for x in extra]]), np.concatenate([v1, [x[1] for x in extra]]))
    g = _make(calc, d)
    got, fl, full, flfull = _eval(g, P, P.shape[1])
    g.close()
    ref = np.array([c["ref"] for c in cases])
    zero = ref >= 1e29
    assert np.array_equal(got[:n] == LOGZERO, zero), [c["label"] for c, x, y in zip(cases, got[:n] == LOGZERO, zero)
                                                      if x != y]
    err = np.abs(got[:n][~zero] - ref[~zero])
    print(f"{ini} {tag}: (a) {e['a']:.3e} (b) {e['b']:.3e} bound {bound:.3e}; GPU max |got - golden| = "
          f"{err.max():.3e} over {err.size} finite cases, {zero.sum()} logZero")
    assert np.all(err <= bound), [(c["label"], float(x)) for c, x in zip(np.array(cases)[~zero], err) if x > bound]
    assert np.array_equal(fl[:n], np.zeros(n, dtype=np.int32))         # logZero by the table is no calculator failure
    assert np.array_equal(fl[n:], [x[2] for x in extra])
    assert np.all(got[n:n + 4] == LOGZERO) and got[n + 4] < 1e29
    assert np.all(np.isnan(full[P.shape[1]:])) and np.all(flfull[P.shape[1]:] == -7)


def test_unused_input_nan_in_mgs(fx, calc):
    """The 1-D form reads surface 0 alone, but the box is the calculator's: a
    NaN in the other input is still a failure."""
    d = bf.read_all(fx)["MGS"]
    g = _make(calc, d)
    got, fl, _, _ = _eval(g, _rows([4.0, 4.0], [np.nan, 0.0]), 2)
    g.close()
    assert got[0] == LOGZERO and fl[0] == 1 and got[1] < 1e29 and fl[1] == 0


# ---------------------------------------------------------------- 2. batch shapes
@pytest.mark.parametrize("tag", ["MGS", "DR11CMASS"])
def test_batch_shapes(fx, calc, tag):
    """M = 1, TD_TM - 1, TD_TM, TD_TM + 1 with ld > M: a point's bits are the
    same in every batch and at every slot, and nothing outside out[0..M) is
    written (a NaN-valued guard behind the output, -7 behind the flags)."""
    d = bf.read_all(fx)[tag]
    cases = [c for c in bf.load_cases(fx) if c["tag"] == tag]
    v0, v1 = _case_points(cases, d["kind"])
    Mmax = TD_TM + 1
    idx = np.arange(Mmax + 7) % len(cases)
    P = _rows(v0[idx], v1[idx])
    g = _make(calc, d)
    big = _eval(g, P, Mmax, ld=Mmax + 7, pad=5)[0]
    assert np.any(big == LOGZERO) and np.any(big < 1e29)
    assert not np.any(np.isnan(big))
    assert np.array_equal(big, big[:len(cases)][idx[:Mmax]])           # the same point at another slot
    for M in (1, TD_TM - 1, TD_TM, TD_TM + 1):
        got, fl, full, flfull = _eval(g, P, M, ld=M + 3)
        assert np.array_equal(got, big[:M]), M
        assert np.all(fl == 0)
        assert np.all(np.isnan(full[M:])) and np.all(flfull[M:] == -7), "an element outside [0, M) was written"
        shifted = _eval(g, np.ascontiguousarray(P[:, 5:]), M)[0]        # every point five slots earlier
        assert np.array_equal(shifted, big[:len(cases)][idx[5:5 + M]]), M
    for w in (0, 63, 64, TD_TM - 1, TD_TM):
        alone = _eval(g, np.ascontiguousarray(P[:, w:w + 1]), 1, pad=0)[0]
        assert alone[0] == big[w], w
    host = g.eval(np.ascontiguousarray(P[:, :Mmax].T))                 # host points [M, num_params]
    assert np.array_equal(host.cpu().numpy(), big)
    g.close()


# ---------------------------------------------------------------- 3. argument errors
def test_argument_errors(fx, calc):
    """Every argument error of cmbg_create_table is code -1, never an abort,
    and a good table still works afterwards."""
    from cosmomc_amd import _native as N
    from cosmomc_amd import derivedlike as dl
    specs = bf.read_all(fx)
    m, gr = specs["MGS"], specs["DR12CMASS"]

    def bad(call):
        with pytest.raises(N.NativeError) as e:
            call()
        assert e.value.code == -1 and str(e.value), e.value

    scale = dl.MGS_DVFID / dl.MGS_RSFID
    t = m["table"]

    def one(table=t, scale=scale, x_min=dl.MGS_ALPHA_MIN, x_max=dl.MGS_ALPHA_MAX, step=dl.MGS_STEP, col=MGS_COL):
        DerivedTable.table1d(calc, col, table, scale, x_min, x_max, step).close()

    one()
    bad(lambda: one(table=t[:1]))                                      # n < 2
    bad(lambda: one(table=t[:398]))                                    # ii + 1 reaches n at alpha = x_max
    one(table=t[:399])
    bad(lambda: one(step=0.001 * 397 / 398))                           # a finer step: cell 398 at x_max
    bad(lambda: one(step=0.0))
    bad(lambda: one(step=-dl.MGS_STEP))
    bad(lambda: one(step=np.nan))
    bad(lambda: one(x_min=dl.MGS_ALPHA_MAX))                           # x_min >= x_max
    bad(lambda: one(x_min=1.3))
    bad(lambda: one(x_max=np.inf))
    bad(lambda: one(scale=0.0))
    bad(lambda: one(scale=np.nan))
    for v in (np.nan, np.inf):
        tt = t.copy()
        tt[200] = v
        bad(lambda: one(table=tt))
    bad(lambda: one(col=np.array([np.nan, 0.0])))

    def two(perp=gr["perp"], plel=gr["plel"], prob=gr["prob"], da=gr["DA_rd_fid"], h=gr["Hrd_fid"]):
        DerivedTable.grid(calc, GRID_COLS, perp, plel, prob, da, h).close()

    two()
    bad(lambda: two(perp=gr["perp"][:2], plel=gr["plel"][:2], prob=gr["prob"][:2, :2]))       # np < 3
    for axis in ("perp", "plel"):
        k = gr[axis].copy()
        k[1] = k[0]
        bad(lambda: two(**{axis: k}))                                  # d = 0
        k = gr[axis].copy()
        k[0], k[1] = k[1], k[0]
        bad(lambda: two(**{axis: k}))                                  # d < 0
        k = gr[axis].copy()
        k[3] = np.nan
        bad(lambda: two(**{axis: k}))
        k = gr[axis].copy()
        k[1] = k[0] + (k[1] - k[0]) / 3                                # knot[np - 2] lies in a cell beyond the grid
        bad(lambda: two(**{axis: k}))
    p = gr["prob"].copy()
    p[1, 2] = np.inf
    bad(lambda: two(prob=p))
    bad(lambda: two(da=0.0))
    bad(lambda: two(h=np.nan))

    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (GRID_COLS, t, gr["perp"], gr["plel"], gr["prob"])]

    def raw(form, null=None):
        cfg = N.CmbgTableConfig()
        cfg.form = form
        cfg.n, cfg.scale, cfg.x_min, cfg.x_max, cfg.step = t.size, scale, dl.MGS_ALPHA_MIN, dl.MGS_ALPHA_MAX, dl.MGS_STEP
        cfg.np, cfg.DA_rd_fid, cfg.Hrd_fid = gr["np"], gr["DA_rd_fid"], gr["Hrd_fid"]
        for name, a in zip(("coef", "table", "perp", "plel", "prob"), keep):
            if name != null:
                setattr(cfg, name, a.ctypes.data_as(dp))
        h, err = C.c_void_p(), C.create_string_buffer(256)
        rc = N.lib().cmbg_create_table(calc.handle, C.byref(cfg), C.byref(h), err, 256)
        if rc == 0:
            N.lib().cmbg_destroy(h)
        else:
            assert not h.value and err.value
        return rc

    assert raw(1) == 0 and raw(2) == 0
    assert raw(0) == -1 and raw(3) == -1                               # another form
    assert raw(1, "coef") == -1 and raw(1, "table") == -1
    for null in ("coef", "perp", "plel", "prob"):
        assert raw(2, null) == -1, null
    h = C.c_void_p()
    assert N.lib().cmbg_create_table(calc.handle, None, C.byref(h), None, 0) == -1          # a NULL config

    g = _make(calc, m)                                                 # eval's own errors, and it still works
    P = torch.tensor(_rows([4.0] * 8, [0.0] * 8), device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")

    def ev(M=8, ld=8, num_params=NPAR):
        N.check(N.lib().cmbg_eval(g.handle, M, P.data_ptr(), ld, num_params, out.data_ptr(), None,
                                  N.current_stream_ptr()), g.handle, "cmbg")

    bad(lambda: ev(ld=7))
    bad(lambda: ev(num_params=2))
    bad(lambda: ev(M=0))
    ev()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == bf.bao_table_loglike_host(m, 4.0))
    g.close()
