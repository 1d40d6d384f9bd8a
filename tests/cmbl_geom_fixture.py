"""Shared by test_cmbl_geom.py and test_gpu_cmbl_geom.py: the CMBlikes
window-geometry datasets (cosmomc_amd.synthetic.make_cmbl_geom) written once per
session, their references, and the work-item rule of cmblikes.hip build_items
restated on the windows.

References.  Gaussian cases: a restatement in np.longdouble of
CMBLikesOracle.map_cls / loglike (GetTheoryMapCls, AddAberration, the SMICA
foreground, AdaptTheoryForMaps, TBinWindows_bin, chi^2 / 2 and the calibration
prior) on the arrays the oracle object read from disk, the covariance solved by
a long-double Cholesky factor.  HL cases and the BK selections: CMBLikesOracle
(float64; the HL transform's eigensolves have no long-double LAPACK here).
"""
import os

import numpy as np
import pytest

import cmblikes_oracle as co
from cosmomc_amd import synthetic as syn
from sptpol_fixture import HAVE_LONGDOUBLE, LD, chol_ld, needs_longdouble  # noqa: F401

W_ALL = 67                           # two walker tiles, the second partial
W_GOLDEN = 3                         # walkers recorded from the compiled reference
N_FIELDS = 3                         # TT TE EE rows in the theory buffer
ALL_CASES = list(syn.cmbl_geom_cases())
HL_CASES = [c for c in ALL_CASES if syn.cmbl_geom_cases()[c][1] == "HL"]
GAUSS_CASES = [c for c in ALL_CASES if c not in HL_CASES]
ABER_CASES = [c for c in ALL_CASES if syn.cmbl_geom_cases()[c][2]]
SEG = 256                            # WK_CHUNK * WK_NCH
CHUNK, COLS = 64, 32                 # WK_CHUNK, WK_COLS


def tol(case):
    """(rtol, atol) of test_gpu_cmblikes.py: gaussian 1e-10 / 1e-9, HL and BK 1e-9 / 1e-8."""
    return (1e-9, 1e-8) if case in HL_CASES or case.startswith("bk") else (1e-10, 1e-9)


def tolerances(case, ref):
    rtol, atol = tol(case)
    return rtol * np.abs(np.asarray(ref, dtype=np.float64)) + atol


# ------------------------------------------------------------ long double

def _pair_fields(o):
    """(i, j) of the required maps -> theory row (TT 0, TE 1, EE 2 ...) and whether aberration / calibration apply."""
    out = {}
    dummy = np.zeros((10, 1))
    for i in range(1, o.nreq + 1):
        for j in range(1, i + 1):
            f1, f2, _ = o._theory_field(dummy, i, j)
            out[i, j] = (f1 * (f1 - 1) // 2 + f2 - 1, f1 <= 3 and f2 <= 3, f1 == 1 and f2 == 1)
    return out


def map_cls_ld(o, dl, P, ends=("rule", "rule")):
    """CMBLikesOracle.map_cls for all walkers in long double: {(i, j): [W, lmax-lmin+1]}.
    ends: the aberration derivative at (l = lmin, l = lmax) -- "rule" (the
    reference's: the neighbouring l's derivative), "zero" (the term dropped there) or
    "central" (the central difference through l - 1 / l + 1 as the other l have it,
    with D_lmax repeated behind lmax); the last two are wrong on purpose."""
    lo, hi = o.lmin, o.lmax
    P = np.asarray(P).astype(LD)
    ells = np.arange(lo, hi + 1).astype(LD)
    out = {}
    for k, (f, cmb, tt) in _pair_fields(o).items():
        cl = dl[:, f, lo:hi + 1].astype(LD)
        if o.aberration != 0 and cmb:
            d = cl / (ells * (ells + 1))
            dd = np.zeros_like(d)
            dd[:, 1:-1] = (d[:, 2:] - d[:, :-2]) / 2
            assert set(ends) <= {"rule", "central", "zero"}
            if ends[0] == "rule":
                dd[:, 0] = dd[:, 1]
            elif ends[0] == "central":
                dd[:, 0] = (d[:, 1] - dl[:, f, lo - 1].astype(LD) / LD((lo - 1) * lo)) / 2
            if ends[1] == "rule":
                dd[:, -1] = dd[:, -2]
            elif ends[1] == "central":
                dd[:, -1] = (dl[:, f, hi].astype(LD) / LD((hi + 1) * (hi + 2)) - d[:, -2]) / 2
            cl = cl + LD(o.aberration) * (ells ** 2 * (ells + 1) * dd)
        if o.smica and tt:
            r = np.log(ells / LD(o.SMICA_PIVOT))
            t1 = P[:, 0, None] * np.exp(P[:, 1, None] * r + P[:, 2, None] / 2 * r ** 2)
            t2 = P[:, 3, None] * (ells / LD(o.SMICA_PIVOT)) ** P[:, 4, None]
            cl = (cl + t1) + t2
        if o.cal_index is not None and cmb:
            cl = cl / (P[:, o.cal_index, None] ** 2)
        out[k] = cl
    return out


def gauss_ld(o, L, mc, P, zero=None):
    """-lnL [W] of a gaussian dataset from its map spectra, in long double; L: the
    long-double Cholesky factor of the covariance.  zero = (bin, window entry, l):
    that one window weight taken as 0."""
    assert o.like_approx == 2 and o.fidcorr is None
    P = np.asarray(P).astype(LD)
    win = o.W_main
    W = P.shape[0]
    X = np.zeros((W, len(o.bins) * o.ncl), dtype=LD)
    for bi, b in enumerate(o.bins):
        for k, (ij, out) in enumerate(zip(win["in"], win["out"])):
            if out > 0:
                w = win["W"][b][k].astype(LD)
                if zero is not None and zero[:2] == (b, k):
                    w[zero[2] - o.lmin] = 0
                X[:, bi * o.ncl + out - 1] += mc[ij] @ w
        X[:, bi * o.ncl:(bi + 1) * o.ncl] -= o.clhat[b].astype(LD)
    use = np.array([bi * o.ncl + c - 1 for bi in range(len(o.bins)) for c in o.cl_use])
    d = X[:, use]
    n = L.shape[0]
    y = np.zeros(d.shape, dtype=LD)
    for i in range(n):
        y[:, i] = (d[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    chisq = np.sum(y * y, axis=1)
    if o.log_cal_prior > 0 and o.cal_index is not None:
        chisq = chisq + (np.log(P[:, o.cal_index]) / LD(o.log_cal_prior)) ** 2
    return chisq / 2


# ------------------------------------------------------------ work items

def items(d):
    """The window work items of cmblikes.hip build_items on the default 256-l
    segments, as dicts: per spectrum and segment, groups of <= 32 overlapping
    columns over the union of their support within the segment, the first l moved
    down to an even l where that stays inside the segment."""
    L = d.lmax - d.lmin + 1
    out = []
    for p in range(len(d.pairs)):
        cols = []
        for b in range(d.nbin):
            sup = np.nonzero(d.windows[:, b, p])[0]
            if sup.size:
                cols.append((int(sup[0]), int(sup[-1])))
        for c0 in range(0, L, SEG):
            c1 = min(L - 1, c0 + SEG - 1)
            sel = [c for c in cols if c[1] >= c0 and c[0] <= c1]
            for g0 in range(0, len(sel), COLS):
                grp = sel[g0:g0 + COLS]
                lo = min(max(c0, c[0]) for c in grp)
                hi = max(min(c1, c[1]) for c in grp)
                moved = (lo + d.lmin) % 2 == 1 and lo > c0
                lo -= 1 if moved else 0
                n = hi - lo + 1
                out.append({"pair": p, "seg": c0 // SEG, "l0": lo + d.lmin, "l1": hi + d.lmin, "ncol": len(grp),
                            "nch": (hi - lo + CHUNK) // CHUNK, "moved": moved, "len": n,
                            "clen": n - CHUNK * ((n - 1) // CHUNK), "sub": n - 32 * ((n - 1) // 32)})
    return out


def edges(d):
    """(bin, spectrum, l) of every window weight at an edge: the first and last l of
    the window, and the l on either side of every segment boundary it crosses."""
    out = []
    for p in range(len(d.pairs)):
        for b in range(d.nbin):
            sup = np.nonzero(d.windows[:, b, p])[0]
            if not sup.size:
                continue
            lo, hi = int(sup[0]), int(sup[-1])
            e = {lo, hi}
            for c in range(SEG, hi + 1, SEG):
                if lo < c <= hi:
                    e |= {c - 1, c}
            out += [(b, p, d.lmin + r) for r in sorted(e)]
    return out


# ------------------------------------------------------------ datasets

class Geometry:
    """Datasets, oracle objects, inputs and reference results, made on first use
    and kept for the session."""

    def __init__(self, root):
        self.root = root
        self._c = {}

    def _memo(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def data(self, case):
        return self._memo(("data", case), lambda: syn.make_cmbl_geom(case))

    def path(self, case):
        return self._memo(("path", case), lambda: self.data(case).write(os.path.join(self.root, case)))

    def oracle(self, case):
        return self._memo(("oracle", case),
                          lambda: co.CMBLikesOracle(self.path(case), None, syn.cmbl_geom_tag(case)))

    def theory(self, case):
        """[W_ALL, 3, lmax + 1]; treat as read-only."""
        return self._memo(("theory", case), lambda: syn.cmbl_geom_theory(case, W_ALL))

    def nuis(self, case):
        return self._memo(("nuis", case), lambda: syn.cmbl_geom_nuisance(case, W_ALL))

    def chol(self, case):
        return self._memo(("chol", case), lambda: chol_ld(self.data(case).cov.astype(LD)))

    def oracle_batch(self, case, dl=None, P=None, o=None):
        dl = self.theory(case) if dl is None else dl
        P = self.nuis(case) if P is None else P
        o = self.oracle(case) if o is None else o
        return np.array([o.loglike(dl[w], P[w]) for w in range(dl.shape[0])])

    def reference(self, case, dl=None, P=None):
        """-lnL of every walker: long double for the gaussian cases, CMBLikesOracle
        for HL; of the session's theory and nuisances (cached) unless given."""
        def run(dl, P):
            if case in HL_CASES:
                return self.oracle_batch(case, dl, P)
            o = self.oracle(case)
            return gauss_ld(o, self.chol(case), map_cls_ld(o, dl, P), P)
        if dl is not None or P is not None:
            return run(self.theory(case) if dl is None else dl, self.nuis(case) if P is None else P)
        return self._memo(("ref", case), lambda: run(self.theory(case), self.nuis(case)))

    def open_native(self, case):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        return NativeCMBLikelihood(syn.cmbl_geom_tag(case), self.path(case))


class BKSelections:
    """The BK cases on the reference's own BKPlanck and BK15 datasets (the refdata
    fixture): oracle objects, inputs and oracle results, kept for the session."""

    def __init__(self, refdata):
        self.refdata = refdata
        self._c = {}

    def _memo(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def oracle(self, name):
        ds, over = bk_case(name)
        return self._memo(("oracle", name), lambda: co.CMBLikesOracle(os.path.join(self.refdata, ds), over, "BKPLANCK"))

    def theory(self, name):
        return self._memo(("in", name), lambda: bk_inputs(name, W_ALL))[0]

    def nuis(self, name):
        return self._memo(("in", name), lambda: bk_inputs(name, W_ALL))[1]

    def reference(self, name, dl=None, P=None):
        def run(dl, P):
            o = self.oracle(name)
            return np.array([o.loglike(dl[w], P[w]) for w in range(dl.shape[0])])
        if dl is not None or P is not None:
            return run(self.theory(name) if dl is None else dl, self.nuis(name) if P is None else P)
        return self._memo(("ref", name), lambda: run(self.theory(name), self.nuis(name)))

    def open_native(self, name):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        ds, over = bk_case(name)
        return NativeCMBLikelihood("BKPLANCK", os.path.join(self.refdata, ds), over)


_SESSION = {}


@pytest.fixture(scope="session")
def bksel(refdata):
    if "bksel" not in _SESSION:
        _SESSION["bksel"] = BKSelections(refdata)
    return _SESSION["bksel"]


@pytest.fixture(scope="session")
def cgeom(tmp_path_factory):
    """One Geometry per session, also when two test modules import this fixture."""
    if "cgeom" not in _SESSION:
        _SESSION["cgeom"] = Geometry(str(tmp_path_factory.mktemp("cmbl_geom")))
    return _SESSION["cgeom"]


# ------------------------------------------------------------ BK selections

BKP = "BKPlanck/BKPlanck_detset_comb_dust.dataset"
BK15 = "BK15/BK15_dust.dataset"
BK15_B3 = "BK15_95_B BK15_150_B BK15_220_B"
# name -> (dataset, overrides): the first bin alone, the last bin alone and all bins,
# with flat and with l-dependent decorrelation (cmbl_window_group<false> / <true>)
BK_SELECTIONS = {
    "bkp_first_bin": (BKP, {"maps_use": "B2K_B P217_B P353_B", "use_min": "1", "use_max": "1"}),
    "bkp_last_bin": (BKP, {"maps_use": "B2K_B P217_B P353_B", "use_min": "9", "use_max": "9"}),
    "bkp_all_bins": (BKP, {"maps_use": "B2K_E B2K_B P353_E P353_B"}),
    "bk15_first_bin": (BK15, {"maps_use": BK15_B3, "use_min": "1", "use_max": "1"}),
    "bk15_last_bin": (BK15, {"maps_use": BK15_B3, "use_min": "9", "use_max": "9"}),
    "bk15_all_bins": (BK15, {"maps_use": BK15_B3 + " P353_B"}),
    # cl_lmin = 3: the first window's first l is odd, so its grouped item starts at the even l = lmin - 1
    "bkp_lmin3": (BKP, {"maps_use": "B2K_B P217_B P353_B", "cl_lmin": "3"}),
    "bk15_lmin3": (BK15, {"maps_use": BK15_B3, "cl_lmin": "3"}),
}
BK_LFORM = {"flat": {"lform_dust_decorr": "flat", "lform_sync_decorr": "flat"},
            "lin_quad": {"lform_dust_decorr": "lin", "lform_sync_decorr": "quad"}}
BK_CASES = [f"{s}-{f}" for s in BK_SELECTIONS for f in BK_LFORM]
BK_LMAX = 600


def bk_case(name):
    """(dataset, overrides) of a BK case ``selection-lform``."""
    s, f = name.split("-")
    ds, over = BK_SELECTIONS[s]
    return ds, dict(over, **BK_LFORM[f])


def bk_inputs(name, W):
    """Theory [W, 10, 601] and the 16 BK nuisances [W, 16] with decorrelation on
    (Delta_dust, Delta_sync off 1), every walker its own."""
    seed = 0xB6E0 + 16 * BK_CASES.index(name)
    th = syn.walker_theory(W, seed=seed, lmax=BK_LMAX)
    g = syn.gaussians(seed + 1, W * 16).reshape(W, 16)
    P = np.tile(np.array([3.0, 1.0, -0.42, 1.59, 19.6, -0.6, -3.3, 0.2, 2.0, 1.0, 0.85, 0.9, 0.0, 0.0, 0.0, 0.0]), (W, 1))
    P[:, 0] += 0.5 * g[:, 0]
    P[:, 1] += 0.2 * np.abs(g[:, 1])
    P[:, 2] += 0.05 * g[:, 2]
    P[:, 3] += 0.05 * g[:, 3]
    P[:, 7] += 0.05 * g[:, 7]
    P[:, 10] += 0.02 * g[:, 10]
    P[:, 11] += 0.02 * g[:, 11]
    return th, P
