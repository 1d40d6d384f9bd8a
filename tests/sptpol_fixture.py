"""Shared by test_sptpol_geometry.py and test_gpu_sptpol_geometry.py: the SPTpol
window-geometry datasets (cosmomc_amd.synthetic.make_sptpol_geom) written once
per session, a long-double restatement of both likelihoods, and the work-item
rule of SPTpol::finish (cosmomc_amd/csrc/sptpol.hip) restated on the windows.

The long-double restatement follows oracle/sptpol_oracle.py line by line
(TSPTpolEELike / TSPTpolBBLike of the reference) on the arrays the oracle
object loaded from disk, with every sum, the Cholesky factor, the triangular
solve and the log-determinant in np.longdouble.  The reference's REAL(4)
literals stay REAL(4) values, as in the oracle.
"""
import os

import numpy as np
import pytest

import sptpol_oracle as so
from cosmomc_amd import synthetic as syn

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 1e-18)
needs_longdouble = pytest.mark.skipif(not HAVE_LONGDOUBLE, reason="np.longdouble is no wider than double here")

RTOL, ATOL = 1e-10, 1e-8             # the GPU tolerance of test_gpu_sptpol.py
W_ALL = 67                           # two walker tiles, the second partial
W_GOLDEN = 3                         # walkers recorded from the compiled reference
TEEE_CASES = list(syn.sptpol_geom_teee_cases())
BB_CASES = list(syn.sptpol_geom_bb_cases())
ALL_CASES = TEEE_CASES + BB_CASES
TWOPI = LD(2) * np.arccos(LD(-1))


def F(x):
    return LD(np.float32(x))         # a REAL(4) literal, promoted


def tag_of(case):
    return syn.sptpol_geom_cases()[case]


def n_fields(case):
    return 3 if tag_of(case) == "SPTPOL_TEEE" else 6


# ------------------------------------------------------------ long double

def chol_ld(A):
    """dpotrf 'L' in long double."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def gauss_loglike_ld(L, d):
    """sum log L_ii + d . C^-1 d / 2 = sum log L_ii + |L^-1 d|^2 / 2, rows of d."""
    n = L.shape[0]
    y = np.zeros(d.shape, dtype=LD)
    for i in range(n):
        y[:, i] = (d[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    return np.sum(np.log(np.diag(L))) + np.sum(y * y, axis=1) / 2


def _rows(dl, field, lmax):
    """Theory%ClArray into dls(1:lmax+1): l = 0 is never read."""
    d = np.zeros((dl.shape[0], lmax + 2), dtype=LD)
    n = min(lmax + 1, dl.shape[2] - 1)
    d[:, 1:n + 1] = dl[:, field, 1:n + 1]
    return d


def teee_ld(o, L, dl, P):
    lmin, lmax, nbin = o.lmin, o.lmax, o.nbin
    P = P.astype(LD)
    W = P.shape[0]
    ells = np.arange(lmin - 1, lmax + 2).astype(LD)
    conv = (ells * (ells + 1)) / TWOPI
    rawspec = ells ** 3 / conv
    deriv_factor = LD(0.5) / ells[1:-1] ** 2
    ell = ells[1:-1]
    d3000 = LD(3000 * 3001) / TWOPI
    beta, dcos = F(0.0012309), F(-0.4033)
    win = o.windows.astype(LD)
    tmp2 = np.zeros((W, 2 * nbin), dtype=LD)
    for k in range(2):
        d = _rows(dl, (1, 2)[k], lmax)
        raw = rawspec * d[:, lmin - 1:lmax + 2]
        deriv = deriv_factor * (raw[:, 2:] - raw[:, :-2])
        fg = (P[:, 1 + k, None] / d3000 - P[:, 0, None] * deriv) * conv[1:-1]
        fg = fg + d[:, lmin:lmax + 1]
        if o.aberration:
            fg = fg + (-1 * beta * dcos) * ell * ((d[:, lmin + 1:lmax + 2] - d[:, lmin - 1:lmax]) / 2)
        fg = fg + P[:, 3 + 2 * k, None] * (ell / 80) ** (P[:, 4 + 2 * k, None] + 2)
        cal = (P[:, 7] * P[:, 7]) * P[:, 8] ** (k + 1)
        tmp2[:, k * nbin:(k + 1) * nbin] = (fg @ win[:, k * nbin:(k + 1) * nbin]) / cal[:, None]
    bf = np.ones((W, 2 * nbin), dtype=LD)
    for t in range(2):
        bf = bf * (1 + o.beam_err[t].astype(LD) * P[:, 9 + t, None])
    delta = tmp2 * bf - np.concatenate([o.spec[0], o.spec[1]]).astype(LD)
    out = gauss_loglike_ld(L, delta) + np.sum(P[:, 9:11] ** 2, axis=1) / 2
    if o.Tcal_prior:
        out = out + (np.log(P[:, 7] / LD(o.meanTcal)) / LD(o.sigmaTcal)) ** 2 / 2
    if o.Pcal_prior:
        out = out + (np.log(P[:, 8] / LD(o.meanPcal)) / LD(o.sigmaPcal)) ** 2 / 2
    if o.kappa_prior:
        out = out + ((P[:, 0] - LD(o.meankappa)) / LD(o.sigmakappa)) ** 2 / 2
    if o.aTE_prior:
        out = out + ((P[:, 4] - LD(o.meanAlphaTE)) / LD(o.sigmaAlphaTE)) ** 2 / 2
    if o.aEE_prior:
        out = out + ((P[:, 6] - LD(o.meanAlphaEE)) / LD(o.sigmaAlphaEE)) ** 2 / 2
    return out


def _dBdT_ld(nu, nu0):
    x0, x = nu0 / F(56.78), nu / F(56.78)
    return (x ** 4 * np.exp(x) / (np.exp(x) - 1) ** 2) / (x0 ** 4 * np.exp(x0) / (np.exp(x0) - 1) ** 2)


def _Bnu_ld(nu, nu0, T):
    hk = F(4.799237e-2)
    return (nu / nu0) ** 3 * (np.exp(hk * nu0 / T) - 1) / (np.exp(hk * nu / T) - 1)


def dust_scaling_ld(f1, f2):
    f1, f2, n0 = LD(f1), LD(f2), LD(150)
    s = ((f1 * f2) / (n0 * n0)) ** F(1.59)
    s = s * _Bnu_ld(f1, n0, F(19.6)) * _Bnu_ld(f2, n0, F(19.6))
    return s / _dBdT_ld(f1, n0) / _dBdT_ld(f2, n0)


def bb_ld(o, L, dl, P, eff):
    lmin, lmax, nbin = o.lmin, o.lmax, o.nbin
    P = P.astype(LD)
    W = P.shape[0]
    ell = np.arange(lmin, lmax + 1).astype(LD)
    poisson = (ell * (ell + 1)) / LD(3000.0 * 3001.0)
    galdust = ((ell + 1) / 81) * (80 / ell) ** F(1.42)
    pairs = [(eff[0], eff[0]), (eff[0], eff[1]), (eff[1], eff[1])]
    d = _rows(dl, 5, lmax)[:, lmin:lmax + 1]
    scale = np.where(P[:, 0] != 1, P[:, 0] + LD(o.blind_abb), LD(1))
    d = np.where((P[:, 0] == 0)[:, None], LD(0), d * scale[:, None])
    d = d + P[:, 2, None] + P[:, 1, None] * o.tensor.astype(LD)
    cal = [P[:, 7] * P[:, 7], P[:, 8] * P[:, 7], P[:, 8] * P[:, 8]]
    win = o.windows.astype(LD)
    tmp2 = np.zeros((W, 3 * nbin), dtype=LD)
    for k in range(3):
        fg = P[:, 4 + k, None] * poisson + (P[:, 3, None] * galdust) * dust_scaling_ld(*pairs[k]) + d
        tmp2[:, k * nbin:(k + 1) * nbin] = (fg @ win[:, k * nbin:(k + 1) * nbin]) / cal[k][:, None]
    bf = np.ones((W, 3 * nbin), dtype=LD)
    for t in range(o.beam_err.shape[0]):
        bf = bf * (1 + o.beam_err[t].astype(LD) * P[:, 9 + t, None])
    delta = tmp2 * bf - o.spec.ravel().astype(LD)
    out = gauss_loglike_ld(L, delta) + np.sum(P[:, 9:16] ** 2, axis=1) / 2
    if o.cal_prior:
        y1, y2 = np.log(P[:, 8]), np.log(P[:, 7])
        icc = o.icc.astype(LD)
        out = out + (icc[0, 0] * y1 * y1 + 2 * icc[0, 1] * y1 * y2 + icc[1, 1] * y2 * y2) / 2
    if o.add_prior:
        out = out + ((P[:, 3] - LD(o.meanAdd)) / LD(o.sigmaAdd)) ** 2 / 2
    return out


# ------------------------------------------------------------ work items

SP_COLS, SP_CH = 16, 256


def items(windows, lmin, nband):
    """SPTpol::finish's work items as (band, first column, l0, number of l): per
    band, groups of <= 16 consecutive columns over the union of their non-zero
    support from an even l0, cut into <= 256 l; a group without windows has none."""
    nl, nall = windows.shape
    nbin = nall // nband
    out = []
    for k in range(nband):
        for c0 in range(0, nbin, SP_COLS):
            sup = np.nonzero(windows[:, k * nbin + c0:k * nbin + min(nbin, c0 + SP_COLS)].any(axis=1))[0]
            if sup.size == 0:
                continue
            la, lz = (lmin + int(sup[0])) & ~1, lmin + int(sup[-1])
            out += [(k, c0, s0, min(SP_CH, lz - s0 + 1)) for s0 in range(la, lz + 1, SP_CH)]
    return out


# ------------------------------------------------------------ datasets

class Geometry:
    """Datasets, oracle objects, inputs and long-double results, made on first
    use and kept for the session.  ``on`` is correct_aberration (TE/EE) or
    sptpol_blind_abb (BB)."""

    def __init__(self, root):
        self.root = root
        self._c = {}

    def _memo(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def data(self, case):
        return self._memo(("data", case), lambda: syn.make_sptpol_geom(case))

    def path(self, case):
        return self._memo(("path", case), lambda: self.data(case).write(os.path.join(self.root, case)))

    def overrides(self, case, on):
        d = os.path.dirname(self.path(case))
        return {k: v.replace("@DIR@", d) for k, v in syn.sptpol_geom_overrides(case, on).items()}

    def oracle(self, case, on):
        return self._memo(("oracle", case, on),
                          lambda: so.open_sptpol(tag_of(case), self.path(case), self.overrides(case, on)))

    def theory(self, case):
        """[W_ALL, nf, lmax + 2]; treat as read-only."""
        return self._memo(("theory", case), lambda: syn.sptpol_geom_theory(case, W_ALL))

    def nuis(self, case):
        return self._memo(("nuis", case), lambda: syn.sptpol_geom_nuisance(case, W_ALL))

    def chol(self, case):
        return self._memo(("chol", case), lambda: chol_ld(self.oracle(case, False).cov.astype(LD)))

    def longdouble(self, case, on, dl=None, P=None):
        """-lnL in long double; of the session's theory and nuisances (cached) unless given."""
        o = self.oracle(case, on)

        def run(dl, P):
            if tag_of(case) == "SPTPOL_TEEE":
                return teee_ld(o, self.chol(case), dl, P)
            return bb_ld(o, self.chol(case), dl, P, self.data(case).eff_freqs)
        if dl is not None:
            return run(dl, self.nuis(case) if P is None else P)
        return self._memo(("ld", case, on), lambda: run(self.theory(case), self.nuis(case)))

    def open_native(self, case, on):
        from cosmomc_amd.likelihood import NativeCMBLikelihood
        return NativeCMBLikelihood(tag_of(case), self.path(case), self.overrides(case, on))


_SESSION = {}


@pytest.fixture(scope="session")
def geom(tmp_path_factory):
    """One Geometry per session, also when two test modules import this fixture."""
    if "geom" not in _SESSION:
        _SESSION["geom"] = Geometry(str(tmp_path_factory.mktemp("sptpol_geom")))
    return _SESSION["geom"]


def reach(case):
    """Theory entries (field, l) a case was built to reach: for TE/EE the first
    and last l that carry window weight and their l-1 / l+1 derivative halo, for
    BB the first and last weighted l.  These are lmin-1, lmin, lmax, lmax+1 (BB:
    lmin, lmax) in every case but nine_rows, whose one bin (4, 2052) lies inside
    its l range (2, 2060): there they are 3, 4, 2052, 2053."""
    d = syn.make_sptpol_geom(case)
    nband = 2 if tag_of(case) == "SPTPOL_TEEE" else 3
    sup = np.nonzero(d.windows.any(axis=1))[0]
    if sup.size == 0:
        return []
    a, z = d.lmin + int(sup[0]), d.lmin + int(sup[-1])
    return [a - 1, a, z, z + 1] if nband == 2 else [a, z]
