"""Planck SZ cluster-counts likelihood (reference source/szcounts.f90, the 2D
form N(z, q), ``SZ_switch = 2``).

``SZLikelihood`` is the data set opened in the HIP library (``cmbl_open`` tag
``"SZ"``) from a small ini of the project's own: ``cat_file``, ``thetas_file``,
``skyfracs_file``, ``ylims_file`` (relative to it), optionally
``nuisance_params``, and the option keys ``1D``, ``2D`` and ``prior_*`` of the
reference's run ini.  Its nuisance parameters are ``alpha_SZ, ystar_SZ,
bias_SZ, scatter_SZ, beta_SZ`` and its theory is one row per walker::

    [H0, ns, ombh2, E(z_j)[nzs], dA(z_j)[nzs], grid[nzs][nm]]

``z_j = steps_z``; ``dA`` in Mpc / h; ``grid[j][m]`` is what the reference's
``get_grid`` leaves, ``dndlnM * deg2 * dVdzdO`` at ``(steps_z[j], exp(steps_m[m]))``.
``sz_theory_row`` builds it (Tinker or Watson mass function, growth ODE) from
a sigma(R) table; which mass function fills it is the provider's business.

``SZDataset`` is ``SZ_init`` (:1501-1821) and the fixed part of ``deltaN_yz``
(:649-694) on the host, ``sz_loglike_host`` a literal numpy restatement of
``grid_C_2d`` / ``integrate_m_zq`` / ``SZCC_Cash`` in the reference's types and
summation order; with ``dtype=np.longdouble`` it is the tests' high-precision
reference.  ``sz_likelihood_add`` mirrors ``SZLikelihood_Add`` (:1385-1499).

Many of the reference's literals are default-real and are widened to double
where they meet one (``F32`` below); its completeness table is ``real(sp)``,
so a completeness is rounded to single precision before it is used.

The compiled reference's second pass over the catalogue (:1600-1608) reads
one line more than the file holds; the failed read leaves the last row's
values in place, so a last row at or above the S/N threshold enters twice
(its "total cat" line shows it).  The loader follows the compiled reference.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .ini import IniFile
from .likelihood import NativeCMBLikelihood, read_paramnames

LOGZERO = N.CMBL_LOGZERO
PARAM_NAMES = ["alpha_SZ", "ystar_SZ", "bias_SZ", "scatter_SZ", "beta_SZ"]
PRIOR_KEYS = ["prior_alpha_SZ", "prior_ystar_SZ", "prior_scatter_SZ", "prior_beta_SZ", "prior_wtg", "prior_lens",
              "prior_cccp", "prior_ns", "prior_omegabh2"]
FILE_KEYS = ["cat_file", "thetas_file", "skyfracs_file", "ylims_file"]
SERVED_KEYS = set(FILE_KEYS) | set(PRIOR_KEYS) | {"nuisance_params", "1D", "2D", "name"}


def F32(x) -> float:
    """A default-real literal widened to double."""
    return float(np.float32(x))


def _f32sq2(x) -> float:
    """2.*x**2. in single precision: the denominators of the priors (:1954-1972)."""
    x = np.float32(x)
    return float(np.float32(2) * np.float32(x * x))


Q_CUT = 6.0                      # q, the S/N threshold (massobservable :218)
THETASTAR = F32(6.997)
ALPHA_THETA = float(np.float32(1) / np.float32(3))
M2_3 = float(np.float32(-2) / np.float32(3))
M_PIVOT = F32(3.e14)
SQRT2 = float(np.sqrt(np.float32(2)))           # sqrt(2.) is a single-precision intrinsic
LNYMIN, LNYMAX, DLNY = -11.5, 10.0, F32(0.05)
NLNY = int((LNYMAX - LNYMIN) / DLNY)            # 429
DLNM = 0.05
STIRLING = F32(0.918939)
YSTAR_NORM = F32(0.00472724)
PI = 3.141592653589793238463
# (switch, centre, 2 sigma^2) of the Gaussian priors, in the order they are added
PRIOR_TABLE = {
    "prior_ystar_SZ": (F32(-0.186), _f32sq2(0.021)), "prior_alpha_SZ": (F32(1.789), _f32sq2(0.084)),
    "prior_scatter_SZ": (F32(0.075), _f32sq2(0.01)), "prior_beta_SZ": (F32(0.6666666), _f32sq2(0.5)),
    "prior_ns": (F32(0.9624), _f32sq2(0.014)), "prior_omegabh2": (F32(0.022), _f32sq2(0.002)),
    "prior_lens": (F32(0.99), _f32sq2(0.19)), "prior_wtg": (F32(0.688), _f32sq2(0.072)),
    "prior_cccp": (F32(0.780), _f32sq2(0.092))}


class SZFormatError(ValueError):
    pass


def _next_z(zi, binz):
    if zi < F32(0.2):
        return zi + F32(1.e-3)
    if zi <= 1.0:
        return zi + F32(1.e-2)
    return zi + binz


def _column(path, col=0):
    out = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if t and not t[0].startswith("#"):
                out.append(float(t[col].replace("D", "e").replace("d", "e")))
    return np.array(out, dtype=np.float64)


class SZDataset:
    """SZ_init and the fixed grids of deltaN_yz: z bins ``Z``, S/N bins ``logq``,
    ``thetas``, ``skyfracs``, ``ylims[patch][theta]``, the catalogue counts
    ``DNcat[Nz][nq]``, ``steps_z``, ``steps_m`` and the 0-based ``j1``, ``j2`` of
    every redshift bin (the trapezoid runs over steps j1 ... j2)."""

    def __init__(self, ini: str, overrides: dict | None = None):
        I = IniFile(ini)
        for k, v in (overrides or {}).items():
            I.set(k, v)
        for k in I.keys():
            if k not in SERVED_KEYS:
                raise NotImplementedError("SZ: key %s is not supported" % k)
        if I.read_bool("1D", False):
            raise NotImplementedError("SZ: 1D = T (the N(z) form) is not supported")
        self.ini = ini
        self.priors = {k: I.read_bool(k, False) for k in PRIOR_KEYS}
        base = os.path.dirname(os.path.abspath(ini))

        def path(key):
            if key not in I:
                raise SZFormatError("SZ: %s is missing" % key)
            v = I[key]
            return v if os.path.isabs(v) else os.path.join(base, v)
        self.param_names = read_paramnames(path("nuisance_params")) if "nuisance_params" in I else list(PARAM_NAMES)
        if len(self.param_names) != 5:
            raise SZFormatError("SZ: nuisance_params must name five parameters")
        self.thetas = _column(path("thetas_file"))
        self.skyfracs = _column(path("skyfracs_file"))
        yl = _column(path("ylims_file"))
        nth, npatch = len(self.thetas), len(self.skyfracs)
        if nth < 2:
            raise SZFormatError("SZ: fewer than two thetas")
        # the bracket's second theta (:1020-1027) is outside the reference's table when the nearest theta is the
        # first entry and larger than thp, or the last and smaller: the order in between is free
        if self.thetas[0] > self.thetas.min() or self.thetas[-1] < self.thetas.max():
            raise NotImplementedError("SZ: thetas_file must begin with its least theta and end with its greatest: "
                                      "the reference reads outside its table otherwise")
        if len(yl) != nth * npatch:
            raise SZFormatError("SZ: ylims has %d rows, expected %d" % (len(yl), nth * npatch))
        self.ylims = yl.reshape(nth, npatch).T.copy()                 # [patch][theta]; patch runs fastest in the file
        cat = np.stack([_column(path("cat_file"), c) for c in (0, 2)], axis=1)
        if len(cat) and cat[-1, 1] >= Q_CUT:                          # see the module docstring
            cat = np.vstack([cat, cat[-1:]])
        self.cat = cat[cat[:, 1] >= Q_CUT]

        z0, dz = 0.0, 0.1
        self.Nz = int((1.0 - z0) / dz) + 1
        logymin, logymax, dlogy = F32(0.7), F32(1.5), 0.25
        self.nq = int((logymax - logymin) / dlogy) + 2                # Ny + 1
        self.logq = np.empty(self.nq)
        yi = logymin + dlogy / 2.0
        for i in range(self.nq):
            self.logq[i] = yi
            yi = yi + dlogy
        self.Z = np.array([z0 + i * dz + 0.5 * dz for i in range(self.Nz)])
        self.Z[0] = self.Z[0] + F32(1.e-8)

        # catalogue counts (:1743-1797)
        Ny = self.nq - 1
        D = np.zeros((self.Nz, self.nq))
        zc, qc = self.cat[:, 0], self.cat[:, 1]
        edges = [(10.0 ** (self.logq[j] - dlogy / 2.0), 10.0 ** (self.logq[j] + dlogy / 2.0)) for j in range(Ny)]
        zlo, zhi = z0, z0 + dz
        for i in range(self.Nz):
            inz = (zc >= zlo) & (zc < zhi)
            for j in range(Ny):
                D[i, j] += np.count_nonzero(inz & (qc < edges[j][1]) & (qc >= edges[j][0]))
            D[i, Ny] += np.count_nonzero(inz & (qc >= edges[Ny - 1][1]))
            zlo, zhi = zlo + dz, zhi + dz
        for j in range(self.nq):
            for ii in range(len(zc)):
                hit = qc[ii] >= edges[j][0] and qc[ii] < edges[j][1] if j < Ny else qc[ii] >= edges[Ny - 1][1]
                if zc[ii] == -1 and hit:
                    norm = 0.0
                    for k in range(self.Nz):
                        norm = norm + D[k, j]
                    with np.errstate(all="ignore"):
                        D[:, j] = D[:, j] * (norm + 1.0) / np.float64(norm)
        self.DNcat = D

        # steps in z and ln M (:649-694)
        binz = self.Z[1] - self.Z[0]
        self.binz = binz
        min_z, max_z = self.Z[0] - 0.5 * binz, self.Z[-1] + 0.5 * binz
        zi = 0.0 if min_z < 0 else min_z
        sz = []
        while zi <= max_z:
            sz.append(zi)
            zi = _next_z(zi, binz)
        if sz[0] == 0:
            sz[0] = F32(1.e-5)
        self.steps_z = np.array(sz)
        nm = int((37.0 - 31.0) / DLNM)
        sm, lnm = [], 31.0
        for _ in range(nm):
            sm.append(lnm + DLNM / 2.0)
            lnm = lnm + DLNM
        self.steps_m = np.array(sm)
        self.j1 = np.array([int(np.argmin(np.abs(self.steps_z - (z - 0.5 * binz)))) for z in self.Z], dtype=np.int32)
        self.j2 = np.array([int(np.argmin(np.abs(self.steps_z - (z + 0.5 * binz)))) for z in self.Z], dtype=np.int32)
        # the ln Y grid (:975-1000, 1035-1047): lny accumulated, y0 = exp(lny)
        lny, l = np.empty(NLNY), LNYMIN
        for k in range(NLNY):
            lny[k] = l
            l = l + DLNY
        self.lny = lny
        self._erfs = {}

    @property
    def nzs(self):
        return len(self.steps_z)

    @property
    def nm(self):
        return len(self.steps_m)

    @property
    def n_theory(self):
        return 3 + 2 * self.nzs + self.nzs * self.nm

    def q_limits(self, T):
        """(qmin, qmax)[nq] as grid_C_2d forms them (:893, 987-990)."""
        dlogy = T(self.logq[1]) - T(self.logq[0])
        lq = self.logq.astype(T)
        return T(10) ** (lq - dlogy / T(2)), T(10) ** (lq + dlogy / T(2))

    def erfs(self, T=np.float64):
        """erfs[k][theta][qbin] (:975-1000): constant, patches summed in order."""
        key = np.dtype(T).name
        if key not in self._erfs:
            qmin, qmax = self.q_limits(T)
            y0 = np.exp(self.lny.astype(T))[:, None]
            out = np.zeros((NLNY, len(self.thetas), self.nq), dtype=T)
            for i in range(len(self.skyfracs)):
                y1 = self.ylims[i].astype(T)[None, :]
                out += _bin_compl(y0, y1, qmin, qmax, T) * T(self.skyfracs[i])
            self._erfs[key] = out
        return self._erfs[key]


def _erf(x, T):
    if np.dtype(T) == np.float64:
        from scipy.special import erf
        return erf(x)
    # long double: erf(x) = 2/sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!, every term of one sign
    x = np.asarray(x, dtype=T)
    ax = np.minimum(np.abs(x), T(7))
    term = ax.copy()
    s = ax.copy()
    x2 = T(2) * ax * ax
    for n in range(1, 260):
        term = term * x2 / T(2 * n + 1)
        s = s + term
    r = T(2) / np.sqrt(np.arccos(T(-1))) * np.exp(-ax * ax) * s
    r = np.where(np.abs(x) >= T(7), T(1), r)
    return np.where(x < 0, -r, r)


def _erf_compl(y, sn, q, T):
    arg = (y - q * sn) / T(SQRT2) / sn
    return (_erf(arg, T) + T(1)) / T(2)


def _bin_compl(y, sn, qmin, qmax, T):
    """c2[..., qbin] of :991-993 / :949-951 for broadcastable y and sn."""
    nq = len(qmin)
    e0 = _erf_compl(y, sn, T(Q_CUT), T)
    out = np.empty(np.broadcast(y, sn).shape + (nq,), dtype=T)
    for k in range(nq):
        if k == 0:
            out[..., k] = e0 * (T(1) - _erf_compl(y, sn, qmax[k], T))
        elif k == nq - 1:
            out[..., k] = e0 * _erf_compl(y, sn, qmin[k], T)
        else:
            out[..., k] = e0 * _erf_compl(y, sn, qmin[k], T) * (T(1) - _erf_compl(y, sn, qmax[k], T))
    return out


def _seqsum(a, axis=-1):
    """The running sum in index order, as a Fortran loop adds."""
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def sz_completeness(ds: SZDataset, row, nuis, dtype=np.float64):
    """completeness_2d[z][m][qbin] of grid_C_2d (:872-1059), rounded to single
    precision as the reference stores it, returned in ``dtype``."""
    T = np.dtype(dtype).type
    nzs, nm, nq, nth = ds.nzs, ds.nm, ds.nq, len(ds.thetas)
    row = np.asarray(row)
    H0 = T(row[0])
    E, dA = row[3:3 + nzs].astype(T), row[3 + nzs:3 + 2 * nzs].astype(T)
    alpha, logystar, bias, sigmaM, beta = (T(x) for x in nuis)
    ystar = T(10) ** logystar / (T(2) ** alpha) * T(YSTAR_NORM)
    m2 = np.exp(ds.steps_m.astype(T)) * bias
    h70 = H0 / T(70)
    dfac = T(100) * dA / T(500) / H0                                    # [nzs]
    mfac = m2 / T(M_PIVOT) * (T(100) / H0)                              # [nm]
    thp = (THETASTAR * h70 ** T(M2_3)) * mfac[None, :] ** T(ALPHA_THETA) * (E ** T(M2_3))[:, None] / dfac[:, None]
    yp = (ystar * h70 ** (T(-2) + alpha)) * mfac[None, :] ** alpha * (E ** beta)[:, None] / (dfac * dfac)[:, None]
    th = ds.thetas.astype(T)
    # the bracket (:1010-1028); the first minimum wins a tie
    near = np.argmin(np.abs(th[None, None, :] - thp[:, :, None]), axis=2)
    l1 = np.where(thp > th.max(), nth - 1, np.where(thp < th.min(), 0, near))
    l2 = np.where(thp > th.max(), nth - 2, np.where(thp < th.min(), 1, np.where(th[near] > thp, near - 1, near + 1)))
    l2 = np.where(l2 >= nth, nth - 2, l2)          # thp == the last theta: the weight of l2 is zero
    th1, th2 = th[l1], th[l2]
    w = (thp - th1)
    fsky = T(0)
    for s in ds.skyfracs:
        fsky = fsky + T(s)
    comp = np.zeros((nzs, nm, nq), dtype=np.float32)
    with np.errstate(all="ignore"):
        if sigmaM == 0:
            qmin, qmax = ds.q_limits(T)
            for i in range(len(ds.skyfracs)):
                yl = ds.ylims[i].astype(T)
                y1, y2 = yl[l1], yl[l2]
                y = y1 + (y2 - y1) / (th2 - th1) * w
                c2 = _bin_compl(yp, y, qmin, qmax, T)
                comp = (comp.astype(T) + c2 * T(ds.skyfracs[i])).astype(np.float32)    # a real(sp) running sum
            return comp.astype(T)
        erfs = ds.erfs(T)
        lny = ds.lny.astype(T)
        y0 = np.exp(lny)
        dy = y0[1:] - y0[:-1]
        fac = T(1) / np.sqrt(T(2) * T(PI) * sigmaM ** 2)
        mu = np.log(yp)
        for j in range(nzs):
            arg = (lny[None, :] - mu[j][:, None]) / (T(SQRT2) * sigmaM)        # [nm][N]
            g = np.exp(-arg ** 2)
            e1, e2 = erfs[:, l1[j], :], erfs[:, l2[j], :]                      # [N][nm][nq]
            win = e1 + (e2 - e1) / (th2[j] - th1[j])[None, :, None] * w[j][None, :, None]
            f = win * fac / y0[:, None, None] * g.T[:, :, None]                # [N][nm][nq]
            py = (f[:-1] + f[1:]) * T(0.5)
            v = _seqsum(py * dy[:, None, None], axis=0)                         # [nm][nq]
            v = np.where(v > fsky, fsky, v)
            v = np.where(v < 0, T(0), v)
            comp[j] = v.astype(np.float32)
    return comp.astype(T)


def sz_counts(ds: SZDataset, row, nuis, dtype=np.float64, comp=None):
    """DN[Nz][nq] of integrate_m_zq (:827-869): one running sum, z outer.
    ``comp``: sz_completeness of these arguments when the caller has it (it
    does not depend on the row's grid block)."""
    T = np.dtype(dtype).type
    nzs, nm = ds.nzs, ds.nm
    if comp is None:
        comp = sz_completeness(ds, row, nuis, dtype)
    grid = np.asarray(row)[3 + 2 * nzs:3 + 2 * nzs + nzs * nm].astype(T).reshape(nzs, nm)
    sz = ds.steps_z.astype(T)
    DN = np.zeros((ds.Nz, ds.nq), dtype=T)
    with np.errstate(all="ignore"):
        fc = grid[:, :, None] * comp                                              # [nzs][nm][nq]
        terms = T(0.5) * (fc[:-1] + fc[1:]) * (sz[1:] - sz[:-1])[:, None, None] * T(DLNM)
        for i in range(ds.Nz):
            a, b = int(ds.j1[i]), int(ds.j2[i])
            if b > a:
                DN[i] = _seqsum(terms[a:b].reshape((b - a) * nm, ds.nq), axis=0)
    return DN


def sz_loglike_host(ds, row, nuis, dtype=np.float64, DN=None):
    """-lnL of SZCC_Cash (:1825-1975) for one theory row and the five nuisance
    values; ``ds`` an SZDataset or an ini path.  LOGZERO where it is not finite.
    ``DN``: the predicted counts when the caller has them (sz_counts: they do
    not depend on the prior switches)."""
    D = ds if isinstance(ds, SZDataset) else SZDataset(ds)
    T = np.dtype(dtype).type
    if DN is None:
        DN = sz_counts(D, row, nuis, dtype)
    alpha, logystar, bias, sigmaM, beta = (T(x) for x in nuis)
    ns, ombh2 = T(np.asarray(row)[1]), T(np.asarray(row)[2])
    s = T(0)
    with np.errstate(all="ignore"):
        for i in range(D.Nz):
            for j in range(D.nq):
                if DN[i, j] != 0:
                    c = T(D.DNcat[i, j])
                    lnf = T(0)
                    if c != 0:
                        if c > 10:
                            lnf = T(STIRLING) + (c + T(0.5)) * np.log(c) - c
                        else:
                            fact = T(1)
                            for ii in range(1, int(c) + 1):
                                fact = T(ii) * fact
                            lnf = np.log(fact)
                    s = s - T(1) * (c * np.log(DN[i, j]) - DN[i, j] - lnf)

        def pr(key, x):
            c, d = PRIOR_TABLE[key]
            return T(1.0 if D.priors[key] else 0.0) * (x - T(c)) ** 2 / T(d)
        s = s + pr("prior_ystar_SZ", logystar) + pr("prior_alpha_SZ", alpha) + pr("prior_scatter_SZ", sigmaM)
        s = s + pr("prior_beta_SZ", beta)
        s = s + pr("prior_ns", ns) + pr("prior_omegabh2", ombh2)
        s = s + pr("prior_lens", T(1) / bias)
        s = s + pr("prior_wtg", bias)
        s = s + pr("prior_cccp", bias)
    return s if np.isfinite(s) else T(LOGZERO)


# ---------------------------------------------------------------- theory row

RHOCRIT0 = 2.7751973751261264e11
DEG2 = 3.046174198e-4 * 41253.0
C_KMS5 = 3.0e8 / 1.0e5                      # c / 1.0d5 with the reference's c = 3.0d8
_TINKER_DEL = np.log10(np.array([200., 300., 400., 600., 800., 1200., 1600., 2400., 3200.]))
_TINKER = {
    "aa": ([0.186, 0.200, 0.212, 0.218, 0.248, 0.255, 0.260, 0.260, 0.260],
           [0.00, 0.50, -1.56, 3.05, -2.95, 1.07, -0.71, 0.21, 0.00]),
    "a": ([1.47, 1.52, 1.56, 1.61, 1.87, 2.13, 2.30, 2.53, 2.66],
          [0.00, 1.19, -6.34, 21.36, -10.95, 2.59, -0.85, -2.07, 0.00]),
    "b": ([2.57, 2.25, 2.05, 1.87, 1.59, 1.51, 1.46, 1.44, 1.41],
          [0.00, -1.08, 12.61, -20.96, 24.08, -6.64, 3.84, -2.09, 0.00]),
    "c": ([1.19, 1.27, 1.34, 1.45, 1.58, 1.80, 1.97, 2.24, 2.44],
          [0.00, 0.94, -0.43, 4.61, 0.01, 1.21, 1.43, 0.33, 0.00])}


def _splint(xa, ya, y2a, x):
    """The cubic-spline evaluation of the Tinker parameter tables (:563-584)."""
    klo, khi = 0, len(xa) - 1
    while khi - klo > 1:
        k = (khi + klo + 2) // 2 - 1
        if xa[k] > x:
            khi = k
        else:
            klo = k
    h = xa[khi] - xa[klo]
    a, b = (xa[khi] - x) / h, (x - xa[klo]) / h
    return a * ya[klo] + b * ya[khi] + ((a ** 3 - a) * y2a[klo] + (b ** 3 - b) * y2a[khi]) * h ** 2 / 6.0


def sz_theory_row(ds: SZDataset, H0, omegam, omegav, omegak, w0, ns, ombh2, sigma_R, use_watson=False):
    """The theory row of a cosmology.  ``sigma_R`` is ``(R, sigma)``: a table of
    sigma(R) at z = 0, R in Mpc / h, splined (natural cubic) as the reference's
    TCubicSpline does.  E(z) of :74-83 with w1 = 0, dA of :128-173, the growth
    factor of :270-333 (the ODE from z = 1000, normalised to 1 today), the
    Tinker (default) or Watson mass function of :366-560 at Delta = 500
    critical, and get_grid (:1317-1334).  The reference integrates 1 / E and the
    growth ODE to relative tolerances of 1e-5 and 1e-8; here both are integrated
    to 1e-12, so the rows agree to the reference's tolerance."""
    from scipy.integrate import quad, solve_ivp
    from scipy.interpolate import CubicSpline
    sz, sm = ds.steps_z, ds.steps_m

    def E(z):
        a = 1.0 / (1.0 + z)
        return np.sqrt(omegam * a ** -3 + omegav * a ** (-3.0 * (1.0 + w0)) + omegak * a ** -2)

    def Om(z):
        return omegam * (1.0 + z) ** 3 / E(z) ** 2

    def Ode(z):
        return omegav * (1.0 + z) ** (3.0 * (1.0 + w0)) / E(z) ** 2

    def r(z):
        integ = quad(lambda x: 1.0 / E(x), 0.0, z, epsabs=0, epsrel=1e-12)[0]
        if omegak == 0:
            return C_KMS5 * integ
        if omegak > 0:
            return 3.0e8 / np.sqrt(omegak) * np.sinh(np.sqrt(omegak) * integ) / 1.0e5
        return 3.0e8 / np.sqrt(-omegak) * np.sin(np.sqrt(-omegak) * integ) / 1.0e5

    def rhs(a, y):
        z = 1.0 / a - 1.0
        ok = 1.0 - Om(z) - Ode(z)
        return [-1.5 * (1.0 + ok / 3.0 - w0 * Ode(z)) * y[0] / a + 1.5 * Om(z) * y[1] / a / a, y[0]]
    a_of = 1.0 / (1.0 + sz[::-1])                                     # increasing a
    sol = solve_ivp(rhs, (1.0 / 1001.0, 1.0), [1.0, 0.0], method="DOP853", t_eval=np.append(a_of, 1.0),
                    rtol=1e-12, atol=1e-14)
    growth = (sol.y[1][:-1] / sol.y[1][-1])[::-1]

    R_tab, s_tab = (np.asarray(x, dtype=np.float64) for x in sigma_R)
    spl = CubicSpline(R_tab, s_tab, bc_type="natural")
    rhom0 = omegam * RHOCRIT0
    M = np.exp(sm)
    R = (0.75 * M / PI / rhom0) ** (1.0 / 3.0)
    dMdR = 3 * M / R
    sR, dsR = spl(R), spl(R, 1)
    Es = np.array([E(z) for z in sz])
    rs = np.array([r(z) for z in sz])
    row = np.empty(ds.n_theory)
    row[:3] = H0, ns, ombh2
    row[3:3 + len(sz)] = Es
    row[3 + len(sz):3 + 2 * len(sz)] = rs / (1.0 + sz)
    grid = np.empty((len(sz), len(sm)))
    for j, z in enumerate(sz):
        g = growth[j]
        dsoz = 500.0 / Om(z)
        if use_watson:
            A, eps, B, p = 0.282, 2.163, 1.406, 1.210
            f = A * ((g * sR / B) ** (-eps) + 1.0) * np.exp(-p / sR / sR / g / g)
            ddz = -0.456 * Om(z) - F32(0.139)
            CD = np.exp(0.023 * (dsoz / 178.0 - 1.0)) * F32(0.947)
            f = f * CD * (dsoz / 178.0) ** ddz * np.exp(0.072 * (1.0 - dsoz / 178.0) / (sR * g) ** 2.130)
        else:
            x = np.log10(dsoz)
            p1, p2, p3, p4 = (_splint(_TINKER_DEL, np.array(_TINKER[k][0]), np.array(_TINKER[k][1]), x)
                              for k in ("aa", "a", "b", "c"))
            al = 10 ** (-((0.75 / np.log10(dsoz / 75.0)) ** 1.2))
            A, eps, B = p1 * (1.0 + z) ** -0.14, p2 * (1.0 + z) ** -0.06, p3 * (1.0 + z) ** -al
            f = A * ((g * sR / B) ** (-eps) + 1.0) * np.exp(-p4 / sR / sR / g / g)
        vol = C_KMS5 * rs[j] ** 2 / Es[j]
        grid[j] = -rhom0 * f * dsR / dMdR / sR * DEG2 * vol
    row[3 + 2 * len(sz):] = grid.ravel()
    return row


# ---------------------------------------------------------------- the library's likelihood

class SZLikelihood(NativeCMBLikelihood):
    """The SZ cluster counts in the HIP library.  ``loglike_batch(dl, nuis)`` takes
    ``dl`` as a cuda float64 tensor [W, 1, n_theory] of theory rows (or [W, nf,
    L >= n_theory]: field 0 is read) and ``nuis`` [W, 5]."""
    LikelihoodType = "SZ"

    def __init__(self, ini: str, overrides: dict | None = None, use_watson: bool = False):
        super().__init__("SZ", ini, overrides)
        self.name = "SZ"
        self.tag = "SZ"
        self.use_watson = bool(use_watson)
        self.ini, self._overrides, self._ds = ini, dict(overrides or {}), None
        self.n_theory = N.lib().cmbl_theory_len(self._h)
        dims = (C.c_int * 8)()
        N.check(N.lib().cmbl_sz_info(self._h, dims), self._h)
        (self.nzs, self.nm, self.Nz, self.nq, self.n_thetas, self.n_patches, self.n_lny, self.n_cat) = list(dims)

    def loader_arrays(self):
        """(steps_z, DNcat [Nz][nq], j1, j2) as the library's loader built them (cmbl_sz_arrays)."""
        sz, dn = np.zeros(self.nzs), np.zeros((self.Nz, self.nq))
        j1, j2 = np.zeros(self.Nz, dtype=np.int32), np.zeros(self.Nz, dtype=np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        N.check(N.lib().cmbl_sz_arrays(self._h, sz.ctypes.data_as(dp), dn.ctypes.data_as(dp), j1.ctypes.data_as(ip),
                                       j2.ctypes.data_as(ip)), self._h)
        return sz, dn, j1, j2

    @property
    def ds(self) -> SZDataset:
        """The loader's view on the host (steps_z, steps_m), to build theory rows."""
        if self._ds is None:
            self._ds = SZDataset(self.ini, self._overrides)
        return self._ds


def sz_likelihood_add(like_list, ini: IniFile):
    """SZLikelihood_Add (:1385-1499): ``use_SZ``, ``1D``, ``2D``, the ``prior_*``
    switches and ``use_watson`` of the run ini.  The data set is ``sz_dataset``,
    the project's own ini with the four file paths (the reference opens
    ``data/SZ_*.txt`` by name); the run ini's switches override its own.  The
    term is named SZ (the chain column chi2_SZ) and takes its parameter names
    from ``SZ.paramnames`` beside the data, as the reference's does."""
    if not ini.read_bool("use_SZ", False):
        return []
    one_d, two_d = ini.read_bool("1D", False), ini.read_bool("2D", False)
    if one_d and two_d:
        raise ValueError("SZ: 1D and 2D likelihood both selected")
    if "sz_dataset" not in ini:
        raise ValueError("SZ: use_SZ = T needs sz_dataset = <ini with cat_file, thetas_file, skyfracs_file, ylims_file>")
    over = {k: ini[k] for k in PRIOR_KEYS + ["1D", "2D"] if k in ini}
    dataset = ini.relative_filename("sz_dataset")
    pn = os.path.join(os.path.dirname(os.path.abspath(dataset)), "SZ.paramnames")
    if "nuisance_params" not in IniFile(dataset) and os.path.exists(pn):
        over["nuisance_params"] = pn
    like = SZLikelihood(dataset, over, use_watson=ini.read_bool("use_watson", False))
    spd = ini.get("sz_dataset_speed")
    if spd is not None:
        like.speed = int(spd)
    like_list.add(like)
    return [like]
