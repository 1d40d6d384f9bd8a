"""Galaxy power-spectrum likelihoods (source/mpk.f90, source/wigglez.f90):
``use_mpk`` (SDSS LRG DR4 and data sets of its format) and ``use_wigglez_mpk``
(the four WiggleZ redshift bins, with the GiggleZ correction).

Neither has sampled nuisance parameters: bias and Q are marginalised inside
the likelihood.  A walker's theory is one row of ``2 + nk`` doubles,

    [ a_scl, kh_min, P_0 .. P_{nk-1} ]

a_scl = DV_fid / (H0 D_V(z)) (1 without use_scaling; compute_scaling_factor,
mpk.f90:46-56), kh_min the lower edge of the provider's k grid (exp(PK%x(1)))
and P_i = PowerAt(max(kh_min, a_scl k_i), z) as the provider's interpolator
returns it -- before the division by a_scl^3 and before the GiggleZ factor.
``mpk_theory_row`` builds it from a callable P(k).  Everything after it
(MPK_LnLike :312-407, WiggleZ_LnLike :545-641) is done by the library's
kernels (csrc/mpk.hip, tags ``"MPK"`` and ``"WIGGLEZ"``) and restated here in
numpy (``mpk_loglike_host``, ``wigglez_loglike_host``) in any float type.

Roundings of the reference that the restatement makes explicit:
 * dQ = 0.4 is a default-real literal, and Ag, Q_mid, Q_sigma are read with
   Read_Real: all are single-precision values widened to double;
 * the last coefficient of the GiggleZ polynomial of bins 3 and 4 is a
   default-real literal (41.2564, 132.782);
 * in WiggleZ_LnLike normV, Q and minchisq are ``real``: single precision.
   normV is also not reset between the points of the Q grid, so with
   Q_marge = T, Q_flat = F, Q_sigma != 0 point iQ divides by the running sum
   over the points so far.

Where the reference stops the program (a non-finite row entry, a_scl <= 0, a
k outside the GiggleZ spline, a 2 x 2 matrix that is not positive definite,
normV <= 0) or would return a non-finite value, the value is logZero.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .derivedlike import _DerivedLike
from .ini import IniFile
from .likelihood import NativeCMBLikelihood

LOGZERO = N.CMBL_LOGZERO


def F32(x) -> float:
    """A default-real literal, or a value read with Read_Real, widened to double."""
    return float(np.float32(x))


NQ = 6
DQ = F32(0.4)
ZBINS = (0.22, 0.41, 0.6, 0.78)
GIGGLEZ_NUMK = 500
GIGGLEZ_FILES = ["gigglezfiducialmodel_matterpower_%s.dat" % c for c in "abcd"]
# log10 of the GiggleZ-to-initial-conditions ratio: the degree-5 polynomial fit
# of every redshift bin (Parkinson et al. 2012, arXiv:1210.2130), lowest order first
GIGGLEZ_POLY = [[4.619, -13.7787, 58.941, -175.24, 284.321, -187.284],
                [4.63079, -12.6293, 42.9265, -91.8068, 97.808, -37.633],
                [4.69659, -12.7287, 42.5681, -89.5578, 96.664, -F32(41.2564)],
                [4.6849, -13.4747, 53.7172, -145.832, 216.638, -F32(132.782)]]
# TWiggleZCommon_ReadIni's keys in its order: regions 5-7 are asked for as 1-hr, 3-hr, 0-hr (:234-251)
REGION_KEYS = ["Use_9-hr_region", "Use_11-hr_region", "Use_15-hr_region", "Use_22-hr_region", "Use_1-hr_region",
               "Use_3-hr_region", "Use_0-hr_region"]
WIGGLEZ_REGION_ROWS = 50          # the rows of a switched-off region the reference skips (:373)
Q_NONE, Q_FLAT, Q_GAUSS, Q_POINT = 0, 1, 2, 3      # cmbl_mpk_info's Q mode

COMMON_KEYS = {"name", "num_mpk_points_full", "num_mpk_kbands_full", "min_mpk_points_use", "max_mpk_points_use",
               "min_mpk_kbands_use", "max_mpk_kbands_use", "use_scaling", "Q_marge", "Q_flat", "Q_mid", "Q_sigma", "Ag",
               "num_conflicts", "type_conflict1", "name_conflict1"}
FILE_KEYS = {"kbands_file", "measurements_file", "windows_file", "cov_file"}
MPK_KEYS = COMMON_KEYS | FILE_KEYS | {"DV_fid", "redshift", "mpk_dataset_nonlinear"}
WIGGLEZ_KEYS = COMMON_KEYS | FILE_KEYS | set(REGION_KEYS) | {"DV_fid", "redshift", "Use_gigglez", "nonlinear_wigglez",
                                                             "gigglez_dir"}


class MPKFormatError(ValueError):
    pass


def _num(t):
    return float(t.replace("D", "e").replace("d", "e"))


def _data_lines(path):
    with open(path) as f:
        return [ln for ln in f.read().split("\n")]


def _text_vector(path, n):
    v = [_num(ln.split()[0]) for ln in _data_lines(path) if ln.strip() and not ln.lstrip().startswith("#")]
    if len(v) < n:
        raise MPKFormatError("%s holds %d values, fewer than %d" % (path, len(v), n))
    return np.array(v[:n], dtype=np.float64)


def _text_matrix(path, m, n):
    rows = [[_num(t) for t in ln.split()] for ln in _data_lines(path) if ln.strip() and not ln.lstrip().startswith("#")]
    if len(rows) < m or any(len(r) < n for r in rows[:m]):
        raise MPKFormatError("%s is not a %d x %d matrix" % (path, m, n))
    return np.array([r[:n] for r in rows[:m]], dtype=np.float64)


def _region_matrices(path, nreg, m, n):
    """ReadWiggleZMatrices (:439-471): one comment line, then m rows of n numbers, for every region."""
    lines = [ln for ln in _data_lines(path) if ln.strip()]
    if len(lines) < nreg * (m + 1):
        raise MPKFormatError("%s holds %d lines, fewer than %d regions x (1 + %d)" % (path, len(lines), nreg, m))
    out = np.zeros((nreg, m, n))
    for r in range(nreg):
        for j in range(m):
            t = lines[r * (m + 1) + 1 + j].split()
            if len(t) < n:
                raise MPKFormatError("%s: region %d row %d holds %d numbers, fewer than %d" % (path, r + 1, j + 1, len(t), n))
            out[r, j] = [_num(x) for x in t[:n]]
    return out


def chol_inverse(M, T=np.float64):
    """Matrix_Inverse (dpotrf 'L', dpotri 'L', mirrored): the inverse of a
    symmetric positive definite matrix in the float type T; None if it is not."""
    A = np.array(M, dtype=T)
    n = len(A)
    L = np.zeros((n, n), dtype=T)
    for j in range(n):
        if abs(A[j, j]) < 1e-30:
            return None
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum() if j else A[j, j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    Li = np.zeros((n, n), dtype=T)
    for j in range(n):
        Li[j, j] = T(1) / L[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(L[i, j:i] * Li[j:i, j]).sum() / L[i, i]
    return Li.T @ Li


class _PKDataset:
    """What both loaders share: the selections, the Q settings and the scaling."""

    def _read_common(self, I):
        name = I.get("name", "")
        if name in ("twodf", "lrg_2009"):
            raise NotImplementedError("%s is not supported (the reference stops on it)" % name)
        self.name = name
        self.npf, self.nkf = I.read_int("num_mpk_points_full", 0), I.read_int("num_mpk_kbands_full", 0)
        if self.npf <= 0 or self.nkf <= 0:
            raise MPKFormatError("num_mpk_points_full and num_mpk_kbands_full must be set")
        self.minp, self.maxp = I.read_int("min_mpk_points_use", 1), I.read_int("max_mpk_points_use", self.npf)
        self.mink, self.maxk = I.read_int("min_mpk_kbands_use", 1), I.read_int("max_mpk_kbands_use", self.nkf)
        if not (1 <= self.minp <= self.maxp <= self.npf and 1 <= self.mink <= self.maxk <= self.nkf):
            raise MPKFormatError("the points or kbands selection is outside the files")
        self.np, self.nk = self.maxp - self.minp + 1, self.maxk - self.mink + 1
        self.use_scaling = I.read_bool("use_scaling", False)
        self.Q_marge = I.read_bool("Q_marge", False)
        self.Q_flat = self.Q_marge and I.read_bool("Q_flat", False)
        self.Q_mid = self.Q_sigma = 0.0
        self.Ag = F32(1.4)
        if self.Q_marge:
            if not self.Q_flat:
                if "Q_mid" not in I or "Q_sigma" not in I:
                    raise MPKFormatError("Q_marge = T without Q_flat needs Q_mid and Q_sigma")
                self.Q_mid, self.Q_sigma = F32(_num(I["Q_mid"])), F32(_num(I["Q_sigma"]))
            self.Ag = F32(_num(I.get("Ag", "1.4")))
        self.q_mode = Q_NONE if not self.Q_marge else Q_FLAT if self.Q_flat else Q_POINT if self.Q_sigma == 0 else Q_GAUSS

    def _read_scaling(self, I):
        self.DV_fid = 0.0
        if self.use_scaling:
            if "DV_fid" not in I or _num(I["DV_fid"]) == -1.0:
                raise MPKFormatError("use_scaling = T and no DV_fid given for dataset %s" % self.name)
            self.DV_fid = _num(I["DV_fid"])

    def invcov_as(self, T):
        """[regions][np][np] inverse covariance (Matrix_Inverse of the selected block) in the float type T."""
        key = np.dtype(T).name
        if key not in self._invcov:
            inv = [chol_inverse(c, T) for c in self.cov]
            if any(x is None for x in inv):
                raise MPKFormatError("%s: a covariance block is not positive definite" % self.name)
            self._invcov[key] = np.array(inv, dtype=T)
        return self._invcov[key]

    @property
    def n_theory(self):
        return 2 + self.nk


class MPKDataset(_PKDataset):
    """MPK_ReadIni (mpk.f90:117-244): ``k`` [nk], ``P`` and ``sdev`` [np], ``W``
    [np][nk], ``cov`` [1][np][np] or None, the Q settings, ``use_scaling``,
    ``DV_fid``, ``redshift``; ``nonlinear`` is the run ini's
    mpk_dataset_nonlinear, which only says which P(k) the provider is to use."""
    wigglez = False

    def __init__(self, dataset: str, overrides: dict | None = None):
        I = IniFile(dataset)
        for k, v in (overrides or {}).items():
            I.set(k, v)
        for k in I.keys():
            if k not in MPK_KEYS:
                raise NotImplementedError("MPK: key %s is not supported" % k)
        self.dataset, self._invcov = dataset, {}
        self._read_common(I)
        self.nonlinear = I.read_bool("mpk_dataset_nonlinear", False)
        self.k = _text_vector(I.relative_filename("kbands_file"), self.nkf)[self.mink - 1:self.maxk]
        rows = [ln.split() for ln in _data_lines(I.relative_filename("measurements_file"))[2:] if ln.strip()]
        if len(rows) < self.maxp or any(len(r) < 6 for r in rows[:self.maxp]):
            raise MPKFormatError("Error reading mpk file: the measurements hold fewer than %d rows of 6" % self.maxp)
        sel = np.array([[_num(x) for x in r[:6]] for r in rows[self.minp - 1:self.maxp]])
        self.P, self.sdev = sel[:, 3].copy(), sel[:, 4].copy()
        W = _text_matrix(I.relative_filename("windows_file"), self.npf, self.nkf)
        self.W = W[self.minp - 1:self.maxp, self.mink - 1:self.maxk][None].copy()
        self.cov = None
        if I.get("cov_file", ""):
            c = _text_matrix(I.relative_filename("cov_file"), self.npf, self.npf)
            self.cov = c[self.minp - 1:self.maxp, self.minp - 1:self.maxp][None].copy()
        self.P = self.P[None]
        self.nr, self.zbin, self.use_gigglez = 1, 0, False
        self._read_scaling(I)
        self.redshift = _num(I.get("redshift", "0.35"))


class WiggleZDataset(_PKDataset):
    """TWiggleZCommon_ReadIni and WiggleZ_ReadIni (wigglez.f90:203-437) for one
    redshift bin: ``k`` [nk], and per active region ``P`` [nr][np], ``W``
    [nr][np][nk], ``cov`` [nr][np][np]; ``regions`` the 1-based regions in use,
    ``zbin`` 1..4, and with ``use_gigglez`` the fiducial spline ``gk``, ``gf`` (ln P)
    of that bin.  The keys of the common file, Use_gigglez and nonlinear_wigglez
    arrive as overrides (``wigglez_overrides`` merges them)."""
    wigglez = True

    def __init__(self, dataset: str, overrides: dict | None = None):
        I = IniFile(dataset)
        for k, v in (overrides or {}).items():
            I.set(k, v)
        for k in I.keys():
            if k not in WIGGLEZ_KEYS:
                raise NotImplementedError("WiggleZ: key %s is not supported" % k)
        self.dataset, self._invcov = dataset, {}
        self._read_common(I)
        self.use_gigglez, self.nonlinear = I.read_bool("Use_gigglez", False), I.read_bool("nonlinear_wigglez", False)
        self.regions = [r + 1 for r, key in enumerate(REGION_KEYS) if I.read_bool(key, False)]
        if not self.regions:
            raise MPKFormatError("WiggleZ_mpk: no regions being used in this data set")
        if self.use_gigglez and not self.nonlinear:
            raise MPKFormatError("the GiggleZ prescription needs nonlinear_wigglez = T")
        self.nr = len(self.regions)
        self.redshift = _num(I.get("redshift", "0"))
        zb = [i + 1 for i, z in enumerate(ZBINS) if abs(self.redshift - z) <= 0.001]
        if not zb:
            raise MPKFormatError("WiggleZMPK: could not identify the redshift %r" % self.redshift)
        self.zbin = zb[-1]
        self.k = _text_vector(I.relative_filename("kbands_file"), self.nkf)[self.mink - 1:self.maxk]
        lines = [ln for ln in _data_lines(I.relative_filename("measurements_file")) if ln.strip()]
        P, at = [], 0
        for r in range(7):
            rows = self.npf if r + 1 in self.regions else WIGGLEZ_REGION_ROWS
            block = lines[at + 2:at + 2 + rows]
            if len(block) < rows:
                raise MPKFormatError("Error reading WiggleZ mpk file: region %d is short" % (r + 1))
            if r + 1 in self.regions:
                P.append([_num(ln.split()[3]) for ln in block[self.minp - 1:self.maxp]])
            at += 2 + rows
        self.P = np.array(P, dtype=np.float64)
        act = [r - 1 for r in self.regions]
        W = _region_matrices(I.relative_filename("windows_file"), 7, self.npf, self.nkf)
        self.W = W[act][:, self.minp - 1:self.maxp, self.mink - 1:self.maxk].copy()
        if not I.get("cov_file", ""):
            raise MPKFormatError("WiggleZ: cov_file is missing")       # WiggleZ_LnLike reads mpk_invcov unconditionally
        c = _region_matrices(I.relative_filename("cov_file"), 7, self.npf, self.npf)
        self.cov = c[act][:, self.minp - 1:self.maxp, self.minp - 1:self.maxp].copy()
        self.sdev = None
        self._read_scaling(I)
        self.gk = self.gf = None
        if self.use_gigglez:
            gdir = I.get("gigglez_dir", "") or os.path.dirname(os.path.abspath(dataset))
            rows = [ln.split() for ln in _data_lines(os.path.join(gdir, GIGGLEZ_FILES[self.zbin - 1])) if ln.strip()]
            if len(rows) < GIGGLEZ_NUMK:
                raise MPKFormatError("Error reading model or fiducial theory files.")
            self.gk = np.array([_num(r[0]) for r in rows[:GIGGLEZ_NUMK]])
            self.gp = np.array([_num(r[1]) for r in rows[:GIGGLEZ_NUMK]])
        self._spl = {}

    def gigglez_spline(self, T):
        """(knots, ln P, second derivatives): GiggleZPK%Init(kval, log(power_nl)), the natural spline of Interpolation.f90:693-734."""
        key = np.dtype(T).name
        if key not in self._spl:
            x, y = self.gk.astype(T), np.log(self.gp.astype(T))
            n = len(x)
            d2, u = np.zeros(n, dtype=T), np.zeros(n, dtype=T)
            d1r = (y[1] - y[0]) / (x[1] - x[0])
            for i in range(1, n - 1):
                d1l = d1r
                d1r = (y[i + 1] - y[i]) / (x[i + 1] - x[i])
                xxdiv = T(1) / (x[i + 1] - x[i - 1])
                sig = (x[i] - x[i - 1]) * xxdiv
                xp = T(1) / (sig * d2[i - 1] + T(2))
                d2[i] = (sig - T(1)) * xp
                u[i] = (T(6) * (d1r - d1l) * xxdiv - sig * u[i - 1]) * xp
            d2[n - 1] = T(0)
            for i in range(n - 2, -1, -1):
                d2[i] = d2[i] * d2[i + 1] + u[i]
            self._spl[key] = (x, y, d2)
        return self._spl[key]


def wigglez_overrides(common: str, use_gigglez: bool, nonlinear: bool, gigglez_dir: str | None = None) -> dict:
    """The keys of the wigglez_common_dataset file plus Use_gigglez and
    nonlinear_wigglez (and gigglez_dir), as the overrides one bin's dataset is opened with."""
    I = IniFile(common)
    over = {k: I[k] for k in I.keys() if k != "name"}
    over["Use_gigglez"] = "T" if use_gigglez else "F"
    over["nonlinear_wigglez"] = "T" if nonlinear else "F"
    if gigglez_dir:
        over["gigglez_dir"] = gigglez_dir
    return over


# ---------------------------------------------------------------- the host restatement

def _matvec(M, x):
    """matmul(M, x) with every element's sum taken in the order of the columns."""
    acc = M[:, 0] * x[0]
    for j in range(1, M.shape[1]):
        acc = acc + M[:, j] * x[j]
    return acc


def _ssum(a):
    s = a[0]
    for x in a[1:]:
        s = s + x
    return s


def _finite(x):
    return bool(np.all(np.isfinite(np.asarray(x, dtype=np.float64))))


def _lin(ds, row, T):
    """k_scaled and mpk_lin (with the GiggleZ factor), or None where the reference stops."""
    row = np.asarray(row)
    if len(row) < 2 + ds.nk:
        raise ValueError("the theory row holds %d doubles, not %d" % (len(row), 2 + ds.nk))
    if not _finite(row[:2 + ds.nk]):
        return None
    a, khmin, P = T(row[0]), T(row[1]), row[2:2 + ds.nk].astype(T)
    if not a > 0:
        return None
    ak = a * ds.k.astype(T)
    ks = np.where(ak > khmin, ak, khmin)
    lin = P / (a * a * a)
    if ds.use_gigglez:
        x, y, d2 = ds.gigglez_spline(T)
        tol = (x[1] - x[0]) * T(1e-5)
        if np.any(ks < x[0] - tol) or np.any(ks > x[-1]):
            return None
        c = [T(v) for v in GIGGLEZ_POLY[ds.zbin - 1]]
        k2 = ks * ks
        k3, k4 = k2 * ks, k2 * k2
        k5 = k4 * ks
        fidz = c[0] + c[1] * ks + c[2] * k2 + c[3] * k3 + c[4] * k4 + c[5] * k5
        lo = np.clip(np.searchsorted(x, ks, side="left") - 1, 0, len(x) - 2)
        xlo, xhi = x[lo], x[lo + 1]
        ho = xhi - xlo
        a0 = (xhi - ks) / ho
        b0 = T(1) - a0
        s = b0 * y[lo + 1] + a0 * (y[lo] - b0 * ((a0 + T(1)) * d2[lo] + (T(2) - a0) * d2[lo + 1]) * (ho * ho) / T(6))
        lin = lin * (T(10) ** fidz) / np.exp(s)
    return ks, lin


def _flat_2x2(M11, M22, M12, v1, v2, final, T):
    """log det, Matrix_Inverse(Mat) and the quadratic form of the Q_flat branch; None where the reference stops."""
    det = M11 * M22 - M12 * M12
    if not det > 0 or abs(M11) < 1e-30 or abs(M22) < 1e-30 or not M11 > 0:
        return None
    lndet = np.log(det)
    L11 = np.sqrt(M11)
    L21 = M12 / L11
    d = M22 - L21 * L21
    if not d > 0:
        return None
    L22 = np.sqrt(d)
    i11, i22 = T(1) / L11, T(1) / L22
    i21 = -(L21 * i11) * i22
    A11, A21, A22 = i11 * i11 + i21 * i21, i22 * i21, i22 * i22
    quad = v1 * (A11 * v1 + A21 * v2) + v2 * (A21 * v1 + A22 * v2)
    return (final - quad + lndet) / T(2)


def _calweights(T):
    return np.array([np.exp(-(T(iQ) * T(DQ)) ** 2 / T(2)) for iQ in range(-NQ, NQ + 1)], dtype=T)


def _out(v):
    v = float(v) if v is not None else float("nan")
    return v if np.isfinite(v) else LOGZERO


def mpk_loglike_host(ds: MPKDataset, row, dtype=np.float64):
    """MPK_LnLike (mpk.f90:289-407) at one theory row, in the float type dtype."""
    T = dtype
    r = _lin(ds, row, T)
    if r is None:
        return LOGZERO
    ks, lin = r
    W, P = ds.W[0].astype(T), ds.P[0].astype(T)
    Ag, Qmid, Qsig, dQ = T(ds.Ag), T(ds.Q_mid), T(ds.Q_sigma), T(DQ)
    inv = ds.invcov_as(T)[0] if ds.cov is not None else None
    w = T(1) / (ds.sdev.astype(T) ** 2) if inv is None else None
    if ds.Q_marge and ds.Q_flat:
        Pth = lin / (T(1) + Ag * ks)
        k2 = Pth * (ks * ks)
        WP, WP2 = _matvec(W, Pth), _matvec(W, k2)
        if inv is not None:
            covdat, covth, covth2 = _matvec(inv, P), _matvec(inv, WP), _matvec(inv, WP2)
        else:
            covdat, covth, covth2 = P * w, WP * w, WP2 * w
        return _out(_flat_2x2(_ssum(covth * WP), _ssum(covth2 * WP2), _ssum(covth * WP2), _ssum(covdat * WP),
                              _ssum(covdat * WP2), _ssum(P * covdat), T))
    do_marge = ds.Q_marge and ds.Q_sigma != 0
    chisq = np.zeros(2 * NQ + 1, dtype=T)
    for iQ in range(-NQ, NQ + 1):
        Q = Qmid + T(iQ) * Qsig * dQ
        Pth = lin * (T(1) + Q * (ks * ks)) / (T(1) + Ag * ks) if ds.Q_marge else lin
        WP = _matvec(W, Pth)
        if inv is not None:
            covdat, covth = _matvec(inv, P), _matvec(inv, WP)
            normV = _ssum(WP * covth)
            if not normV > 0:
                return LOGZERO
            chisq[iQ + NQ] = _ssum(P * covdat) - _ssum(WP * covdat) ** 2 / normV + np.log(normV)
        else:
            normV = _ssum(WP * WP * w)
            if not normV > 0:
                return LOGZERO
            tmp = _ssum(WP * P * w) / normV
            chisq[iQ + NQ] = _ssum(P * (P - WP * tmp) * w) + np.log(normV)
        if not do_marge:
            return _out(chisq[iQ + NQ] / T(2))
    cw = _calweights(T)
    mn = chisq.min()
    s = _ssum(np.exp(-(chisq - mn) / T(2)) * cw) / _ssum(cw)
    if not np.isfinite(float(s)):
        return LOGZERO
    return LOGZERO if s == 0 else _out(-np.log(s) + mn / T(2))


def wigglez_loglike_host(ds: WiggleZDataset, row, dtype=np.float64, normv_single=True, normv_running=True):
    """WiggleZ_LnLike (wigglez.f90:524-641) at one theory row, in the float type
    dtype; normV, Q and minchisq are rounded to single precision as the
    reference declares them, and normV runs on over the Q grid as it does there.
    normv_single = False keeps normV in dtype and normv_running = False restarts
    it at every grid point: what the reference would give had it declared normV
    real(mcp), or reset it -- for the tests that show the goldens pin both."""
    T = dtype
    r = _lin(ds, row, T)
    if r is None:
        return LOGZERO
    ks, lin = r
    f32 = np.float32
    Ag, Qmid, Qsig, dQ = T(ds.Ag), T(ds.Q_mid), T(ds.Q_sigma), T(DQ)
    inv = ds.invcov_as(T)
    Ws, Ps = ds.W.astype(T), ds.P.astype(T)
    if ds.Q_marge and ds.Q_flat:
        M11 = M22 = M12 = v1 = v2 = final = T(0)
        for g in range(ds.nr):
            Pth = lin / (T(1) + Ag * ks)
            k2 = Pth * (ks * ks)
            WP, WP2 = _matvec(Ws[g], Pth), _matvec(Ws[g], k2)
            covdat, covth, covth2 = _matvec(inv[g], Ps[g]), _matvec(inv[g], WP), _matvec(inv[g], WP2)
            M11, M22, M12 = M11 + _ssum(covth * WP), M22 + _ssum(covth2 * WP2), M12 + _ssum(covth * WP2)
            v1, v2 = v1 + _ssum(covdat * WP), v2 + _ssum(covdat * WP2)
            final = final + _ssum(Ps[g] * covdat)
        return _out(_flat_2x2(M11, M22, M12, v1, v2, final, T))
    do_marge = ds.Q_marge and ds.Q_sigma != 0
    chisq = np.zeros(2 * NQ + 1, dtype=T)
    normV = f32(0) if normv_single else T(0)
    for iQ in range(-NQ, NQ + 1):
        Q = T(f32(Qmid + T(iQ) * Qsig * dQ))
        Pth = lin * (T(1) + Q * (ks * ks)) / (T(1) + Ag * ks) if ds.Q_marge else lin
        WPl = np.concatenate([_matvec(Ws[g], Pth) for g in range(ds.nr)])
        WPg = WPl.reshape(ds.nr, ds.np)
        covdat = np.concatenate([_matvec(inv[g], Ps[g]) for g in range(ds.nr)])
        covth = np.concatenate([_matvec(inv[g], WPg[g]) for g in range(ds.nr)])
        Pl = Ps.reshape(-1)
        if not normv_running:
            normV = f32(0) if normv_single else T(0)
        normV = f32(T(normV) + _ssum(WPl * covth)) if normv_single else normV + _ssum(WPl * covth)
        if not normV > 0:
            return LOGZERO
        chisq[iQ + NQ] = _ssum(Pl * covdat) - _ssum(WPl * covdat) ** 2 / T(normV)
        if not do_marge:
            return _out(chisq[iQ + NQ] / T(2))
    cw = _calweights(T)
    mn32 = f32(chisq.min())
    if not np.isfinite(mn32):
        return LOGZERO
    mn = T(mn32)
    s = _ssum(np.exp(-(chisq - mn) / T(2)) * cw) / _ssum(cw)
    if not np.isfinite(float(s)):
        return LOGZERO
    return LOGZERO if s == 0 else _out(-np.log(s) + T(mn32 / f32(2)))


def mpk_theory_row(ds, H0, DV, pk, kh_min):
    """The theory row of one cosmology: ``pk(k) -> P`` is the provider's P(k, z)
    at the data set's redshift (nonlinear if ``ds.nonlinear``), ``kh_min`` the
    lower edge of its k grid, ``DV`` = BAO_D_v(z)."""
    a = ds.DV_fid / (H0 * DV) if ds.use_scaling else 1.0
    ak = a * ds.k
    ks = np.where(ak > kh_min, ak, kh_min)
    row = np.empty(2 + ds.nk)
    row[0], row[1] = a, kh_min
    row[2:] = pk(ks)
    return row


# ---------------------------------------------------------------- the library's likelihoods

class _NativePK(NativeCMBLikelihood):
    LikelihoodType = "MPK"
    _dataset_class = None

    def _init_info(self, dataset, overrides):
        self.dataset, self._overrides, self._ds = dataset, dict(overrides or {}), None
        self.n_theory = N.lib().cmbl_theory_len(self._h)
        dims = (C.c_int * 8)()
        N.check(N.lib().cmbl_mpk_info(self._h, dims), self._h)
        (self.n_points, self.n_kbands, self.n_regions, self.zbin, self.q_mode, self.has_cov, self.use_scaling,
         self.use_gigglez) = list(dims)
        self.tag = ""                       # GetTag falls back to the name: chi2_<name>

    def loader_arrays(self):
        """(k [nk], data [regions][np], inverse covariance [regions][np][np]) as the library's loader built
        them (cmbl_mpk_arrays); without a cov_file the inverse covariance is diag(1 / sdev^2)."""
        k, P = np.zeros(self.n_kbands), np.zeros((self.n_regions, self.n_points))
        inv = np.zeros((self.n_regions, self.n_points, self.n_points))
        dp = C.POINTER(C.c_double)
        N.check(N.lib().cmbl_mpk_arrays(self._h, k.ctypes.data_as(dp), P.ctypes.data_as(dp), inv.ctypes.data_as(dp)), self._h)
        return k, P, inv

    @property
    def ds(self):
        """The numpy loader's view of the same data set (k, DV_fid, use_scaling: what mpk_theory_row needs)."""
        if self._ds is None:
            self._ds = self._dataset_class(self.dataset, self._overrides)
        return self._ds

    def loglike_batch(self, dl, nuis=None, out=None, workspace=None):
        import torch
        if nuis is None:
            nuis = torch.empty((dl.shape[0], 0), dtype=torch.float64, device=dl.device)
        return super().loglike_batch(dl, nuis, out, workspace)

    def loglike_batch_sparse(self, dl, nuis, out, count, workspace=None):
        import torch
        if nuis is None:
            nuis = torch.empty((dl.shape[0], 0), dtype=torch.float64, device=dl.device)
        return super().loglike_batch_sparse(dl, nuis, out, count, workspace)

    def loglike_host(self, dl, nuis=None):
        dl = np.asarray(dl)
        return super().loglike_host(dl, np.empty((dl.shape[0], 0)) if nuis is None else nuis)


class MPKLikelihood(_NativePK):
    """An mpk.f90 data set in the HIP library (tag ``"MPK"``).  ``loglike_batch(dl)``
    takes ``dl`` as a cuda float64 tensor [W, 1, n_theory] of theory rows (or [W,
    nf, L >= n_theory]: field 0 is read); there are no nuisance parameters."""
    _dataset_class = MPKDataset

    def __init__(self, dataset: str, nonlinear: bool = False, overrides: dict | None = None):
        over = dict(overrides or {})
        over["mpk_dataset_nonlinear"] = "T" if nonlinear else "F"
        super().__init__("MPK", dataset, over)
        self.nonlinear = bool(nonlinear)
        self._init_info(dataset, over)


class WiggleZLikelihood(_NativePK):
    """One WiggleZ redshift bin in the HIP library (tag ``"WIGGLEZ"``): ``dataset``
    the bin's file, ``common`` the wigglez_common_dataset file whose keys are
    merged in.  ``gigglez_dir`` says where gigglezfiducialmodel_matterpower_{a..d}.dat
    are (default: the dataset's directory)."""
    _dataset_class = WiggleZDataset

    def __init__(self, dataset: str, common: str, use_gigglez: bool = False, nonlinear: bool = False,
                 gigglez_dir: str | None = None, overrides: dict | None = None):
        over = wigglez_overrides(common, use_gigglez, nonlinear, gigglez_dir)
        over.update(overrides or {})
        super().__init__("WIGGLEZ", dataset, over)
        self.nonlinear = bool(nonlinear)
        self._init_info(dataset, over)


def mpk_likelihood_add(like_list, ini: IniFile):
    """MPKLikelihood_Add (mpk.f90:90-115): ``use_mpk``, ``mpk_numdatasets``,
    ``mpk_dataset<i>`` and ``mpk_dataset_nonlinear<i>``.  Every likelihood is
    named by its data set's ``name`` key (the chain column chi2_<name>)."""
    if not ini.read_bool("use_mpk", False):
        return []
    out = []
    for i in range(1, ini.read_int("mpk_numdatasets", 0) + 1):
        like = MPKLikelihood(ini.relative_filename("mpk_dataset%d" % i), ini.read_bool("mpk_dataset_nonlinear%d" % i, False))
        like_list.add(like)
        out.append(like)
    return out


def wigglez_likelihood_add(like_list, ini: IniFile, gigglez_dir: str | None = None):
    """WiggleZLikelihood_Add (wigglez.f90:170-200): ``use_wigglez_mpk``,
    ``Use_gigglez``, ``nonlinear_wigglez``, ``wigglez_common_dataset``,
    ``mpk_wigglez_numdatasets`` and ``wigglez_dataset<i>``; the common file's keys
    are merged into every bin's.  The common file declares a conflict with the
    BAO likelihood named WiggleZ (type_conflict1, name_conflict1;
    likelihood.f90:54-60): a list that already holds it is refused."""
    if not ini.read_bool("use_wigglez_mpk", False):
        return []
    common = ini.relative_filename("wigglez_common_dataset")
    CI = IniFile(common)
    for i in range(1, CI.read_int("num_conflicts", 0) + 1):
        ctype, cname = CI.get("type_conflict%d" % i, ""), CI.get("name_conflict%d" % i, "")
        for other in like_list:
            # the BAO likelihoods are the derived ones (derivedlike.py), named by their dataset tag
            is_type = isinstance(other, _DerivedLike) if ctype == "BAO" else getattr(other, "LikelihoodType", "") == ctype
            if is_type and getattr(other, "name", "") == cname:
                raise ValueError("the %s likelihood %s conflicts with the WiggleZ power-spectrum likelihood %s: "
                                 "use one of them" % (ctype, cname, CI.get("name", "WiggleZ_MPK")))
    use_gigglez, nonlinear = ini.read_bool("Use_gigglez", False), ini.read_bool("nonlinear_wigglez", False)
    out = []
    for i in range(1, ini.read_int("mpk_wigglez_numdatasets", 0) + 1):
        like = WiggleZLikelihood(ini.relative_filename("wigglez_dataset%d" % i), common, use_gigglez, nonlinear,
                                 gigglez_dir or ini.get("gigglez_dir"))
        like_list.add(like)
        out.append(like)
    return out


def datasets_from_ini(ini: IniFile, gigglez_dir: str | None = None):
    """The numpy loaders' data sets of a run ini, in the order the two *_likelihood_add add them."""
    out = []
    if ini.read_bool("use_mpk", False):
        for i in range(1, ini.read_int("mpk_numdatasets", 0) + 1):
            nl = "T" if ini.read_bool("mpk_dataset_nonlinear%d" % i, False) else "F"
            out.append(MPKDataset(ini.relative_filename("mpk_dataset%d" % i), {"mpk_dataset_nonlinear": nl}))
    if ini.read_bool("use_wigglez_mpk", False):
        over = wigglez_overrides(ini.relative_filename("wigglez_common_dataset"), ini.read_bool("Use_gigglez", False),
                                 ini.read_bool("nonlinear_wigglez", False), gigglez_dir or ini.get("gigglez_dir"))
        for i in range(1, ini.read_int("mpk_wigglez_numdatasets", 0) + 1):
            out.append(WiggleZDataset(ini.relative_filename("wigglez_dataset%d" % i), over))
    return out
