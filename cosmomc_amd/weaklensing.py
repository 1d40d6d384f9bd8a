"""DES Y1 weak-lensing and galaxy-clustering likelihood (reference source/wl.f90).

``WLLikelihood`` is the dataset opened in the HIP library (``cmbl_open`` tag
``"WL"``).  Its nuisance parameters are those of the dataset's
``nuisance_params`` file in ``DataParams`` order (b, m, A, alpha, z0, DzL,
DzS), and its theory is one row per walker instead of C_l::

    [h, omm, chis[nz], Hs[nz], D_growth[nz], P[nl][nz]]

``nz = num_z_p`` (n(z) file rows + 2), ``nl = len(ls_cl)``; ``P[l][j]`` is the
power the reference's ``calc_theory`` holds in ``powers`` for
``kh = (ls_cl[l] + 1/2) / (chis[j] h)`` at ``z_p[j]``, 0 where it writes 0.
``wl_theory_row`` builds that row from a P(k, z) callable; which spectrum
(linear or not, Weyl or not) fills it is the provider's business.

``WLDataset`` is ``WL_ReadIni`` (:104-299) and ``init_bessel_integration``
(:320-369) on the host, ``wl_loglike_host`` a literal numpy restatement of
``calc_theory`` / ``cl2corr`` / ``WL_LnLike`` (:301-653) in the reference's
summation order; with ``dtype=np.longdouble`` it is the tests' high-precision
reference.  ``wl_likelihood_add`` mirrors ``WLLikelihood_Add`` (:72-102).
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import _native as N
from .ini import IniFile
from .likelihood import NativeCMBLikelihood, read_paramnames

LOGZERO = N.CMBL_LOGZERO
TYPES = ("xip", "xim", "gammat", "wtheta")
XIP, XIM, GAMMAT, WTHETA = range(4)
CONST_C = 2.99792458e8
IA_NORM = float(np.float32(0.0134))          # a single-precision literal (:488)
# the keys WL_ReadIni and ReadDatasetFile read; any other key of a dataset is refused
SERVED_KEYS = {"name", "measurements_format", "nz_wl", "max_z", "num_z_bins", "num_gal_bins", "acc", "lmax", "nz_file",
               "nz_gal_file", "theta_bins_file", "num_theta_bins", "kmax", "ah_factor", "cov_file",
               "intrinsic_alignment_model", "data_types", "used_data_types", "nuisance_params", "data_selection",
               "wl_use_weyl"} | {"measurements[%s]" % t for t in TYPES}


def spline_d2(x, y):
    """Second derivatives of the natural ("dangle") cubic spline (Interpolation.f90:693-734), in y's dtype."""
    n = len(x)
    T = y.dtype.type
    d2, u = np.zeros(n, dtype=y.dtype), np.zeros(n, dtype=y.dtype)
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
    return d2


def spline_eval(x, y, d2, lo, xv):
    """TSpline1D_Value's formula (:283, :334) on the intervals lo (0-based) for the points xv."""
    T = y.dtype.type
    ho = x[lo + 1] - x[lo]
    a0 = (x[lo + 1] - xv) / ho
    b0 = T(1) - a0
    return b0 * y[lo + 1] + a0 * (y[lo] - b0 * ((a0 + T(1)) * d2[lo] + (T(2) - a0) * d2[lo + 1]) * ho ** 2 / T(6))


def make_ls_cl(acc: float, lmax: int) -> np.ndarray:
    """The l of the Limber C_l: linear then log (:284-297).  0.1266 * i is a single-precision product."""
    ls = list(range(2, 100 - int(4 / acc) + 1, max(1, int(4 / acc))))
    i = 0
    while ls[-1] < lmax:
        ls.append(int(np.rint(100 * np.exp(float(np.float32(0.1266) * np.float32(i)) / acc))))
        i += 1
    return np.array(ls, dtype=np.int64)


def make_bessel_bins(acc: float, lmax: int):
    """(ls_bessel, first l, last l) of the roughly log-spaced l bins (:326-348); dlog is a single-precision quotient."""
    n = int(500 * acc)
    dlog = float(np.log(np.float32(lmax)) / np.float32(n))
    lo, hi, ls = [], [], []
    ell, last = 2, 1
    for i in range(1, n + 1):
        e = int(np.exp(i * dlog))
        if e != last:
            d = e - last
            last = e
            ls.append((2 * ell + d - 1.0) / 2)
            lo.append(ell)
            hi.append(ell + d - 1)
            ell += d
    return np.array(ls), np.array(lo), np.array(hi)


def _load_txt(path):
    rows = [[float(x) for x in l.replace(",", " ").split()] for l in open(path)
            if l.strip() and not l.strip().startswith("#")]
    return np.array(rows, dtype=np.float64)


class WLDataset:
    """WL_ReadIni (:104-299) and init_bessel_integration (:320-369) on the host."""

    def __init__(self, dataset: str, overrides: dict | None = None, use_weyl: bool | None = None):
        ini = IniFile(text="".join(f"{k} = {v}\n" for k, v in (overrides or {}).items()))
        ini._open(dataset, 0)          # first definition wins: the overrides
        self.filename = dataset
        for k in ini.keys():
            if k not in SERVED_KEYS:
                raise NotImplementedError(f"WL: key {k} is not supported")
        self.name = ini.get("name") or os.path.splitext(os.path.basename(dataset))[0]
        if ini.get("measurements_format") != "DES":
            raise NotImplementedError("WL: measurements_format = %s is not supported (only DES)"
                                      % ini.get("measurements_format"))
        self.use_weyl = ini.read_bool("wl_use_weyl", False) if use_weyl is None else bool(use_weyl)
        self.nzb = int(ini["num_z_bins"])
        self.ngal = ini.read_int("num_gal_bins", 0)
        maxbin = max(self.nzb, self.ngal)
        self.acc = ini.read_float("acc", 1.0)
        self.lmax = ini.read_int("lmax", 50000)
        self.ah_factor = ini.read_float("ah_factor", 1.0)      # read and, as in the reference, not applied

        def rel(key):
            return ini.resolve(ini[key], dataset)
        nzs = _load_txt(rel("nz_file"))
        zm = nzs[:, 1]
        self.nz = len(zm) + 2
        self.z_p = np.concatenate([zm, [2 * zm[-1] - zm[-2], 3 * zm[-1] - 2 * zm[-2]]])
        self.p_src = np.zeros((self.nzb, self.nz))
        self.p_src[:, :-2] = nzs[:, 3:3 + self.nzb].T
        self.p_gal = np.zeros((self.ngal, self.nz))
        if self.ngal > 0:
            nzg = _load_txt(rel("nz_gal_file"))
            if len(nzg) != self.nz - 2 or np.any(nzg[:, 1] != zm):
                raise ValueError("wl assumes windows used same bins")
            self.p_gal[:, :-2] = nzg[:, 3:3 + self.ngal].T
        self.theta_bins = _load_txt(rel("theta_bins_file")).ravel()
        self.ntheta = ini.read_int("num_theta_bins", len(self.theta_bins))
        if self.ntheta != len(self.theta_bins):
            raise ValueError("size mismatch in theta_bins_file")
        self.theta_rad = self.theta_bins / 60 * np.pi / 180
        cov = _load_txt(rel("cov_file"))
        ia = ini.get("intrinsic_alignment_model", "DES1YR")
        if ia not in ("none", "DES1YR"):
            raise NotImplementedError(f"WL: intrinsic_alignment_model = {ia} is not supported")
        self.ia_des1yr = ia == "DES1YR"
        self.data_types = [TYPES.index(t) for t in ini["data_types"].split()]
        used = [TYPES.index(t) for t in ini.get("used_data_types", ini["data_types"]).split()]
        self.want = [t in used for t in range(4)]
        if self.use_weyl and (self.want[GAMMAT] or self.want[WTHETA]):
            raise NotImplementedError("WL: wl_use_weyl can only be used with weak lensing data (xip, xim)")
        self.param_names = read_paramnames(rel("nuisance_params"))
        if len(self.param_names) != 2 * (self.ngal + self.nzb) + 3:
            raise ValueError("nuisance_params: %d names, %d expected" % (len(self.param_names),
                                                                         2 * (self.ngal + self.nzb) + 3))
        # data_selection is a single-precision array (:37)
        sel = np.full((4, maxbin + 1, maxbin + 1, 2), -1.0)
        for line in open(rel("data_selection")):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            tp, b1, b2 = TYPES.index(t[0]), int(t[1]), int(t[2])
            if not (1 <= b1 <= maxbin and 1 <= b2 <= maxbin):
                raise ValueError("data_selection: invalid bin")
            if self.want[tp]:
                sel[tp, b1, b2] = [float(np.float32(float(t[3]))), float(np.float32(float(t[4])))]
        self.pairs = []                 # per data type: the (bin1, bin2) of its measurement file, in file order
        self.used_items, self.used_indices, data = [], [], []
        self.first_theta_bin_used = self.ntheta
        cov_ix = 0
        for ti, tp in enumerate(self.data_types):
            pr, last = [], (0, 0)
            for line in open(rel("measurements[%s]" % TYPES[tp])):
                t = line.split()
                if not t or t[0].startswith("#"):
                    continue
                b1, b2, tb, dat = int(t[0]), int(t[1]), int(t[2]), float(t[3])
                if not 1 <= tb <= self.ntheta:
                    raise ValueError("WL: invalid theta bin: " + line)
                cov_ix += 1
                if (b1, b2) != last:
                    pr.append((b1, b2))
                    last = (b1, b2)
                if self.want[tp]:
                    lo, hi = sel[tp, b1, b2]
                    if lo <= self.theta_bins[tb - 1] <= hi:
                        self.used_items.append((ti + 1, b1, b2, tb))
                        self.used_indices.append(cov_ix)
                        data.append(dat)
                        self.first_theta_bin_used = min(self.first_theta_bin_used, tb)
            self.pairs.append(pr)
        if cov.shape != (cov_ix, cov_ix):
            raise ValueError("WL: cov size does not match data size")
        self.n_used = len(data)
        self.data_vector = np.array(data)
        ix = np.array(self.used_indices, dtype=int) - 1
        self.invcov = np.linalg.inv(cov[np.ix_(ix, ix)]) if self.n_used else np.zeros((0, 0))
        self.ls_cl = make_ls_cl(self.acc, self.lmax)
        self.nl = len(self.ls_cl)
        self.ls_bessel, self._ell_lo, self._ell_hi = make_bessel_bins(self.acc, self.lmax)
        self._bessel = None
        # the Limber columns: every pair of the wanted types but xim, which is read off xip's C_l
        self.columns = []               # (type, bin1, bin2)
        for ti, tp in enumerate(self.data_types):
            if tp != XIM and self.want[tp]:
                self.columns += [(tp, b1, b2) for b1, b2 in self.pairs[ti]]
        self.xim_index = self.data_types.index(XIM) + 1 if XIM in self.data_types else 0
        self._d2 = {}

    @property
    def n_theory(self) -> int:
        return 2 + 3 * self.nz + self.nl * self.nz

    @property
    def bessel(self):
        """Bin-summed l J_n(l theta) / (2 pi) over the used theta bins (:354-369):
        [order 0, 2, 4][l bin][theta bin - first], each bin summed in l order.
        Built on first use, with scipy.special.jv: only wl_loglike_host needs it
        (and so scipy); theory rows need z_p and ls_cl alone."""
        if self._bessel is None:
            from scipy.special import jv
            th = self.theta_rad[self.first_theta_bin_used - 1:]
            self._bessel = np.zeros((3, len(self.ls_bessel), len(th)))
            for i, (lo, hi) in enumerate(zip(self._ell_lo, self._ell_hi)):
                ell = np.arange(lo, hi + 1, dtype=np.float64)[:, None]
                for o, order in enumerate((0, 2, 4)):
                    self._bessel[o, i] = _seqsum(ell * jv(order, ell * th[None, :]), 0) / (2 * np.pi)
        return self._bessel

    def d2(self, dtype):
        """(source, lens) second derivatives of the n(z) splines in dtype."""
        if dtype not in self._d2:
            z = self.z_p.astype(dtype)
            self._d2[dtype] = tuple([spline_d2(z, p.astype(dtype)) for p in P] for P in (self.p_src, self.p_gal))
        return self._d2[dtype]


def wl_theory_row(ds: WLDataset, h, omm, chis, Hs, D_growth, pk, kh_min, kh_max):
    """One walker's theory row.  ``pk(kh, z)`` returns P at arrays of kh and z;
    it is asked only for kh in [kh_min, kh_max], the other entries are 0 (:549-569)."""
    chis = np.asarray(chis, dtype=np.float64)
    kh = (ds.ls_cl[:, None] + 0.5) / chis[None, :] / h
    z = np.broadcast_to(ds.z_p[None, :], kh.shape)
    ok = (kh >= kh_min) & (kh <= kh_max)
    P = np.zeros(kh.shape)
    P[ok] = pk(kh[ok], z[ok])
    return np.concatenate([[h, omm], chis, np.asarray(Hs, dtype=np.float64), np.asarray(D_growth, dtype=np.float64),
                           P.ravel()])


def _seqsum(a, axis=-1):
    """Sum along an axis in index order from 0 (numpy's own sum is pairwise)."""
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def _shifted(z, y, d2, shift, T):
    """Spline value at z_p - shift, 0 where that leaves [z_p(1), z_p(n)] (:499-512); knot by FindValue's bisection."""
    zs = z - T(shift)
    inside = ~((zs < z[0]) | (zs > z[-1]))
    lo = np.clip(np.searchsorted(z, zs, side="right") - 1, 0, len(z) - 2)
    return np.where(inside, spline_eval(z, y, d2, lo, zs), T(0))


def wl_theory_vector(ds: WLDataset, row, nuis, dtype=np.float64):
    """make_vector(corr_theory) of WL_LnLike: the theory at the used items, in dtype."""
    T = np.dtype(dtype).type
    row = np.asarray(row, dtype=np.float64).astype(dtype)
    nuis = np.asarray(nuis, dtype=np.float64).astype(dtype)
    nz, nl, ngal, nzb = ds.nz, ds.nl, ds.ngal, ds.nzb
    if row.shape != (ds.n_theory,) or nuis.shape != (len(ds.param_names),):
        raise ValueError("theory row or nuisance vector of the wrong length")
    h, omm = row[0], row[1]
    chis, Hs, Dg = row[2:2 + nz], row[2 + nz:2 + 2 * nz], row[2 + 2 * nz:2 + 3 * nz]
    P = row[2 + 3 * nz:].reshape(nl, nz)
    bias, m = nuis[:ngal], nuis[ngal:ngal + nzb]
    A, alpha, z0 = nuis[ngal + nzb:ngal + nzb + 3]
    dzl, dzs = nuis[ngal + nzb + 3:2 * ngal + nzb + 3], nuis[2 * ngal + nzb + 3:]
    z = ds.z_p.astype(dtype)
    dchis = np.empty(nz, dtype=dtype)
    dchis[0] = (chis[1] + chis[0]) / T(2)
    dchis[-1] = chis[-1] - chis[-2]
    dchis[1:-1] = (chis[2:] - chis[:-2]) / T(2)
    align = A * ((T(1) + z) / (T(1) + z0)) ** alpha * T(IA_NORM) / Dg
    d2s, d2g = ds.d2(np.dtype(dtype))
    n_chi = [Hs * _shifted(z, ds.p_src[b].astype(dtype), d2s[b], dzs[b], T) for b in range(nzb)]
    qgal = [Hs * _shifted(z, ds.p_gal[b].astype(dtype), d2g[b], dzl[b], T) * bias[b] for b in range(ngal)]
    c5 = T(1e5) / T(CONST_C)
    upper = np.triu(np.ones((nz, nz), dtype=bool))
    qs = []
    for b in range(nzb):
        fac = dchis * n_chi[b]
        terms = np.where(upper, fac[None, :] * (T(1) - chis[:, None] / chis[None, :]), T(0))
        q = _seqsum(terms, 1)
        if ds.ia_des1yr:
            q = q - align * n_chi[b] / (chis * (T(1) + z) * T(3) * h ** 2 * c5 ** 2 / T(2))
        if ds.use_weyl:
            q = q * chis
        else:
            q = q * (T(3) / T(2) * omm * h ** 2 * c5 ** 2) * chis * (T(1) + z)
        qs.append(q)
    fac = dchis / chis ** 2
    if not ds.use_weyl:
        fac = fac / h ** 3
    tmp = fac[None, :] * P
    cl = {}
    for tp, f1, f2 in ds.columns:
        if tp == XIP:
            cl[tp, f1, f2] = _seqsum(tmp * qs[f1 - 1][None, :] * qs[f2 - 1][None, :])
        elif tp == WTHETA:
            cl[tp, f1, f2] = _seqsum(tmp * (qgal[f1 - 1] * qgal[f2 - 1])[None, :])
        else:
            cl[tp, f1, f2] = _seqsum(tmp * (qgal[f1 - 1] * qs[f2 - 1])[None, :])
    # cl2corr: natural spline in l at ls_bessel (ArrayValue's forward search), times the Bessel tables
    lsc, lsb = ds.ls_cl.astype(dtype), ds.ls_bessel.astype(dtype)
    lo = np.clip(np.searchsorted(ds.ls_cl, ds.ls_bessel, side="left") - 1, 0, nl - 2)
    bes = ds.bessel.astype(dtype)
    corr = {}
    for (tp, f1, f2), c in cl.items():
        clb = spline_eval(lsc, c, spline_d2(lsc, c), lo, lsb)
        if tp == XIP:
            fac2 = (T(1) + m[f1 - 1]) * (T(1) + m[f2 - 1])
            corr[XIP, f1, f2] = _seqsum(clb[:, None] * bes[0], 0) * fac2
            if ds.xim_index:
                corr[XIM, f1, f2] = _seqsum(clb[:, None] * bes[2], 0) * fac2
        elif tp == GAMMAT:
            corr[tp, f1, f2] = _seqsum(clb[:, None] * bes[1], 0) * (T(1) + m[f2 - 1])
        else:
            corr[tp, f1, f2] = _seqsum(clb[:, None] * bes[0], 0)
    vec = np.zeros(ds.n_used, dtype=dtype)
    for i, (ti, f1, f2, tb) in enumerate(ds.used_items):
        c = corr.get((ds.data_types[ti - 1], f1, f2))
        if c is not None:
            vec[i] = c[tb - ds.first_theta_bin_used]
    return vec


def wl_loglike_host(ds, row, nuis, dtype=np.float64):
    """-lnL of WL_LnLike (:301-318) for one theory row and one nuisance vector;
    ``ds`` a WLDataset or a dataset path.  LOGZERO where the result is not finite."""
    D = ds if isinstance(ds, WLDataset) else WLDataset(ds)
    with np.errstate(all="ignore"):
        v = wl_theory_vector(D, row, nuis, dtype) - D.data_vector.astype(dtype)
        r = v @ (D.invcov.astype(dtype) @ v) / np.dtype(dtype).type(2)
    return r if np.isfinite(r) else np.dtype(dtype).type(LOGZERO)


class WLLikelihood(NativeCMBLikelihood):
    """A DES-format weak-lensing dataset in the HIP library.  ``loglike_batch(dl,
    nuis)`` takes ``dl`` as a cuda float64 tensor [W, 1, n_theory] of theory rows
    (or [W, nf, L >= n_theory]: field 0 is read) and ``nuis`` [W, n_nuis]."""
    LikelihoodType = "WL"

    def __init__(self, dataset: str, overrides: dict | None = None, use_weyl: bool = False,
                 use_non_linear: bool = True, tag: str = "WL"):
        over = dict(overrides or {})
        if use_weyl:
            over["wl_use_weyl"] = "T"
        super().__init__("WL", dataset, over)
        self.tag = tag
        self.use_weyl, self.use_non_linear = bool(use_weyl), bool(use_non_linear)
        self.n_theory = N.lib().cmbl_theory_len(self._h)
        self.dataset = dataset
        self._overrides = over
        self._ds = None
        dims = (C.c_int * 8)()
        N.check(N.lib().cmbl_wl_info(self._h, dims), self._h)
        (self.nz, self.nl, self.n_bessel, self.n_columns, self.n_used, self.first_theta_bin_used, self.num_z_bins,
         self.num_gal_bins) = list(dims)

    def loader_arrays(self):
        """(ls_cl, ls_bessel, used_items [n_used][4]) as the library's loader built them (cmbl_wl_arrays)."""
        ls_cl, ls_b = np.zeros(self.nl, dtype=np.int32), np.zeros(self.n_bessel)
        items = np.zeros((self.n_used, 4), dtype=np.int32)
        N.check(N.lib().cmbl_wl_arrays(self._h, ls_cl.ctypes.data_as(C.POINTER(C.c_int)),
                                       ls_b.ctypes.data_as(C.POINTER(C.c_double)),
                                       items.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        return ls_cl, ls_b, items

    @property
    def ds(self) -> WLDataset:
        """The loader's view on the host (z_p, ls_cl, pairs), to build theory rows."""
        if self._ds is None:
            self._ds = WLDataset(self.dataset, self._overrides)
        return self._ds


def wl_likelihood_add(like_list, ini: IniFile):
    """WLLikelihood_Add (:72-102): use_WL, wl_dataset[TAG], wl_dataset[TAG,key],
    wl_use_non_linear, wl_use_weyl, wl_dataset_speed[TAG]."""
    added = []
    if not ini.read_bool("use_WL", False):
        return added
    nonlinear = ini.read_bool("wl_use_non_linear", True)
    weyl = ini.read_bool("wl_use_weyl", False)
    pat = re.compile(r"^wl_dataset\[([^,\]]+)\]$")
    for key in ini.keys():
        mt = pat.match(key)
        if not mt:
            continue
        tag = mt.group(1)
        opat = re.compile(r"^wl_dataset\[" + re.escape(tag) + r",(.+)\]$")
        over = {mo.group(1): ini[k] for k in ini.keys() for mo in [opat.match(k)] if mo}
        like = WLLikelihood(ini.relative_filename(key), over, use_weyl=weyl, use_non_linear=nonlinear, tag=tag)
        spd = ini.get(f"wl_dataset_speed[{tag}]")
        if spd is not None:
            like.speed = int(spd)
        like_list.add(like)
        added.append(like)
    return added
