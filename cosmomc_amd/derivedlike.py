"""Gaussian likelihoods on calculator-derived quantities (host wrapper of
``cmbg_*``), and the reference's Gaussian BAO datasets.

The reference adds Gaussian priors on derived parameters (``H0_prior``,
``zre_prior``, source/CosmologyParameterizations.f90:105-110) and Gaussian
background likelihoods (``TBAOLikelihood``, source/bao.f90:265-308) whose theory
vector ``t`` is a handful of numbers per slow point: D_V/r_s, D_M/r_s, H r_s,
A(z), f sigma8 at the dataset's redshifts.  Here ``t`` comes from scalar
response surfaces over a ``PolynomialTheory``'s monomials, fitted offline
(``bao_theory`` at a design of points, then ``theory.fit_derived``), and

    -lnL = (t - obs)^T invcov (t - obs) / 2

is evaluated on the GPU (``DerivedGaussian``).  ``BatchedMCMC.
add_derived_likelihood`` gives it a term row of its own in the sampler.
``read_bao_dataset`` reads the reference's ``.dataset`` files of this form;
``bao_theory`` is pure numpy.

The BAO likelihoods that are no Gaussians (``MGSLikelihood``, a chi^2 table in
alpha, and ``DR1xLikelihood``, a probability grid in alpha_perp x alpha_plel,
bao.f90:311-410) are ``DerivedTable`` on one or two such surfaces
(``read_bao_likelihood``, ``bao_alpha_theory``).  The H0 measurement (HST.f90)
and the element abundances (ElementAbundances.f90) are Gaussians on one
surface (``read_hst``, ``hst_theory``, ``read_abundance_dataset``).
``derived_likelihoods_from_ini`` makes the objects an ini switches on.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import _native as N
from .ini import IniFile

MAXN = 32                                            # CMBG_MAXN
C_KM_S = 299792.458                                  # const_c / 1e3 (source/constants.f90)

# measurement_types of bao.f90:29-31
BAO_TYPES = ("Az", "DV_over_rs", "rs_over_DV", "DA_over_rs", "F_AP", "f_sigma8", "bao_Hz_rs", "bao_Hz_rs_103",
             "dilation", "DM_over_rs")
# the dataset tags BAOLikelihood_Add gives a probability-grid class (bao.f90:91-98)
GRID_SETS = ("MGS", "DR11CMASS", "DR12CMASS", "DR12LOWZ")


class _DerivedLike:
    """What every ``cmbg_t`` wrapper shares: ``handle``, ``calc``, eval and
    close."""

    def eval(self, P_rows, out=None, fail=None, stream=None):
        """-lnL at P_rows (the forms PolynomialTheory.derived accepts): a cuda
        float64 tensor [M] (``out``, stride 1, when given); a point outside the
        calculator's box gets logZero (1e30).  fail: a cuda int32 tensor [M]
        that receives 1 for those points, else 0."""
        import torch
        P_rows, ld = self.calc._rows(P_rows)
        num_params, M = P_rows.shape
        if out is None:
            out = torch.empty((M,), dtype=torch.float64, device="cuda")
        if out.dim() != 1 or out.dtype != torch.float64 or out.shape[0] != M or (M > 1 and out.stride(0) != 1):
            raise ValueError(f"out must be float64 [{M}] with stride 1")
        if fail is not None and (fail.dtype != torch.int32 or fail.numel() < M or not fail.is_contiguous()):
            raise ValueError("fail must be a contiguous int32 tensor [M]")
        if stream is None:
            stream = N.current_stream_ptr()
        N.check(N.lib().cmbg_eval(self.handle, M, P_rows.data_ptr(), ld, num_params, out.data_ptr(),
                                  None if fail is None else fail.data_ptr(), stream), self.handle, "cmbg")
        return out

    def close(self):
        if getattr(self, "handle", None):
            N.lib().cmbg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DerivedGaussian(_DerivedLike):
    """A ``cmbg_t``: n <= 32 scalar surfaces coef [n_terms, n] over the
    monomials of ``calc`` (theory.fit_derived, theory.dl_columns), the
    measurement ``obs`` [n] and its inverse covariance ``invcov`` [n, n]
    (symmetric bit for bit), or ``cov``, which is inverted with numpy and
    symmetrised as (A + A^T) / 2.  The object copies its tables; ``calc`` must
    outlive it.  name: the tag of its ``chi2_<name>`` chain column."""

    def __init__(self, calc, coef, obs, invcov=None, cov=None, name="derived"):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1)
        n = obs.size
        if coef.ndim != 2 or coef.shape != (calc.n_terms, n):
            raise ValueError(f"coef must be [n_terms = {calc.n_terms}, n = {n}]")
        if (invcov is None) == (cov is None):
            raise ValueError("give one of invcov and cov")
        if invcov is None:
            a = np.linalg.inv(np.asarray(cov, dtype=np.float64).reshape(n, n))
            invcov = (a + a.T) / 2
        invcov = np.ascontiguousarray(invcov, dtype=np.float64).reshape(n, n)
        dp = C.POINTER(C.c_double)
        cfg = N.CmbgConfig()
        cfg.n, cfg.coef = n, coef.ctypes.data_as(dp)
        cfg.obs, cfg.invcov = obs.ctypes.data_as(dp), invcov.ctypes.data_as(dp)
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = N.lib().cmbg_create(calc.handle, C.byref(cfg), C.byref(h), err, 1024)
        if rc:
            raise N.NativeError(rc, err.value.decode())
        self.handle = h
        self.calc, self.n, self.name = calc, n, str(name)
        self.obs, self.invcov = obs, invcov

    @classmethod
    def prior(cls, calc, coef_column, mean, std, name="prior"):
        """A Gaussian prior on one derived quantity (H0_prior, zre_prior):
        n = 1 with invcov = 1 / std^2."""
        col = np.asarray(coef_column, dtype=np.float64).reshape(-1, 1)
        return cls(calc, col, [mean], invcov=[[1.0 / (float(std) * float(std))]], name=name)


# BAO_MGS_loglike's constants (bao.f90:397-405).  The cell width is the
# reference's default-real literal 0.001 widened to double: the cell index
# depends on it, so it must not be the double 0.001.
MGS_RSFID, MGS_DVFID = 148.69, 638.9518
MGS_ALPHA_MIN, MGS_ALPHA_MAX = 0.8005, 1.1985
MGS_STEP = float(np.float32(0.001))


class DerivedTable(_DerivedLike):
    """A ``cmbg_t`` of a tabulated form (``cmbg_create_table``): the BAO
    likelihoods that are no Gaussians.  Use ``mgs`` or ``grid``.  The object
    copies its tables; ``calc`` must outlive it.  name: the tag of its
    ``chi2_<name>`` chain column."""

    def __init__(self, calc, cfg, n, name):
        """cfg: a CmbgTableConfig whose arrays the caller keeps alive over the call"""
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = N.lib().cmbg_create_table(calc.handle, C.byref(cfg), C.byref(h), err, 1024)
        if rc:
            raise N.NativeError(rc, err.value.decode())
        self.handle = h
        self.calc, self.n, self.name = calc, n, str(name)

    @staticmethod
    def _coef(calc, coef, ns):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim == 1 and ns == 1:
            coef = coef.reshape(-1, 1)
        if coef.shape != (calc.n_terms, ns):
            raise ValueError(f"coef must be [n_terms = {calc.n_terms}, {ns}]")
        return coef

    @classmethod
    def table1d(cls, calc, coef_column, table, scale, x_min, x_max, step, name="table"):
        """The 1-D form with parameters of one's own (``mgs`` gives the
        reference's): -lnL = (table[ii] + table[ii + 1]) / 4 with ii =
        floor((v / scale - x_min) / step), logZero outside [x_min, x_max]."""
        coef = cls._coef(calc, coef_column, 1)
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        dp = C.POINTER(C.c_double)
        cfg = N.CmbgTableConfig()
        cfg.form, cfg.coef = 1, coef.ctypes.data_as(dp)
        cfg.n, cfg.table = table.size, table.ctypes.data_as(dp)
        cfg.scale, cfg.x_min, cfg.x_max, cfg.step = float(scale), float(x_min), float(x_max), float(step)
        self = cls(calc, cfg, 1, name)
        self.kind, self.table = "mgs", table
        self.scale, self.x_min, self.x_max, self.step = cfg.scale, cfg.x_min, cfg.x_max, cfg.step
        return self

    @classmethod
    def mgs(cls, calc, coef_column, table, name="MGS"):
        """BAO_MGS_loglike (bao.f90:390-410) on the surface D_V / r_drag
        (coef_column [n_terms]): table is the dataset's ``prob_dist`` column,
        a chi^2 in steps of 0.001 from alpha = 0.8005."""
        return cls.table1d(calc, coef_column, table, MGS_DVFID / MGS_RSFID, MGS_ALPHA_MIN, MGS_ALPHA_MAX, MGS_STEP,
                           name=name)

    @classmethod
    def grid(cls, calc, coef, perp, plel, prob, DA_rd_fid, Hrd_fid, name="grid"):
        """BAO_DR1x_loglike (bao.f90:346-376) on the surfaces coef [n_terms, 2]
        = D_A / r_drag and Hofz_Hunit r_drag: knots perp [np] and plel [np],
        prob [np, np] (perp the outer index) already divided by its maximum,
        and the fiducial D_A / r_d and H r_d."""
        coef = cls._coef(calc, coef, 2)
        perp = np.ascontiguousarray(perp, dtype=np.float64).reshape(-1)
        plel = np.ascontiguousarray(plel, dtype=np.float64).reshape(-1)
        prob = np.ascontiguousarray(prob, dtype=np.float64)
        npts = perp.size
        if plel.size != npts or prob.shape != (npts, npts):
            raise ValueError(f"plel must be [{npts}] and prob [{npts}, {npts}]")
        dp = C.POINTER(C.c_double)
        cfg = N.CmbgTableConfig()
        cfg.form, cfg.coef = 2, coef.ctypes.data_as(dp)
        cfg.np, cfg.perp, cfg.plel, cfg.prob = npts, perp.ctypes.data_as(dp), plel.ctypes.data_as(dp), prob.ctypes.data_as(dp)
        cfg.DA_rd_fid, cfg.Hrd_fid = float(DA_rd_fid), float(Hrd_fid)
        self = cls(calc, cfg, 2, name)
        self.kind, self.perp, self.plel, self.prob = "grid", perp, plel, prob
        self.DA_rd_fid, self.Hrd_fid = cfg.DA_rd_fid, cfg.Hrd_fid
        return self


def _data_lines(path):
    """ReadLineSkipEmptyAndComments"""
    with open(path) as f:
        return [t for t in (line.strip() for line in f) if t and not t.startswith("#")]


def read_bao_dataset(path, overrides=None):
    """A Gaussian BAO ``.dataset`` file (BAO_ReadIni / BAO_InitProbDist,
    bao.f90:113-234) as a dict: name, types [n] (names of BAO_TYPES), z [n],
    obs [n], invcov [n, n] and rs_rescale.  overrides: key -> value, which win
    over the file's (the reference's ``bao_dataset[TAG]`` settings).  Refuses
    what is not a plain Gaussian: a ``prob_dist`` table (MGS), the ``dilation``
    type and the DR11CMASS / DR12CMASS / DR12LOWZ probability grids
    (bao.f90:91-98)."""
    ini = IniFile(path)
    for k, v in (overrides or {}).items():
        ini.set(k, v)
    name = ini.get("name", os.path.splitext(os.path.basename(path))[0])
    if "prob_dist" in ini:
        raise ValueError(f"BAO dataset {name}: prob_dist (a tabulated probability, not a Gaussian) is not supported")
    if name in GRID_SETS:
        raise ValueError(f"BAO dataset {name}: a probability-grid likelihood, not a Gaussian, is not supported")
    n = ini.read_int("num_bao", 1)
    rs_rescale = ini.read_float("rs_rescale", 1.0)
    has_type = "measurement_type" in ini
    types = []
    if has_type:
        types = ini["measurement_type"].split()
        if len(types) == 1:
            types = types * n
        if len(types) != n:
            raise ValueError(f"BAO dataset {name}: measurement_type needs 1 or num_bao = {n} entries")
    err = None
    if "zeff" in ini:
        z = [float(v) for v in ini["zeff"].split()]
        if len(z) == 1:
            z = z * n
        vals = [float(v) for v in ini["bao_measurement"].split()]
        if n > 1:
            obs = vals[:n]
        else:
            obs, err = vals[:1], vals[1:2]
    else:
        has_err = ini.read_bool("bao_measurements_file_has_error", True)
        lines = _data_lines(ini.relative_filename("bao_measurements_file"))
        if len(lines) < n:
            raise ValueError(f"BAO dataset {name}: missing line in bao_measurements_file")
        z, obs, err = [], [], []
        for line in lines[:n]:
            f = line.split()
            z.append(float(f[0]))
            obs.append(float(f[1]))
            if has_err:
                err.append(float(f[2]))
            if not has_type:
                types.append(f[3 if has_err else 2])
        if not has_err:
            err = None
    for t in types:
        if t not in BAO_TYPES:
            raise ValueError(f"BAO dataset {name}: unknown measurement_type {t}")
        if t == "dilation":
            raise ValueError(f"BAO dataset {name}: measurement_type dilation (a probability grid) is not supported")
    if len(z) != n or len(obs) != n or any(v < 0.0001 for v in z):
        raise ValueError(f"BAO dataset {name}: error reading BAO measurements")
    if "bao_invcov_file" in ini:
        invcov = np.loadtxt(ini.relative_filename("bao_invcov_file"), dtype=np.float64).reshape(n, n)
    elif "bao_cov_file" in ini:
        a = np.linalg.inv(np.loadtxt(ini.relative_filename("bao_cov_file"), dtype=np.float64).reshape(n, n))
        invcov = (a + a.T) / 2
    else:
        if not err or len(err) != n:
            raise ValueError(f"BAO dataset {name}: no covariance and no error per measurement")
        invcov = np.diag([1.0 / e ** 2 for e in err])
    return {"name": name, "types": list(types), "z": np.array(z, dtype=np.float64),
            "obs": np.array(obs, dtype=np.float64), "invcov": np.ascontiguousarray(invcov),
            "rs_rescale": float(rs_rescale)}


def bao_theory(types, z, rs_rescale, *, DV, DA, H, rdrag, omegam_h2, fsigma8=None):
    """The theory vector of BAO_LnLike (bao.f90:274-301, Acoustic :250-263) at
    M design points: t [M, n] from the background quantities DV, DA, H
    [M, n] at the dataset's redshifts z [n] (BAO_D_v and
    AngularDiameterDistance in Mpc, H = Hofz_Hunit in km/s/Mpc), rdrag [M] in
    Mpc, omegam_h2 [M] = omegam h^2, and fsigma8 [M, n] when a type needs it.
    F_AP uses Hofz = H / c in 1/Mpc.  The target one hands to
    ``theory.fit_derived``."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = z.size
    if len(types) != n:
        raise ValueError("types and z differ in length")
    rs = np.asarray(rdrag, dtype=np.float64).reshape(-1) * rs_rescale
    M = rs.size
    DV, DA, H = [np.broadcast_to(np.asarray(a, dtype=np.float64), (M, n)) for a in (DV, DA, H)]
    omh2 = np.broadcast_to(np.asarray(omegam_h2, dtype=np.float64).reshape(-1), (M,))
    t = np.empty((M, n))
    for j, tp in enumerate(types):
        if tp == "DV_over_rs":
            t[:, j] = DV[:, j] / rs
        elif tp == "bao_Hz_rs":
            t[:, j] = H[:, j] * rs
        elif tp == "bao_Hz_rs_103":
            t[:, j] = H[:, j] * rs * 1.0e-3
        elif tp == "rs_over_DV":
            t[:, j] = rs / DV[:, j]
        elif tp == "Az":
            t[:, j] = 100 * DV[:, j] * np.sqrt(omh2) / (C_KM_S * z[j])
        elif tp == "DA_over_rs":
            t[:, j] = DA[:, j] / rs
        elif tp == "DM_over_rs":
            t[:, j] = (1 + z[j]) * DA[:, j] / rs
        elif tp == "F_AP":
            t[:, j] = (1 + z[j]) * DA[:, j] * (H[:, j] / C_KM_S)
        elif tp == "f_sigma8":
            if fsigma8 is None:
                raise ValueError("type f_sigma8 needs fsigma8")
            t[:, j] = np.broadcast_to(np.asarray(fsigma8, dtype=np.float64), (M, n))[:, j]
        else:
            raise ValueError(f"bao_theory: unknown or unsupported type {tp}")
    return t


# ---------------------------------------------------------------- tabulated BAO
def _overridden(path, overrides):
    ini = IniFile(path)
    for k, v in (overrides or {}).items():
        ini.set(k, v)
    return ini


def read_bao_likelihood(path, tag, overrides=None):
    """The BAO likelihood the reference makes of ``bao_dataset[tag] = path``.
    BAOLikelihood_Add picks the class by the tag, not by the file's ``name``
    (bao.f90:91-101): MGS a tabulated chi^2(alpha), DR11CMASS / DR12CMASS /
    DR12LOWZ a probability grid, every other tag the Gaussian.  Returns a dict
    with ``kind``:

    "gaussian": what ``read_bao_dataset`` returns.  A ``prob_dist`` key or the
        ``dilation`` type under such a tag is refused: the Gaussian class reads
        neither, and with ``dilation`` its ``bao_obs`` stays unset.
    "mgs": name, z, table [n] (BAO_MGS_InitProbDist: the ``prob_dist`` file).
    "grid": name, z, np, perp [np], plel [np], prob [np, np] divided by its
        maximum, DA_rd_fid and Hrd_fid (from ``Hrd_fid`` + ``DA_rd_fid``, or from
        ``rd_fid``, ``H_fid``, ``DA_fid``, :141-150).  The file is read as
        BAO_DR1x_InitProbDist does (:326-334): np x np lines of alpha_perp,
        alpha_plel, prob, the outer index over perp; perp[i] is the first
        column of block i's last line and plel[j] the second column of the
        last block's line j."""
    ini = _overridden(path, overrides)
    name = ini.get("name", os.path.splitext(os.path.basename(path))[0])
    types = ini.get("measurement_type", "").split()
    if tag not in GRID_SETS:
        if "prob_dist" in ini:
            raise ValueError(f"bao_dataset[{tag}]: prob_dist is read only under the tags {', '.join(GRID_SETS)}")
        if "dilation" in types:
            raise ValueError(f"bao_dataset[{tag}]: measurement_type dilation is served only under the tags "
                             f"{', '.join(GRID_SETS[1:])}")
        over = dict(overrides or {})
        if name in GRID_SETS:                            # the class follows the tag: a Gaussian whatever its name
            over["name"] = tag
        d = read_bao_dataset(path, over)
        d["name"] = name
        d["kind"] = "gaussian"
        return d
    if "prob_dist" not in ini:
        raise ValueError(f"bao_dataset[{tag}]: no prob_dist key")
    if "zeff" not in ini:
        raise ValueError(f"bao_dataset[{tag}]: no zeff key")
    z = float(ini["zeff"].split()[0])
    if z < 0.0001:
        raise ValueError(f"bao_dataset[{tag}]: error reading BAO measurements")
    if tag == "MGS":
        table = np.loadtxt(ini.relative_filename("prob_dist"), dtype=np.float64).reshape(-1)
        return {"kind": "mgs", "name": name, "z": z, "table": table}
    if "alpha_npoints" not in ini:
        raise ValueError(f"bao_dataset[{tag}]: no alpha_npoints key")
    npts = ini.read_int("alpha_npoints")
    if "Hrd_fid" in ini and "DA_rd_fid" in ini:
        Hrd_fid, DA_rd_fid = ini.read_float("Hrd_fid"), ini.read_float("DA_rd_fid")
    elif "rd_fid" in ini and "H_fid" in ini and "DA_fid" in ini:
        rd_fid, H_fid, DA_fid = ini.read_float("rd_fid"), ini.read_float("H_fid"), ini.read_float("DA_fid")
        Hrd_fid, DA_rd_fid = H_fid * rd_fid, DA_fid / rd_fid
    else:
        raise ValueError(f"bao_dataset[{tag}]: needs Hrd_fid and DA_rd_fid, or rd_fid, H_fid and DA_fid")
    a = np.loadtxt(ini.relative_filename("prob_dist"), dtype=np.float64).reshape(-1)
    if npts < 1 or a.size < 3 * npts * npts:
        raise ValueError(f"bao_dataset[{tag}]: Error reading BAO file")
    a = a[:3 * npts * npts].reshape(npts, npts, 3)
    prob = a[:, :, 2]
    return {"kind": "grid", "name": name, "z": z, "np": npts, "perp": np.ascontiguousarray(a[:, -1, 0]),
            "plel": np.ascontiguousarray(a[-1, :, 1]), "prob": np.ascontiguousarray(prob / np.max(prob)),
            "DA_rd_fid": float(DA_rd_fid), "Hrd_fid": float(Hrd_fid)}


def bao_alpha_theory(kind, z, *, DV=None, DA=None, H=None, rdrag):
    """The fit targets of a tabulated BAO likelihood's surfaces at M design
    points, the pendant of ``bao_theory``: "mgs" D_V / r_drag [M]; "grid"
    [D_A / r_drag, H r_drag] [M, 2], from BAO_D_v and AngularDiameterDistance
    in Mpc and H = Hofz_Hunit in km/s/Mpc at the dataset's z (which the caller
    has used already: it is taken for the record only) and rdrag [M] in Mpc.
    rs_rescale does not enter (get_rs_drag is called bare, bao.f90:356, 401)."""
    del z
    rs = np.asarray(rdrag, dtype=np.float64).reshape(-1)
    if kind == "mgs":
        return np.broadcast_to(np.asarray(DV, dtype=np.float64).reshape(-1), rs.shape) / rs
    if kind == "grid":
        DA, H = [np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1), rs.shape) for a in (DA, H)]
        return np.stack([DA / rs, H * rs], axis=1)
    raise ValueError(f"bao_alpha_theory: unknown kind {kind}")


# ---------------------------------------------------------------- HST and abundances
def _as_ini(ini):
    return ini if isinstance(ini, IniFile) else IniFile(ini)


def read_hst(ini):
    """HSTLikelihood_Add (HST.f90:26-45): None without ``use_HST``, else name
    (``Hubble_name``), H0, H0_err, zeff (``Hubble_zeff``, 0.04) and
    angconversion (``Hubble_angconversion``, 11425.8; read only for zeff > 0).
    The likelihood is ``DerivedGaussian.prior`` with mean H0 and std H0_err on
    the surface ``hst_theory``."""
    ini = _as_ini(ini)
    if not ini.read_bool("use_HST", False):
        return None
    for k in ("Hubble_name", "Hubble_H0", "Hubble_H0_err"):
        if k not in ini:
            raise ValueError(f"use_HST: no {k} key")
    zeff = ini.read_float("Hubble_zeff", 0.04)
    ang = ini.read_float("Hubble_angconversion", 11425.8) if zeff > 0 else 11425.8
    return {"name": ini["Hubble_name"], "H0": ini.read_float("Hubble_H0"), "H0_err": ini.read_float("Hubble_H0_err"),
            "zeff": zeff, "angconversion": ang}


def hst_theory(zeff, angconversion, *, DA=None, H0=None):
    """HST_LnLike's theory value (HST.f90:52-56): H0 with zeff = 0, else
    angconversion / AngularDiameterDistance(zeff)."""
    if zeff > 0:
        return angconversion / np.asarray(DA, dtype=np.float64)
    return np.asarray(H0, dtype=np.float64)


def read_abundance_dataset(path, overrides=None, bbn_consistency=True):
    """An ``abundance_dataset[TAG]`` file (Abundance_ReadIni,
    ElementAbundances.f90:52-94) as a dict: name, measurement (``Yp`` or
    ``D/H``), theory_table, and the Gaussian (theory + offset - mean)^2 / (2
    (error^2 + theory_effective_error^2)) of :112-113 as obs = mean - offset
    and std = sqrt(error^2 + theory_effective_error^2), for
    ``DerivedGaussian.prior`` on a surface fitted to the BBN table's value at
    the design points.  Refuses theory_effective_error = 0 with BBN
    consistency: the reference then takes the error from a table as well, so
    the variance moves with the point.  Without BBN consistency ``Yp`` is
    compared with the nucleon fraction of the free Y_He and no theory key is
    read; ``D/H`` needs BBN consistency."""
    ini = _overridden(path, overrides)
    name = ini.get("name", os.path.splitext(os.path.basename(path))[0])
    if "measurement" not in ini:
        raise ValueError(f"abundance dataset {name}: no measurement key")
    meas = ini["measurement"]
    if meas not in ("Yp", "D/H"):
        raise ValueError(f"abundance dataset {name}: un-recognised measurement name {meas}")
    if meas == "D/H" and not bbn_consistency:
        raise ValueError(f"abundance dataset {name}: D/H abundance measurement requires BBN consistency")
    for k in ("mean", "error"):
        if k not in ini:
            raise ValueError(f"abundance dataset {name}: no {k} key")
    mean, error = ini.read_float("mean"), ini.read_float("error")
    offset = terr = 0.0
    table = ""
    if bbn_consistency:
        offset = ini.read_float("theory_bias_offset", 0.0)
        terr = ini.read_float("theory_effective_error", 0.0)
        table = ini.get("theory_table", "")
        if not terr > 0:
            raise ValueError(f"abundance dataset {name}: theory_effective_error = 0 takes the theory error from the "
                             "BBN table, a variance that moves with the point; not supported")
    return {"name": name, "measurement": meas, "mean": mean, "error": error, "theory_bias_offset": offset,
            "theory_effective_error": terr, "theory_table": table, "obs": mean - offset,
            "std": float(np.sqrt(error ** 2 + terr ** 2))}


def _tagged(ini, prefix):
    """(tag, file, overrides) of every ``prefix[TAG] = file`` in the ini's key
    order, with its ``prefix[TAG,key] = value`` settings (TagValuesForName,
    SettingValuesForTagName)."""
    out = []
    pat = re.compile(r"^" + re.escape(prefix) + r"\[([^,\]]+)\]$")
    for key in ini.keys():
        mt = pat.match(key)
        if not mt:
            continue
        tag = mt.group(1)
        opat = re.compile(r"^" + re.escape(prefix) + r"\[" + re.escape(tag) + r",(.+)\]$")
        over = {mo.group(1): ini[k] for k in ini.keys() for mo in [opat.match(k)] if mo}
        out.append((tag, ini.relative_filename(key), over))
    return out


def derived_likelihood_specs(ini, bbn_consistency=True):
    """The derived likelihoods an ini (an IniFile or a path) switches on, in
    the reference's order (DataLikelihoods.f90: abundances, HST, BAO), each as
    the dict its reader returns with ``name`` set to the name of its
    ``chi2_<name>`` chain column and ``kind`` "prior" (obs, std), "gaussian",
    "mgs" or "grid":

      ``abundance_dataset[TAG]`` (+ ``[TAG,key]`` settings): a prior named TAG
      ``use_HST``: a prior named by ``Hubble_name``
      ``use_BAO`` with ``bao_dataset[TAG]`` (+ settings): named TAG, of the
          kind ``read_bao_likelihood`` gives the tag

    ``BAO_fixed_rs`` is refused: it changes the theory, which is the surface
    provider's."""
    ini = _as_ini(ini)
    out = []
    for tag, path, over in _tagged(ini, "abundance_dataset"):
        d = read_abundance_dataset(path, over, bbn_consistency)
        out.append({**d, "kind": "prior", "dataset_name": d["name"], "name": tag})
    h = read_hst(ini)
    if h is not None:
        out.append({**h, "kind": "prior", "obs": h["H0"], "std": h["H0_err"]})
    if ini.read_bool("use_BAO", False):
        sets = _tagged(ini, "bao_dataset")
        if not sets:
            raise ValueError("Use_BAO but no bao_dataset[NAMETAG] defined")
        if "BAO_fixed_rs" in ini:
            raise ValueError("BAO_fixed_rs is not supported: it replaces r_drag in the theory, which the provider of "
                             "the surfaces computes")
        for tag, path, over in sets:
            d = read_bao_likelihood(path, tag, over)
            out.append({**d, "dataset_name": d["name"], "name": tag})
    return out


def derived_likelihoods_from_ini(ini, calc, surfaces, bbn_consistency=True):
    """``derived_likelihood_specs`` as objects on ``calc`` for
    ``BatchedMCMC.add_derived_likelihood``: a list of ``DerivedGaussian`` /
    ``DerivedTable`` named as the specs.  surfaces: name -> coefficient
    columns over calc's monomials, fitted by the theory provider to
    ``bao_theory`` ([n_terms, n]), ``bao_alpha_theory`` ([n_terms] or
    [n_terms, 2]), ``hst_theory`` or the BBN table's value ([n_terms])."""
    specs = derived_likelihood_specs(ini, bbn_consistency)
    for d in specs:
        if d["name"] not in surfaces:
            raise KeyError(f"no surface given for the likelihood {d['name']}")
    out = []
    try:
        for d in specs:
            s, name = surfaces[d["name"]], d["name"]
            if d["kind"] == "prior":
                out.append(DerivedGaussian.prior(calc, s, d["obs"], d["std"], name=name))
            elif d["kind"] == "gaussian":
                out.append(DerivedGaussian(calc, s, d["obs"], invcov=d["invcov"], name=name))
            elif d["kind"] == "mgs":
                out.append(DerivedTable.mgs(calc, s, d["table"], name=name))
            else:
                out.append(DerivedTable.grid(calc, s, d["perp"], d["plel"], d["prob"], d["DA_rd_fid"], d["Hrd_fid"],
                                             name=name))
    except Exception:
        for g in out:
            g.close()
        raise
    return out

