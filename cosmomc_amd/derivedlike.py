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
"""
from __future__ import annotations

import ctypes as C
import os

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


class DerivedGaussian:
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
