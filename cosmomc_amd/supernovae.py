"""JLA supernova likelihood (reference source/supernovae_JLA.f90).

``JLALikelihood`` is the dataset opened in the HIP library (``cmbl_open`` tag
``"JLA"``): nuisance parameters ``alpha_JLA beta_JLA``, and as theory one row
of distance moduli per walker (``jla_distance_moduli``) instead of C_l.
``jla_likelihood_add`` mirrors ``JLALikelihood_Add`` (:221-262).

``JLAMargeLikelihood`` is the same dataset with ``JLA_marginalize = T``
(``cmbl_open`` tag ``"JLA_MARGE"``): alpha and beta are integrated over the
reference's fixed grid (:235-252, 1207-1217) inside the likelihood, which then
has no nuisance parameters.  ``jla_marge_grid`` and ``jla_marge_loglike_host``
restate the grid and the integral on the host.

``jla_loglike_host`` is a float64 numpy restatement of
``JLA_alpha_beta_like`` (:1028-1168): the public host reference.  It factors
V(alpha, beta) and solves for the three right-hand sides instead of forming
the reference's explicit inverse, and keeps the reference's single-precision
details (the squared errors of the light-curve file and ``zfacsq``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .ini import IniFile
from .likelihood import NativeCMBLikelihood

LOGZERO = N.CMBL_LOGZERO
JLA_VERSION = "December_2013"
COMPONENTS = ("mag", "stretch", "colour", "mag_stretch", "mag_colour", "stretch_colour")


def _open_as_written(name: str, dataset: str) -> str:
    """The reference's plain OPEN: the name as written, else beside the dataset file."""
    if os.path.isabs(name) or os.path.exists(name):
        return name
    cand = os.path.join(os.path.dirname(dataset), name)
    return cand if os.path.exists(cand) else name


class JLADataset:
    """read_jla_dataset + jla_prep (:602-760, 874-957) on the host."""

    def __init__(self, dataset: str, overrides: dict | None = None, marginalised: bool = False):
        ini = IniFile(text="".join(f"{k} = {v}\n" for k, v in (overrides or {}).items()))
        ini._open(dataset, 0)          # first definition wins: the overrides
        self.filename = dataset
        self.name = ini.get("name", "")
        if ini.read_bool("JLA_marginalize") and not marginalised:    # marginalised: JLAMargeLikelihood's own use
            raise NotImplementedError("JLA_marginalize = T is not supported")
        if ini.read_bool("absdist_file"):
            raise NotImplementedError("absdist_file is not supported")
        rows = []
        with open(_open_as_written(ini.get("data_file", "data/jla_lcparams.txt"), dataset)) as f:
            for line in f:
                t = line.split()
                if not t or t[0].startswith("#"):
                    continue
                if len(t) != 16:
                    raise ValueError(f"light-curve row of {len(t)} columns; only the 16-column layout is read")
                rows.append([float(x) for x in t[1:15]] + [int(t[15])])
        d = np.array(rows, dtype=np.float64)
        self.nsn = n = len(d)
        self.zcmb, self.zhel, self.mag = d[:, 0], d[:, 1], d[:, 3]
        self.stretch, self.colour, self.thirdvar = d[:, 5], d[:, 7], d[:, 9]

        def sq(x):                                       # REAL squared before promotion (:378, 475-479)
            f = x.astype(np.float32)
            return (f * f).astype(np.float64)
        mag_var, self.stretch_var, self.colour_var = sq(d[:, 4]), sq(d[:, 6]), sq(d[:, 8])
        self.cov_ms, self.cov_mc, self.cov_sc = d[:, 11], d[:, 12], d[:, 13]
        sets = d[:, 14].astype(int)
        if sets.min() < 0 or sets.max() > 9:
            raise ValueError("invalid dataset number (0..9 allowed)")
        idz = float(ini.get("intrinsicdisp", "0.13"))
        idisp = np.array([float(ini.get(f"intrinsicdisp{i}", idz)) for i in range(10)])
        pecz = float(ini.get("pecz", "0.001"))
        zfacsq = float(np.float32(25.0) / np.log(np.float32(10.0)) ** 2)   # :882
        z = self.zcmb
        self.pre_vars = mag_var + idisp[sets] ** 2 + zfacsq * pecz ** 2 * ((1 + z) / (z * (1 + 0.5 * z))) ** 2
        self.twoscriptmfit = ini.read_bool("twoscriptmfit")
        cut = float(ini.get("scriptmcut", "10"))
        first = self.thirdvar <= cut
        if self.twoscriptmfit and first.all():
            self.twoscriptmfit = False                   # an empty second set (:950-956)
        self.one = first.astype(np.float64) if self.twoscriptmfit else np.ones(n)
        self.A2 = 1.0 - first if self.twoscriptmfit else np.zeros(n)
        self.comp = {}
        for k in COMPONENTS:
            if not ini.read_bool(f"has_{k}_covmat"):
                continue
            with open(_open_as_written(ini[f"{k}_covmat_file"], dataset)) as f:
                nfile = int(f.readline().split()[0])
                if nfile != n:
                    raise ValueError(f"{k}_covmat_file: expected size {n} got {nfile}")
                m = np.array(f.read().split(), dtype=np.float64)
            if m.size != n * n:
                raise ValueError(f"{k}_covmat_file is the wrong size")
            m = m.reshape(n, n)
            self.comp[k] = np.triu(m) + np.triu(m, 1).T   # uplo = 'U' (:135)
        self.diag_errors = not self.comp


def jla_loglike_host(dataset, alpha: float, beta: float, mu) -> float:
    """-lnL of JLA_alpha_beta_like at one point: ``dataset`` a JLADataset or a
    jla.dataset path, ``mu`` the nsn distance moduli (lumdists)."""
    D = dataset if isinstance(dataset, JLADataset) else JLADataset(dataset)
    mu = np.asarray(mu, dtype=np.float64)
    a, b = float(alpha), float(beta)
    dv = D.pre_vars + a * a * D.stretch_var + b * b * D.colour_var + 2 * a * D.cov_ms - 2 * b * D.cov_mc \
        - 2 * a * b * D.cov_sc
    iv = 1.0 / dv
    scriptm = np.sum((D.mag - mu) * iv) / iv.sum()
    dm = D.mag - mu + a * D.stretch - b * D.colour - scriptm
    R = np.stack([dm, D.one, D.A2], 1)
    if D.diag_errors:
        G = R.T @ (iv[:, None] * R)
    else:
        coef = {"mag": 1.0, "stretch": a * a, "colour": b * b, "mag_stretch": 2 * a, "mag_colour": -2 * b,
                "stretch_colour": -2 * a * b}
        V = np.diag(dv)
        for k in COMPONENTS:
            if k in D.comp:
                V = V + coef[k] * D.comp[k]
        try:
            L = np.linalg.cholesky(V)
        except np.linalg.LinAlgError:
            return LOGZERO                               # DPOTRF status /= 0 (:1085-1092)
        Y = _forward_solve(L, R)
        G = Y.T @ Y
    A, B, C, E, Dd, F = G[0, 0], G[0, 1], G[0, 2], G[1, 1], G[1, 2], G[2, 2]
    tp = 1.0 / (2 * np.pi)
    if D.twoscriptmfit:
        g = F - Dd * Dd / E
        if not g > 0:
            return LOGZERO
        chisq = A + np.log(E * tp) + np.log(g * tp) - C * C / g - B * B * F / (E * g) + 2 * B * C * Dd / (E * g)
    else:
        chisq = A + np.log(E * tp) - B * B / E
    return float(chisq / 2)


def _forward_solve(L, R):
    """L^-1 R for lower-triangular L, by blocked forward substitution."""
    n = len(L)
    Y = np.array(R, dtype=np.float64)
    nb = 32
    for i0 in range(0, n, nb):
        i1 = min(n, i0 + nb)
        if i0:
            Y[i0:i1] -= L[i0:i1, :i0] @ Y[:i0]
        for i in range(i0, i1):
            Y[i] = (Y[i] - L[i, i0:i] @ Y[i0:i]) / L[i, i]
    return Y


def jla_distance_moduli(zcmb, zhel, DA):
    """The theory row of jla_LnLike (:1195-1199): 5 log10((1+zhel)(1+zcmb) D_A(zcmb)),
    D_A the angular diameter distance in Mpc.  DA may carry leading walker axes."""
    zcmb, zhel = np.asarray(zcmb, dtype=np.float64), np.asarray(zhel, dtype=np.float64)
    return 5.0 * np.log10((1.0 + zhel) * (1.0 + zcmb) * np.asarray(DA, dtype=np.float64))


class _LightCurves:
    def __init__(self, zcmb, zhel):
        self.zcmb, self.zhel = zcmb, zhel


class JLALikelihood(NativeCMBLikelihood):
    """The JLA dataset in the HIP library.  ``loglike_batch(dl, nuis)`` takes
    ``dl`` as a cuda float64 tensor [W, 1, n_theory] of distance moduli (or
    [W, nf, L >= n_theory]: field 0 is read) and ``nuis`` [W, 2] = (alpha, beta)."""
    LikelihoodType = "SN"

    def __init__(self, dataset: str, overrides: dict | None = None):
        super().__init__("JLA", dataset, overrides)
        self.name = "JLA"
        self.tag = ""                      # GetTag falls back to the name: chi2_JLA
        self.version = JLA_VERSION
        self.n_theory = N.lib().cmbl_theory_len(self._h)
        self.dataset = dataset
        self._overrides = overrides
        self._lc = None

    @property
    def lc(self):
        """zcmb / zhel of the light-curve file, to build theory rows from distances."""
        if self._lc is None:
            d = JLADataset(self.dataset, self._overrides)
            self._lc = _LightCurves(d.zcmb, d.zhel)
        return self._lc


# ------------------------------------------------------------ JLA_marginalize = T

ALPHA_CENTER = float(np.float32(0.14))       # JLA_alpha_center, JLA_beta_center: single-precision
BETA_CENTER = float(np.float32(3.123))       # literals promoted to double (:119-120)
MARGE_DEFAULTS = dict(steps=7, width_alpha=0.003, width_beta=0.04)     # :237-239


def jla_marge_grid(steps: int = 7, width_alpha: float = 0.003, width_beta: float = 0.04, center=None):
    """(alpha, beta) of the marginalisation grid in the reference's order
    (:243-251): alpha_i outer, beta_i inner, alpha_i^2 + beta_i^2 <= steps^2."""
    ca, cb = (ALPHA_CENTER, BETA_CENTER) if center is None else (float(center[0]), float(center[1]))
    pts = [(ai, bi) for ai in range(-steps, steps + 1) for bi in range(-steps, steps + 1)
           if ai * ai + bi * bi <= steps * steps]
    return (np.array([ca + ai * float(width_alpha) for ai, _ in pts]),
            np.array([cb + bi * float(width_beta) for _, bi in pts]))


def jla_marge_points_host(dataset, mu, steps: int = 7, width_alpha: float = 0.003, width_beta: float = 0.04,
                          center=None):
    """JLA_marge_grid (:1209-1213): jla_loglike_host at every grid point, LOGZERO where V does not factor."""
    D = dataset if isinstance(dataset, JLADataset) else JLADataset(dataset, marginalised=True)
    al, be = jla_marge_grid(steps, width_alpha, width_beta, center)
    return np.array([jla_loglike_host(D, a, b, mu) for a, b in zip(al, be)])


def jla_marge_loglike_host(dataset, mu, steps: int = 7, width_alpha: float = 0.003, width_beta: float = 0.04,
                           center=None) -> float:
    """-lnL of jla_LnLike with JLA_marginalize = T (:1207-1217) for one row of
    distance moduli, in float64 numpy on top of jla_loglike_host: the points
    that return LOGZERO are masked out of the minimum and of the sum."""
    L = jla_marge_points_host(dataset, mu, steps, width_alpha, width_beta, center)
    L = L[L != LOGZERO]
    if L.size == 0:
        raise ValueError("V(alpha, beta) is not positive definite at any grid point")
    best = L.min()
    v = best - np.log(np.sum(np.exp(-L + best)) * float(width_alpha) * float(width_beta))
    return float(v) if np.isfinite(v) else LOGZERO


class JLAMargeLikelihood(NativeCMBLikelihood):
    """The JLA dataset with alpha and beta marginalised on the reference's grid,
    in the HIP library (tag ``"JLA_MARGE"``).  V(alpha, beta)^-1 of every grid
    point is formed on the device when the dataset is opened; an evaluation is
    then one batched quadratic form per grid point.  ``loglike_batch(dl, None)``
    takes ``dl`` as for JLALikelihood; there are no nuisance parameters."""
    LikelihoodType = "SN"

    def __init__(self, dataset: str, steps: int = 7, width_alpha: float = 0.003, width_beta: float = 0.04,
                 overrides: dict | None = None):
        over = dict(overrides or {})
        over.update(JLA_marge_steps=int(steps), JLA_step_width_alpha=repr(float(width_alpha)),
                    JLA_step_width_beta=repr(float(width_beta)))
        super().__init__("JLA_MARGE", dataset, over)
        self.name = "JLA"
        self.tag = ""                      # GetTag falls back to the name: chi2_JLA
        self.version = JLA_VERSION
        self.n_theory = N.lib().cmbl_theory_len(self._h)
        self.dataset = dataset
        self.steps, self.width_alpha, self.width_beta = int(steps), float(width_alpha), float(width_beta)
        self._overrides = over
        self._lc = None
        ng, npts, nb = C.c_int(), C.c_int(), C.c_size_t()
        N.check(N.lib().cmbl_jla_marge_info(self._h, C.byref(ng), C.byref(npts), C.byref(nb)), self._h)
        self._n_grid, self.n_points, self._grid_bytes = ng.value, npts.value, nb.value

    @property
    def n_grid(self) -> int:
        """Grid points integrated over: those of the grid at which V(alpha, beta) factors."""
        return self._n_grid

    @property
    def grid_bytes(self) -> int:
        """Device bytes of the stored V(alpha_g, beta_g)^-1 (0 with diag_errors)."""
        return self._grid_bytes

    @property
    def lc(self):
        """zcmb / zhel of the light-curve file, to build theory rows from distances."""
        if self._lc is None:
            d = JLADataset(self.dataset, self._overrides, marginalised=True)
            self._lc = _LightCurves(d.zcmb, d.zhel)
        return self._lc

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


def jla_likelihood_add(like_list, ini: IniFile, allow_marginalize: bool = False):
    """JLALikelihood_Add (:221-262): use_JLA, jla_dataset, jla_version.  JLA_marginalize = T
    is refused unless allow_marginalize: then JLA_marge_steps, JLA_step_width_alpha and
    JLA_step_width_beta are read from the same ini (:237-239) and a JLAMargeLikelihood is added."""
    if not ini.read_bool("use_JLA", False):
        return None
    marge = ini.read_bool("JLA_marginalize", False)
    if marge and not allow_marginalize:
        raise NotImplementedError("JLA_marginalize = T is not supported: alpha_JLA and beta_JLA are sampled")
    if "jla_dataset" in ini:
        fname = ini.relative_filename("jla_dataset")
    else:
        fname = os.path.join(ini.datasetdir, "jla.dataset")
    if marge:
        like = JLAMargeLikelihood(fname, int(ini.get("JLA_marge_steps", "7")),
                                  float(ini.get("JLA_step_width_alpha", "0.003")),
                                  float(ini.get("JLA_step_width_beta", "0.04")))
    else:
        like = JLALikelihood(fname)
    like.version = ini.get("jla_version", JLA_VERSION)
    like_list.add(like)
    return like
