"""Polynomial theory calculator (host wrapper of ``cmbt_*``) and its fit.

The reference fills the theory slot of a likelihood evaluation with a
calculator object; besides CAMB it ships a polynomial emulator of the C_l
(source/Calculator_PICO.f90), whose error flag outside its training box makes
the point logZero (source/calclike.f90:308-313).  ``PolynomialTheory``
evaluates such a response surface of D_l on the GPU, straight into a theory
buffer, and ``BatchedMCMC.set_theory_calculator`` makes it the sampler's
theory source, so slow steps need no host callback.

    x_i     = (P[param_index_i] - center_i) / scale_i
    basis_k = prod_i x_i ** exponents[k, i]
    D_l[field_j] = sum_k basis_k * coef[k, j, l]

``monomials`` and ``fit_coefficients`` are pure numpy: the surface is fitted
offline from theory computed elsewhere (e.g. CAMB at a design of points).

Derived parameters (the parameterization's H0, omegam, sigma8, ..., DL40 ..
DL2000 of the reference's chain rows, CosmologyParameterizations.f90:189-272)
are scalar surfaces over the same monomials, ``derived_d = sum_k basis_k *
dcoef[k, d]`` (``fit_derived``, ``dl_columns``, ``set_derived``,
``derived``); their hard ranges are TP_NonBaseParameterPriors' cuts (:90-112):
a point whose derived value leaves its range fails like one outside the box.
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np

from . import _native as N

MAX_DEGREE = 4                                       # PICO's order, and cmbt_create's limit per term


def monomials(n_in: int, degree: int) -> np.ndarray:
    """Exponent table [K, n_in] of every monomial of total degree <= ``degree``
    in graded lexicographic order, the constant term first: by total degree,
    and within a degree the higher power of the earlier input first, e.g.
    monomials(2, 2) = 00, 10, 01, 20, 11, 02.  K = C(n_in + degree, degree)."""
    if n_in < 1:
        raise ValueError("n_in must be positive")
    if degree < 0 or degree > MAX_DEGREE:
        raise ValueError(f"degree must be in 0..{MAX_DEGREE}")
    rows = []
    for d in range(degree + 1):
        grade = [e for e in itertools.product(range(d, -1, -1), repeat=n_in) if sum(e) == d]
        rows.extend(sorted(grade, reverse=True))
    return np.array(rows, dtype=np.int32).reshape(-1, n_in)


def basis(points, exponents, center, scale) -> np.ndarray:
    """[M, K] monomials at points [M, n_in], formed as cmbt_eval forms them:
    from 1.0, inputs ascending, every power by repeated multiplication."""
    x = (np.asarray(points, dtype=np.float64) - np.asarray(center, dtype=np.float64)) / \
        np.asarray(scale, dtype=np.float64)
    ex = np.asarray(exponents, dtype=np.int64).reshape(-1, x.shape[1])
    B = np.ones((x.shape[0], ex.shape[0]))
    for k, row in enumerate(ex):
        for i, e in enumerate(row):
            for _ in range(int(e)):
                B[:, k] = B[:, k] * x[:, i]
    return B


def fit_coefficients(points, theory, exponents, center, scale):
    """Least-squares fit of a surface: points [M, n_in] (raw parameters),
    theory [M, n_fields, lmax + 1] (D_l at the points).  Returns
    (coef [K, n_fields, lmax + 1], the maximum absolute residual)."""
    th = np.asarray(theory, dtype=np.float64)
    if th.ndim != 3:
        raise ValueError("theory must be [M, n_fields, lmax + 1]")
    B = basis(points, exponents, center, scale)
    if B.shape[0] != th.shape[0]:
        raise ValueError("points and theory differ in their number of rows")
    if B.shape[0] < B.shape[1]:
        raise ValueError(f"{B.shape[1]} terms need at least as many points, got {B.shape[0]}")
    Y = th.reshape(th.shape[0], -1)
    sol = np.linalg.lstsq(B, Y, rcond=None)[0]
    resid = float(np.max(np.abs(B @ sol - Y))) if Y.size else 0.0
    return sol.reshape(B.shape[1], th.shape[1], th.shape[2]), resid


def fit_derived(points, values, exponents, center, scale):
    """Least-squares fit of scalar surfaces over the calculator's monomials:
    points [M, n_in] (raw parameters), values [M, n_derived] (e.g. H0, sigma8
    at the points).  Returns (coef [K, n_derived], the maximum absolute
    residual), as fit_coefficients."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 2:
        raise ValueError("values must be [M, n_derived]")
    coef, resid = fit_coefficients(points, v[:, None, :], exponents, center, scale)
    return np.ascontiguousarray(coef[:, 0, :]), resid


def dl_columns(coef, field_pos, ells):
    """Derived-output coefficients [K, n] that reproduce D_l bit for bit:
    column i is coef[:, field_pos[i], ells[i]] of the calculator's table
    [K, n_fields, lmax + 1] (field_pos: positions in the calculator's field
    list; a scalar applies to every l) -- the reference's DL40 .. DL2000."""
    coef = np.asarray(coef, dtype=np.float64)
    if coef.ndim != 3:
        raise ValueError("coef must be [n_terms, n_fields, lmax + 1]")
    ells = np.asarray(ells, dtype=np.int64).reshape(-1)
    pos = np.broadcast_to(np.asarray(field_pos, dtype=np.int64), ells.shape)
    if np.any(pos < 0) or np.any(pos >= coef.shape[1]) or np.any(ells < 0) or np.any(ells >= coef.shape[2]):
        raise ValueError("field position or l outside the coefficient table")
    return np.ascontiguousarray(coef[:, pos, ells])


class PolynomialTheory:
    """A ``cmbt_t``.  param_index: 1-based indices into P of the n_in inputs;
    lo, hi: the validity box on the raw parameters; exponents [K, n_in];
    fields: theory field indices (TT=0 TE=1 EE=2 ... PP=9); coef
    [K, n_fields, lmax + 1]."""

    def __init__(self, param_index, center, scale, lo, hi, exponents, fields, coef):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 3:
            raise ValueError("coef must be [n_terms, n_fields, lmax + 1]")
        pi = np.ascontiguousarray(param_index, dtype=np.int32).reshape(-1)
        ex = np.ascontiguousarray(exponents, dtype=np.int32)
        fl = np.ascontiguousarray(fields, dtype=np.int32).reshape(-1)
        n_in = pi.size
        dbl = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (center, scale, lo, hi)]
        if any(a.size != n_in for a in dbl):
            raise ValueError("center, scale, lo and hi need one entry per input")
        if ex.size != coef.shape[0] * n_in or fl.size != coef.shape[1]:
            raise ValueError("exponents must be [n_terms, n_in] and fields [n_fields] of coef [n_terms, n_fields, :]")
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        cfg = N.CmbtConfig()
        cfg.n_in, cfg.param_index = n_in, pi.ctypes.data_as(ip)
        cfg.center, cfg.scale, cfg.lo, cfg.hi = [a.ctypes.data_as(dp) for a in dbl]
        cfg.n_terms, cfg.exponents = coef.shape[0], ex.ctypes.data_as(ip)
        cfg.n_fields, cfg.fields = fl.size, fl.ctypes.data_as(ip)
        cfg.lmax, cfg.coef = coef.shape[2] - 1, coef.ctypes.data_as(dp)
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = N.lib().cmbt_create(C.byref(cfg), C.byref(h), err, 1024)
        if rc:
            raise N.NativeError(rc, err.value.decode())
        self.handle = h
        self.n_in, self.n_terms, self.lmax = n_in, coef.shape[0], coef.shape[2] - 1
        self.fields = fl.tolist()
        self.derived_names, self.derived_ranges = [], []     # [(name, label)], [(name, lo or None, hi or None)]

    def eval(self, P_rows, out, fail=None, stream=None):
        """Evaluate into ``out``, a cuda float64 theory tensor [W, n_field_rows, L]
        (last stride 1); only the calculator's fields, l <= lmax, are written.

        P_rows: a cuda float64 tensor [num_params, W] with walker stride 1
        (what a sampler's theory_fn receives), or a host array [W, num_params]
        of points (what importance.GPUEvaluator's theory_fn receives).
        fail: a cuda int32 tensor [W] that receives 1 for the walkers outside
        the box (which are evaluated at their clamped inputs), else 0."""
        import torch
        P_rows, ld = self._rows(P_rows)
        num_params, W = P_rows.shape
        if out.dim() != 3 or out.dtype != torch.float64 or out.shape[0] != W or out.stride(2) != 1:
            raise ValueError("out must be float64 [W, fields, L] with last stride 1")
        # (a field row shorter than lmax + 1 in its stride too is cmbt_eval's own argument error)
        if max(self.fields) >= out.shape[1] or (self.lmax >= out.shape[2] and out.stride(1) > self.lmax):
            raise ValueError(f"out {tuple(out.shape)} does not hold fields {self.fields} to lmax {self.lmax}")
        if fail is not None and (fail.dtype != torch.int32 or fail.numel() < W or not fail.is_contiguous()):
            raise ValueError("fail must be a contiguous int32 tensor [W]")
        if stream is None:
            stream = N.current_stream_ptr()
        N.check(N.lib().cmbt_eval(self.handle, W, P_rows.data_ptr(), ld, num_params, out.data_ptr(), out.stride(1),
                                  out.stride(0), None if fail is None else fail.data_ptr(), stream),
                self.handle, "cmbt")

    def set_derived(self, names, coef, lo=None, hi=None, labels=None):
        """Calculator-derived parameters (``cmbt_set_derived``): ``names`` of
        the n_derived <= 32 outputs, coef [n_terms, n_derived] over the
        calculator's monomials (fit_derived, dl_columns); lo / hi: hard ranges
        per output (None or +-inf: no limit on that side).  With a range set,
        eval's fail flags -- and so the sampler's slow steps -- also reject a
        point whose output leaves its range (TP_NonBaseParameterPriors'
        cuts).  names=None removes the derived outputs."""
        self.derived_names, self.derived_ranges = [], []
        if names is None:
            N.check(N.lib().cmbt_set_derived(self.handle, None), self.handle, "cmbt")
            return
        names = [str(n) for n in names]
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] != self.n_terms or coef.shape[1] != len(names):
            raise ValueError(f"coef must be [n_terms = {self.n_terms}, n_derived = {len(names)}]")
        labels = list(labels) if labels is not None else names
        if len(labels) != len(names):
            raise ValueError("labels need one entry per name")
        dp = C.POINTER(C.c_double)
        cfg = N.CmbtDerivedConfig()
        cfg.n_derived, cfg.coef = len(names), coef.ctypes.data_as(dp)
        lims = []
        for side, fill in ((lo, -np.inf), (hi, np.inf)):
            if side is None:
                lims.append(None)
                continue
            a = np.array([fill if v is None else v for v in side], dtype=np.float64).reshape(-1)
            if a.size != len(names):
                raise ValueError("lo and hi need one entry per name")
            lims.append(a)
        cfg.lo = lims[0].ctypes.data_as(dp) if lims[0] is not None else None
        cfg.hi = lims[1].ctypes.data_as(dp) if lims[1] is not None else None
        N.check(N.lib().cmbt_set_derived(self.handle, C.byref(cfg)), self.handle, "cmbt")
        self.derived_names = list(zip(names, labels))
        for k, n in enumerate(names):
            mn = None if lims[0] is None or not np.isfinite(lims[0][k]) else float(lims[0][k])
            mx = None if lims[1] is None or not np.isfinite(lims[1][k]) else float(lims[1][k])
            self.derived_ranges.append((n, mn, mx))

    def derived(self, P_rows, out=None, fail=None, stream=None):
        """The derived outputs at P_rows (the forms eval accepts): a cuda
        float64 tensor [n_derived, M] (``out``, last stride 1, when given).
        fail: a cuda int32 tensor [M] that receives 1 for the points outside
        the box or, with ranges set, outside a range."""
        import torch
        P_rows, ld = self._rows(P_rows)
        num_params, M = P_rows.shape
        nd = N.lib().cmbt_derived_count(self.handle)
        if out is None:
            out = torch.empty((max(nd, 1), M), dtype=torch.float64, device="cuda")[:nd]
        if out.dim() != 2 or out.dtype != torch.float64 or out.shape != (nd, M) or (M > 1 and out.stride(1) != 1):
            raise ValueError(f"out must be float64 [{nd}, {M}] with last stride 1")
        if fail is not None and (fail.dtype != torch.int32 or fail.numel() < M or not fail.is_contiguous()):
            raise ValueError("fail must be a contiguous int32 tensor [M]")
        if stream is None:
            stream = N.current_stream_ptr()
        ld_out = out.stride(0) if nd > 1 else max(M, out.stride(0))
        N.check(N.lib().cmbt_derived_eval(self.handle, M, P_rows.data_ptr(), ld, num_params, out.data_ptr(), ld_out,
                                          None if fail is None else fail.data_ptr(), stream),
                self.handle, "cmbt")
        return out

    @staticmethod
    def _rows(P_rows):
        """(cuda float64 rows [num_params, M] with point stride 1, their ld)"""
        import torch
        if not torch.is_tensor(P_rows):
            P_rows = torch.as_tensor(np.ascontiguousarray(np.asarray(P_rows, dtype=np.float64).T), device="cuda")
        if P_rows.dim() != 2 or P_rows.dtype != torch.float64 or (P_rows.shape[1] > 1 and P_rows.stride(1) != 1):
            raise ValueError("P_rows must be float64 [num_params, W] with walker stride 1")
        num_params, W = P_rows.shape
        return P_rows, (P_rows.stride(0) if num_params > 1 else max(W, P_rows.stride(0)))

    def close(self):
        if getattr(self, "handle", None):
            N.lib().cmbt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
