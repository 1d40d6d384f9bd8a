"""Shared by the SZ cluster-counts tests: the goldens of the compiled reference
(tests/golden/sz/sz_fixture.tar.xz: inputs from tools/sz_make_fixture.py, which
calls make_synthetic below; outputs from tools/sz_ref_harness.f90).

A synthetic dataset is seeded: 1-8 sky patches whose fractions sum to about
0.65, 2-6 filter sizes theta (ascending, but for syn_unsorted), noise levels ylims[patch][theta] rising with
theta, and a catalogue of (z, z error, S/N) rows.  The grid of the model
(steps in z and ln M, the S/N bins, the ln Y integration) is the reference's
own and is in the code, not in the data, so a small dataset runs every path
of the full one."""
import io
import lzma
import os
import tarfile

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "the long-double reference needs x87 extended precision"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sz", "sz_fixture.tar.xz")
PARAM_NAMES = ["alpha_SZ", "ystar_SZ", "bias_SZ", "scatter_SZ", "beta_SZ"]
PRIORS = ["prior_alpha_SZ", "prior_ystar_SZ", "prior_scatter_SZ", "prior_beta_SZ", "prior_wtg", "prior_lens",
          "prior_cccp", "prior_ns", "prior_omegabh2"]
# H0 omegam omegav omegak w0 ns ombh2 of every golden
COSMO = (68.0, 0.31, 0.69, 0.0, -1.0, 0.955, 0.0226)
SIGMA_GRID = (64, float(np.log(0.5)), float(np.log(150.0)))      # nR, ln R range of the harness's sigma(R) table
CENTRE = (1.789, -0.186, 0.8, 0.075, 2.0 / 3.0)                  # batch2/SZ_plus_CMB.ini

# the filter sizes [arcmin] of the two geometries: the model's theta500 runs
# from about 0.7 (z = 1, the least mass) to about 2e8 (the first step in z)
THETA_INSIDE = (2.0, 40.0)
THETA_CONTAINS = (0.3, 1e10)

# syn_unsorted: the file's thetas are these positions of the ascending list.  The least stays first and the
# greatest last (the reference reads outside its table otherwise, and the loaders refuse such a file); the inner
# three are out of order, so the nearest theta is found by the linear search
UNSORTED_ORDER = (0, 3, 1, 2, 4)

#            name            keyword arguments of make_synthetic
GOLDENS = [("syn_inside", dict(seed=201, npatch=5, ntheta=6, theta=THETA_INSIDE, priors=("prior_scatter_SZ", "prior_ystar_SZ"),
                               points="all")),
           ("syn_contains", dict(seed=202, npatch=8, ntheta=5, theta=THETA_CONTAINS, points="all")),
           ("syn_cat", dict(seed=203, npatch=3, ntheta=4, theta=THETA_INSIDE, cat="edges", points="few")),
           ("syn_lastrow", dict(seed=204, npatch=3, ntheta=4, theta=THETA_INSIDE, cat="lastrow", points="few")),
           ("syn_two", dict(seed=206, npatch=1, ntheta=2, theta=THETA_INSIDE, points="few")),
           ("syn_unsorted", dict(seed=207, npatch=3, ntheta=5, theta=THETA_INSIDE, points="few", order=UNSORTED_ORDER))] + \
          [("syn_" + p, dict(seed=205, npatch=3, ntheta=4, theta=THETA_INSIDE, priors=(p,), points="prior")) for p in PRIORS] + \
          [("syn_prior_all", dict(seed=205, npatch=3, ntheta=4, theta=THETA_INSIDE, priors=tuple(PRIORS), points="prior"))]
WATSON_STRIDE = 37                     # sz/watson/row_sample.txt keeps every 37th number of the Watson row
SYNTHETIC = [n for n, _ in GOLDENS]
NAMES = SYNTHETIC + ["real"]          # the real SZ_* data files with a few points (tools/sz_make_fixture.py --real)


# ---- the pointwise tests of the completeness table (test_gpu_sz_edges.py; measured in test_szcounts.py)

def _with(**kw):
    p = dict(zip(PARAM_NAMES, CENTRE))
    p.update({k + "_SZ": v for k, v in kw.items()})
    return tuple(p[n] for n in PARAM_NAMES)


ZERO_SCATTER = (1.789, -0.186, 0.8, 0.0, 2.0 / 3.0)               # the scatter_SZ = 0 point of "few" and "all"
# dataset -> the nuisance points whose tables are compared entry by entry.  On syn_inside the scatters are
# chosen by the window of ln Y nodes they give (window_classes below)
EDGE_CASES = {"syn_inside": [CENTRE, _with(scatter=1e-3), _with(scatter=0.5), _with(scatter=3.0), _with(scatter=-0.075),
                             ZERO_SCATTER, _with(scatter=0.0, beta=0.3)],
              "syn_two": [CENTRE, ZERO_SCATTER],
              "syn_unsorted": [CENTRE, ZERO_SCATTER]}
# the points at which test_szcounts.py measures f64 against long double entry by entry, a dataset at a time: the
# cases above but -0.075 (it gives +0.075's table), 0.5 (2.2e-16, measured once) and the second scatter_SZ = 0
# point of syn_inside; and the worse of the two ill-conditioned goldens (alpha_SZ = 1, bias_SZ = 0.1,
# scatter_SZ = 0.022).  COMP_LD_ABS is what it measures, the largest absolute difference of an entry: 2^-47
# (7.105e-15) and 2^-44 (5.684e-14), each a single-precision ulp of a small entry whose rounding tipped
LD_TABLE_CASES = {"syn_inside": [CENTRE, _with(scatter=1e-3), _with(scatter=3.0), ZERO_SCATTER,
                                 (1.0, -0.186, 0.1, 0.022, 2.0 / 3.0)],
                  "syn_two": [CENTRE, ZERO_SCATTER], "syn_unsorted": [CENTRE, ZERO_SCATTER]}
COMP_LD_ABS = {"syn_inside": 7.11e-15, "syn_two": 7.11e-15, "syn_unsorted": 5.69e-14}
WINDOW_CLASSES = ("below", "cut_low", "inside", "cut_high", "above", "wider")


def scaling(ds, row, nuis):
    """theta500 and y500 [nzs][nm] of a theory row and nuisance point (:221-243), in f64."""
    from cosmomc_amd import szcounts as S
    row = np.asarray(row, dtype=np.float64)
    alpha, logystar, bias, _, beta = (float(x) for x in nuis)
    H0, E, dA = row[0], row[3:3 + ds.nzs], row[3 + ds.nzs:3 + 2 * ds.nzs]
    mfac = np.exp(ds.steps_m) * bias / S.M_PIVOT * (100 / H0)
    dfac = (100 * dA / 500 / H0)[:, None]
    thp = S.THETASTAR * (H0 / 70) ** S.M2_3 * mfac[None, :] ** S.ALPHA_THETA * (E ** S.M2_3)[:, None] / dfac
    ystar = 10.0 ** logystar / 2.0 ** alpha * S.YSTAR_NORM
    yp = ystar * (H0 / 70) ** (-2 + alpha) * mfac[None, :] ** alpha * (E ** beta)[:, None] / (dfac * dfac)
    return thp, yp


def window_classes(ds, row, nuis):
    """How many (z, m) have their window of ln Y nodes, |lny - ln y500| <= sqrt(746) sqrt(2) |scatter_SZ|,
    wholly below the grid of nodes, cut at its lower end, inside it, cut at its upper end, wholly above it,
    or wider than all of it; and how many of those below leave sz_compl_kernel's loop without a node (the
    window's upper end two steps or more under the first node)."""
    from cosmomc_amd import szcounts as S
    mu = np.log(scaling(ds, row, nuis)[1])
    reach = np.sqrt(746.0) * S.SQRT2 * abs(float(nuis[3]))
    lo, hi, first, last = mu - reach, mu + reach, ds.lny[0], ds.lny[-1]
    n = {"below": hi < first, "above": lo > last, "wider": (lo < first) & (hi > last),
         "cut_low": (lo < first) & (hi >= first) & (hi <= last), "cut_high": (lo >= first) & (lo <= last) & (hi > last),
         "inside": (lo >= first) & (hi <= last), "empty": hi <= first - 2 * S.DLNY}
    assert sum(np.count_nonzero(n[c]) for c in WINDOW_CLASSES) == mu.size
    return {c: int(np.count_nonzero(v)) for c, v in n.items()}


def ulp_apart(a, b):
    """Where two float32 arrays of finite numbers of one sign are neighbouring floats."""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(ia - ib) == 1


def analytic_sigma(R):
    """sigma(R) of tools/sz_ref_harness.f90 (R in Mpc / h)."""
    R = np.asarray(R, dtype=np.float64)
    return 0.8 * (R / 8.0) ** (-0.55) * np.exp(-(R - 8.0) / 60.0)


def sigma_table():
    n, lo, hi = SIGMA_GRID
    R = np.array([np.exp(lo + (hi - lo) * i / (n - 1)) for i in range(n)])
    return R, analytic_sigma(R)


def nuisance_points(kind):
    """The points of a golden.  "all": the centre of SZ_plus_CMB.ini, the corners
    of its ranges of alpha_SZ, bias_SZ and scatter_SZ (the least scatter is
    narrower than the ln Y step, so the trapezoid overshoots and completeness
    clips at fsky), scatter_SZ = 0 with beta_SZ at and away from 2/3, and
    beta_SZ != 2/3 with scatter."""
    c = np.array(CENTRE)
    if kind == "prior":
        return np.array([c, [2.1, -0.15, 0.688, 0.09, 0.4]])
    if kind == "few":
        return np.array([c, [1.5, -0.2, 1.0, 0.1, 0.5], [1.789, -0.186, 0.8, 0.0, 2.0 / 3.0]])
    pts = [c.copy()]
    for a in (1.0, 3.0):
        for b in (0.1, 1.3):
            for s in (0.022, 0.122):
                pts.append([a, -0.186, b, s, 2.0 / 3.0])
    pts.append([1.789, -0.186, 0.8, 0.0, 2.0 / 3.0])
    pts.append([1.6, -0.25, 0.7, 0.0, 0.3])
    pts.append([1.789, -0.1, 0.8, 0.075, 0.3])
    pts.append([2.2, -0.29, 0.6, 0.05, 1.0])
    return np.array(pts)


def catalogue(rng, kind):
    """Rows (z, z error, S/N).  Every kind has rows below S/N 6, a (z, q) bin
    with more than 10 clusters and bins with none; "edges" adds clusters without
    a redshift (z = -1) in an inner S/N bin and in the open one, and rows on
    the z and S/N bin edges; "lastrow" ends with a row above the threshold."""
    rows = []
    for _ in range(14):                                  # > 10 in (z bin 2, q bin 1)
        rows.append((rng.uniform(0.105, 0.195), 0.0, rng.uniform(6.05, 8.5)))
    for _ in range(40):
        z = rng.beta(1.6, 4.0) * 0.98
        rows.append((z, 0.0, 6.0 * 10 ** rng.exponential(0.22)))
    for _ in range(8):                                   # below the threshold
        rows.append((rng.uniform(0.02, 0.9), 0.0, rng.uniform(4.5, 5.99)))
    rows = [r for r in rows if not (0.8 <= r[0] < 0.9)]  # an empty z bin
    if kind == "edges":
        rows += [(-1.0, 0.0, 7.2), (-1.0, 0.0, 6.4), (-1.0, 0.0, 12.0), (-1.0, 0.0, 45.0), (-1.0, 0.0, 80.0),
                 (-1.0, 0.0, 5.0), (0.3, 0.0, 6.0), (0.5, 0.0, 33.0), (0.0, 0.0, 9.0), (0.95, 0.0, 150.0)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rows.append((0.42, 0.0, 7.7) if kind == "lastrow" else (0.42, 0.0, 5.5))
    return rows


def write_ini(path, priors=(), extra=""):
    with open(path, "w") as f:
        f.write("cat_file = data/SZ_cat.txt\nthetas_file = data/SZ_thetas.txt\nskyfracs_file = data/SZ_skyfracs.txt\n"
                "ylims_file = data/SZ_ylims.txt\nnuisance_params = data/SZ.paramnames\n2D = T\n")
        f.write("".join("%s = T\n" % p for p in priors) + extra)


def write_cases(d, pts):
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write(" ".join("%.17g" % x for x in COSMO) + "\n")
        f.write("%d %.17g %.17g\n" % SIGMA_GRID)
        f.write("%d\n" % len(pts))
        f.write("".join(" ".join("%.17g" % x for x in p) + "\n" for p in pts))


def make_synthetic(d, seed, npatch, ntheta, theta, cat="plain", priors=(), points="all", order=None):
    """Write a dataset under d: data/SZ_*.txt and data/SZ.paramnames as the
    reference opens them, the project's sz.ini, the reference's run ini
    sz_ref.ini, and cases.txt; returns the nuisance points.  ``order``: the
    positions of the ascending thetas in file order (default: ascending); the
    rows of ylims follow their thetas."""
    rng = np.random.RandomState(seed)
    dd = os.path.join(d, "data")
    os.makedirs(dd, exist_ok=True)
    th = np.exp(np.linspace(np.log(theta[0]), np.log(theta[1]), ntheta))
    order = list(range(ntheta)) if order is None else list(order)
    assert sorted(order) == list(range(ntheta))
    with open(os.path.join(dd, "SZ_thetas.txt"), "w") as f:
        f.write("".join("%.6e\n" % th[k] for k in order))
    sky = rng.uniform(0.5, 1.5, npatch)
    sky = 0.65 * sky / sky.sum()
    with open(os.path.join(dd, "SZ_skyfracs.txt"), "w") as f:
        f.write("".join("%.6e\n" % s for s in sky))
    yl = [["%.5e\n" % (6e-5 * (1 + 0.5 * i / npatch) * (1 + 0.1 * rng.uniform()) * (1 + t) ** 0.7) for i in range(npatch)]
          for t in th]                                               # drawn in ascending order of theta
    with open(os.path.join(dd, "SZ_ylims.txt"), "w") as f:        # patch fastest
        f.write("".join("".join(yl[k]) for k in order))
    with open(os.path.join(dd, "SZ_cat.txt"), "w") as f:
        f.write("".join("%12.6f %12.5f %12.5f\n" % r for r in catalogue(rng, cat)))
    with open(os.path.join(dd, "SZ.paramnames"), "w") as f:
        f.write("".join("%s  %s\n" % (n, n) for n in PARAM_NAMES))
    write_ini(os.path.join(d, "sz.ini"), priors)
    with open(os.path.join(d, "sz_ref.ini"), "w") as f:
        f.write("action = 0\nuse_SZ = T\n2D = T\n" + "".join("%s = T\n" % p for p in priors))
    pts = nuisance_points(points)
    write_cases(d, pts)
    return pts


class Golden:
    """One golden dataset: its ini, the cosmology, the nuisance points, the
    harness's theory row, the reference's -lnL, and the loader quantities the
    harness prints (sizes, steps_z, DNcat)."""

    def __init__(self, d, row=None):
        self.dir, self.ini = d, os.path.join(d, "sz.ini")
        lines = open(os.path.join(d, "cases.txt")).read().split("\n")
        self.cosmo = tuple(float(x) for x in lines[0].split())
        nc = int(lines[2])
        self.points = np.array([lines[3 + i].split() for i in range(nc)], dtype=np.float64)
        self.ref = np.array(open(os.path.join(d, "ref.txt")).read().split(), dtype=np.float64)
        assert len(self.ref) == nc and self.points.shape == (nc, 5)
        self.row = row
        t = open(os.path.join(d, "info.txt")).read().split()
        self.nzs, self.nm, self.nz, self.nq = (int(x) for x in t[:4])
        self.steps_z = np.array(t[4:4 + self.nzs], dtype=np.float64)
        self.DNcat = np.array(t[4 + self.nzs:], dtype=np.float64).reshape(self.nz, self.nq)
        self.priors = [ln.split()[0] for ln in open(self.ini) if ln.startswith("prior_")]


def watson_sample(tmpdir):
    """Every WATSON_STRIDE-th number of the row the reference forms with use_watson = T (after extract)."""
    return np.array(open(os.path.join(str(tmpdir), "sz", "watson", "row_sample.txt")).read().split(), dtype=np.float64)


def extract(tmpdir, archive=GOLDEN, names=None):
    """{name: Golden} with the archive extracted under tmpdir.  Every golden has
    the same cosmology and so the same theory row, kept once as sz/row.txt."""
    with open(archive, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    base = os.path.join(str(tmpdir), "sz")
    row = np.array(open(os.path.join(base, "row.txt")).read().split(), dtype=np.float64)
    if names is None:
        names = NAMES
    return {n: Golden(os.path.join(base, n), row) for n in names}
