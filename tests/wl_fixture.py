"""Shared by the weak-lensing tests: the goldens of the compiled reference
(tests/golden/wl/wl_fixture.tar.xz: inputs from tools/wl_make_fixture.py, which
calls make_synthetic below; outputs from tools/wl_ref_harness.f90) and the
in-test synthetic datasets of test_gpu_wl_edges.py.

A synthetic dataset is seeded: Gaussian-bump n(z) on a uniform z grid, log
spaced theta bins, a flat LCDM table of chi(z) and H(z), the harness's analytic
P(kh, z) (analytic_lnpk restates it), a data vector equal to the model at a
fiducial point times (1 + 5 % noise), and a covariance D (I/2 + A A^T / 2m) D
with D 15 % of the data: condition number of order 10, so -lnL of order the
number of points carries the rounding of its inputs and little more."""
import io
import lzma
import os
import tarfile

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "the long-double reference needs x87 extended precision"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wl", "wl_fixture.tar.xz")
TYPES = ("xip", "xim", "gammat", "wtheta")
H0, OMM = 70.0, 0.3
PK_GRID = (60, 12, float(np.log(2e-3)), float(np.log(10.0)))      # nk, nz, ln kh range of the harness's grid

#            name            keyword arguments of make_synthetic
GOLDENS = [("syn_all", dict(seed=101)),
           ("syn_lens_weyl", dict(seed=102, used="xip xim", weyl=True)),
           ("syn_gg", dict(seed=103, used="gammat wtheta")),
           ("syn_noxim", dict(seed=104, data_types="xip gammat wtheta", ia="none")),
           ("syn_nogal", dict(seed=105, ngal=0, data_types="xip xim")),
           ("syn_acc", dict(seed=106, acc=2)),
           ("syn_cut", dict(seed=107, select="cut"))]
NAMES = [n for n, _ in GOLDENS]


def analytic_lnpk(which, lk, z):
    """ln P(ln kh, z) of tools/wl_ref_harness.f90: which = 1 MPK, 2 NL_MPK, 3 MPK_WEYL, 4 NL_MPK_WEYL."""
    k = np.exp(lk)
    v = 10.0 + lk - 1.5 * np.log(1 + (k / 0.02) ** 2) - 2 * np.log(1 + 0.6 * z)
    if which in (2, 4):
        v = v + 0.5 * np.log(1 + (k / 0.3) ** 2) / (1 + z)
    if which >= 3:
        v = v - 16.0 + 0.3 * z
    return v


def pk_which(weyl, nonlinear=True):
    return (4 if nonlinear else 3) if weyl else (2 if nonlinear else 1)


def cosmology(z):
    """(chi [Mpc], H / c [1 / Mpc], D_growth) of flat LCDM (H0, OMM) at the redshifts z; D as the harness forms it."""
    c = 299792.458

    def E(x):
        return np.sqrt(OMM * (1 + x) ** 3 + 1 - OMM)
    chis = np.empty(len(z))
    for i, zi in enumerate(z):
        x = np.linspace(0.0, zi, 257)
        y = 1 / E(x)
        chis[i] = c / H0 * (x[1] - x[0]) * (y.sum() - 0.5 * (y[0] + y[-1]))
    lk = np.log(0.01)
    D = np.sqrt(np.exp(analytic_lnpk(1, lk, z)) / np.exp(analytic_lnpk(1, lk, 0.0)))
    return chis, H0 * E(z) / c, D


def pairs_of(nsrc, ngal, drop_gammat=0):
    """The bin pairs of each measurement file, in file order."""
    g = [(a, b) for a in range(1, ngal + 1) for b in range(1, nsrc + 1)]
    lens = [(a, b) for a in range(1, nsrc + 1) for b in range(a, nsrc + 1)]
    return dict(xip=lens, xim=lens, gammat=g[:len(g) - drop_gammat], wtheta=[(a, a) for a in range(1, ngal + 1)])


def param_names(nsrc, ngal):
    return ["WL_b%d" % i for i in range(1, ngal + 1)] + ["WL_m%d" % i for i in range(1, nsrc + 1)] \
        + ["WL_AIA", "WL_alphaIA", "WL_z0AI"] + ["WL_DzL%d" % i for i in range(1, ngal + 1)] \
        + ["WL_DzS%d" % i for i in range(1, nsrc + 1)]


def fiducial(nsrc, ngal):
    return np.concatenate([1.2 + 0.2 * np.arange(ngal), 0.01 * (1 + np.arange(nsrc)), [0.5, 0.3, 0.62],
                           np.zeros(ngal + nsrc)])


def nuisance_points(nsrc, ngal, dz, seed):
    """The points of a golden: all shifts zero; every shift one knot spacing;
    shifts that leave the table at both ends; A_IA = 0; negative alphaIA and
    negative m; a generic one."""
    rng = np.random.RandomState(seed + 7)
    f = fiducial(nsrc, ngal)
    s0 = ngal + nsrc + 3
    pts = [f.copy() for _ in range(6)]
    pts[1][s0:] = dz
    pts[2][s0:] = np.where(np.arange(ngal + nsrc) % 2 == 0, 0.9, -0.9)
    pts[3][ngal + nsrc] = 0.0
    pts[3][s0:] = 0.01 * rng.standard_normal(ngal + nsrc)
    pts[4][ngal + nsrc + 1] = -1.2
    pts[4][ngal:ngal + nsrc] = -0.02
    pts[4][s0:] = 0.02 * rng.standard_normal(ngal + nsrc)
    pts[5] = f * (1 + 0.05 * rng.standard_normal(len(f)))
    pts[5][s0:] = 0.015 * rng.standard_normal(ngal + nsrc)
    return np.array(pts)


def _write_measurements(d, pr, types, ntheta, values):
    for t in types:
        with open(os.path.join(d, t + ".dat"), "w") as f:
            f.write("# BIN1 BIN2 ANGBIN VALUE\n")
            for a, b in pr[t]:
                for k in range(1, ntheta + 1):
                    f.write("%d %d %d %.8e\n" % (a, b, k, values[t, a, b, k]))


def make_synthetic(d, seed, nsrc=3, ngal=2, ntheta=7, nrows=29, lmax=3000, acc=None, data_types="xip xim gammat wtheta",
                   used=None, ia=None, weyl=False, select="drop2", drop_gammat=0, cov_fmt="%.6g", cov_scale=1.0):
    """Write a dataset under d (wl.dataset, the reference's main ini wl.ini and
    the data files); returns a dict with its paths, the host dataset, the theory
    row of the fiducial cosmology and the nuisance points.

    select: "drop2" drops the first two theta bins of every pair; "all" keeps
    everything; "one" keeps theta bin 3 alone; "last" the last theta bin alone;
    "cut" gives the first xip pair a range that holds no theta bin and leaves
    the last pair of the last used type without a row (the default -1 range
    rejects it), the rest as drop2."""
    from cosmomc_amd import weaklensing as wl
    rng = np.random.RandomState(seed)
    os.makedirs(d, exist_ok=True)
    types = data_types.split()
    used_types = (used or data_types).split()
    pr = pairs_of(nsrc, ngal, drop_gammat)
    dz = 1.45 / nrows
    zm = 0.05 + dz * np.arange(nrows)
    for fname, nb in (("nz_source.dat", nsrc), ("nz_lens.dat", ngal)):
        if nb == 0:
            continue
        mu = np.linspace(0.35, 1.0, nb) if fname == "nz_source.dat" else np.linspace(0.2, 0.7, nb)
        sg = 0.18 if fname == "nz_source.dat" else 0.08
        with open(os.path.join(d, fname), "w") as f:
            f.write("# Z_LOW Z_MID Z_HIGH BINS\n")
            for z in zm:
                n = np.exp(-0.5 * ((z - mu) / sg) ** 2) / (sg * np.sqrt(2 * np.pi)) * (1 + 0.05 * rng.standard_normal(nb))
                f.write("%.6e %.6e %.6e " % (z - dz / 2, z, z + dz / 2) + " ".join("%.6e" % x for x in n) + "\n")
    theta = np.exp(np.linspace(np.log(3.0), np.log(200.0), ntheta))
    with open(os.path.join(d, "theta.dat"), "w") as f:
        f.write("# theta_arcmin\n" + "".join("%.12e\n" % t for t in theta))
    names = param_names(nsrc, ngal)
    with open(os.path.join(d, "wl.paramnames"), "w") as f:
        f.write("".join("%s  %s\n" % (n, n) for n in names))
    with open(os.path.join(d, "wl.dataset"), "w") as f:
        f.write("measurements_format = DES\nkmax = 10\nnum_z_bins = %d\nnum_theta_bins = %d\n" % (nsrc, ntheta))
        if ngal:
            f.write("num_gal_bins = %d\nnz_gal_file = nz_lens.dat\n" % ngal)
        f.write("data_types = %s\n" % data_types)
        if used:
            f.write("used_data_types = %s\n" % used)
        if ia:
            f.write("intrinsic_alignment_model = %s\n" % ia)
        if acc:
            f.write("acc = %r\n" % acc)
        f.write("lmax = %d\ntheta_bins_file = theta.dat\ncov_file = cov.dat\nnz_file = nz_source.dat\n" % lmax)
        f.write("data_selection = selection.dat\nnuisance_params = wl.paramnames\n")
        f.write("".join("measurements[%s] = %s.dat\n" % (t, t) for t in types))
    with open(os.path.join(d, "wl.ini"), "w") as f:
        f.write("use_WL = T\nwl_use_weyl = %s\nwl_dataset[WL] = wl.dataset\nwl_dataset_speed[WL] = 8\n"
                % ("T" if weyl else "F"))

    def write_selection(rows):
        with open(os.path.join(d, "selection.dat"), "w") as f:
            f.write("#  type bin1 bin2 theta_min theta_max\n")
            f.write("".join("%s %d %d %.6f %.6f\n" % r for r in rows))
    # pass 1: zero data, unit covariance, everything of the used types selected: the model at the fiducial point
    N = sum(len(pr[t]) for t in types) * ntheta
    zero = {(t, a, b, k): 0.0 for t in types for a, b in pr[t] for k in range(1, ntheta + 1)}
    _write_measurements(d, pr, types, ntheta, zero)
    write_selection([(t, a, b, 0.0, 1e4) for t in types for a, b in pr[t]])
    with open(os.path.join(d, "cov.dat"), "w") as f:
        f.write("\n".join(" ".join("1" if i == j else "0" for j in range(N)) for i in range(N)) + "\n")
    path = os.path.join(d, "wl.dataset")
    ds = wl.WLDataset(path, use_weyl=weyl)
    chis, Hs, Dg = cosmology(ds.z_p)
    which = pk_which(weyl)
    row = wl.wl_theory_row(ds, H0 / 100, OMM, chis, Hs, Dg, lambda kh, z: np.exp(analytic_lnpk(which, np.log(kh), z)),
                           np.exp(PK_GRID[2]), np.exp(PK_GRID[3]))
    fid = fiducial(nsrc, ngal)
    model = wl.wl_theory_vector(ds, row, fid)
    values = {key: 1e-6 * (1 + rng.uniform()) for key in zero}        # entries of unused types never enter
    for (ti, a, b, k), v in zip(ds.used_items, model):
        values[types[ti - 1], a, b, k] = v * (1 + 0.05 * rng.standard_normal())
    _write_measurements(d, pr, types, ntheta, values)
    # pass 2: the selection and the covariance
    lo2 = 0.5 * (theta[1] + theta[2])
    rows = [(t, a, b, lo2, 250.0) for t in types for a, b in pr[t]]
    if select == "all":
        rows = [(t, a, b, 0.0, 1e4) for t, a, b, _, _ in rows]
    elif select == "one":
        rows = [(t, a, b, 0.99 * theta[2], 1.01 * theta[2]) for t, a, b, _, _ in rows]
    elif select == "last":
        rows = [(t, a, b, 0.99 * theta[-1], 1e4) for t, a, b, _, _ in rows]
    elif select == "cut":
        rows[0] = rows[0][:3] + (0.6 * theta[2] + 0.4 * theta[3], 0.5 * (theta[2] + theta[3]))
        last = max(i for i, r in enumerate(rows) if r[0] in used_types)
        del rows[last]
    write_selection(rows)
    order = [values[t, a, b, k] for t in types for a, b in pr[t] for k in range(1, ntheta + 1)]
    sig = 0.15 * np.abs(np.array(order)) * np.sqrt(cov_scale)
    A = rng.standard_normal((N, 2 * N))
    cov = (0.5 * np.eye(N) + 0.5 * (A @ A.T) / (2 * N)) * sig[:, None] * sig[None, :]
    with open(os.path.join(d, "cov.dat"), "w") as f:
        f.write("\n".join(" ".join(cov_fmt % x for x in r) for r in cov) + "\n")
    ds = wl.WLDataset(path, use_weyl=weyl)
    pts = nuisance_points(nsrc, ngal, float(ds.z_p[1] - ds.z_p[0]), seed)
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("%.17g %.17g 0\n" % (H0, OMM))
        f.write("%d %d %.17g %.17g %.17g\n" % (PK_GRID + (float(ds.z_p[-1]) + 0.1,)))
        f.write("%d\n" % ds.nz)
        f.write(" ".join("%.17g" % x for x in chis) + "\n" + " ".join("%.17g" % x for x in Hs) + "\n")
        f.write("%d\n" % ds.nl + " ".join("%d" % x for x in ds.ls_cl) + "\n")
        f.write("%d %d\n" % pts.shape)
        f.write("".join(" ".join("%.17g" % x for x in p) + "\n" for p in pts))
    return dict(dataset=path, ini=os.path.join(d, "wl.ini"), ds=ds, row=row, points=pts, weyl=weyl)


class Golden:
    """One golden dataset: its paths, the nuisance points, the harness's theory
    row, the reference's -lnL, and the loader quantities the reference exposes
    (used_items, first_theta_bin_used; its ls_cl and ls_bessel are private)."""

    def __init__(self, d, weyl):
        self.dir, self.weyl = d, weyl
        self.dataset, self.ini = os.path.join(d, "wl.dataset"), os.path.join(d, "wl.ini")
        lines = open(os.path.join(d, "cases.txt")).read().split("\n")
        self.h0, self.omdm = (float(x) for x in lines[0].split()[:2])
        self.zg_max = float(lines[1].split()[4])
        self.chis = np.array(lines[3].split(), dtype=np.float64)
        self.Hs = np.array(lines[4].split(), dtype=np.float64)
        self.ls_row = np.array(lines[6].split(), dtype=int)        # the l at which the harness formed the row's P
        nc, nn = (int(x) for x in lines[7].split())
        self.points = np.array([lines[8 + i].split() for i in range(nc)], dtype=np.float64)
        assert self.points.shape == (nc, nn)
        self.ref = np.array(open(os.path.join(d, "ref.txt")).read().split(), dtype=np.float64)
        assert len(self.ref) == nc
        r = np.array(open(os.path.join(d, "row.txt")).read().split(), dtype=np.float64)
        nz = len(self.chis)
        self.kh_min, self.kh_max = r[2 + 3 * nz], r[3 + 3 * nz]
        self.row = np.concatenate([r[:2 + 3 * nz], r[4 + 3 * nz:]])
        t = open(os.path.join(d, "info.txt")).read().split()
        self.first_theta_bin_used, nu = int(t[0]), int(t[1])
        self.used_items = [tuple(int(x) for x in t[2 + 4 * i:6 + 4 * i]) for i in range(nu)]


def extract(tmpdir, archive=GOLDEN, names=NAMES):
    """{name: Golden} with the archive extracted under tmpdir."""
    with open(archive, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    kw = dict(GOLDENS)
    return {n: Golden(os.path.join(str(tmpdir), "wl", n), kw[n].get("weyl", False)) for n in names}
