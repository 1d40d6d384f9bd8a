"""Shared by the galaxy power-spectrum tests (tags MPK and WIGGLEZ): the goldens
of the compiled reference (tests/golden/mpk/mpk_fixture.tar.xz: inputs from
tools/mpk_make_fixture.py, which calls the makers below and copies the real
sdss_lrgDR4*, wigglez_nov11* and gigglezfiducialmodel_matterpower_* data
files; outputs from tools/mpk_ref_harness.f90), the analytic P(k, z) of the
harness, and seeded synthetic data sets of any shape for the edge tests.

A golden's directory holds ref.ini (the reference's run ini: use_mpk or
use_wigglez_mpk and the dataset names), the .dataset files, their data files
under data/, cases.txt, and the harness's ref.txt, row.txt and info.txt."""
import io
import lzma
import os
import tarfile

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "the long-double reference needs x87 extended precision"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpk", "mpk_fixture.tar.xz")
GRID = (160, 5, float(np.log(2.0)))          # nk, nz, ln kh_max of the harness's (ln kh, z) grid
LKMIN = float(np.log(1e-4))
H0 = 70.0
ZBINS = (0.22, 0.41, 0.6, 0.78)
# The GPU tests' absolute bound on -lnL per tag: 10 x the larger of (a) the numpy restatement in f64 against the
# goldens and (b) f64 against long double (test_mpk.py measures both and asserts this is that rule):
# MPK (a) 1.2e-12 (b) 2.7e-12; WIGGLEZ (a) 5.5e-12 (b) 7.3e-11
GPU_ATOL = {"MPK": 2.7e-11, "WIGGLEZ": 7.3e-10}
REGION_KEYS = ["Use_9-hr_region", "Use_11-hr_region", "Use_15-hr_region", "Use_22-hr_region", "Use_1-hr_region",
               "Use_3-hr_region", "Use_0-hr_region"]          # in the reference's key order (wigglez.f90:234-251)
GIGGLEZ = ["gigglezfiducialmodel_matterpower_%s.dat" % c for c in "abcd"]

# (a_scl, amp, tilt, ln kh_min) of a golden's cases; the last two put the grid's lower edge above a_scl k_1
CASES = [(1.0, 14.5, 1.0, LKMIN), (0.85, 14.3, 0.92, LKMIN), (1.15, 14.9, 1.05, LKMIN), (0.93, 14.7, 0.97, LKMIN),
         (1.08, 14.4, 1.02, LKMIN), (1.02, 14.6, 0.9, float(np.log(0.012))), (0.9, 14.8, 1.0, float(np.log(0.03)))]

REAL = ["lrg_dr4", "wigglez_a", "wigglez_b", "wigglez_c", "wigglez_d"]
#               name            maker      keyword arguments
SYNTHETIC = [("mpk_cov_flat", "mpk", dict(seed=11, npf=9, nkf=21, cov=True, q="flat")),
             ("mpk_grid", "mpk", dict(seed=12, npf=17, nkf=30, cov=False, q="gauss")),
             ("mpk_grid_cov", "mpk", dict(seed=13, npf=17, nkf=30, cov=True, q="gauss")),
             ("mpk_qsigma0", "mpk", dict(seed=14, npf=8, nkf=19, cov=False, q="sigma0")),
             ("mpk_qsigma0_cov", "mpk", dict(seed=15, npf=8, nkf=19, cov=True, q="sigma0")),
             ("mpk_nomarge", "mpk", dict(seed=16, npf=12, nkf=25, cov=False, q="none")),
             ("mpk_noscale", "mpk", dict(seed=17, npf=12, nkf=25, cov=True, q="none", use_scaling=False, nonlinear=False)),
             ("mpk_select", "mpk", dict(seed=18, npf=24, nkf=40, cov=True, q="flat", sel=(4, 20, 3, 36))),
             ("wz_flat_r25", "wigglez", dict(seed=21, nkf=30, q="flat", regions=(2, 5), z=0.41, sel=(3, 20, 1, 30))),
             ("wz_grid", "wigglez", dict(seed=22, nkf=26, q="gauss", regions=(1, 2, 3, 4, 5, 6, 7), z=0.6,
                                         sel=(2, 18, 2, 25))),
             ("wz_linear", "wigglez", dict(seed=23, nkf=30, q="none", regions=(1, 3, 6), z=0.22, sel=(3, 20, 1, 30),
                                           gigglez=False, nonlinear=False)),
             ("wz_region7", "wigglez", dict(seed=24, nkf=24, q="none", regions=(7,), z=0.78, sel=(1, 16, 1, 24)))]
NAMES = REAL + [n for n, _, _ in SYNTHETIC]


def analytic_lnp(lk, z, amp, tilt, nonlinear):
    """mpk_harness_pk of tools/mpk_ref_harness.f90: ln P(ln kh, z)."""
    lk = np.asarray(lk, dtype=np.float64)
    k = np.exp(lk)
    v = amp + tilt * lk - 1.5 * np.log(1 + (k / 0.02) ** 2) - 2 * np.log(1 + 0.6 * z)
    if nonlinear:
        v = v + 0.5 * np.log(1 + (k / 0.3) ** 2) / (1 + z)
    return v


def analytic_pk(z, amp, tilt, nonlinear):
    """k -> P(k, z): what the harness's grid interpolates (not its interpolant)."""
    return lambda k: np.exp(analytic_lnp(np.log(np.asarray(k, dtype=np.float64)), z, amp, tilt, nonlinear))


def grid_kh_min(lkmin):
    """exp(PK%x(1)) of the harness's grid."""
    return float(np.exp(np.float64(lkmin)))


# ---------------------------------------------------------------- synthetic data sets

def _windows(rng, npf, kfull):
    lk = np.log(kfull)
    cen = np.linspace(lk[0] + 0.15 * (lk[-1] - lk[0]), lk[-1] - 0.1 * (lk[-1] - lk[0]), npf) if npf > 1 else \
        np.array([0.5 * (lk[0] + lk[-1])])
    wid = 0.12 * (lk[-1] - lk[0]) + 0.05
    W = np.exp(-0.5 * ((lk[None, :] - cen[:, None]) / wid) ** 2) * (1 + 0.2 * rng.standard_normal((npf, len(kfull))))
    W = W - 0.02 * np.abs(W).max(axis=1, keepdims=True) * rng.uniform(0, 1, W.shape)
    return W / np.abs(W.sum(axis=1, keepdims=True)), np.exp(cen)


def _obs(rng, W, kfull, z, nonlinear):
    model = W @ analytic_pk(z, 14.5, 0.98, nonlinear)(kfull) * 1.7
    sdev = np.abs(model) * rng.uniform(0.04, 0.1, len(model))
    return model + sdev * rng.standard_normal(len(model)), sdev


def _cov(rng, sdev):
    n = len(sdev)
    i = np.arange(n)
    R = 0.75 * np.eye(n) + 0.25 * np.exp(-np.abs(i[:, None] - i[None, :]) / 2.0)
    return sdev[:, None] * R * sdev[None, :]


def _matrix_text(M, fmt="%.9e"):
    return "".join(" ".join(fmt % x for x in row) + "\n" for row in M)


def _q_lines(q):
    return {"flat": "Q_marge = T\nQ_flat = T\nAg = 1.4\n", "gauss": "Q_marge = T\nQ_flat = F\nQ_mid = 4.0\nQ_sigma = 1.5\nAg = 1.3\n",
            "sigma0": "Q_marge = T\nQ_flat = F\nQ_mid = 3.1\nQ_sigma = 0\n", "none": "Q_marge = F\n"}[q]


def make_mpk(d, seed, npf, nkf, cov, q, use_scaling=True, nonlinear=True, sel=None, z=0.35, name=None, cases=CASES):
    """An mpk.f90 data set under d: syn.dataset, data/syn_{kbands,measurements,windows,cov}.txt, ref.ini, cases.txt."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    kfull = np.exp(np.linspace(np.log(2e-3), np.log(0.6), nkf)) if nkf > 1 else np.array([0.05])
    W, keff = _windows(rng, npf, kfull)
    obs, sdev = _obs(rng, W, kfull, z, nonlinear)
    with open(os.path.join(d, "data", "syn_kbands.txt"), "w") as f:
        f.write("".join("%.8e\n" % k for k in kfull))
    with open(os.path.join(d, "data", "syn_measurements.txt"), "w") as f:
        f.write("# keff klo khi obs sdev b_dummy\n#\n")
        f.write("".join("%.6e %.6e %.6e %.8e %.8e 1.\n" % (k, 0.9 * k, 1.1 * k, o, s) for k, o, s in zip(keff, obs, sdev)))
    with open(os.path.join(d, "data", "syn_windows.txt"), "w") as f:
        f.write(_matrix_text(W))
    if cov:
        with open(os.path.join(d, "data", "syn_cov.txt"), "w") as f:
            f.write(_matrix_text(_cov(rng, sdev)))
    DV_fid = 94874.8118745411
    with open(os.path.join(d, "syn.dataset"), "w") as f:
        f.write("name = %s\nnum_mpk_points_full = %d\nnum_mpk_kbands_full = %d\n" % (name or os.path.basename(d), npf, nkf))
        if sel:
            f.write("min_mpk_points_use = %d\nmax_mpk_points_use = %d\nmin_mpk_kbands_use = %d\nmax_mpk_kbands_use = %d\n" % sel)
        f.write(_q_lines(q))
        f.write("use_scaling = %s\n" % ("T" if use_scaling else "F"))
        if use_scaling:
            f.write("DV_fid = %.13f\n" % DV_fid)
        f.write("redshift = %s\n" % repr(z))
        f.write("windows_file = %DATASETDIR%syn_windows.txt\nkbands_file = %DATASETDIR%syn_kbands.txt\n"
                "measurements_file = %DATASETDIR%syn_measurements.txt\n")
        if cov:
            f.write("cov_file = %DATASETDIR%syn_cov.txt\n")
    with open(os.path.join(d, "ref.ini"), "w") as f:
        f.write("action = 0\nuse_mpk = T\nmpk_numdatasets = 1\nmpk_dataset1 = syn.dataset\nmpk_dataset_nonlinear1 = %s\n"
                % ("T" if nonlinear else "F"))
    write_cases(d, DV_fid, use_scaling, os.path.join(d, "data", "syn_kbands.txt"), sel[2] if sel else 1,
                sel[3] if sel else nkf, cases)
    return os.path.join(d, "syn.dataset")


def make_wigglez(d, seed, nkf, q, regions, z, sel, gigglez=True, nonlinear=True, use_scaling=True, gigglez_src=None,
                 cases=CASES):
    """A wigglez.f90 redshift bin under d: common.dataset, wz.dataset and the region-blocked data files (50 points
    a region, as the reference's skip of a switched-off region requires), ref.ini, cases.txt.  With gigglez the four
    fiducial files are copied from gigglez_src into d/data."""
    rng = np.random.RandomState(seed)
    npf = 50
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    kfull = 0.005 + 0.02 * np.arange(nkf)
    with open(os.path.join(d, "data", "wz_kbands.txt"), "w") as f:
        f.write("".join("%.4f\n" % k for k in kfull))
    fm = open(os.path.join(d, "data", "wz_measurements.txt"), "w")
    fw = open(os.path.join(d, "data", "wz_windows.txt"), "w")
    fc = open(os.path.join(d, "data", "wz_cov.txt"), "w")
    used = np.zeros(npf, dtype=bool)
    used[sel[0] - 1:sel[1]] = True
    for r in range(7):
        W, keff = _windows(rng, npf, kfull)
        obs, sdev = _obs(rng, W, kfull, z, nonlinear)
        cv = _cov(rng, sdev)
        # what no loader may use (a switched-off region, the points outside the selection) is constant, so that
        # the archive stays small; it differs from region to region, so that a loader which uses it shows
        keep = used if r + 1 in regions else np.zeros(npf, dtype=bool)
        W[~keep], obs[~keep] = 0.01 * (r + 1), 1000.0 * (r + 1)
        cv[~keep, :] = 0.0
        cv[:, ~keep] = 0.0
        cv[~keep, ~keep] = 1e6 * (r + 1)
        fm.write("# region %d\n# k, klo, khi, P(k), -1.0, -1.0\n" % (r + 1))
        fm.write("".join("%.4f %.4f %.4f %.6e -1.0 -1.0\n" % (k, 0.9 * k, 1.1 * k, o) for k, o in zip(keff, obs)))
        fw.write("# windows of region %d\n" % (r + 1) + _matrix_text(W, "%.6e"))
        fc.write("# covariance of region %d\n" % (r + 1) + _matrix_text(cv, "%.7e"))
    fm.close(), fw.close(), fc.close()
    DV_fid = 61461.2751075690 * (1 + z)
    with open(os.path.join(d, "common.dataset"), "w") as f:
        f.write("name = WiggleZ_syn\nnum_mpk_points_full = %d\nnum_mpk_kbands_full = %d\n" % (npf, nkf))
        f.write("num_conflicts = 1\ntype_conflict1 = BAO\nname_conflict1 = WiggleZ\n")
        f.write("use_scaling = %s\n" % ("T" if use_scaling else "F"))
        f.write("min_mpk_points_use = %d\nmax_mpk_points_use = %d\nmin_mpk_kbands_use = %d\nmax_mpk_kbands_use = %d\n" % sel)
        f.write(_q_lines(q))
        f.write("".join("%s = %s\n" % (key, "T" if i + 1 in regions else "F") for i, key in enumerate(REGION_KEYS)))
    with open(os.path.join(d, "wz.dataset"), "w") as f:
        f.write("name = %s\nredshift = %s\nDV_fid = %.10f\n" % (os.path.basename(d), repr(z), DV_fid))
        f.write("windows_file = data/wz_windows.txt\nkbands_file = data/wz_kbands.txt\n"
                "measurements_file = data/wz_measurements.txt\ncov_file = data/wz_cov.txt\n")
    with open(os.path.join(d, "ref.ini"), "w") as f:
        f.write("action = 0\nuse_wigglez_mpk = T\nnonlinear_wigglez = %s\nUse_gigglez = %s\n"
                "wigglez_common_dataset = common.dataset\nmpk_wigglez_numdatasets = 1\nwigglez_dataset1 = wz.dataset\n"
                % ("T" if nonlinear else "F", "T" if gigglez else "F"))
    if gigglez and gigglez_src:
        import shutil
        for g in GIGGLEZ:
            shutil.copy(os.path.join(gigglez_src, g), os.path.join(d, "data", g))
    write_cases(d, DV_fid, use_scaling, os.path.join(d, "data", "wz_kbands.txt"), sel[2], sel[3], cases)
    return os.path.join(d, "wz.dataset")


def write_cases(d, DV_fid, use_scaling, kfile, kmin, kmax, cases=CASES):
    """cases.txt of tools/mpk_ref_harness.f90; the k are rows kmin .. kmax (1-based) of the kbands file."""
    k = [float(ln.split()[0].replace("D", "e")) for ln in open(kfile) if ln.strip()][kmin - 1:kmax]
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("%d %d %.17g %d\n%d\n" % (GRID[0], GRID[1], GRID[2], 1 if use_scaling else 0, len(k)))
        f.write("".join("%.17g\n" % x for x in k))
        f.write("%d\n" % len(cases))
        for a, amp, tilt, lkmin in cases:
            f.write("%.17g %.17g %.17g %.17g %.17g\n" % (H0, DV_fid / (H0 * a), amp, tilt, lkmin))


# ---------------------------------------------------------------- goldens

class Golden:
    """One golden: ``ini`` (the run ini; cosmomc_amd.mpk's *_likelihood_add and
    datasets_from_ini take it), the cases (H0, DV, amp, tilt, lkmin), the
    harness's rows [ncase][2 + nk], the reference's -lnL, and the loader
    quantities the harness prints (MPK: k, P, sdev, invcov; WiggleZ, whose type the
    reference keeps private: DV_fid, redshift, kmax)."""

    def __init__(self, d):
        self.dir, self.ini = d, os.path.join(d, "ref.ini")
        self.gigglez_dir = os.path.join(d, "data")
        lines = open(os.path.join(d, "cases.txt")).read().split("\n")
        self.use_scaling = int(lines[0].split()[3]) != 0
        nk = int(lines[1])
        self.case_k = np.array(lines[2:2 + nk], dtype=np.float64)
        nc = int(lines[2 + nk])
        self.cases = np.array([lines[3 + nk + i].split() for i in range(nc)], dtype=np.float64)
        self.ref = np.array(open(os.path.join(d, "ref.txt")).read().split(), dtype=np.float64)
        t = open(os.path.join(d, "info.txt")).read().split()
        self.np, self.nk, _, _, self.has_cov, self.is_wigglez = (int(x) for x in t[:6])
        assert self.nk == nk
        v = np.array(t[6:], dtype=np.float64)
        if self.is_wigglez:          # the reference keeps WiggleZLikelihood private: only its parent's components
            self.DV_fid, self.redshift, self.kmax = v
            self.k = self.P = self.sdev = self.invcov = None
        else:
            self.k, v = v[:nk], v[nk:]
            self.P, v = v[:self.np], v[self.np:]
            self.sdev, v = v[:self.np], v[self.np:]
            self.invcov = v.reshape(self.np, self.np) if self.has_cov else None
        self.rows = np.array(open(os.path.join(d, "row.txt")).read().split(), dtype=np.float64).reshape(nc, 2 + self.nk)
        assert len(self.ref) == nc


def extract(tmpdir, archive=GOLDEN, names=None):
    """{name: Golden} with the archive extracted under tmpdir."""
    with open(archive, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    base = os.path.join(str(tmpdir), "mpk")
    return {n: Golden(os.path.join(base, n)) for n in (NAMES if names is None else names)}
