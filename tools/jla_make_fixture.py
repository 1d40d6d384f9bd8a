#!/usr/bin/env python3
"""Inputs of the JLA goldens (tests/golden/jla/jla_fixture.tar.xz, jla_upper.tar.xz).

  python tools/jla_make_fixture.py --lcparams <reference>/data/jla_lcparams.txt --out DIR
  (run tools/jla_ref_harness on every DIR/<name>, see its header)
  python tools/jla_make_fixture.py --pack DIR

--archive upper does the same for the second archive (default: fixture); each
archive is made and packed on its own, so one can be added without touching
the other.

--archive marge (tests/golden/jla/jla_marge.tar.xz) holds the goldens of the
alpha, beta-marginalised likelihood (JLA_marginalize = T): per case the option
lines and the reference's jla_LnLike at the five mu rows of a dataset of the
first archive, which it names and does not repeat.  --out DIR extracts those
datasets from the committed first archive where DIR lacks them, and writes per
case DIR/marge/<case>/options.txt and the reference's main ini
DIR/<dataset>/<case>.ini; tools/jla_marge_ref_harness (see its header), run in
DIR/<dataset> on that ini, writes DIR/marge/<case>/ref.txt.  syn5_indef_s2 has
widths that put a grid point near (0.2, 2.5), where that dataset's V is
indefinite: the reference drops it and keeps the rest.

Seeded (np.random.RandomState, whose stream is frozen) synthetic datasets: SN
rows taken from the JLA light-curve file, component matrices cut from one
jointly positive-semidefinite 3n x 3n matrix with blocks scaled by
(0.02, 0.1, 0.01), so V(alpha, beta) is positive definite for every alpha,
beta; pecz = 0.0005, intrinsicdisp = 0.1 and intrinsicdisp1 = 0.08 so those
paths differ from their defaults.  syn5_indef instead has a mag_stretch matrix
that makes V indefinite at (0.2, 2.5) only.  Every number is written to 9
significant digits; the archive holds text data only.

syn21_upper (jla_upper.tar.xz) tells the two triangles of a matrix file apart:
the reference reads mat(j, 1:n) row by row and DPOTRF takes the upper triangle
only (:329-331, 135), so the strict lower triangle of every matrix file is
overwritten with seeded noise of the entries' own scale; a loader that read it
would give another, usually still finite, answer.  Its stretch matrix is
written one number a line, the reference's second layout (:335-342).
"""
import argparse
import io
import os
import tarfile

import numpy as np

CASES = [(0.141, 3.101), (0.0, 0.0), (0.2, 2.5), (-0.05, 3.6), (0.14, 3.1)]
BLOCK = dict(mag=(0, 0), stretch=(1, 1), colour=(2, 2), mag_stretch=(0, 1), mag_colour=(0, 2), stretch_colour=(1, 2))
#           name          nsn  components                         twoscriptmfit  seed
DATASETS = [("syn37", 37, tuple(BLOCK), True, 3701),
            ("syn70", 70, tuple(BLOCK), False, 7001),
            ("syn131", 131, ("mag", "stretch", "mag_colour"), True, 13101),
            ("syn37_diag", 37, (), True, 3702),
            ("syn5_indef", 5, ("mag", "mag_stretch"), False, 501)]
UPPER = [("syn21_upper", 21, ("mag", "stretch", "mag_colour"), False, 2101)]
ARCHIVES = {"fixture": ("jla_fixture.tar.xz", DATASETS), "upper": ("jla_upper.tar.xz", UPPER)}
#        case             dataset       steps  width_alpha  width_beta
MARGE = [("syn37_s7", "syn37", 7, 0.003, 0.04),
         ("syn37_s0", "syn37", 0, 0.003, 0.04),
         ("syn70_s2", "syn70", 2, 0.003, 0.04),
         ("syn131_s1", "syn131", 1, 0.003, 0.04),
         ("syn37_diag_s7", "syn37_diag", 7, 0.003, 0.04),
         ("syn5_indef_s2", "syn5_indef", 2, 0.06, 0.623)]
MARGE_ARCHIVE = "jla_marge.tar.xz"
FILES = ["jla.dataset", "lc.txt", "cases.txt", "ref.txt"] + [k + ".dat" for k in BLOCK]


def g9(x):
    return "%.9g" % x


def write_matrix(path, M, flat=False):
    with open(path, "w") as f:
        f.write("%d\n" % len(M))
        for r in M:
            f.write(("\n" if flat else " ").join(g9(x) for x in r) + "\n")


def diag_terms(d, a, b):
    f32 = lambda x: (x.astype(np.float32) * x.astype(np.float32)).astype(np.float64)
    z = d[:, 0]
    sets = d[:, 14].astype(int)
    idisp = np.where(sets == 1, 0.08, 0.1)
    zfacsq = float(np.float32(25.0) / np.log(np.float32(10.0)) ** 2)
    pre = f32(d[:, 4]) + idisp ** 2 + zfacsq * 0.0005 ** 2 * ((1 + z) / (z * (1 + 0.5 * z))) ** 2
    return pre + a * a * f32(d[:, 6]) + b * b * f32(d[:, 8]) + 2 * a * d[:, 11] - 2 * b * d[:, 12] - 2 * a * b * d[:, 13]


def make(name, n, comps, two, seed, src, out):
    rng = np.random.RandomState(seed)
    os.makedirs(out, exist_ok=True)
    idx = np.sort(rng.choice(len(src), n, replace=False))
    with open(os.path.join(out, "lc.txt"), "w") as f:
        f.write("#name zcmb zhel dz mb dmb x1 dx1 color dcolor 3rdvar d3rdvar cov_m_s cov_m_c cov_s_c set\n")
        f.write("".join(src[i] for i in idx))
    d = np.loadtxt(os.path.join(out, "lc.txt"), usecols=range(1, 16), ndmin=2)
    A = rng.standard_normal((3 * n, 3 * n + 7))
    Jm = A @ A.T / (3 * n + 7)
    sc = np.repeat(np.array([0.02, 0.1, 0.01]), n)
    Jm = Jm * sc[:, None] * sc[None, :]
    mats = {}
    for k in comps:
        a, b = BLOCK[k]
        M = Jm[a * n:(a + 1) * n, b * n:(b + 1) * n]
        mats[k] = (M + M.T) / 2
    if name == "syn5_indef":
        # V = mag + 2 alpha mag_stretch + diag: mag_stretch = -c B, B positive definite, c such that
        # V is indefinite at (0.2, 2.5) and positive definite at the other cases
        B = Jm[n:2 * n, n:2 * n]
        B = (B + B.T) / 2

        def mineig(c, a, b):
            M = np.array([[float(g9(x)) for x in r] for r in mats["mag"]])
            S = np.array([[float(g9(x)) for x in r] for r in -c * B])
            return np.linalg.eigvalsh(M + 2 * a * S + np.diag(diag_terms(d, a, b))).min()
        c = 0.01
        while not mineig(c, 0.2, 2.5) < -1e-3:
            c *= 1.05
        assert all(mineig(c, a, b) > 1e-3 for a, b in CASES if a != 0.2), c
        mats["mag_stretch"] = -c * B
    if name == "syn21_upper":
        for k in comps:
            noise = np.std(mats[k]) * rng.standard_normal((n, n))
            mats[k] = np.triu(mats[k]) + np.tril(noise, -1)
    with open(os.path.join(out, "jla.dataset"), "w") as f:
        f.write("name = JLA%s\ndata_file = lc.txt\npecz = 0.0005\nintrinsicdisp = 0.1\nintrinsicdisp1 = 0.08\n" % name)
        f.write("twoscriptmfit = %s\nscriptmcut = 10.0\n" % ("T" if two else "F"))
        for k in comps:
            write_matrix(os.path.join(out, k + ".dat"), mats[k], flat=name == "syn21_upper" and k == "stretch")
            f.write("has_%s_covmat = T\n%s_covmat_file = %s.dat\n" % (k, k, k))
    zc = d[:, 0]
    mu0 = 5 * np.log10((1 + zc) * zc * (1 + 0.5 * zc) * 299792.458 / 70) + 25
    with open(os.path.join(out, "cases.txt"), "w") as f:
        f.write("%d\n" % len(CASES))
        for i, (a, b) in enumerate(CASES):
            mu = mu0 + 0.05 * rng.standard_normal(n) + 0.01 * i
            f.write("%s %s\n" % (g9(a), g9(b)))
            f.write(" ".join(g9(x) for x in mu) + "\n")


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jla")


def make_marge(out):
    import lzma
    if not all(os.path.exists(os.path.join(out, ds, "jla.dataset")) for _, ds, *_ in MARGE):
        with open(os.path.join(GOLDEN_DIR, ARCHIVES["fixture"][0]), "rb") as f:
            tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
            for m in tar.getmembers():              # jla/<name>/<file> -> out/<name>/<file>
                m.name = m.name.split("/", 1)[1]
                tar.extract(m, out)
    for case, ds, steps, wa, wb in MARGE:
        opts = "JLA_marge_steps = %d\nJLA_step_width_alpha = %s\nJLA_step_width_beta = %s\n" % (steps, g9(wa), g9(wb))
        os.makedirs(os.path.join(out, "marge", case), exist_ok=True)
        with open(os.path.join(out, "marge", case, "options.txt"), "w") as f:
            f.write("dataset = %s\n" % ds + opts)
        with open(os.path.join(out, ds, case + ".ini"), "w") as f:
            f.write("use_JLA = T\nJLA_marginalize = T\njla_dataset = jla.dataset\n" + opts)
        print("wrote", os.path.join(out, "marge", case))


def pack(root, archive="fixture"):
    if archive == "marge":
        datasets, files, top = [(os.path.join("marge", c),) for c, *_ in MARGE], ["options.txt", "ref.txt"], "jla_"
        fname = MARGE_ARCHIVE
    else:
        (fname, datasets), files, top = ARCHIVES[archive], FILES, "jla/"
    dst = GOLDEN_DIR
    os.makedirs(dst, exist_ok=True)
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w:xz", preset=9) as tar:
        for name, *_ in datasets:
            for fn in files:
                p = os.path.join(root, name, fn)
                if not os.path.exists(p):
                    if fn == "ref.txt":
                        raise SystemExit("missing %s: run the reference harness first" % p)
                    continue
                ti = tarfile.TarInfo("%s%s/%s" % (top, name, fn))
                data = open(p, "rb").read()
                ti.size, ti.mtime, ti.mode = len(data), 0, 0o644
                tar.addfile(ti, io.BytesIO(data))
    with open(os.path.join(dst, fname), "wb") as f:
        f.write(buf.getvalue())
    print("wrote", os.path.join(dst, fname), len(buf.getvalue()), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lcparams")
    ap.add_argument("--out")
    ap.add_argument("--pack")
    ap.add_argument("--archive", choices=sorted(ARCHIVES) + ["marge"], default="fixture")
    a = ap.parse_args()
    if a.pack:
        return pack(a.pack, a.archive)
    if a.archive == "marge":
        return make_marge(a.out)
    src = [l for l in open(a.lcparams) if not l.lstrip().startswith("#")]
    for name, n, comps, two, seed in ARCHIVES[a.archive][1]:
        make(name, n, comps, two, seed, src, os.path.join(a.out, name))
        print("wrote", os.path.join(a.out, name))


if __name__ == "__main__":
    main()
