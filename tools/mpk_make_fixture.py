#!/usr/bin/env python3
"""Inputs of the galaxy power-spectrum goldens (tests/golden/mpk/mpk_fixture.tar.xz).

  python tools/mpk_make_fixture.py --out DIR --real <reference>/data
  (build tools/mpk_ref_harness, see its header)
  python tools/mpk_make_fixture.py --run oracle/_ref/mpk_ref_harness DIR
  python tools/mpk_make_fixture.py --pack DIR

--real names the directory that holds the real sdss_lrgDR4*, wigglez_nov11* and
gigglezfiducialmodel_matterpower_{a..d}.dat files; they are copied, as data,
into the goldens lrg_dr4 and wigglez_a .. wigglez_d (and the GiggleZ files into
the synthetic WiggleZ sets that use them).  The seeded synthetic sets are
those of tests/mpk_fixture.py (SYNTHETIC there says what each holds).  The
archive holds text data only; --pack asserts that every golden -lnL is finite.
"""
import argparse
import io
import lzma
import os
import shutil
import subprocess
import sys
import tarfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpk_fixture as mf  # noqa: E402

OUTPUTS = ("ref.txt", "row.txt", "info.txt")


def real_lrg(d, src):
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    shutil.copy(os.path.join(src, "sdss_lrgDR4.dataset"), d)
    for f in ("sdss_lrgDR4_kbands.txt", "sdss_lrgDR4_measurements.txt", "sdss_lrgDR4_windows.txt"):
        shutil.copy(os.path.join(src, f), os.path.join(d, "data", f))
    with open(os.path.join(d, "ref.ini"), "w") as f:        # batch2/MPK.ini
        f.write("action = 0\nuse_mpk = T\nmpk_numdatasets = 1\nmpk_dataset1 = sdss_lrgDR4.dataset\n"
                "mpk_dataset_nonlinear1 = T\n")
    mf.write_cases(d, 94874.8118745411, True, os.path.join(d, "data", "sdss_lrgDR4_kbands.txt"), 1, 65)


def real_wigglez(d, src, c):
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    shutil.copy(os.path.join(src, "wigglez_nov11_common.dataset"), d)
    shutil.copy(os.path.join(src, "wigglez_nov11%s.dataset" % c), d)
    for f in ["wigglez_nov11_kbands.txt"] + ["wigglez_nov11%s_%s.txt" % (c, x) for x in ("measurements", "windows", "cov")] \
            + mf.GIGGLEZ:
        shutil.copy(os.path.join(src, f), os.path.join(d, "data", f))
    with open(os.path.join(d, "ref.ini"), "w") as f:        # batch2/WiggleZ_MPK.ini, one bin
        f.write("action = 0\nuse_wigglez_mpk = T\nnonlinear_wigglez = T\nUse_gigglez = T\n"
                "wigglez_common_dataset = wigglez_nov11_common.dataset\nmpk_wigglez_numdatasets = 1\n"
                "wigglez_dataset1 = wigglez_nov11%s.dataset\n" % c)
    dv = [ln.split("=")[1] for ln in open(os.path.join(d, "wigglez_nov11%s.dataset" % c)) if ln.startswith("DV_fid")]
    mf.write_cases(d, float(dv[0]), True, os.path.join(d, "data", "wigglez_nov11_kbands.txt"), 1, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--real")
    ap.add_argument("--run", nargs=2, metavar=("HARNESS", "DIR"))
    ap.add_argument("--pack")
    a = ap.parse_args()
    if a.out:
        base = os.path.join(a.out, "mpk")
        if a.real:
            real_lrg(os.path.join(base, "lrg_dr4"), a.real)
            for c in "abcd":
                real_wigglez(os.path.join(base, "wigglez_" + c), a.real, c)
        for name, kind, kw in mf.SYNTHETIC:
            d = os.path.join(base, name)
            if kind == "mpk":
                mf.make_mpk(d, **kw)
            else:
                if kw.get("gigglez", True) and not a.real:
                    sys.exit("%s needs the GiggleZ fiducial files: give --real" % name)
                mf.make_wigglez(d, gigglez_src=a.real, **kw)
            print("wrote", name)
    if a.run:
        exe, base = os.path.abspath(a.run[0]), os.path.join(a.run[1], "mpk")
        for name in sorted(os.listdir(base)):
            for f in OUTPUTS:
                if os.path.exists(os.path.join(base, name, f)):
                    os.remove(os.path.join(base, name, f))
            subprocess.run([exe, "ref.ini", "cases.txt", *OUTPUTS], cwd=os.path.join(base, name), check=True,
                           stdout=subprocess.DEVNULL)
            ncase = len(mf.Golden(os.path.join(base, name)).cases)      # a Fortran STOP exits 0: the outputs say
            print("ran", name)
    if a.pack:
        base = os.path.join(a.pack, "mpk")
        buf = io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w") as tar:
            for n in sorted(os.listdir(base)):
                ref = np.array(open(os.path.join(base, n, "ref.txt")).read().split(), dtype=np.float64)
                assert len(ref) and np.all(np.isfinite(ref)) and np.all(np.abs(ref) < 1e29), "%s: a golden -lnL is not finite" % n
                for dirpath, _, files in sorted(os.walk(os.path.join(base, n))):
                    for f in sorted(files):
                        path = os.path.join(dirpath, f)
                        ti = tar.gettarinfo(path, "mpk/" + os.path.relpath(path, base))
                        ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, "", "", 0o644
                        with open(path, "rb") as fh:
                            tar.addfile(ti, fh)
        os.makedirs(os.path.dirname(mf.GOLDEN), exist_ok=True)
        with open(mf.GOLDEN, "wb") as f:
            f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
        print(mf.GOLDEN, os.path.getsize(mf.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
