#!/usr/bin/env python3
"""Inputs of the SZ cluster-counts goldens (tests/golden/sz/sz_fixture.tar.xz).

  python tools/sz_make_fixture.py --out DIR [--real <reference>/data]
  (build tools/sz_ref_harness, see its header)
  python tools/sz_make_fixture.py --run oracle/_ref/sz_ref_harness DIR
  python tools/sz_make_fixture.py --pack DIR

The datasets are the seeded synthetic ones of tests/sz_fixture.py (GOLDENS and
make_synthetic there say what each holds).  --real copies the real SZ_* data
files, as data, into a dataset "real" with a few points; it is packed when it
is there.  Every golden has the same cosmology and so the same theory row,
which --pack keeps once (sz/row.txt) after checking that the copies agree
and that every dataset the archive already holds keeps its inputs and its
recorded -lnL byte for byte;
of the row the reference forms with use_watson = T every WATSON_STRIDE-th
number is kept (sz/watson/row_sample.txt), for sz_theory_row's Watson branch.
The archive holds text data only.
"""
import argparse
import filecmp
import io
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sz_fixture as sf  # noqa: E402

DATA = ("SZ_cat.txt", "SZ_thetas.txt", "SZ_skyfracs.txt", "SZ_ylims.txt", "SZ.paramnames")
PACKED = ("sz.ini", "sz_ref.ini", "cases.txt", "ref.txt", "info.txt") + tuple("data/" + f for f in DATA)


def real_dataset(d, src):
    os.makedirs(os.path.join(d, "data"), exist_ok=True)
    for f in DATA:
        shutil.copy(os.path.join(src, f), os.path.join(d, "data", f))
    priors = ("prior_scatter_SZ", "prior_ystar_SZ")
    sf.write_ini(os.path.join(d, "sz.ini"), priors)
    with open(os.path.join(d, "sz_ref.ini"), "w") as f:
        f.write("action = 0\nuse_SZ = T\n2D = T\n" + "".join("%s = T\n" % p for p in priors))
    sf.write_cases(d, sf.nuisance_points("few"))


def datasets(base):
    return sorted(n for n in os.listdir(base) if os.path.isdir(os.path.join(base, n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--real")
    ap.add_argument("--run", nargs=2, metavar=("HARNESS", "DIR"))
    ap.add_argument("--pack")
    a = ap.parse_args()
    if a.out:
        for name, kw in sf.GOLDENS:
            sf.make_synthetic(os.path.join(a.out, "sz", name), **kw)
            print("wrote", name)
        # the Watson mass function: only a sample of its row is packed (sz/watson/row_sample.txt)
        d = os.path.join(a.out, "sz", "watson")
        sf.make_synthetic(d, **dict(sf.GOLDENS)["syn_prior_all"])
        with open(os.path.join(d, "sz_ref.ini"), "a") as f:
            f.write("use_watson = T\n")
        print("wrote watson")
        if a.real:
            real_dataset(os.path.join(a.out, "sz", "real"), a.real)
            print("wrote real")
    if a.run:
        exe, base = os.path.abspath(a.run[0]), os.path.join(a.run[1], "sz")
        for name in datasets(base):
            subprocess.run([exe, "sz_ref.ini", "cases.txt", "ref.txt", "row.txt", "info.txt"], cwd=os.path.join(base, name),
                           check=True, stdout=subprocess.DEVNULL)
            print("ran", name)
    if a.pack:
        base = os.path.join(a.pack, "sz")
        names = [n for n in datasets(base) if n != "watson"]
        rows = [open(os.path.join(base, n, "row.txt")).read() for n in names]
        assert all(r == rows[0] for r in rows), "the goldens' theory rows differ"
        # a dataset the archive already holds keeps its inputs byte for byte and its recorded -lnL
        if os.path.exists(sf.GOLDEN):
            with tempfile.TemporaryDirectory() as old:
                sf.extract(old, names=[])
                for n in names:
                    for f in PACKED:
                        was = os.path.join(old, "sz", n, f)
                        if os.path.exists(was):
                            assert filecmp.cmp(was, os.path.join(base, n, f), shallow=False), \
                                "%s/%s differs from the archive's" % (n, f)
        buf = io.BytesIO()

        def add(path, arc):
            ti = tar.gettarinfo(path, arc)
            ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, "", "", 0o644
            with open(path, "rb") as fh:
                tar.addfile(ti, fh)
        with tarfile.open(fileobj=buf, mode="w") as tar:
            add(os.path.join(base, names[0], "row.txt"), "sz/row.txt")
            wrow = open(os.path.join(base, "watson", "row.txt")).read().split()
            with open(os.path.join(base, "watson", "row_sample.txt"), "w") as f:
                f.write("\n".join(wrow[::sf.WATSON_STRIDE]) + "\n")
            add(os.path.join(base, "watson", "row_sample.txt"), "sz/watson/row_sample.txt")
            for n in names:
                ref = np.array(open(os.path.join(base, n, "ref.txt")).read().split(), dtype=np.float64)
                assert np.all(np.isfinite(ref)) and np.all(np.abs(ref) < 1e29), "%s: a golden -lnL is not finite" % n
                for f in PACKED:
                    add(os.path.join(base, n, f), "sz/%s/%s" % (n, f))
        import lzma
        os.makedirs(os.path.dirname(sf.GOLDEN), exist_ok=True)
        with open(sf.GOLDEN, "wb") as f:
            f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
        print(sf.GOLDEN, os.path.getsize(sf.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
