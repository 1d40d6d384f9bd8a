#!/usr/bin/env python3
"""Inputs and packing of the tabulated-BAO goldens
(tests/golden/bao/bao_table.tar.xz; tests/bao_fixture.py says what it holds).

  python tools/bao_make_fixture.py --out DIR --data <reference>/data [--dr11 <reference>/data]
  (build tools/bao_ref_harness, see its header, then)
  python tools/bao_make_fixture.py --run DIR
  python tools/bao_make_fixture.py --pack DIR

--out writes DIR/bao: the real MGS dataset and its chi^2 table and the two
abundance datasets copied as data from --data, the seeded synthetic grids, the
inis and the case files.  --dr11 adds the real DR11 CMASS consensus grid (280 x
280, 3.9 MB of text, 270 KB in the archive) from the directory that holds it.
The real DR12 dilation grids are not distributed with the reference, so those
tags have synthetic grids only.  --run calls oracle/_ref/bao_ref_harness for
every ini; --pack writes the archive, data files only.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bao_fixture as bf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--data")
    ap.add_argument("--dr11")
    ap.add_argument("--run")
    ap.add_argument("--pack")
    a = ap.parse_args()
    if a.out:
        bf.make_fixture(os.path.join(a.out, "bao"), a.data, a.dr11)
        print("wrote", os.path.join(a.out, "bao"))
    if a.run:
        d = os.path.join(a.run, "bao")
        exe = os.path.join(ROOT, "oracle", "_ref", "bao_ref_harness")
        for ini, (cases, _, ref) in bf.INIS.items():
            if os.path.exists(os.path.join(d, ini)):
                subprocess.run([exe, ini, cases, ref], cwd=d, check=True)
                print("ran", ini)
    if a.pack:
        print(bf.GOLDEN, bf.pack(os.path.join(a.pack, "bao")), "bytes")


if __name__ == "__main__":
    main()
