#!/usr/bin/env python3
"""Galaxy power-spectrum kernel timing on the real data sets (as tools/sz_profile.py).

    python tools/mpk_profile.py [iters = 20] [W ...= 64 256 1024]

The real LRG DR4 set and the real WiggleZ bin a of
tests/golden/mpk/mpk_fixture.tar.xz, with the fixture's theory rows.  Per W the
HIP-event time of each of the two kernels of one evaluation after a warm-up,
next to two floors: the flops of the two products (2 regions vectors np (nk +
np) per walker) over the f64 MFMA rate (78.6e12 flop/s), and the bytes of the
theory rows read and the operand workspace written and read once over the
measured HBM rate (6.3e12 B/s).  At these sizes both floors are a small part
of a microsecond: the evaluation is two kernel launches, and the time printed
is launch latency and the dependent chain of one workgroup.
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mpk_fixture as mf  # noqa: E402
from cosmomc_amd import _native as N  # noqa: E402
from cosmomc_amd import mpk as M  # noqa: E402
from cosmomc_amd.ini import IniFile  # noqa: E402
from cosmomc_amd.likelihood import LikelihoodList  # noqa: E402

MFMA_F64, HBM = 78.6e12, 6.3e12
KERNELS = ("mpk_prologue_kernel", "mpk_contract_kernel")


def main():
    a = sys.argv[1:]
    iters = int(a[0]) if a else 20
    Ws = [int(x) for x in a[1:]] or [64, 256, 1024]
    with tempfile.TemporaryDirectory() as td:
        goldens = mf.extract(td, names=["lrg_dr4", "wigglez_a"])
        for name, g in goldens.items():
            lst, ini = LikelihoodList(), IniFile(g.ini)
            like, = M.mpk_likelihood_add(lst, ini) + M.wigglez_likelihood_add(lst, ini, gigglez_dir=g.gigglez_dir)
            nv = 2 if like.q_mode == M.Q_FLAT else 13 if like.q_mode == M.Q_GAUSS else 1
            flops = 2.0 * like.n_regions * nv * like.n_points * (like.n_kbands + like.n_points)
            print(f"{name}: {like.n_regions} regions x {like.n_points} points x {like.n_kbands} kbands, {nv} vectors, "
                  f"{flops:.0f} flop a walker", flush=True)
            rng = np.random.RandomState(1)
            for W in Ws:
                rows = g.rows[rng.randint(0, len(g.rows), W)]
                dl = torch.tensor(np.ascontiguousarray(rows[:, None, :]), device="cuda")
                ws = torch.empty(like.workspace_bytes(W), dtype=torch.uint8, device="cuda")
                out = torch.empty(W, dtype=torch.float64, device="cuda")
                like.loglike_batch(dl, None, out, ws)
                torch.cuda.synchronize()
                assert bool((out < 1e29).all()) and bool(torch.isfinite(out).all())
                N.profile_reset()
                N.profile_enable(True)
                for _ in range(iters):
                    like.loglike_batch(dl, None, out, ws)
                torch.cuda.synchronize()
                N.profile_enable(False)
                ms = {k: N.profile_read(k)[0] / iters for k in KERNELS}
                tot = sum(ms.values())
                f_mfma = W * flops / MFMA_F64 * 1e3
                f_hbm = W * (like.n_theory + 2 * like.n_kbands * nv) * 8 / HBM * 1e3
                print(f"  W = {W:5d}: evaluation {tot * 1e3:8.1f} us ("
                      + ", ".join(f"{k} {v * 1e3:.1f}" for k, v in ms.items())
                      + f"); floors: f64 MFMA {f_mfma * 1e3:.3f} us, HBM {f_hbm * 1e3:.3f} us", flush=True)
                del ws, dl


if __name__ == "__main__":
    main()
