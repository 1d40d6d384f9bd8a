#!/usr/bin/env python3
"""SZ cluster-counts kernel timing on the real Planck files (as tools/wl_profile.py).

    python tools/sz_profile.py [--data DIR] [iters = 5] [W ...= 64 256 1024]

--data names a directory that holds SZ_cat.txt, SZ_thetas.txt, SZ_skyfracs.txt
and SZ_ylims.txt (the reference's data/); without it the copy of those files in
tests/golden/sz/sz_fixture.tar.xz (data set "real") is used, with the fixture's
theory row.  Per W the HIP-event time of each kernel of one evaluation after a
warm-up, at the centre of batch2/SZ_plus_CMB.ini scattered by 1 %, next to two
floors per walker: the ln Y nodes sz_compl_kernel visits (nzs nm points x the
window of 2 sqrt(746) sqrt(2) scatter / dlny + 3 nodes) x 25 f64 instructions a
node (4 per S/N bin, 4 for the argument, the exp counted as ONE: a lower bound)
over the f64 vector rate without FMA (39.3e12 lane-instructions/s), and the
theory row read once over the measured HBM rate (6 TB/s).
"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sz_fixture as sf  # noqa: E402
from cosmomc_amd import _native as N  # noqa: E402
from cosmomc_amd import szcounts as S  # noqa: E402

VALU_F64, HBM = 39.3e12, 6.0e12
KERNELS = ("sz_compl_kernel", "sz_compl0_kernel", "sz_counts_kernel")


def main():
    a = sys.argv[1:]
    data = None
    if a and a[0] == "--data":
        data, a = os.path.abspath(a[1]), a[2:]
    iters = int(a[0]) if a else 5
    Ws = [int(x) for x in a[1:]] or [64, 256, 1024]
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        g = sf.extract(td, names=["real"])["real"]
        ini = g.ini
        if data is not None:
            ini = os.path.join(td, "sz_data.ini")
            with open(ini, "w") as f:
                f.write("".join("%s = %s\n" % (k, os.path.join(data, n)) for k, n in
                                (("cat_file", "SZ_cat.txt"), ("thetas_file", "SZ_thetas.txt"),
                                 ("skyfracs_file", "SZ_skyfracs.txt"), ("ylims_file", "SZ_ylims.txt"))))
                f.write("prior_scatter_SZ = T\nprior_ystar_SZ = T\n")
        like = S.SZLikelihood(ini)
        torch.cuda.synchronize()
        print(f"{ini}: {like.n_thetas} thetas, {like.n_patches} patches, {like.n_cat} clusters, nzs = {like.nzs}, "
              f"nm = {like.nm}, {like.n_lny} ln Y nodes; opened (erfs table formed) in {time.perf_counter() - t0:.1f} s",
              flush=True)
        row = g.row
        rng = np.random.RandomState(1)
        centre = np.array(sf.CENTRE)
        nodes = min(like.n_lny, 2 * np.sqrt(746.0) * S.SQRT2 * centre[3] / S.DLNY + 3)
        work = like.nzs * like.nm * nodes * 25.0
        for W in Ws:
            dl = torch.tensor(np.tile(row, (W, 1))[:, None, :].copy(), device="cuda")
            nu = np.tile(centre, (W, 1)) * (1 + 0.01 * rng.standard_normal((W, 5)))
            nu[:, 4] = centre[4]
            nu = torch.tensor(nu, device="cuda")
            ws = torch.empty(like.workspace_bytes(W), dtype=torch.uint8, device="cuda")
            out = torch.empty(W, dtype=torch.float64, device="cuda")
            like.loglike_batch(dl, nu, out, ws)
            torch.cuda.synchronize()
            assert bool((out < 1e29).all()) and bool(torch.isfinite(out).all())
            N.profile_reset()
            N.profile_enable(True)
            for _ in range(iters):
                like.loglike_batch(dl, nu, out, ws)
            torch.cuda.synchronize()
            N.profile_enable(False)
            ms = {k: N.profile_read(k)[0] / iters for k in KERNELS}
            tot = sum(ms.values())
            f_valu = W * work / VALU_F64 * 1e3
            f_hbm = W * like.n_theory * 8 / HBM * 1e3
            print(f"W = {W:5d}: evaluation {tot:8.3f} ms = {tot / W * 1e3:7.2f} us per walker ("
                  + ", ".join(f"{k} {v:.3f}" for k, v in ms.items())
                  + f"); floors: {nodes:.0f} nodes a point, f64 VALU {f_valu:.4f} ms ({f_valu / tot:.1%} achieved), "
                  f"row read {f_hbm:.4f} ms ({f_hbm / tot:.1%})", flush=True)
            del ws, dl


if __name__ == "__main__":
    main()
