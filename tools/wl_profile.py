#!/usr/bin/env python3
"""Weak-lensing kernel timing at the DES Y1 shape (as tools/jla_profile.py).

    python tools/wl_profile.py [--dataset DIR/DES_1YR_final.dataset] [iters = 5] [W ...= 64 256 1024]

Without --dataset, a seeded synthetic dataset of the DES shape is written
(tests/wl_fixture.make_synthetic: 4 source and 5 lens bins, 20 theta bins, 351
n(z) rows, lmax = 50000: nz = 353, nl = 75, 35 Limber columns); --dataset takes
the des_shape dataset of tools/wl_make_fixture.py --des-shape (the real DES
files, 457 points used).  Per W the HIP-event time of each kernel of one
evaluation after a warm-up, next to two floors per walker: the flops of the
Limber product, the operator and the quadratic form (2 nl nz columns + 2 n_used
nl + 2 n_used^2) over the f64 MFMA peak (78.6 TF/s), and the theory row read
once over the measured HBM rate (6 TB/s).
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

import wl_fixture as wf  # noqa: E402
from cosmomc_amd import _native as N  # noqa: E402
from cosmomc_amd import weaklensing as wl  # noqa: E402

PEAK_F64, HBM = 78.6e12, 6.0e12
KERNELS = ("wl_kernel_q", "wl_kernel_corr", "wl_quadform_ksplit", "wl_kernel_finish")


def main():
    a = sys.argv[1:]
    dataset = None
    if a and a[0] == "--dataset":
        dataset, a = a[1], a[2:]
    iters = int(a[0]) if a else 5
    Ws = [int(x) for x in a[1:]] or [64, 256, 1024]
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        if dataset is None:
            dataset = wf.make_synthetic(td, seed=900, nsrc=4, ngal=5, ntheta=20, nrows=351, lmax=50000,
                                        cov_fmt="%.9g")["dataset"]
        like = wl.WLLikelihood(dataset)
        ds = like.ds
        print(f"{dataset}: nz = {like.nz}, nl = {like.nl}, {like.n_columns} Limber columns, {like.n_used} points used; "
              f"written and loaded in {time.perf_counter() - t0:.1f} s", flush=True)
        chis, Hs, Dg = wf.cosmology(ds.z_p)
        row = wl.wl_theory_row(ds, wf.H0 / 100, wf.OMM, chis, Hs, Dg,
                               lambda kh, z: np.exp(wf.analytic_lnpk(2, np.log(kh), z)), np.exp(wf.PK_GRID[2]),
                               np.exp(wf.PK_GRID[3]))
        nn = len(like.nuisance_names)
        fid = wf.fiducial(like.num_z_bins, like.num_gal_bins)
        rng = np.random.RandomState(1)
        flops = 2.0 * like.nl * like.nz * like.n_columns + 2.0 * like.n_used * like.nl + 2.0 * like.n_used ** 2
        for W in Ws:
            dl = torch.tensor(np.tile(row, (W, 1))[:, None, :].copy(), device="cuda")
            nu = torch.tensor(np.tile(fid, (W, 1)) * (1 + 0.01 * rng.standard_normal((W, nn))), device="cuda")
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
            f_flop = W * flops / PEAK_F64 * 1e3
            f_hbm = W * like.n_theory * 8 / HBM * 1e3
            print(f"W = {W:5d}: evaluation {tot:8.3f} ms = {tot / W * 1e3:7.2f} us per walker ("
                  + ", ".join(f"{k} {v:.3f}" for k, v in ms.items())
                  + f"); floors: flops {f_flop:.4f} ms ({f_flop / tot:.1%} achieved), row read {f_hbm:.4f} ms "
                  f"({f_hbm / tot:.1%})", flush=True)
            del ws, dl


if __name__ == "__main__":
    main()
