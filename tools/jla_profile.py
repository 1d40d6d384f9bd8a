#!/usr/bin/env python3
"""JLA factorisation kernel timing at the full JLA size (as tools/cmbl_profile.py).

    python tools/jla_profile.py [nsn = 740] [iters = 3] [W ...= 64 256 1024]
    python tools/jla_profile.py --marge [nsn = 740] [iters = 3] [W ...= 64 256 1024]

A seeded synthetic dataset with all six covariance components; the kernel's
HIP-event time per launch next to two floors: W n^3/3 flops over the f64 MFMA
peak (78.6 TF/s), and the bytes the algorithm has to move through HBM -- each
walker's factor L written once and read once (it does not fit on chip) -- over
the measured HBM rate (6 TB/s).  The third figure is what the
left-looking update reads through the caches: both operand rows of every tile
for every earlier block column.

--marge times the alpha, beta-marginalised likelihood (JLAMargeLikelihood, the
reference's default grid of 149 points) on the same dataset: the time to open
it (V^-1 of every grid point formed on the device), the HIP-event time of one
evaluation's kernels after a warm-up, and in the same run the route it
replaces, JLALikelihood.loglike_batch once per grid point.  Its floors: the
MFMA flops the quadratic-form kernel issues over the f64 MFMA peak, and the
bytes of the stored inverses read once over the HBM rate.
"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cosmomc_amd import _native as N  # noqa: E402
from cosmomc_amd.supernovae import COMPONENTS, JLALikelihood, JLAMargeLikelihood, jla_marge_grid  # noqa: E402

BLOCK = dict(mag=(0, 0), stretch=(1, 1), colour=(2, 2), mag_stretch=(0, 1), mag_colour=(0, 2), stretch_colour=(1, 2))
PEAK_F64, HBM = 78.6e12, 6.0e12


def write_dataset(d, n, seed=740):
    rng = np.random.RandomState(seed)
    z = np.sort(rng.uniform(0.01, 1.2, n))
    third = rng.uniform(8.0, 12.0, n)
    mu0 = 5 * np.log10((1 + z) * z * (1 + 0.5 * z) * 299792.458 / 70) + 25
    with open(os.path.join(d, "lc.txt"), "w") as f:
        for i in range(n):
            row = [z[i], z[i], 0.0, mu0[i] - 19.05 + 0.1 * rng.standard_normal(), rng.uniform(0.08, 0.2),
                   rng.standard_normal(), rng.uniform(0.1, 0.5), 0.1 * rng.standard_normal(), rng.uniform(0.02, 0.06),
                   third[i], 0.1, 1e-3 * rng.standard_normal(), 1e-4 * rng.standard_normal(),
                   1e-4 * rng.standard_normal()]
            f.write("sn%04d " % i + " ".join("%.9g" % x for x in row) + " %d\n" % rng.randint(0, 4))
    A = rng.standard_normal((3 * n, 3 * n + 7))
    Jm = A @ A.T / (3 * n + 7)
    sc = np.repeat(np.array([0.02, 0.1, 0.01]), n)
    Jm = Jm * sc[:, None] * sc[None, :]
    with open(os.path.join(d, "jla.dataset"), "w") as f:
        f.write("name = JLAprofile\ndata_file = lc.txt\ntwoscriptmfit = T\nscriptmcut = 10.0\n")
        for k in COMPONENTS:
            a, b = BLOCK[k]
            M = Jm[a * n:(a + 1) * n, b * n:(b + 1) * n]
            with open(os.path.join(d, k + ".dat"), "w") as g:
                g.write("%d\n" % n)
                np.savetxt(g, (M + M.T) / 2, fmt="%.9g")
            f.write("has_%s_covmat = T\n%s_covmat_file = %s.dat\n" % (k, k, k))
    return os.path.join(d, "jla.dataset"), mu0


MARGE_KERNELS = ("jla_marge_pro_kernel", "jla_marge_qf_kernel", "jla_marge_chi_kernel", "jla_marge_fin_kernel")


def _kernel_ms(names, iters):
    """HIP-event time per evaluation of the named kernels, summed over the launches of an evaluation."""
    ms = {}
    for k in names:
        t, cnt = N.profile_read(k)
        ms[k] = t / iters if cnt else 0.0
    return ms


def marge(n, iters, Ws):
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        ds, mu0 = write_dataset(td, n)
        print(f"nsn = {n}, six components; dataset written in {time.perf_counter() - t0:.1f} s", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        like = JLAMargeLikelihood(ds)
        torch.cuda.synchronize()
        t_open = time.perf_counter() - t0
        t0 = time.perf_counter()
        old = JLALikelihood(ds)
        t_old = time.perf_counter() - t0
        G = like.n_grid
        al, be = jla_marge_grid()
        assert G == len(al)
        Np = (n + 15) // 16 * 16
        print(f"open: {t_open:.2f} s for {G} grid points, {like.grid_bytes / 1e6:.0f} MB of inverses "
              f"(the sampled JLA likelihood opens the same files in {t_old:.2f} s)", flush=True)
        rng = np.random.RandomState(1)
        for W in Ws:
            mu = torch.tensor((mu0[None, :] + 0.05 * rng.standard_normal((W, n)))[:, None, :], device="cuda")
            ws = torch.empty(like.workspace_bytes(W), dtype=torch.uint8, device="cuda")
            out = torch.empty(W, dtype=torch.float64, device="cuda")
            like.loglike_batch(mu, None, out, ws)                # warm-up
            torch.cuda.synchronize()
            assert bool((out < 1e29).all()) and bool(torch.isfinite(out).all())
            N.profile_reset()
            N.profile_enable(True)
            for _ in range(iters):
                like.loglike_batch(mu, None, out, ws)
            torch.cuda.synchronize()
            N.profile_enable(False)
            k = _kernel_ms(MARGE_KERNELS, iters)
            ms = sum(k.values())
            # the route it replaces: one factorisation launch per grid point
            ws_old = torch.empty(old.workspace_bytes(W), dtype=torch.uint8, device="cuda")
            got = torch.empty((G, W), dtype=torch.float64, device="cuda")
            nus = [torch.tensor(np.tile([a, b], (W, 1)), device="cuda") for a, b in zip(al, be)]
            old.loglike_batch(mu, nus[0], got[0], ws_old)        # warm-up
            torch.cuda.synchronize()
            N.profile_reset()
            N.profile_enable(True)
            for g in range(G):
                old.loglike_batch(mu, nus[g], got[g], ws_old)
            torch.cuda.synchronize()
            N.profile_enable(False)
            t_rep, _ = N.profile_read("jla_chol_kernel")
            best = got.min(0).values
            via = best - torch.log(torch.exp(-got + best).sum(0) * like.width_alpha * like.width_beta)
            err = float(((out - via).abs() / via.abs()).max())
            Wt = sum(-(-min(1024, W - w0) // 16) * 16 for w0 in range(0, W, 1024))    # whole 16-walker tiles
            f_flop = 2.0 * G * Np * Np * Wt / PEAK_F64 * 1e3
            f_hbm = like.grid_bytes / HBM * 1e3
            print(f"W = {W:5d}: evaluation {ms:8.3f} ms (prologue {k[MARGE_KERNELS[0]]:.3f}, quadratic forms "
                  f"{k[MARGE_KERNELS[1]]:.3f}, chi^2 and integral {k[MARGE_KERNELS[2]] + k[MARGE_KERNELS[3]]:.3f}); replaced route {t_rep:9.2f} ms "
                  f"= {t_rep / ms:6.1f} x; floors: flops {f_flop:.3f} ms ({f_flop / ms:.1%} achieved), HBM "
                  f"{f_hbm:.3f} ms ({f_hbm / ms:.1%}); max rel. difference of the two routes {err:.1e}", flush=True)
            del ws, ws_old, mu, got, nus


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--marge":
        a = sys.argv[2:]
        marge(int(a[0]) if a else 740, int(a[1]) if len(a) > 1 else 3, [int(x) for x in a[2:]] or [64, 256, 1024])
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 740
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    Ws = [int(x) for x in sys.argv[3:]] or [64, 256, 1024]
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        ds, mu0 = write_dataset(td, n)
        like = JLALikelihood(ds)
        print(f"nsn = {n}, six components; dataset written and loaded in {time.perf_counter() - t0:.1f} s", flush=True)
        Np = (n + 15) // 16 * 16
        T = Np // 16
        l_bytes = Np * (Np + 16) / 2 * 8                     # the lower triangle and the right-hand-side rows
        cache_bytes = 4096 * sum(J * (T + 1 - J) for J in range(T))
        rng = np.random.RandomState(1)
        for W in Ws:
            mu = torch.tensor((mu0[None, :] + 0.05 * rng.standard_normal((W, n)))[:, None, :], device="cuda")
            nu = torch.tensor(np.tile([0.141, 3.101], (W, 1)) + 0.01 * rng.standard_normal((W, 2)), device="cuda")
            ws = torch.empty(like.workspace_bytes(W), dtype=torch.uint8, device="cuda")
            out = torch.empty(W, dtype=torch.float64, device="cuda")
            like.loglike_batch(mu, nu, out, ws)
            torch.cuda.synchronize()
            assert bool((out < 1e29).all()) and bool(torch.isfinite(out).all())
            N.profile_reset()
            N.profile_enable(True)
            for _ in range(iters):
                like.loglike_batch(mu, nu, out, ws)
            torch.cuda.synchronize()
            N.profile_enable(False)
            t, cnt = N.profile_read("jla_chol_kernel")
            ms = t / cnt
            f_flop = W * n ** 3 / 3 / PEAK_F64 * 1e3
            f_hbm = W * 2 * l_bytes / HBM * 1e3
            print(f"W = {W:5d}: jla_chol_kernel {ms:9.3f} ms ({ms / W * 1e3:8.2f} us per walker); floors: flops "
                  f"{f_flop:.3f} ms ({f_flop / ms:.1%} achieved), HBM {f_hbm:.3f} ms ({f_hbm / ms:.1%}); "
                  f"operand reads through the caches {W * cache_bytes / 1e9:.1f} GB = "
                  f"{W * cache_bytes / ms / 1e9:.2f} TB/s", flush=True)
            del ws, mu
