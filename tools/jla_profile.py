#!/usr/bin/env python3
"""JLA factorisation kernel timing at the full JLA size (as tools/cmbl_profile.py).

    python tools/jla_profile.py [nsn = 740] [iters = 3] [W ...= 64 256 1024]

A seeded synthetic dataset with all six covariance components; the kernel's
HIP-event time per launch next to two floors: W n^3/3 flops over the f64 MFMA
peak (78.6 TF/s), and the bytes the algorithm has to move through HBM -- each
walker's factor L written once and read once (it does not fit on chip) -- over
the measured HBM rate (6 TB/s).  The third figure is what the
left-looking update reads through the caches: both operand rows of every tile
for every earlier block column.
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
from cosmomc_amd.supernovae import COMPONENTS, JLALikelihood  # noqa: E402

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


if __name__ == "__main__":
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
