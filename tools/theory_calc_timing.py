#!/usr/bin/env python3
"""Timing of the polynomial theory calculator on the GPU.

  kernel  cmbt_eval at W = 1024, lmax 2508, for fields TT/TE/EE and for all
          ten, K in {1, 28, 210} (one term; quadratic and quartic in six
          parameters): HIP events round a batch of launches after a warm-up;
          bytes written per second against the 6.3 TB/s achievable HBM rate
          and FLOP/s (2 W K N) against the 78.6 TF f64 peak.
  steps   microseconds per cmbs_step_theory step at W = 1024 on the synthetic
          plik_lite problem with theory = A x base: the torch callback
          (trial = base x A, one host call per step) against the one-term
          calculator (no callback), alternating in one process.
  derived cmbt_derived_eval at M = 1024 x 1000 points (a chain block), K = 210,
          24 outputs, next to cmbt_eval of the same 24 columns as one field of
          lmax 23 (theory_calc_kernel's 256-wide l tile on a padded table) for
          the same M: device times from the library's own launch events
          (cmbl_profile_*), and whether the two give the same bits.

Without --part each part runs in a child process of its own under a time
limit, and a part that fails stops the run.  Results: one JSON line per part
on stdout, appended to --out when given.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS, F64_TF = 6.3, 78.6
W, LMAX = 1024, 2508


def _events_us(torch, fn, warmup, iters, repeats=5):
    """Median over `repeats` of the microseconds per call of fn, HIP events round `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(out)[len(out) // 2], min(out), max(out)


def part_kernel():
    import numpy as np
    import torch
    from cosmomc_amd import theory as th
    rng = np.random.default_rng(1)
    n_in = 6
    center, scale = np.zeros(n_in), np.ones(n_in)
    P = torch.tensor(rng.uniform(-1.0, 1.0, size=(n_in, W)), device="cuda")
    out = torch.zeros((W, 10, LMAX + 1), dtype=torch.float64, device="cuda")
    fail = torch.zeros(W, dtype=torch.int32, device="cuda")
    tables = {1: np.array([[1, 0, 0, 0, 0, 0]]), 28: th.monomials(6, 2), 210: th.monomials(6, 4)}
    rows = []
    for fields in ([0, 1, 2], list(range(10))):
        for K, ex in tables.items():
            coef = rng.normal(size=(K, len(fields), LMAX + 1))
            calc = th.PolynomialTheory(list(range(1, n_in + 1)), center, scale, -2 * scale, 2 * scale, ex, fields, coef)
            us, lo, hi = _events_us(torch, lambda: calc.eval(P, out, fail), 10, 50)
            nbytes = W * len(fields) * (LMAX + 1) * 8
            flop = 2.0 * W * K * len(fields) * (LMAX + 1)
            floor = max(nbytes / (HBM_TBS * 1e12), flop / (F64_TF * 1e12)) * 1e6
            rows.append({"fields": len(fields), "K": K, "us": round(us, 2), "us_min": round(lo, 2),
                         "us_max": round(hi, 2), "MB_written": round(nbytes / 1e6, 1),
                         "TB_per_s": round(nbytes / us / 1e6, 3), "TFLOP_per_s": round(flop / us / 1e6, 2),
                         "floor_us": round(floor, 2), "bound": "write" if nbytes / HBM_TBS > flop / F64_TF else "f64",
                         "roofline_fraction": round(floor / us, 3)})
            print(rows[-1], file=sys.stderr, flush=True)
            assert int(fail.sum()) == 0
            calc.close()
    return {"part": "kernel", "W": W, "lmax": LMAX, "hbm_TB_per_s": HBM_TBS, "f64_TFLOP_per_s": F64_TF, "rows": rows}


def part_steps():
    import numpy as np
    import torch
    from cosmomc_amd import synthetic as syn
    from cosmomc_amd import theory as th
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    from cosmomc_amd.sampler import BatchedMCMC
    data = syn.make_plik_lite(12345)
    bh = np.ascontiguousarray(syn.base_theory(LMAX)[:3])
    base = torch.tensor(bh, device="cuda")
    tmp = tempfile.mkdtemp(prefix="tctiming")
    runs = {}
    for mode in ("callback", "native"):
        like = NativeCMBLikelihood("PLIK_LITE", data.write(os.path.join(tmp, mode)))
        like.nuisance_indices = [2]
        theory = base.unsqueeze(0).repeat(W, 1, 1).contiguous()
        trial = torch.empty_like(theory)
        s = BatchedMCMC(W, 2, [1, 2], [[1], [2]], 1, [0.9, 0.9], [1.1, 1.1], [0.0, 1.0], [0.0, 0.0025],
                        oversample_fast=1, propose_scale=2.4, temperature=1.0, seed_ij=71, seed_kl=72)
        s.set_covariance(np.diag([0.002 ** 2, 0.0025 ** 2]))
        s.add_likelihood(like, theory)
        s.set_trial_theory(0, trial)
        s.set_start(np.tile([1.0, 1.0], (W, 1)))
        fn = None
        if mode == "callback":
            def fn(Pt, trial=trial):
                trial.copy_(base.unsqueeze(0) * Pt[0].reshape(-1, 1, 1))
        else:
            calc = th.PolynomialTheory([1], [0.0], [1.0], [0.5], [1.5], [[1]], [0, 1, 2], bh[None])
            s.set_theory_calculator(calc)
            runs["_calc"] = calc
        runs[mode] = (s, fn, like, theory, trial)
    n, res = 100, {"callback": [], "native": []}
    for rep in range(6):                                # alternating; the first round is the warm-up
        for mode in ("callback", "native"):
            s, fn = runs[mode][:2]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s.step_theory(n, theory_fn=fn)
            b.record()
            b.synchronize()
            if rep:
                res[mode].append(a.elapsed_time(b) * 1e3 / n)
    Pa, Pb = runs["callback"][0].state()[0], runs["native"][0].state()[0]
    same = bool(np.array_equal(Pa, Pb))
    med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
    return {"part": "steps", "W": W, "steps_per_call": n,
            "us_per_step": {m: round(med[m], 2) for m in med},
            "us_per_step_all": {m: [round(x, 2) for x in v] for m, v in res.items()},
            "native_over_callback": round(med["native"] / med["callback"], 4), "same_chains": same}


def part_derived():
    import numpy as np
    import torch
    from cosmomc_amd import _native as N
    from cosmomc_amd import theory as th
    rng = np.random.default_rng(2)
    n_in, M, nd = 6, 1024 * 1000, 24
    ex = th.monomials(n_in, 4)
    K = len(ex)
    center, scale = np.zeros(n_in), np.ones(n_in)
    coef = rng.normal(size=(K, 1, nd))
    calc = th.PolynomialTheory(list(range(1, n_in + 1)), center, scale, -2 * scale, 2 * scale, ex, [0], coef)
    P = torch.tensor(rng.uniform(-1.0, 1.0, size=(n_in, M)), device="cuda")
    out = torch.zeros((nd, M), dtype=torch.float64, device="cuda")
    dl = torch.zeros((M, 1, nd), dtype=torch.float64, device="cuda")
    fail = torch.zeros(M, dtype=torch.int32, device="cuda")
    calc.set_derived([f"d{i}" for i in range(nd)], coef[:, 0, :])        # no range: cmbt_eval is one launch
    res = {}
    for name, fn in (("theory_derived_kernel", lambda: calc.derived(P, out=out, fail=fail)),
                     ("theory_calc_kernel", lambda: calc.eval(P, dl, fail))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        N.profile_reset()
        N.profile_enable(True)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        N.profile_enable(False)
        ms, n = N.profile_read(name)
        res[name] = {"launches": n, "us": round(ms * 1e3 / max(n, 1), 1)}
    same = bool(torch.equal(out.T, dl[:, 0, :]))
    calc.close()
    nbytes = (n_in + nd) * M * 8 + M * 4
    return {"part": "derived", "M": M, "K": K, "n_derived": nd, "kernels": res, "same_bits": same,
            "derived_TB_per_s": round(nbytes / res["theory_derived_kernel"]["us"] / 1e6, 3),
            "derived_TFLOP_per_s": round(2.0 * M * K * nd / res["theory_derived_kernel"]["us"] / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["kernel", "steps", "derived"])
    ap.add_argument("--out", help="append the JSON lines to this file")
    ap.add_argument("--timeout", type=int, default=240, help="seconds for each part")
    a = ap.parse_args()
    if a.part:
        print(json.dumps({"kernel": part_kernel, "steps": part_steps, "derived": part_derived}[a.part]()), flush=True)
        return 0
    for part in ("kernel", "steps", "derived"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part], stdout=subprocess.PIPE,
                           text=True, timeout=a.timeout)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"part {part} failed with status {r.returncode}: stopping", file=sys.stderr)
            return r.returncode or 1
        if a.out:
            with open(a.out, "a") as f:
                f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
