"""The unified step launch's register budget, read from the built library's
code-object metadata on the CPU (tools/codeobj.py): 168 VGPRs is the most at
which three 256-thread workgroups share a CU (512 / 168 = 3 waves per SIMD),
which the launch's slot count assumes, and the kernels'
scratch stays at the 32 bytes they had before the raw sums went bin-major."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")

MAX_VGPR = 168
MAX_SCRATCH = 32


def test_step_kernels_keep_three_workgroups_per_cu():
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    step = {n: k for n, k in codeobj.kernels(LIB).items() if "mh_step_kernel" in n or "mh_tail_kernel" in n}
    assert len(step) == 5, sorted(step)      # mh_step_kernel x 3 and mh_tail_kernel x 2 (accept / propose forms)
    for n, k in step.items():
        assert k["vgpr"] + k["agpr"] <= MAX_VGPR, (n, k)
        assert k["scratch"] <= MAX_SCRATCH, (n, k)
