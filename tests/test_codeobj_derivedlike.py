"""The derived-likelihood kernel in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_theory_derived.py): one kernel, not one per
width, and with no scratch -- its accumulators stay in registers and the
n-wide loops of the quadratic form run over an LDS column."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


def test_theory_gauss_kernel_present_without_scratch():
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if "theory_gauss_kernel" in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    assert v["scratch"] == 0, (name, v)
