"""The weak-lensing kernels in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_jla.py): each present once and with no
scratch -- the MFMA operands and the spline's few values stay in registers.
Nothing else is inspected."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


@pytest.mark.parametrize("kernel", ["wl_kernel_q", "wl_kernel_corr", "wl_kernel_finish"])
def test_wl_kernel_present_without_scratch(kernel):
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if kernel in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    assert v["scratch"] == 0, (name, v)
