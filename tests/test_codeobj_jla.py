"""The JLA factorisation kernel in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_derivedlike.py): present, one kernel, and
with no scratch -- the 16-wide rows of the diagonal Cholesky and of the forward
substitution stay in registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


def test_jla_chol_kernel_present_without_scratch():
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if "jla_chol_kernel" in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    assert v["scratch"] == 0, (name, v)
    assert v["lds"] <= 64 * 1024, (name, v)      # fixed: it does not grow with nsn
