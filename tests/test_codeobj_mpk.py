"""The galaxy power-spectrum kernels in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_sz.py): each present once, and the
contraction kernel with no scratch -- a wave's eight 16 x 16 f64 tiles of the
two products stay in registers.  Nothing else is inspected."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


@pytest.mark.parametrize("kernel", ["mpk_prologue_kernel", "mpk_contract_kernel"])
def test_mpk_kernel_present(kernel):
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if kernel in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    if kernel == "mpk_contract_kernel":
        assert v["scratch"] == 0, (name, v)
