"""The kernels of the marginalised JLA likelihood in the built library's gfx950
code object (tools/codeobj.py, as test_codeobj_jla.py): present, one of each,
no scratch, and LDS that is fixed at compile time -- it grows neither with nsn
nor with the grid."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")

KERNELS = ["jla_marge_chol_kernel", "jla_marge_inv_kernel", "jla_marge_consts_kernel", "jla_marge_pro_kernel",
           "jla_marge_qf_kernel", "jla_marge_chi_kernel", "jla_marge_fin_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_present_without_scratch(kernel):
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if kernel in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    assert v["scratch"] == 0, (name, v)
    assert v["lds"] <= 64 * 1024, (name, v)      # static LDS only: no launch passes a dynamic size
    if kernel == "jla_marge_qf_kernel":
        assert v["lds"] > 0 and v["vgpr"] + v["agpr"] <= 256, (name, v)     # two waves a SIMD
