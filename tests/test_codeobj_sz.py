"""The SZ cluster-counts kernels in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_wl.py): each present once, and the hot one,
sz_compl_kernel, with no scratch -- its five accumulators and the point's few
values stay in registers.  Nothing else is inspected."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


@pytest.mark.parametrize("kernel", ["sz_erfs_kernel", "sz_compl_kernel", "sz_compl0_kernel", "sz_counts_kernel"])
def test_sz_kernel_present(kernel):
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if kernel in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    if kernel == "sz_compl_kernel":
        assert v["scratch"] == 0, (name, v)
