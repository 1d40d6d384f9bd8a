"""The tabulated-likelihood kernel in the built library's gfx950 code object
(tools/codeobj.py, as test_codeobj_derivedlike.py): one kernel for both forms,
with no scratch and no static LDS -- its only LDS is the dynamic n_in x TD_TM
doubles of scaled inputs the launch asks for, as theory_derived_kernel's -- and
few enough registers for full occupancy."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "cosmomc_amd", "lib", "libcosmomc_amd.so")


def test_theory_table_kernel_present_without_scratch_or_static_lds():
    if not os.path.exists(LIB):
        pytest.skip("libcosmomc_amd.so not built (make -C cosmomc_amd/csrc)")
    import codeobj
    k = {n: v for n, v in codeobj.kernels(LIB).items() if "theory_table_kernel" in n}
    assert len(k) == 1, sorted(k)
    (name, v), = k.items()
    print(name, v)
    assert v["scratch"] == 0, (name, v)
    assert v["lds"] == 0, (name, v)                  # static LDS: none; the launch gives n_in x TD_TM doubles
    assert v["agpr"] == 0 and v["vgpr"] <= 64, (name, v)   # 8 waves a SIMD
    with open(os.path.join(ROOT, "cosmomc_amd", "csrc", "theorycalc.hip")) as f:
        src = f.read()
    launch = src[src.index('timed_launch("theory_table_kernel"'):]
    assert "td_lds_bytes(t->n_in)" in launch[:launch.index("HIP_CHECK")]
