"""The CMBlikes dataset reader's refusals (CMBLikes_ReadIni, CMBlikes.f90:466-749,
and the TSmica_planck / TBK_planck ReadIni that follow it).  No GPU: cmbl_open
on a dataset the reader refuses returns its code and message before any
device call.  Each case is a synthetic exact (unbinned) or SMICA (binned TT)
dataset plus override text, the TIniFile%Override of cmbl_open."""
import ctypes as C

import pytest

from cosmomc_amd import _native as N
from cosmomc_amd import synthetic as syn

FORMAT, UNSUPPORTED = -3, -6
EXACT_LMAX = 40


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    d = tmp_path_factory.mktemp("loader")
    exact = syn.make_exact(lmax=EXACT_LMAX).write(str(d / "exact"))
    smica = syn.make_smica().write(str(d / "smica"))
    # the same exact dataset without its 'binned' line, and with keys appended through extra=
    nobinned = d / "exact" / "exact_nobinned.dataset"
    nobinned.write_text("".join(l for l in open(exact) if not l.startswith("binned")))
    extra = syn.make_exact(lmax=EXACT_LMAX).write(str(d / "exact_extra"), extra={"point_source_cl": "ps.dat"})
    (d / "smica" / "short.paramnames").write_text("A1_smica  A_1\nn1_smica  n_1\nn1run_smica  n_r\n")
    return {"exact": exact, "smica": smica, "nobinned": str(nobinned), "extra": extra}


# (id, tag, dataset, override text, return code, substring of the message)
CASES = [
    ("exact_binned", "X", "exact", "binned = T\n", FORMAT, "exact like cannot be binned"),
    ("binned_absent", "X", "nobinned", "", FORMAT, "binned not given"),
    ("unknown_approx", "X", "exact", "like_approx = pseudo\n", FORMAT, "unknown like_approx pseudo"),
    ("smica_exact", "SMICA", "smica", "like_approx = exact\n", UNSUPPORTED, "SMICA with like_approx = exact"),
    ("bk_exact", "BKPLANCK", "smica", "like_approx = exact\n", UNSUPPORTED, "BKPLANCK with like_approx = exact"),
    ("unbinned_gaussian", "X", "exact", "like_approx = gaussian\n", UNSUPPORTED, "unbinned HL / gaussian"),
    ("unbinned_use_max", "X", "exact", f"use_max = {EXACT_LMAX + 1}\n", FORMAT,
     "use_min/use_max outside cl_lmin..cl_lmax"),
    ("binned_use_max", "SMICA", "smica", "use_max = 55\n", FORMAT, "use_min/use_max outside 1..nbins"),
    ("binned_use_min", "SMICA", "smica", "use_min = 0\n", FORMAT, "use_min/use_max outside 1..nbins"),
    ("maps_use_unknown", "X", "exact", "maps_use = T Q\n", FORMAT, "maps_use item not found - Q"),
    ("fields_required_with_map_names", "X", "exact",
     "map_names = T1 E1 B1\nmap_fields = T E B\nfields_required = T1\n", FORMAT,
     "use maps_required not fields_required"),
    ("map_fields_count", "X", "exact", "map_names = T1 E1 B1\nmap_fields = T E\n", FORMAT,
     "number of map_fields does not match map_names"),
    ("point_source_cl", "X", "extra", "", FORMAT, "keywords no longer supported"),
    ("old_format", "X", "exact", "dataset_format = CMBLike\n", FORMAT, "dataset_format now CMBLike2"),
    ("wrong_format", "X", "exact", "dataset_format = WMAP\n", FORMAT, "wrong dataset_format"),
    ("cl_hat_short", "X", "exact", f"cl_lmax = {EXACT_LMAX + 10}\n", FORMAT,
     f"C_l file does not go up to maximum used: {EXACT_LMAX + 10}"),
    ("smica_few_nuisance", "SMICA", "smica", "nuisance_params = short.paramnames\n", FORMAT,
     "nuisance_params needs the foreground parameters A1 n1 n1run A2 n2"),
    ("smica_cal_derived", "SMICA", "smica", "calibration_paramname = Dl2000_smica\n", FORMAT,
     "calibration_paramname Dl2000_smica is a derived parameter"),
]


@pytest.mark.parametrize("tag,which,override,code,text", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_reader_refuses(datasets, tag, which, override, code, text):
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = N.lib().cmbl_open(tag.encode(), datasets[which].encode(), override.encode() or None, C.byref(h), err, 512)
    assert (rc, not h.value) == (code, True), err.value
    assert text.encode() in err.value, err.value
