"""cosmomc_amd.derivedlike on the host: the reference's Gaussian BAO dataset
files (fixtures under tests/golden/bao, data only) through read_bao_dataset,
the refusal of what is not a plain Gaussian, and bao_theory against the
formulas of BAO_LnLike written out by hand.  No GPU."""
import os

import numpy as np
import pytest

from cosmomc_amd.derivedlike import BAO_TYPES, bao_theory, read_bao_dataset

BAO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bao")


def test_6df():
    d = read_bao_dataset(os.path.join(BAO, "sdss_6DF_bao.dataset"))
    assert d["name"] == "6DF" and d["types"] == ["rs_over_DV"]
    assert d["z"].tolist() == [0.106] and d["obs"].tolist() == [0.336]
    assert d["invcov"].shape == (1, 1) and d["invcov"][0, 0] == 1 / 0.015 ** 2
    assert d["rs_rescale"] == 1.027369826


def test_wigglez():
    d = read_bao_dataset(os.path.join(BAO, "wigglez_bao.dataset"))
    assert d["name"] == "WiggleZ" and d["types"] == ["Az"] * 3 and d["rs_rescale"] == 1.0
    assert d["z"].tolist() == [0.44, 0.60, 0.73] and d["obs"].tolist() == [0.474, 0.442, 0.424]
    want = np.array([[1040.3, -807.5, 336.8], [-807.5, 3720.3, -1551.9], [336.8, -1551.9, 2914.9]])
    assert np.array_equal(d["invcov"], want)


def test_dr12_consensus():
    d = read_bao_dataset(os.path.join(BAO, "DR12", "sdss_DR12Consensus_bao.dataset"))
    assert d["name"] == "DR12BAO" and d["types"] == ["DM_over_rs", "bao_Hz_rs"] * 3
    assert d["z"].tolist() == [0.38, 0.38, 0.51, 0.51, 0.61, 0.61]
    assert d["obs"].tolist() == [1512.39, 81.2087, 1975.22, 90.9029, 2306.68, 98.9647]
    assert d["rs_rescale"] == .6766815537e-2
    cov = np.loadtxt(os.path.join(BAO, "DR12", "BAO_consensus_covtot_dM_Hz.txt"))
    assert cov.shape == (6, 6) and cov[0, 0] == 624.707 and cov[5, 4] == 40.4327
    inv = np.linalg.inv(cov)
    assert np.array_equal(d["invcov"], (inv + inv.T) / 2)
    assert np.array_equal(d["invcov"], d["invcov"].T)
    assert np.allclose(d["invcov"] @ cov, np.eye(6), atol=1e-12)


def test_overrides_win():
    d = read_bao_dataset(os.path.join(BAO, "sdss_6DF_bao.dataset"), {"rs_rescale": "1.0", "name": "six"})
    assert d["rs_rescale"] == 1.0 and d["name"] == "six"


def test_mgs_refused():
    with pytest.raises(ValueError, match="prob_dist"):
        read_bao_dataset(os.path.join(BAO, "sdss_MGS_bao.dataset"))


def test_grids_and_dilation_refused(tmp_path):
    p = tmp_path / "grid.dataset"
    p.write_text("name = DR12CMASS\nmeasurement_type = DV_over_rs\nzeff = 0.57\nbao_measurement = 13.7 0.1\n")
    with pytest.raises(ValueError, match="DR12CMASS"):
        read_bao_dataset(str(p))
    p.write_text("name = other\nmeasurement_type = dilation\nzeff = 0.57\nbao_measurement = 1.0 0.1\n")
    with pytest.raises(ValueError, match="dilation"):
        read_bao_dataset(str(p))


# two design points, two redshifts
Z = np.array([0.38, 0.61])
DV = np.array([[1477.0, 2140.5], [1501.25, 2170.0]])
DA = np.array([[1108.5, 1412.75], [1120.0, 1431.5]])
H = np.array([[81.5, 97.25], [83.0, 99.5]])
FS8 = np.array([[0.47, 0.45], [0.48, 0.44]])
RD = np.array([147.5, 149.25])
OMH2 = np.array([0.1425, 0.14])
RESC = 1.027369826
CKM = 299792.458


@pytest.mark.parametrize("tp", [t for t in BAO_TYPES if t != "dilation"])
def test_bao_theory_by_hand(tp):
    """Every type of BAO_LnLike's select case (bao.f90:274-301), the formula
    written out here, at two redshifts and two design points."""
    got = bao_theory([tp, tp], Z, RESC, DV=DV, DA=DA, H=H, rdrag=RD, omegam_h2=OMH2, fsigma8=FS8)
    assert got.shape == (2, 2)
    for m in range(2):
        rs = RD[m] * RESC
        for j in range(2):
            z = Z[j]
            want = {"Az": 100 * DV[m, j] * np.sqrt(OMH2[m]) / (CKM * z),
                    "DV_over_rs": DV[m, j] / rs,
                    "rs_over_DV": rs / DV[m, j],
                    "DA_over_rs": DA[m, j] / rs,
                    "F_AP": (1 + z) * DA[m, j] * (H[m, j] / CKM),
                    "f_sigma8": FS8[m, j],
                    "bao_Hz_rs": H[m, j] * rs,
                    "bao_Hz_rs_103": H[m, j] * rs * 1.0e-3,
                    "DM_over_rs": (1 + z) * DA[m, j] / rs}[tp]
            assert got[m, j] == pytest.approx(want, rel=4e-16), (tp, m, j)


def test_bao_theory_mixed_types_and_refusals():
    got = bao_theory(["DM_over_rs", "bao_Hz_rs"], Z, RESC, DV=DV, DA=DA, H=H, rdrag=RD, omegam_h2=OMH2)
    assert got[1, 0] == pytest.approx((1 + Z[0]) * DA[1, 0] / (RD[1] * RESC), rel=4e-16)
    assert got[1, 1] == pytest.approx(H[1, 1] * RD[1] * RESC, rel=4e-16)
    with pytest.raises(ValueError):
        bao_theory(["dilation", "Az"], Z, RESC, DV=DV, DA=DA, H=H, rdrag=RD, omegam_h2=OMH2)
    with pytest.raises(ValueError):
        bao_theory(["f_sigma8", "Az"], Z, RESC, DV=DV, DA=DA, H=H, rdrag=RD, omegam_h2=OMH2)
