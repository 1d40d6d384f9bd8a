"""The tabulated BAO likelihoods (MGS, the DR1x probability grids), HST and the
element abundances on the host: the readers against the fixture of
tests/golden/bao/bao_table.tar.xz and against their formulas restated here,
the ini walk, and the host restatement of the two table forms against the
compiled reference's -lnL.  No GPU."""
import os

import numpy as np
import pytest

import bao_fixture as bf
from cosmomc_amd import derivedlike as dl

BAO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bao")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return bf.extract(tmp_path_factory.mktemp("bao_table"))


@pytest.fixture(scope="module")
def specs(fx):
    return bf.read_all(fx)


def _raw_grid(path):
    return np.loadtxt(path)


# ---------------------------------------------------------------- read_bao_likelihood
def test_dispatch_is_by_tag_not_by_name(fx):
    """MGS -> mgs, DR11CMASS / DR12CMASS / DR12LOWZ -> grid, anything else the
    Gaussian, whatever the file's name key says (bao.f90:91-101)."""
    assert dl.read_bao_likelihood(os.path.join(fx, "sdss_MGS_bao.dataset"), "MGS")["kind"] == "mgs"
    for tag in ("DR11CMASS", "DR12CMASS", "DR12LOWZ"):
        d = dl.read_bao_likelihood(os.path.join(fx, f"syn_{tag}_bao.dataset"), tag)
        assert d["kind"] == "grid" and d["name"] == tag
    # a grid dataset under another grid tag is still a grid: the tag decides
    d = dl.read_bao_likelihood(os.path.join(fx, "syn_DR12LOWZ_bao.dataset"), "DR12CMASS")
    assert d["kind"] == "grid" and d["name"] == "DR12LOWZ" and d["np"] == 3
    # the 6DF file under its own tag, and under any non-grid tag, is the Gaussian
    for tag in ("6DF", "anything"):
        g = dl.read_bao_likelihood(os.path.join(BAO, "sdss_6DF_bao.dataset"), tag)
        assert g["kind"] == "gaussian" and g["name"] == "6DF" and g["types"] == ["rs_over_DV"]
        want = dl.read_bao_dataset(os.path.join(BAO, "sdss_6DF_bao.dataset"))
        assert np.array_equal(g["obs"], want["obs"]) and np.array_equal(g["invcov"], want["invcov"])
    # a Gaussian file whose name key is a grid set's, under a plain tag: the Gaussian
    g = dl.read_bao_likelihood(os.path.join(BAO, "sdss_6DF_bao.dataset"), "sixdf", {"name": "DR12CMASS"})
    assert g["kind"] == "gaussian" and g["name"] == "DR12CMASS"
    # and read_bao_dataset itself still refuses what it refused
    with pytest.raises(ValueError, match="prob_dist"):
        dl.read_bao_dataset(os.path.join(fx, "sdss_MGS_bao.dataset"))
    with pytest.raises(ValueError, match="probability-grid"):
        dl.read_bao_dataset(os.path.join(BAO, "sdss_6DF_bao.dataset"), {"name": "DR12CMASS"})


def test_mgs_table(fx):
    d = dl.read_bao_likelihood(os.path.join(fx, "sdss_MGS_bao.dataset"), "MGS")
    assert d["name"] == "MGS" and d["z"] == 0.15
    t = np.loadtxt(os.path.join(fx, "sdss_MGS_prob.txt"))
    assert d["table"].shape == (399,) and np.array_equal(d["table"], t)
    # the cell width is the default-real 0.001, and the last cell read at alpha_max lies in the table
    assert dl.MGS_STEP == float(np.float32(0.001)) and dl.MGS_STEP != 0.001
    top = int(np.floor((dl.MGS_ALPHA_MAX - dl.MGS_ALPHA_MIN) / dl.MGS_STEP))
    assert top == 397 and top + 1 < 399


@pytest.mark.parametrize("tag", ["DR11CMASS", "DR12CMASS", "DR12LOWZ"])
def test_grid_read_order_and_normalisation(fx, tag):
    """The file's lines run over perp (outer) x plel (inner): prob[i][j] is
    line i np + j, perp[i] that block's first column, plel[j] the second column
    (bao.f90:326-334); prob is divided by its maximum (:341)."""
    d = dl.read_bao_likelihood(os.path.join(fx, f"syn_{tag}_bao.dataset"), tag)
    n = bf.SYNTHETIC[tag][0]
    raw = _raw_grid(os.path.join(fx, f"syn_{tag}.dat"))
    assert d["np"] == n and raw.shape == (n * n, 3)
    assert d["z"] == bf.SYNTHETIC[tag][2]
    for i in (0, 1, n - 1):
        for j in (0, 1, n - 1):
            assert d["perp"][i] == raw[i * n + j, 0] and d["plel"][j] == raw[i * n + j, 1]
            assert d["prob"][i, j] == raw[i * n + j, 2] / raw[:, 2].max()
    assert d["prob"].max() == 1.0 and d["prob"].min() >= 0.0
    assert not np.array_equal(d["prob"], d["prob"].T)              # a transposed read would show
    assert np.all(np.diff(d["perp"]) > 0) and np.all(np.diff(d["plel"]) > 0)
    if n >= 4:                                                     # 9-digit prints: not uniform
        assert len(set(np.diff(d["perp"]))) > 1
    if n >= 40:
        i, j = bf.ZERO_CELL
        assert np.all(d["prob"][i:i + 2, j:j + 2] == 0) and np.sum(d["prob"] == 0) > 4
        assert bf.floor_search_disagree(d["perp"]) and bf.floor_search_disagree(d["plel"])


def test_both_fiducial_key_sets_and_overrides(fx, specs):
    """Hrd_fid + DA_rd_fid as given; else H_fid rd_fid and DA_fid / rd_fid
    (bao.f90:141-150); a bao_dataset[TAG,key] setting wins over the file's."""
    a = dl.read_bao_likelihood(os.path.join(fx, "syn_DR11CMASS_bao.dataset"), "DR11CMASS")
    assert a["Hrd_fid"] == 93.558 * 149.28 and a["DA_rd_fid"] == 1359.72 / 149.28
    b = dl.read_bao_likelihood(os.path.join(fx, "syn_DR12CMASS_bao.dataset"), "DR12CMASS")
    assert b["Hrd_fid"] == 13827.0 and b["DA_rd_fid"] == 9.330
    c = dl.read_bao_likelihood(os.path.join(fx, "syn_DR12LOWZ_bao.dataset"), "DR12LOWZ")
    assert c["Hrd_fid"] == 11914.0 and c["DA_rd_fid"] == 6.667
    assert specs["DR12LOWZ"]["DA_rd_fid"] == float(bf.LOWZ_DA_RD_FID_SETTING)      # through the ini's setting
    # Hrd_fid + DA_rd_fid win when both sets are there
    d = dl.read_bao_likelihood(os.path.join(fx, "syn_DR11CMASS_bao.dataset"), "DR11CMASS",
                               {"Hrd_fid": "14000", "DA_rd_fid": "9"})
    assert d["Hrd_fid"] == 14000.0 and d["DA_rd_fid"] == 9.0


def test_refusals_name_the_key(fx, tmp_path):
    with pytest.raises(ValueError, match="prob_dist"):             # a table under a tag that reads none
        dl.read_bao_likelihood(os.path.join(fx, "sdss_MGS_bao.dataset"), "MGS2")
    with pytest.raises(ValueError, match="dilation"):
        dl.read_bao_likelihood(os.path.join(BAO, "sdss_6DF_bao.dataset"), "6DF", {"measurement_type": "dilation"})
    with pytest.raises(ValueError, match="prob_dist"):             # a grid tag without its table
        dl.read_bao_likelihood(os.path.join(BAO, "sdss_6DF_bao.dataset"), "MGS")
    p = tmp_path / "nofid.dataset"
    p.write_text("name = X\nzeff = 0.5\nalpha_npoints = 3\nprob_dist = %s\nH_fid = 90\n"
                 % os.path.join(fx, "syn_DR12LOWZ.dat"))
    with pytest.raises(ValueError, match="Hrd_fid and DA_rd_fid, or rd_fid, H_fid and DA_fid"):
        dl.read_bao_likelihood(str(p), "DR12LOWZ")
    with pytest.raises(ValueError, match="alpha_npoints"):
        dl.read_bao_likelihood(os.path.join(fx, "sdss_MGS_bao.dataset"), "DR12CMASS")
    with pytest.raises(ValueError, match="Error reading BAO file"):  # fewer lines than np x np
        dl.read_bao_likelihood(os.path.join(fx, "syn_DR12LOWZ_bao.dataset"), "DR12LOWZ", {"alpha_npoints": "4"})


def test_bao_alpha_theory():
    DV, DA, H, rd = np.array([640.0, 650.0]), np.array([1350.0, 1360.0]), np.array([93.0, 94.0]), np.array([147.1, 148.2])
    assert np.array_equal(dl.bao_alpha_theory("mgs", 0.15, DV=DV, rdrag=rd), DV / rd)
    t = dl.bao_alpha_theory("grid", 0.57, DA=DA, H=H, rdrag=rd)
    assert t.shape == (2, 2) and np.array_equal(t[:, 0], DA / rd) and np.array_equal(t[:, 1], H * rd)
    with pytest.raises(ValueError):
        dl.bao_alpha_theory("gaussian", 0.1, DV=DV, rdrag=rd)


# ---------------------------------------------------------------- HST and abundances
def test_hst(tmp_path):
    from cosmomc_amd.ini import IniFile
    riess = "Hubble_zeff = 0\nHubble_H0 = 73.45\nHubble_H0_err = 1.66\nHubble_name = H073p45\nuse_HST=T\n"
    h = dl.read_hst(IniFile(text=riess))
    assert h == {"name": "H073p45", "H0": 73.45, "H0_err": 1.66, "zeff": 0.0, "angconversion": 11425.8}
    assert dl.read_hst(IniFile(text="use_HST = F\nHubble_H0 = 70\n")) is None
    d = dl.read_hst(IniFile(text="use_HST = T\nHubble_name = x\nHubble_H0 = 70.6\nHubble_H0_err = 3.3\n"))
    assert d["zeff"] == 0.04 and d["angconversion"] == 11425.8
    e = dl.read_hst(IniFile(text="use_HST = T\nHubble_name = x\nHubble_H0 = 70\nHubble_H0_err = 3\n"
                                 "Hubble_zeff = 0.1\nHubble_angconversion = 11000\n"))
    assert e["zeff"] == 0.1 and e["angconversion"] == 11000.0
    with pytest.raises(ValueError, match="Hubble_H0_err"):
        dl.read_hst(IniFile(text="use_HST = T\nHubble_name = x\nHubble_H0 = 70\n"))
    # HST_LnLike: zeff > 0: angconversion / D_A(zeff); else H0
    DA, H0 = np.array([160.0, 161.5]), np.array([67.0, 68.0])
    assert np.array_equal(dl.hst_theory(0.04, 11425.8, DA=DA, H0=H0), 11425.8 / DA)
    assert np.array_equal(dl.hst_theory(0.0, 11425.8, DA=DA, H0=H0), H0)


def test_abundance(fx):
    """(theory + offset - mean)^2 / (2 (error^2 + terr^2)) as obs and std."""
    d = dl.read_abundance_dataset(os.path.join(fx, "D_Cooke2017.dataset"))
    assert d["measurement"] == "D/H" and d["theory_table"] == "PArthENoPE_880.2_standard.dat"
    assert d["obs"] == 2.527e-5 - (-0.091e-5) and d["std"] == np.sqrt(0.030e-5 ** 2 + 0.089e-5 ** 2)
    theory = 2.6e-5
    want = (theory + d["theory_bias_offset"] - d["mean"]) ** 2 / (2 * (d["error"] ** 2 + d["theory_effective_error"] ** 2))
    got = (theory - d["obs"]) ** 2 / d["std"] ** 2 / 2
    assert abs(got - want) <= 4 * 2.0 ** -52 * want
    y = dl.read_abundance_dataset(os.path.join(fx, "Yp_Aver2015.dataset"))
    assert y["measurement"] == "Yp" and y["obs"] == 0.2449 and y["std"] == np.sqrt(0.0040 ** 2 + 0.0003 ** 2)
    # without BBN consistency Yp reads no theory key; D/H is refused
    y0 = dl.read_abundance_dataset(os.path.join(fx, "Yp_Aver2015.dataset"), bbn_consistency=False)
    assert y0["obs"] == 0.2449 and y0["std"] == 0.0040
    with pytest.raises(ValueError, match="requires BBN consistency"):
        dl.read_abundance_dataset(os.path.join(fx, "D_Cooke2017.dataset"), bbn_consistency=False)
    with pytest.raises(ValueError, match="theory_effective_error"):
        dl.read_abundance_dataset(os.path.join(fx, "D_Cooke2017.dataset"), {"theory_effective_error": "0"})
    with pytest.raises(ValueError, match="measurement"):
        dl.read_abundance_dataset(os.path.join(fx, "D_Cooke2017.dataset"), {"measurement": "Li7"})
    o = dl.read_abundance_dataset(os.path.join(fx, "D_Cooke2017.dataset"), {"mean": "2.5e-5"})
    assert o["mean"] == 2.5e-5


# ---------------------------------------------------------------- the ini walk
def batch3_ini(fx, tmp_path, extra="", hst=True):
    """An ini equivalent to batch3/BAO.ini + HST_Riess2018.ini + Cooke17BBN.ini
    with the fixtures' paths: the DR12 consensus set comes in by DEFAULT, as
    batch3/BAO.ini takes DR12_BAO_consensus.ini."""
    (tmp_path / "DR12_BAO_consensus.ini").write_text(
        "use_BAO=T\nbao_dataset[DR12BAO] = %s\n" % os.path.join(BAO, "DR12", "sdss_DR12Consensus_bao.dataset"))
    p = tmp_path / "run.ini"
    p.write_text("use_BAO=T\nDEFAULT(DR12_BAO_consensus.ini)\n"
                 "bao_dataset[6DF] = %s\nbao_dataset[MGS] = %s\n"
                 "Hubble_zeff = 0\nHubble_H0 = 73.45\nHubble_H0_err = 1.66\nHubble_name = H073p45\nuse_HST=%s\n"
                 "abundance_dataset[Cooke17]= %s\n%s"
                 % (os.path.join(BAO, "sdss_6DF_bao.dataset"), os.path.join(fx, "sdss_MGS_bao.dataset"),
                    "T" if hst else "F", os.path.join(fx, "D_Cooke2017.dataset"), extra))
    return str(p)


def test_specs_from_a_batch3_ini(fx, tmp_path):
    """The reference's order (abundances, HST, BAO in the ini's key order) and
    names: chi2_Cooke17, chi2_H073p45, chi2_6DF, chi2_MGS, chi2_DR12BAO."""
    s = dl.derived_likelihood_specs(batch3_ini(fx, tmp_path))
    assert [(d["name"], d["kind"]) for d in s] == [("Cooke17", "prior"), ("H073p45", "prior"), ("6DF", "gaussian"),
                                                   ("MGS", "mgs"), ("DR12BAO", "gaussian")]
    assert s[0]["obs"] == 2.527e-5 + 0.091e-5 and s[1]["obs"] == 73.45 and s[1]["std"] == 1.66
    assert s[3]["table"].shape == (399,) and s[4]["obs"].shape == (6,) and s[4]["dataset_name"] == "DR12BAO"
    assert s[2]["rs_rescale"] == 1.027369826
    only = dl.derived_likelihood_specs(batch3_ini(fx, tmp_path, hst=False))
    assert [d["name"] for d in only] == ["Cooke17", "6DF", "MGS", "DR12BAO"]
    with pytest.raises(ValueError, match="BAO_fixed_rs"):
        dl.derived_likelihood_specs(batch3_ini(fx, tmp_path, "BAO_fixed_rs = 147.5\n"))
    # a [TAG,key] setting reaches the reader
    s = dl.derived_likelihood_specs(batch3_ini(fx, tmp_path, "bao_dataset[6DF,rs_rescale] = 1.5\n"))
    assert s[2]["rs_rescale"] == 1.5
    (tmp_path / "none.ini").write_text("use_BAO = T\n")
    with pytest.raises(ValueError, match="no bao_dataset"):
        dl.derived_likelihood_specs(str(tmp_path / "none.ini"))
    (tmp_path / "off.ini").write_text("use_BAO = F\nbao_dataset[MGS] = nowhere.dataset\n")
    assert dl.derived_likelihood_specs(str(tmp_path / "off.ini")) == []


# ---------------------------------------------------------------- the restatement against the goldens
@pytest.mark.parametrize("ini", list(bf.INIS))
def test_host_restatement_meets_the_goldens(fx, ini):
    """The f64 restatement against the compiled reference: MGS bit for bit (+,
    -, /, floor and a mean, all in the reference's order); the grids to a few
    ulp of -lnL's ingredients (the two logs may differ), with every logZero
    outcome the same.  Prints (a) and (b), the figures the GPU bound is made of."""
    err = bf.host_errors(fx, ini)
    assert set(err) == set(bf.TAGS[ini])
    for tag, e in err.items():
        print(f"{ini} {tag}: {e['n']} finite, {e['nzero']} logZero; (a) f64 - golden {e['a']:.3e}, "
              f"(b) f64 - long double {e['b']:.3e}")
        assert e["same"], f"{tag}: a logZero outcome differs"
        assert e["n"] >= 8 and e["nzero"] >= 2
        if tag == "MGS":
            assert e["a"] == 0.0 and e["b"] <= 2.0 ** -51          # (b): the one rounding of the mean of two entries < 16
        else:
            # -lnL = -log(prob): prob carries some 10 roundings of terms up to 1 / min(prob) ~ 1e3 times its
            # size where the cell is steep, so 1e-12 absolute is generous and still 1e-12 of a unit of chi^2
            assert e["a"] <= 1e-12 and e["b"] <= 1e-12


def test_fixture_has_the_edge_cases(fx, specs):
    """The cases the GPU test leans on are what their labels say."""
    cases = {c["label"]: c for c in bf.load_cases(fx)}
    scale = dl.MGS_DVFID / dl.MGS_RSFID
    assert cases["MGS:at_x_min"]["DV"] / scale == dl.MGS_ALPHA_MIN and cases["MGS:at_x_min"]["ref"] < 1e29
    assert cases["MGS:at_x_max"]["DV"] / scale == dl.MGS_ALPHA_MAX and cases["MGS:at_x_max"]["ref"] < 1e29
    lo, hi = cases["MGS:below_x_min"]["DV"], cases["MGS:above_x_max"]["DV"]     # the nearest doubles outside
    assert lo / scale < dl.MGS_ALPHA_MIN <= np.nextafter(lo, np.inf) / scale
    assert hi / scale > dl.MGS_ALPHA_MAX >= np.nextafter(hi, -np.inf) / scale
    assert cases["MGS:below_x_min"]["ref"] == 1e30 and cases["MGS:above_x_max"]["ref"] == 1e30
    for tag in ("DR11CMASS", "DR12CMASS", "DR12LOWZ"):
        d = specs[tag]
        n = d["np"]
        c = cases[f"{tag}:corner_hi_hi"]
        assert c["DA"] / d["DA_rd_fid"] == d["perp"][n - 2] and d["Hrd_fid"] / c["H"] == d["plel"][n - 2]
        assert c["ref"] < 1e29
        c = cases[f"{tag}:perp_hi_beyond"]
        assert c["DA"] / d["DA_rd_fid"] > d["perp"][n - 2] >= np.nextafter(c["DA"], -np.inf) / d["DA_rd_fid"]
        assert c["ref"] == 1e30
        c = cases[f"{tag}:plel_hi_beyond"]                         # (a_plel falls as v1 grows)
        assert d["Hrd_fid"] / c["H"] > d["plel"][n - 2] >= d["Hrd_fid"] / np.nextafter(c["H"], np.inf)
        assert c["ref"] == 1e30
        assert cases[f"{tag}:v1_zero"]["ref"] == 1e30 and cases[f"{tag}:v1_negative"]["ref"] == 1e30
    d = specs["DR11CMASS"]
    assert cases["DR11CMASS:zero_cell"]["ref"] == 1e30 and cases["DR11CMASS:beside_zero_cell"]["ref"] < 1e29
    c = cases["DR11CMASS:floor_vs_search_perp"]
    a = c["DA"] / d["DA_rd_fid"]
    assert bf.floor_cell(d["perp"], a) != bf.search_cell(d["perp"], a) and c["ref"] < 1e29
    c = cases["DR11CMASS:floor_vs_search_plel"]
    b = d["Hrd_fid"] / c["H"]
    assert bf.floor_cell(d["plel"], b) != bf.search_cell(d["plel"], b) and c["ref"] < 1e29
