"""The tabulated-BAO goldens (tests/golden/bao/bao_table.tar.xz): how its inputs
are made (make_fixture, called by tools/bao_make_fixture.py), how tests read it
(extract, load_cases) and the host restatement of the two likelihoods
(bao_table_loglike_host).

The archive holds, under bao/: the real MGS dataset with its chi^2 table, three
seeded synthetic probability grids under the tags DR11CMASS (40 knots, the
rd_fid / H_fid / DA_fid keys), DR12CMASS (4 knots) and DR12LOWZ (3 knots, the
dilation type both, with a bao_dataset[DR12LOWZ,DA_rd_fid] setting in the ini),
the real DR11 CMASS consensus grid (280 knots) with an ini of its own, two
abundance datasets, and per ini cases*.txt (what the harness reads), labels*.txt
(a name per case) and ref*.txt (the compiled reference's -lnL,
tools/bao_ref_harness.f90).  A case is "k DV DA H rdrag": with rdrag = 1 the
surfaces D_V / r_d, D_A / r_d and H r_d are DV, DA and H bit for bit, which is
how the edge cases name an exact alpha."""
import io
import lzma
import os
import tarfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bao", "bao_table.tar.xz")
LOGZERO = 1e30
INIS = {"bao.ini": ("cases.txt", "labels.txt", "ref.txt"),
        "bao_dr11.ini": ("cases_dr11.txt", "labels_dr11.txt", "ref_dr11.txt")}
TAGS = {"bao.ini": ["MGS", "DR11CMASS", "DR12CMASS", "DR12LOWZ"], "bao_dr11.ini": ["DR11CMASS"]}
# the synthetic grids: tag -> (alpha_npoints, seed, zeff, fiducial keys, measurement lines)
SYNTHETIC = {
    "DR11CMASS": (40, 11, 0.57, "rd_fid = 149.28\nH_fid = 93.558\nDA_fid = 1359.72\n",
                  "measurement_type = DV_over_rs\nbao_measurement = 13.773  0.134\n"),
    "DR12CMASS": (4, 12, 0.57, "Hrd_fid = 13827\nDA_rd_fid = 9.330\n", "measurement_type = dilation\n"),
    "DR12LOWZ": (3, 13, 0.32, "Hrd_fid = 11914.0\nDA_rd_fid = 6.667\n", "measurement_type = dilation\n"),
}
LOWZ_DA_RD_FID_SETTING = "6.5"                       # bao_dataset[DR12LOWZ,DA_rd_fid]
ZERO_CELL = (5, 7)                                   # the DR11CMASS grid's cell whose four corners are 0


# ---------------------------------------------------------------- the restatement
def bao_table_loglike_host(d, v0, v1=None, dtype=np.float64):
    """-lnL of a tabulated BAO likelihood (a dict of read_bao_likelihood) at the
    surface values v0 (D_V / r_d, or D_A / r_d) and v1 (H r_d), one operation a
    rounding of `dtype` (np.float64 or np.longdouble) in bao.f90's order
    (:401-407, :357-374).  The inputs are the same doubles in both."""
    from cosmomc_amd import derivedlike as dl
    T = dtype
    if d["kind"] == "mgs":
        scale = T(dl.MGS_DVFID) / T(dl.MGS_RSFID)
        alpha = T(v0) / scale
        if alpha > T(dl.MGS_ALPHA_MAX) or alpha < T(dl.MGS_ALPHA_MIN):
            return T(LOGZERO)
        ii = int(np.floor((alpha - T(dl.MGS_ALPHA_MIN)) / T(dl.MGS_STEP)))
        chi2 = (T(d["table"][ii]) + T(d["table"][ii + 1])) / T(2)
        return chi2 / T(2)
    perp, plel, prob = d["perp"].astype(T), d["plel"].astype(T), d["prob"].astype(T)
    n = d["np"]
    with np.errstate(divide="ignore"):
        a, b = T(v0) / T(d["DA_rd_fid"]), T(d["Hrd_fid"]) / T(v1)
    if a < perp[0] or a > perp[n - 2] or b < plel[0] or b > plel[n - 2]:
        return T(LOGZERO)
    i = int(np.floor((a - perp[0]) / (perp[1] - perp[0])))
    j = int(np.floor((b - plel[0]) / (plel[1] - plel[0])))
    p = (T(1) / ((perp[i + 1] - perp[i]) * (plel[j + 1] - plel[j]))) * (
        prob[i, j] * (perp[i + 1] - a) * (plel[j + 1] - b)
        - prob[i + 1, j] * (perp[i] - a) * (plel[j + 1] - b)
        - prob[i, j + 1] * (perp[i + 1] - a) * (plel[j] - b)
        + prob[i + 1, j + 1] * (perp[i] - a) * (plel[j] - b))
    return -np.log(p) if p > 0 else T(LOGZERO)


def surfaces_of(DV, DA, H, rd, kind):
    """The surface values the reference forms from a case, in f64 (one IEEE
    operation each): D_V / r_d, or D_A / r_d and H r_d."""
    DV, DA, H, rd = (np.float64(x) for x in (DV, DA, H, rd))
    with np.errstate(all="ignore"):
        return (DV / rd, None) if kind == "mgs" else (DA / rd, H * rd)


def floor_cell(knots, a):
    return int(np.floor((a - knots[0]) / (knots[1] - knots[0])))


def search_cell(knots, a):
    return int(np.searchsorted(knots, a, side="right")) - 1


def floor_search_disagree(knots):
    """Points inside [knot[0], knot[np - 2]] at which floor((a - knot[0]) /
    (knot[1] - knot[0])) and a search of the knots name different cells: the
    middle of the gap between knot[i] and knot[0] + i (knot[1] - knot[0]),
    wherever the 9-digit prints leave one."""
    d = knots[1] - knots[0]
    out = []
    for i in range(2, len(knots) - 2):
        a = 0.5 * (knots[i] + (knots[0] + i * d))
        if floor_cell(knots, a) != search_cell(knots, a):
            out.append(a)
    return out


# ---------------------------------------------------------------- reading the archive
def extract(dst):
    """Unpacks the archive under dst; returns dst/bao."""
    with open(GOLDEN, "rb") as f:
        raw = lzma.decompress(f.read())
    with tarfile.open(fileobj=io.BytesIO(raw)) as tar:
        for m in tar.getmembers():
            assert m.isfile() and not os.path.isabs(m.name) and ".." not in m.name, m.name
        try:
            tar.extractall(dst, filter="data")
        except TypeError:
            tar.extractall(dst)
    return os.path.join(str(dst), "bao")


def load_cases(d, ini="bao.ini"):
    """The cases of an ini: dicts k (0-based), tag, label, DV, DA, H, rd, ref."""
    cases_f, labels_f, ref_f = INIS[ini]
    with open(os.path.join(d, cases_f)) as f:
        rows = [l.split() for l in f.read().splitlines()[1:]]
    with open(os.path.join(d, labels_f)) as f:
        labels = f.read().split()
    ref = np.loadtxt(os.path.join(d, ref_f)).reshape(-1, 2)
    assert len(rows) == len(labels) == len(ref)
    out = []
    for r, lab, (k, v) in zip(rows, labels, ref):
        assert int(r[0]) == int(k)
        out.append(dict(k=int(k) - 1, tag=TAGS[ini][int(k) - 1], label=lab, DV=float(r[1]), DA=float(r[2]),
                        H=float(r[3]), rd=float(r[4]), ref=float(v)))
    return out


def read_all(d, ini="bao.ini"):
    """read_bao_likelihood of every bao_dataset of an ini of the fixture, by tag."""
    from cosmomc_amd.derivedlike import derived_likelihood_specs
    return {s["name"]: s for s in derived_likelihood_specs(os.path.join(d, ini))}


def host_errors(fx, ini="bao.ini"):
    """Per tag: (a) max |f64 restatement - golden| over the finite cases, (b)
    max |f64 - long double| over the interior cases (an edge case sits on a
    discontinuity by design, where another precision may rightly fall on the
    other side of it), and whether every logZero outcome of the f64
    restatement is the golden's."""
    specs = read_all(fx, ini)
    out = {}
    for c in load_cases(fx, ini):
        d = specs[c["tag"]]
        v0, v1 = surfaces_of(c["DV"], c["DA"], c["H"], c["rd"], d["kind"])
        f64 = bao_table_loglike_host(d, v0, v1)
        e = out.setdefault(c["tag"], dict(a=0.0, b=0.0, n=0, nzero=0, same=True))
        if c["ref"] >= 1e29 or f64 >= 1e29:
            e["same"] &= c["ref"] == LOGZERO and f64 == LOGZERO
            e["nzero"] += 1
            continue
        e["a"] = max(e["a"], abs(f64 - c["ref"]))
        e["n"] += 1
        if any(w in c["label"] for w in ("interior", "peak", "beside")):
            ld = bao_table_loglike_host(d, v0, v1, np.longdouble)
            e["b"] = max(e["b"], float(abs(np.longdouble(f64) - ld)))
    return out


# ---------------------------------------------------------------- making the inputs
def _e9(x):
    """9 significant digits as the real grid files print them"""
    return "%16.8E" % x


def _write_grid(path, npts, seed):
    rng = np.random.RandomState(seed)
    lo, hi = np.array([0.86, 0.80]) + 0.01 * rng.rand(2), np.array([1.14, 1.21]) - 0.01 * rng.rand(2)
    perp = lo[0] + (hi[0] - lo[0]) * np.arange(npts) / (npts - 1)
    plel = lo[1] + (hi[1] - lo[1]) * np.arange(npts) / (npts - 1)
    u, w = (np.arange(npts) / (npts - 1) - 0.55) / 0.22, (np.arange(npts) / (npts - 1) - 0.45) / 0.25
    prob = 3.7 * np.exp(-0.5 * (u[:, None] ** 2 + w[None, :] ** 2 - 0.6 * u[:, None] * w[None, :]))
    prob *= 1 + 0.05 * rng.rand(npts, npts)
    if npts >= 40:
        prob[prob < 2e-3 * prob.max()] = 0.0         # the real files' zero corners
        i, j = ZERO_CELL
        prob[i:i + 2, j:j + 2] = 0.0                 # one whole cell
    elif npts == 4:
        prob[0, 0] = 0.0
    with open(path, "w") as f:
        for i in range(npts):
            for j in range(npts):
                f.write(_e9(perp[i]) + " " + _e9(plel[j]) + " " + _e9(prob[i, j]) + "\n")


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def _reach(target, fn, guess, side):
    """Among the doubles within 64 ulps of guess: (v with fn(v) == target, or
    None; v with fn(v) the nearest value beyond target on `side`)."""
    cand = [_ulps(np.float64(guess), n) for n in range(-64, 65)]
    at = [v for v in cand if fn(v) == target]
    beyond = [v for v in cand if (fn(v) > target if side > 0 else fn(v) < target)]
    out = min(beyond, key=lambda v: abs(fn(v) - target))
    return (at[0] if at else None), out


def _grid_cases(k, d, rng, n_interior):
    """(label, DV, DA, H, rd) cases of a grid likelihood"""
    n, perp, plel = d["np"], d["perp"], d["plel"]
    fa = lambda v: np.float64(v) / np.float64(d["DA_rd_fid"])                       # noqa: E731
    fb = lambda v: np.float64(d["Hrd_fid"]) / np.float64(v)                         # noqa: E731
    v0_of = lambda a, side=1: _reach(a, fa, a * d["DA_rd_fid"], side)               # noqa: E731
    v1_of = lambda b, side=1: _reach(b, fb, d["Hrd_fid"] / b, side)                 # noqa: E731
    mid0, mid1 = 0.5 * (perp[0] + perp[n - 2]) * d["DA_rd_fid"], d["Hrd_fid"] / (0.5 * (plel[0] + plel[n - 2]))
    out = []
    for ia, a in (("lo", perp[0]), ("hi", perp[n - 2])):
        for ib, b in (("lo", plel[0]), ("hi", plel[n - 2])):
            v0, v1 = v0_of(a)[0], v1_of(b)[0]
            assert v0 is not None and v1 is not None, ("a corner is not reachable in f64", k, ia, ib)
            out.append((f"corner_{ia}_{ib}", 0.0, v0, v1, 1.0))
    out.append(("perp_hi_exact", 0.0, v0_of(perp[n - 2])[0], mid1, 1.0))
    out.append(("perp_hi_beyond", 0.0, v0_of(perp[n - 2], 1)[1], mid1, 1.0))
    out.append(("perp_lo_beyond", 0.0, v0_of(perp[0], -1)[1], mid1, 1.0))
    out.append(("plel_hi_exact", 0.0, mid0, v1_of(plel[n - 2])[0], 1.0))
    out.append(("plel_hi_beyond", 0.0, mid0, v1_of(plel[n - 2], 1)[1], 1.0))
    out.append(("plel_lo_beyond", 0.0, mid0, v1_of(plel[0], -1)[1], 1.0))
    out.append(("v1_negative", 0.0, mid0, -mid1, 1.0))
    out.append(("v1_zero", 0.0, mid0, 0.0, 1.0))
    for t in range(n_interior):                     # interior points at a realistic r_drag
        a = perp[0] + (perp[n - 2] - perp[0]) * rng.rand()
        b = plel[0] + (plel[n - 2] - plel[0]) * rng.rand()
        rd = 147.0 + rng.rand()
        out.append((f"interior_{t}", 0.0, a * d["DA_rd_fid"] * rd, d["Hrd_fid"] / b / rd, rd))
    if n >= 40:
        i, j = ZERO_CELL
        out.append(("zero_cell", 0.0, 0.5 * (perp[i] + perp[i + 1]) * d["DA_rd_fid"],
                    d["Hrd_fid"] / (0.5 * (plel[j] + plel[j + 1])), 1.0))
        out.append(("beside_zero_cell", 0.0, 0.5 * (perp[i + 1] + perp[i + 2]) * d["DA_rd_fid"],
                    d["Hrd_fid"] / (0.5 * (plel[j + 1] + plel[j + 2])), 1.0))
        for axis, knots, fn, guess in (("perp", perp, fa, lambda a: a * d["DA_rd_fid"]),
                                       ("plel", plel, fb, lambda b: d["Hrd_fid"] / b)):
            dis = floor_search_disagree(knots)
            assert dis, ("no point where floor and search disagree", k, axis)
            v = np.float64(guess(dis[len(dis) // 2]))
            assert floor_cell(knots, fn(v)) != search_cell(knots, fn(v))
            out.append((f"floor_vs_search_{axis}", 0.0, v if axis == "perp" else mid0, mid1 if axis == "perp" else v,
                        1.0))
    return out


def _mgs_cases(rng):
    from cosmomc_amd import derivedlike as dl
    scale = np.float64(dl.MGS_DVFID) / np.float64(dl.MGS_RSFID)
    f = lambda v: np.float64(v) / scale                                             # noqa: E731
    lo, hi = np.float64(dl.MGS_ALPHA_MIN), np.float64(dl.MGS_ALPHA_MAX)
    at_lo, below = _reach(lo, f, lo * scale, -1)
    at_hi, above = _reach(hi, f, hi * scale, 1)
    assert at_lo is not None and at_hi is not None, "alpha_min or alpha_max is not reachable in f64"
    out = [("at_x_min", at_lo, 0.0, 0.0, 1.0), ("below_x_min", below, 0.0, 0.0, 1.0),
           ("at_x_max", at_hi, 0.0, 0.0, 1.0), ("above_x_max", above, 0.0, 0.0, 1.0),
           ("far_below", 0.5 * scale, 0.0, 0.0, 1.0), ("far_above", 1.5 * scale, 0.0, 0.0, 1.0),
           ("negative", -scale, 0.0, 0.0, 1.0)]
    # alpha just below and at a cell edge x_min + c step
    for c in (1, 200, 397):
        e = lo + c * np.float64(dl.MGS_STEP)
        out.append((f"under_edge_{c}", _reach(e, f, e * scale, -1)[1], 0.0, 0.0, 1.0))
        out.append((f"over_edge_{c}", _reach(e, f, e * scale, 1)[1], 0.0, 0.0, 1.0))
    for t in range(12):
        rd = 147.0 + rng.rand()
        out.append((f"interior_{t}", (lo + (hi - lo) * rng.rand()) * scale * rd, 0.0, 0.0, rd))
    return out


def _write_cases(d, ini, per_tag):
    cases_f, labels_f, _ = INIS[ini]
    rows, labels = [], []
    for k, tag in enumerate(TAGS[ini]):
        for lab, DV, DA, H, rd in per_tag[tag]:
            rows.append("%d %s %s %s %s" % (k + 1, repr(float(DV)), repr(float(DA)), repr(float(H)), repr(float(rd))))
            labels.append(f"{tag}:{lab}")
    with open(os.path.join(d, cases_f), "w") as f:
        f.write("%d\n" % len(rows) + "\n".join(rows) + "\n")
    with open(os.path.join(d, labels_f), "w") as f:
        f.write("\n".join(labels) + "\n")


def make_fixture(d, mgs_dir, dr11_dir=None):
    """Writes the inputs under d (the archive's bao/): mgs_dir holds the real
    sdss_MGS_bao.dataset and sdss_MGS_prob.txt, D_Cooke2017.dataset and
    Yp_Aver2015.dataset; dr11_dir, when given, the real
    sdss_DR11CMASS_bao.dataset and sdss_DR11CMASS_consensus.dat."""
    import shutil
    os.makedirs(d, exist_ok=True)
    for f in ("sdss_MGS_bao.dataset", "sdss_MGS_prob.txt", "D_Cooke2017.dataset", "Yp_Aver2015.dataset"):
        shutil.copy(os.path.join(mgs_dir, f), os.path.join(d, f))
    ini = "use_BAO = T\nbao_dataset[MGS] = sdss_MGS_bao.dataset\n"
    for tag, (npts, seed, z, fid, meas) in SYNTHETIC.items():
        _write_grid(os.path.join(d, f"syn_{tag}.dat"), npts, seed)
        with open(os.path.join(d, f"syn_{tag}_bao.dataset"), "w") as f:
            f.write(f"name = {tag}\nzeff = {z}\n{meas}alpha_npoints = {npts}\nprob_dist = syn_{tag}.dat\n{fid}")
        ini += f"bao_dataset[{tag}] = syn_{tag}_bao.dataset\n"
    ini += f"bao_dataset[DR12LOWZ,DA_rd_fid] = {LOWZ_DA_RD_FID_SETTING}\n"
    with open(os.path.join(d, "bao.ini"), "w") as f:
        f.write(ini)
    rng = np.random.RandomState(2018)
    per_tag = {"MGS": _mgs_cases(rng)}
    for k, tag in enumerate(TAGS["bao.ini"][1:]):
        npts, seed = SYNTHETIC[tag][:2]
        # an alpha equal to a knot needs a double v with fl(v / fid) or fl(fid / v)
        # that knot, which about half the knots have: the first seed (in steps
        # of 100) whose bounds all have one, and which leaves a gap between
        # floor and search on both axes
        for s in range(seed, seed + 100000, 100):
            _write_grid(os.path.join(d, f"syn_{tag}.dat"), npts, s)
            spec = read_all(d)[tag]
            try:
                per_tag[tag] = _grid_cases(k + 1, spec, np.random.RandomState(s), 12 if npts >= 40 else 4)
                print(tag, "seed", s)
                break
            except AssertionError:
                continue
        else:
            raise RuntimeError("no seed gives reachable bounds")
    _write_cases(d, "bao.ini", per_tag)
    if dr11_dir:
        for f in ("sdss_DR11CMASS_bao.dataset", "sdss_DR11CMASS_consensus.dat"):
            shutil.copy(os.path.join(dr11_dir, f), os.path.join(d, f))
        with open(os.path.join(d, "bao_dr11.ini"), "w") as f:
            f.write("use_BAO = T\nbao_dataset[DR11CMASS] = sdss_DR11CMASS_bao.dataset\n")
        s = read_all(d, "bao_dr11.ini")["DR11CMASS"]
        n, perp, plel = s["np"], s["perp"], s["plel"]
        cases = []
        for t in range(16):                            # around the peak, where the real grid is not 0
            i, j = np.unravel_index(np.argmax(s["prob"]), s["prob"].shape)
            a = perp[i] + (perp[min(i + 40, n - 2)] - perp[i]) * (2 * rng.rand() - 1) * 0.5
            b = plel[j] + (plel[min(j + 40, n - 2)] - plel[j]) * (2 * rng.rand() - 1) * 0.5
            rd = 147.0 + rng.rand()
            cases.append((f"peak_{t}", 0.0, a * s["DA_rd_fid"] * rd, s["Hrd_fid"] / b / rd, rd))
        cases.append(("zero_corner", 0.0, 0.5 * (perp[0] + perp[1]) * s["DA_rd_fid"],
                      s["Hrd_fid"] / (0.5 * (plel[0] + plel[1])), 1.0))
        cases.append(("outside", 0.0, 2 * perp[n - 1] * s["DA_rd_fid"], s["Hrd_fid"], 1.0))
        _write_cases(d, "bao_dr11.ini", {"DR11CMASS": cases})


def pack(d):
    """Packs d (the archive's bao/) into GOLDEN, data files only."""
    names = sorted(f for f in os.listdir(d) if f.endswith((".ini", ".dataset", ".dat", ".txt")))
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w") as tar:
        for f in names:
            p = os.path.join(d, f)
            ti = tar.gettarinfo(p, "bao/" + f)
            ti.mtime, ti.uid, ti.gid, ti.uname, ti.gname, ti.mode = 0, 0, 0, "", "", 0o644
            with open(p, "rb") as fh:
                tar.addfile(ti, fh)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    return os.path.getsize(GOLDEN)
