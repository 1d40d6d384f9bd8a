"""ChainWriter with theory-derived columns (theory_derived=): the order of
.paramnames and of the row columns, the .ranges lines, and a checkpoint /
restore in mid-run.  Duck-typed derived objects; no GPU."""
import json
import os

import numpy as np

from cosmomc_amd.chains import ChainWriter, fortran_e

NAMES, LABELS = ["omegabh2", "calPlanck"], ["\\Omega_b h^2", "y_{\\rm cal}"]
RANGES = [(0.005, 0.1), (0.9, 1.1)]
LIKES = [("plikHM", "CMB", "plik_lite", "v18"), ("lowl", "CMB", "commander", "v2"), ("BAO6", "BAO", "sixdf", "2011")]


class FakeTheoryDerived:
    names = [("H0", "H_0"), ("omegam", "\\Omega_m"), ("zrei", "z_{\\rm re}"), ("DL40", "D_{40}")]
    ranges = [("H0", 40.0, 100.0), ("omegam", None, 0.9), ("zrei", 6.5, None)]    # both, max only, min only

    def columns(self, P_used):
        a, b = P_used[:, 0, :], P_used[:, 1, :]
        return np.stack([3000.0 * a, a + b, 7.0 + b, 1e3 * a * b], axis=1)


class FakeLikeDerived:
    names = [("Dl2000_smica", "D_{2000}")]

    def columns(self, P_used):
        return (P_used[:, 0:1, :] - P_used[:, 1:2, :]) * 5.0


def _history(steps, W, seed):
    """[steps, 3, W] (2 parameters, CurLike) and terms [steps, 3, W]: each walker
    stays 1-3 steps at a point, then moves."""
    rng = np.random.default_rng(seed)
    rows, terms = np.empty((steps, 3, W)), np.empty((steps, 3, W))
    for w in range(W):
        t = 0
        while t < steps:
            n = int(rng.integers(1, 4))
            p = np.array([rng.uniform(0.02, 0.025), rng.uniform(0.99, 1.01)])
            tr = rng.uniform(1.0, 300.0, size=3)
            rows[t:t + n, :2, w] = p
            rows[t:t + n, 2, w] = tr.sum() + 0.125
            terms[t:t + n, :, w] = tr
            t += n
    return rows, terms


def _writer(root, **kw):
    return ChainWriter(root, NAMES, LABELS, RANGES, likelihoods=LIKES, burn_in=0, **kw)


def _fields(line):
    assert len(line) % 16 == 0
    return [line[i:i + 16] for i in range(0, len(line), 16)]


def test_paramnames_ranges_and_row_order(tmp_path):
    root = str(tmp_path / "chain")
    td, ld = FakeTheoryDerived(), FakeLikeDerived()
    cw = _writer(root, derived=ld, theory_derived=td)
    chi2 = ["chi2_plikHM", "chi2_lowl", "chi2_BAO6", "chi2_prior", "chi2_CMB"]
    with open(root + ".paramnames") as f:
        names = [l.split("\t")[0] for l in f.read().splitlines()]
    assert names == NAMES + ["H0*", "omegam*", "zrei*", "DL40*"] + ["Dl2000_smica*"] + [c + "*" for c in chi2]

    with open(root + ".ranges", "rb") as f:
        got = f.read()
    want = "omegabh2\t0.005\t0.1\ncalPlanck\t0.9\t1.1\n"
    want += "H0                    " + "    0.4000000E+02" + "    0.1000000E+03" + "\n"
    want += "omegam                " + "    N            " + "    0.9000000E+00" + "\n"
    want += "zrei                  " + "    0.6500000E+01" + "    N            " + "\n"
    for c in chi2:
        want += f"{c:<22}" + "    0.0000000E+00" + "    N            " + "\n"
    assert got == want.encode()

    W, steps = 3, 30
    rows, terms = _history(steps, W, 1)
    cw.add_rows(rows, terms)
    tcols, lcols = td.columns(rows[:, :2, :]), ld.columns(rows[:, :2, :])
    for w in range(W):
        with open(f"{root}_{w + 1}.txt") as f:
            lines = f.read().splitlines()
        assert len(lines) >= 5
        # the stays of walker w in order; the first is dropped (burn_in 0), the last still open
        starts = [t for t in range(steps) if t == 0 or not np.array_equal(rows[t, :, w], rows[t - 1, :, w])]
        assert len(lines) == len(starts) - 2
        for line, t, t_next in zip(lines, starts[1:], starts[2:]):
            tr = terms[t, :, w]
            like = rows[t, 2, w]
            want_row = [float(t_next - t), like, *rows[t, :2, w], *tcols[t, :, w], *lcols[t, :, w],
                        *(2.0 * tr), 2.0 * (like - tr.sum()), 2.0 * (tr[0] + tr[1])]
            assert _fields(line) == [fortran_e(v, 16) for v in want_row]


def test_default_files_do_not_change(tmp_path):
    """theory_derived=None: the files are those of a writer that is not given
    the argument at all."""
    rows, terms = _history(20, 2, 2)
    for tag, kw in (("a", {}), ("b", {"theory_derived": None})):
        cw = _writer(str(tmp_path / tag), derived=FakeLikeDerived(), **kw)
        cw.add_rows(rows, terms)
    for ext in (".paramnames", ".ranges", ".likelihoods", "_1.txt", "_2.txt"):
        with open(str(tmp_path / "a") + ext, "rb") as fa, open(str(tmp_path / "b") + ext, "rb") as fb:
            assert fa.read() == fb.read(), ext


def test_checkpoint_and_restore_reproduce_the_uninterrupted_files(tmp_path):
    W = 4
    rows, terms = _history(48, W, 3)
    cut = 21
    full = _writer(str(tmp_path / "full"), derived=FakeLikeDerived(), theory_derived=FakeTheoryDerived())
    full.add_rows(rows[:cut], terms[:cut])
    full.add_rows(rows[cut:], terms[cut:])

    root = str(tmp_path / "part")
    a = _writer(root, derived=FakeLikeDerived(), theory_derived=FakeTheoryDerived())
    a.add_rows(rows[:cut], terms[:cut])
    state = json.loads(json.dumps(a.checkpoint_state(W)))
    a.add_rows(rows[cut:cut + 9], terms[cut:cut + 9])          # written after the checkpoint: cut off on resume
    b = _writer(root, derived=FakeLikeDerived(), theory_derived=FakeTheoryDerived())
    b.restore(state, W)
    b.add_rows(rows[cut:], terms[cut:])
    for ext in [".paramnames", ".ranges", ".likelihoods"] + [f"_{w + 1}.txt" for w in range(W)]:
        with open(str(tmp_path / "full") + ext, "rb") as fa, open(root + ext, "rb") as fb:
            x, y = fa.read(), fb.read()
        assert x == y, ext
        assert os.path.getsize(root + ext) > 0
