"""The SZ kernels (sz.hip) pointwise and at their edges: the completeness table
entry by entry on every kind of ln Y node window, the theta bracket on two
thetas and on unsorted ones, irregular nuisance values, batches of more than
1024 walkers (the chunk loop of SzLike::run) and a caller's workspace.

The table is in the workspace after a call: float32 comp[w][q][j * nm + m] for
the walkers of the last chunk, workspace_bytes(W) = 5 nzs nm 4 min(W, 1024)
bytes (the workspace paragraph of the SZ section).  Its
reference is sz_completeness in f64, [z][m][q], rounded to single precision as
the compiled reference's real(sp) table is; test_szcounts.py holds that
restatement to the compiled reference's -lnL on every golden, syn_two (two
thetas, one patch) and syn_unsorted (the linear search) among them.

Bound, per entry.  test_szcounts.py::test_completeness_f64_against_long_double
measures (c), the largest absolute difference of an entry between the f64 and
the long-double restatement over this file's cases, and prints it:
syn_inside 7.1e-15, syn_two 7.1e-15, syn_unsorted 5.7e-14 (sf.COMP_LD_ABS;
each is one single-precision ulp of a small entry whose rounding tipped).  A
device entry passes if
  * |device - f64| <= 10 x (c) of its dataset, the project's rule: 7.1e-14,
    7.1e-14, 5.7e-13; or
  * it is exactly one single-precision ulp from the f64 entry: a rounding that
    tipped, on the ln Y sum taken by nodes in a 16-lane tree or on the device's
    exp, erf, pow and log.  At most 16 entries of a table (1e-4 of its 168 600)
    may use this; the f64 and long-double tables use it 0 times.
Entries clipped at fsky or at 0 fall under the same rule, and every entry is
finite on both sides.  Measured on the MI355X: every entry of the 11 tables
has the bits of the f64 entry (largest |device - f64| 0, no entry one ulp off),
so neither allowance is used; the test prints both figures per table.

-lnL of every case is held to test_gpu_sz.py's WELL_ATOL, 10 x 1.5e-10: f64
against long double is 1.0e-11 at most over the points used here (syn_two at
(1.5, -0.2, 1.0, 0.1, 0.5) with the grid doubled, -lnL = 4608; 1.4e-12 at
scatter_SZ = 3, -lnL = 1.1e5), none of them ill-conditioned.  Measured on the
MI355X: 1.8e-12 at most over the table cases, 3.6e-12 over the 1027 slots.
"""
import numpy as np
import pytest

import sz_fixture as sf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WELL_ATOL = 10 * 1.5e-10
LOGZERO = 1e30
ONE_ULP_MAX = 16                       # entries of a table that may be one float ulp off beyond the absolute bound
SZ_MAXW = 1024                         # walkers a launch of the per-walker kernels takes (sz.hip)
PAD = 3                                # ld_walker = n_theory + PAD
NAN = float("nan")


@pytest.fixture(scope="module")
def goldens(tmp_path_factory):
    return sf.extract(tmp_path_factory.mktemp("sz"), names=sorted(sf.EDGE_CASES))


_open, _host = {}, {}


def _data(goldens, name):
    """(golden, the library's likelihood, the host's dataset), opened once."""
    from cosmomc_amd.szcounts import SZDataset, SZLikelihood
    if name not in _open:
        _open[name] = (goldens[name], SZLikelihood(goldens[name].ini), SZDataset(goldens[name].ini))
    return _open[name]


def _table(name, ds, row, nu):
    """sz_completeness in f64, once per (dataset, nuisance point); it does not depend on the row's grid block."""
    from cosmomc_amd.szcounts import sz_completeness
    key = (name, tuple(float(x) for x in nu))
    if key not in _host:
        _host[key] = sz_completeness(ds, row, nu)
    return _host[key]


def _host_loglike(name, ds, row, nu, table_nu=None):
    """sz_loglike_host with the cached table (table_nu: the point whose table it is, when not nu's own)."""
    from cosmomc_amd.szcounts import sz_counts, sz_loglike_host
    comp = _table(name, ds, row, nu if table_nu is None else table_nu)
    return float(sz_loglike_host(ds, row, nu, DN=sz_counts(ds, row, nu, comp=comp)))


def _rows(row, W):
    """[W, 1, n] theory rows on the device with ld_walker = n + PAD, the padding NaN."""
    buf = torch.full((W, 1, len(row) + PAD), NAN, dtype=torch.float64, device="cuda")
    buf[:, 0, :len(row)] = torch.tensor(row, device="cuda")
    return buf[:, :, :len(row)]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _patterned(nbytes, tail=0):
    """A uint8 device buffer of nbytes + tail bytes filled with 0xA5 (as floats: -2.9e-16, in no table)."""
    return torch.full((nbytes + tail,), 0xA5, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------- the table, entry by entry

@pytest.mark.parametrize("name", sorted(sf.EDGE_CASES))
def test_completeness_entry_by_entry(goldens, name):
    g, like, ds = _data(goldens, name)
    cases = sf.EDGE_CASES[name]
    W, npts = len(cases), like.nzs * like.nm
    assert like.workspace_bytes(W) == 5 * npts * 4 * W
    ws = _patterned(like.workspace_bytes(W))
    got = like.loglike_batch(_rows(g.row, W), _dev(cases), workspace=ws).cpu().numpy()
    dev = ws.view(torch.float32)[:W * 5 * npts].reshape(W, 5, like.nzs, like.nm).cpu().numpy()
    atol = 10 * sf.COMP_LD_ABS[name]
    for w, nu in enumerate(cases):
        # the host's table of -|scatter_SZ| is that of +|scatter_SZ| (asserted in test_szcounts.py); the device's too
        pos = tuple(nu[:3]) + (abs(nu[3]),) + tuple(nu[4:])
        if pos != tuple(nu):
            assert np.array_equal(dev[w].view(np.int32), dev[cases.index(pos)].view(np.int32))
        ref = np.ascontiguousarray(np.transpose(_table(name, ds, g.row, pos), (2, 0, 1)))     # [q][z][m]
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(dev[w])), (name, nu)
        diff = np.abs(dev[w].astype(np.float64) - ref)
        beyond = diff > atol
        one = sf.ulp_apart(dev[w], ref)
        fsky = np.float32(ds.skyfracs.sum())
        print(name, nu, "max |device - f64| per entry:", diff.max(), "; entries beyond", atol, "and one ulp off:",
              np.count_nonzero(beyond & one), "; beyond and further off:", np.count_nonzero(beyond & ~one),
              "; one ulp off in all:", np.count_nonzero(one), "; at fsky:", np.count_nonzero(ref == fsky),
              np.count_nonzero(dev[w] == fsky), "; at 0:", np.count_nonzero(ref == 0), np.count_nonzero(dev[w] == 0))
        worst = np.unravel_index(np.argmax(np.where(beyond & ~one, diff, 0)), diff.shape)
        assert not np.any(beyond & ~one), (name, nu, "entry [q, z, m]", worst, dev[w][worst], ref[worst])
        assert np.count_nonzero(beyond) <= ONE_ULP_MAX, (name, nu, np.count_nonzero(beyond))
        want = _host_loglike(name, ds, g.row, nu, table_nu=pos)
        print(name, nu, "-lnL", got[w], "|gpu - f64|:", abs(got[w] - want))
        assert abs(got[w] - want) <= WELL_ATOL, (name, nu, got[w], want)
    if name == "syn_inside":
        assert "prior_scatter_SZ" in g.priors and got[4] != got[0]
        total = dict.fromkeys(sf.WINDOW_CLASSES + ("empty",), 0)
        for nu in cases:
            if nu[3] != 0:
                for c, n in sf.window_classes(ds, g.row, nu).items():
                    total[c] += n
        assert all(n > 0 for n in total.values()), total
        assert sum(1 for nu in cases if nu[3] == 0) == 2
    else:
        assert any(nu[3] == 0 for nu in cases) and any(nu[3] != 0 for nu in cases)
    if name == "syn_two":
        assert (like.n_thetas, like.n_patches) == (2, 1)
    if name == "syn_unsorted":
        th = ds.thetas
        assert np.any(np.diff(th) < 0) and th[0] == th.min() and th[-1] == th.max()
        thp = sf.scaling(ds, g.row, sf.CENTRE)[0]
        ins = (thp >= th.min()) & (thp <= th.max())
        near = np.argmin(np.abs(th[None, None, :] - thp[:, :, None]), axis=2)
        for t in range(1, len(th) - 1):
            assert np.any(ins & (near == t) & (th[t] > thp)) and np.any(ins & (near == t) & (th[t] < thp)), t


# ---------------------------------------------------------------- irregular nuisance values

def _five(goldens):
    g, like, ds = _data(goldens, "syn_inside")
    full = sf.nuisance_points("all")
    nu = full[[0, 9, 3, 10, 12]]                          # walkers 1 and 3 have scatter_SZ == 0
    assert tuple(nu[0]) == sf.CENTRE and tuple(nu[1]) == sf.ZERO_SCATTER and nu[3, 3] == 0 and np.all(nu[[0, 2, 4], 3] != 0)
    return g, like, ds, nu


@pytest.mark.parametrize("k", range(5), ids=sf.PARAM_NAMES)
def test_nan_nuisance_is_logzero_for_that_walker_alone(goldens, k):
    g, like, ds, nu = _five(goldens)
    rows = _rows(g.row, 5)
    clean = like.loglike_batch(rows, _dev(nu)).cpu().numpy()
    assert np.all(clean < 1e29)
    for bad in (1, 2):                                    # a walker of either branch
        n2 = nu.copy()
        n2[bad, k] = NAN
        got = like.loglike_batch(rows, _dev(n2)).cpu().numpy()
        assert got[bad] == LOGZERO
        keep = np.arange(5) != bad
        assert np.array_equal(got[keep], clean[keep])


@pytest.mark.parametrize("name", ["syn_inside", "syn_unsorted"])
@pytest.mark.parametrize("bias", [0.0, -0.8])
def test_non_positive_bias_is_what_the_host_gives(goldens, name, bias):
    """bias_SZ = 0: theta500 = y500 = 0, ln y500 = -inf, every node is visited and adds 0; bias_SZ < 0: pow of a
    negative base, theta500 and y500 are NaN and the bracket stays inside its table by either search.  The host
    gives logZero for both (1 / bias_SZ of prior_lens; NaN counts), with scatter and without."""
    g, like, ds = _data(goldens, name)
    nu = sf.nuisance_points("all")[[0, 9, 3, 10, 12]]
    rows = _rows(g.row, 5)
    clean = like.loglike_batch(rows, _dev(nu)).cpu().numpy()
    for bad in (0, 1):                                    # the centre, and the scatter_SZ == 0 point
        n2 = nu.copy()
        n2[bad, 2] = bias
        want = _host_loglike(name, ds, g.row, tuple(n2[bad]))
        got = like.loglike_batch(rows, _dev(n2)).cpu().numpy()
        assert want == LOGZERO and got[bad] == want, (got[bad], want)
        keep = np.arange(5) != bad
        assert np.array_equal(got[keep], clean[keep])


# ---------------------------------------------------------------- more than 1024 walkers; the caller's workspace

W_BIG = SZ_MAXW + 3
SCALES = (1.0, 0.5, 2.0)               # of the row's grid block, by slot % 3: powers of two, so DN scales exactly
SEVEN = [sf.CENTRE, sf.ZERO_SCATTER, (1.5, -0.2, 1.0, 0.1, 0.5), (1.6, -0.25, 0.7, 0.0, 0.3), (2.2, -0.29, 0.6, 0.05, 1.0),
         (1.789, -0.1, 0.8, 0.075, 0.3), (2.1, -0.15, 0.688, 0.09, 0.4)]          # the nuisance point, by slot % 7
NAMED = (0, SZ_MAXW - 1, SZ_MAXW, W_BIG - 1)


class Big:
    """W_BIG walkers on syn_two.  1024 is 1 mod 3 and 2 mod 7, so slot w and slot w - 1024 differ in row and in
    nuisance point: an index formed from the slot within the chunk where the slot is meant, or the reverse,
    in dl, nuis, out or the workspace, lands on another pair and changes the result."""

    def __init__(self, goldens):
        self.g, self.like, self.ds = _data(goldens, "syn_two")
        n, nzs = len(self.g.row), self.like.nzs
        self.grid0 = 3 + 2 * nzs
        slot = np.arange(W_BIG)
        self.pair = np.stack([slot % 3, slot % 7], axis=1)
        assert SZ_MAXW % 3 == 1 and SZ_MAXW % 7 == 2
        assert any(p[3] == 0 for p in SEVEN) and any(p[3] != 0 for p in SEVEN)
        self.rows = _rows(self.g.row, W_BIG)                                       # built on the device: 280 MB
        self.rows[:, 0, self.grid0:] *= _dev(np.array(SCALES)[self.pair[:, 0]])[:, None]
        self.nu = _dev(np.array(SEVEN)[self.pair[:, 1]])
        self.dense_dev = self.like.loglike_batch(self.rows, self.nu)
        self.dense = self.dense_dev.cpu().numpy()

    def host_row(self, s):
        r = np.array(self.g.row)
        r[self.grid0:] *= s
        return r


@pytest.fixture(scope="module")
def big(goldens):
    return Big(goldens)


def test_chunked_batch_carries_every_slots_own_pair(big):
    assert big.like.n_theory == len(big.g.row) and big.rows.stride(0) == len(big.g.row) + PAD
    want = np.array([[_host_loglike("syn_two", big.ds, big.host_row(s), p) for p in SEVEN] for s in SCALES])
    assert len({x for x in want.ravel()}) == 21 and np.all(np.abs(want) < 1e29)
    per_slot = want[big.pair[:, 0], big.pair[:, 1]]
    err = np.abs(big.dense - per_slot)
    print("W =", W_BIG, "max |gpu - f64| over the slots:", err.max(), "of", per_slot.max())
    assert np.all(err <= WELL_ATOL), "slots %s: gpu %s, f64 %s; the worst slot is %d" % (
        NAMED, big.dense[list(NAMED)], per_slot[list(NAMED)], int(np.argmax(err)))
    # every slot of a pair has the bits of the pair's first slot
    first = {}
    for w, p in enumerate(map(tuple, big.pair)):
        first.setdefault(p, w)
        assert big.dense[w].tobytes() == big.dense[first[p]].tobytes(), (w, first[p])


def test_chunked_batch_equals_its_chunks_apart_and_a_shared_row(big):
    a = big.like.loglike_batch(big.rows[:SZ_MAXW], big.nu[:SZ_MAXW]).cpu().numpy()
    b = big.like.loglike_batch(big.rows[SZ_MAXW:], big.nu[SZ_MAXW:]).cpu().numpy()
    assert np.array_equal(np.concatenate([a, b]), big.dense)
    for i, s in enumerate(SCALES):                           # ld_walker = 0: one row for all the walkers
        shared = _dev(big.host_row(s)).reshape(1, 1, -1).expand(W_BIG, 1, -1)
        assert shared.stride(0) == 0
        got = big.like.loglike_batch(shared, big.nu).cpu().numpy()
        use = big.pair[:, 0] == i
        assert np.array_equal(got[use], big.dense[use]), (s, [w for w in NAMED if use[w]])


def test_chunked_sparse_entry_at_the_live_count_edges(big):
    """out beyond the live count keeps its sentinel, in every chunk; the counts run back to back on the stream
    with no host synchronisation between them, so a chunk left over from one call would show in the next."""
    counts = (W_BIG, 1, SZ_MAXW + 1, SZ_MAXW - 1, SZ_MAXW, 0)
    live = torch.tensor([[c] for c in counts], dtype=torch.int32, device="cuda")
    outs = torch.full((len(counts), W_BIG), -7.0, dtype=torch.float64, device="cuda")
    for i in range(len(counts)):                              # queued one after another; read back below
        big.like.loglike_batch_sparse(big.rows, big.nu, outs[i], live[i])
    for c, got in zip(counts, outs.cpu().numpy()):
        assert np.array_equal(got[:c], big.dense[:c]), c
        assert np.all(got[c:] == -7.0), c


@pytest.mark.parametrize("W", [W_BIG, 3])
def test_kernels_stay_inside_the_callers_workspace(big, W):
    like, npts = big.like, big.like.nzs * big.like.nm
    assert like.workspace_bytes(W_BIG) == like.workspace_bytes(SZ_MAXW) == 5 * npts * 4 * SZ_MAXW
    assert like.workspace_bytes(3) == 5 * npts * 4 * 3
    nbytes, tail = like.workspace_bytes(W), 1 << 20
    ws = _patterned(nbytes, tail)
    got = like.loglike_batch(big.rows[:W], big.nu[:W], workspace=ws[:nbytes]).cpu().numpy()
    assert np.array_equal(got, big.dense[:W])
    assert bool(torch.all(ws[nbytes:] == 0xA5)), "the kernels wrote beyond workspace_bytes(%d)" % W
    # and they wrote the table: the last chunk's walkers, from the workspace's first byte
    last = W - (W - 1) // SZ_MAXW * SZ_MAXW
    tab = ws[:nbytes].view(torch.float32)[:last * 5 * npts]
    assert bool(torch.all((tab >= 0) & (tab <= 1)))
    alone = _patterned(like.workspace_bytes(last))
    like.loglike_batch(big.rows[W - last:W], big.nu[W - last:W], workspace=alone)
    assert bool(torch.equal(tab.view(torch.int32), alone.view(torch.float32)[:last * 5 * npts].view(torch.int32)))
