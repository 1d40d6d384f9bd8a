"""cmbl_loglike_batch_sparse, likelihood by likelihood, at live-count edges.
GPU only, through the C ABI.

The sampler's change mask compacts the walkers whose parameters moved into
slots [0, count) and calls the sparse entry on all W slots with the count in
device memory; every kernel of the likelihood exits past the count, each at its
own granularity (a block per walker, 64-walker tiles, 4 walkers per workgroup,
problems packed into a wave, whole quadratic-form tiles).  The header's
contract (include/cosmomc_amd.h): out of a slot at or beyond the count is not
written, and a live slot's result has the bits cmbl_loglike_batch gives the
same inputs.  Both are checked here bit for bit -- no tolerance -- with the
theory and nuisance rows of the dead slots NaN, so a dead row that reaches a
live result, an eigensolve or out shows.  The dense values themselves are
pinned to the numpy oracles at three slots with the tolerances of the
datasets' own test files (plik_lite and gaussian rtol 1e-10, HL rtol 1e-9), so
what the sparse calls reproduce is the right number.

Datasets and the count checks they reach:
  plik_lite TTTEEE / TT        plik_bin_delta's exit, quadratic form Np = 640 / 256
  lensing_consext8             cmbl_window_direct (+ linear corrections), small chi^2
  sptsz_aberration_calprior    cmbl_window_kernel<ABER>, small chi^2 + calibration prior
  bkplanck_3map / all_maps     T_dust table, cmbl_bk_prologue, cmbl_window_group,
                               cmbl_reduce_kernel, cmbl_hl_rows_kernel (two packed widths),
                               quadratic form
  bk15_B_decorr_bandcentre     the same with decorrelation and band-centre errors (12 maps x 9 bins)
  smica_gauss_run              cmbl_smica_prologue, cmbl_window_kernel<false, FG>, small chi^2
  smica_hl_aber_calname        cmbl_smica_prologue, cmbl_window_kernel<ABER, FG>, reduce, HL rows
"""
import os

import numpy as np
import pytest

import cmblikes_oracle as co
import pyoracle as po
from cosmomc_amd import synthetic as syn

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W = 70                                   # one full 64-walker tile and a tail of 6
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 69, 70, 75)
SLOTS = (0, 35, 69)                      # compared with the oracles
SENTINEL = -7.25
ERR_ARG, ERR_UNSUPPORTED = -1, -6

PLIK = {"plik_lite_TTTEEE": {}, "plik_lite_TT": {"use_cl": "TT"}}
CMBL = ["lensing_consext8", "sptsz_aberration_calprior", "bkplanck_3map_bins1to5", "bkplanck_all_maps",
        "bk15_B_decorr_bandcentre"]
SMICA = ["smica_gauss_run", "smica_hl_aber_calname"]
DATASETS = list(PLIK) + CMBL + SMICA
HL = {"bkplanck_3map_bins1to5", "bkplanck_all_maps", "bk15_B_decorr_bandcentre", "smica_hl_aber_calname"}
SHARED_WS = ["plik_lite_TTTEEE", "lensing_consext8", "bkplanck_3map_bins1to5", "smica_hl_aber_calname"]


def nuisance_rows(base, n, seed):
    """n DataParams rows cycled from the golden case's rows, each entry times a
    seeded 1 + O(1e-3) factor of its own so that no two slots have equal
    inputs.  A column in which the golden rows all agree is one of the case's
    fixed parameters (T_dust with its table, Delta = 1 for "no decorrelation",
    the zero band-centre errors) and stays as it is."""
    base = np.asarray(base, dtype=np.float64).reshape(len(base), -1)
    nu = base[np.arange(n) % len(base)].copy()
    f = 1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1.0, 1.0, nu.shape)
    f[:, np.all(base == base[0], axis=0)] = 1.0
    return nu * f


class Problem:
    """A dataset with its W slots of host inputs, its oracle, and (on first
    use) its open handle, device inputs and dense result: made once per module
    and left unchanged."""

    def __init__(self, name, open_like, oracle, th, base, tol):
        self.name, self.hl, self.tol = name, name in HL, tol
        self.seed = 1000 + DATASETS.index(name)
        self.base = np.asarray(base, dtype=np.float64).reshape(len(base), -1)
        self.th, self.nu = th, nuisance_rows(base, W, self.seed)
        self._open, self._oracle = open_like, oracle
        self._like = self._dev = self._dense = self._ref = None

    @property
    def like(self):
        if self._like is None:
            self._like = self._open()
        return self._like

    def oracle_ref(self):
        if self._ref is None:
            o = self._oracle()
            self._ref = np.array([o(self.th[w], self.nu[w]) for w in SLOTS])
        return self._ref

    def bufs(self):
        if self._dev is None:
            self._dev = (torch.tensor(self.th, device="cuda"), torch.tensor(self.nu, device="cuda"))
        return self._dev

    def dense(self):
        if self._dense is None:
            th, nu = self.bufs()
            self._dense = self.like.loglike_batch(th, nu).cpu().numpy()
            assert np.all(np.isfinite(self._dense)) and len(np.unique(self._dense)) == W, self._dense
            assert self.like.status() == 0
        return self._dense


def host_problem(name, cmbl_golden, refdata, smica_golden, smica_data, plik_data, plik_path):
    """The dataset's Problem; everything up to the first use of .like runs without a GPU."""
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    if name in PLIK:
        over = PLIK[name]

        def orc():
            o = po.PlikLite(plik_data, over.get("use_cl", "TT TE EE"))
            return lambda dl, nu: o.loglike(dl, nu[0])
        return Problem(name, lambda: NativeCMBLikelihood("PLIK_LITE", plik_path, over), orc,
                       syn.walker_theory(W, seed=777, n_fields=3), syn.walker_calibrations(6, seed=99)[:, None],
                       (1e-10, 0.0))
    if name in CMBL:
        c = cmbl_golden["cases"][name]
        tag, path, over, nf = c["tag"], os.path.join(refdata, c["dataset"]), c["overrides"], 10
    else:
        c = smica_golden["cases"][name]
        tag, path, over, nf = "SMICA", smica_data[c["like_approx"]], c["overrides"], 6
    return Problem(name, lambda: NativeCMBLikelihood(tag, path, over),
                   lambda: co.CMBLikesOracle(path, over, tag).loglike,
                   syn.walker_theory(W, seed=c["theory_seed"] + 17, lmax=c["lmax"], n_fields=nf), c["nuis"],
                   (1e-9, 1e-8) if name in HL else (1e-10, 1e-9))


@pytest.fixture(scope="module")
def problems(cmbl_golden, refdata, smica_golden, smica_data, tmp_path_factory):
    cache = {}
    plik_data = syn.make_plik_lite(12345)
    plik_path = plik_data.write(str(tmp_path_factory.mktemp("plik_sparse")))

    def get(name):
        if name not in cache:
            cache[name] = host_problem(name, cmbl_golden, refdata, smica_golden, smica_data, plik_data, plik_path)
        return cache[name]
    return get


def plain(th_buf, nu_buf):
    return th_buf, nu_buf


def sparse_call(like, bufs, count, view=plain, workspace=None, keep=0):
    """The sparse entry on copies of the input buffers whose slots at and
    beyond max(count, keep) are NaN (a single shared theory row stays), viewed
    in the layout under test, with out full of the sentinel."""
    th_buf, nu_buf = (b.clone() for b in bufs)
    n = nu_buf.shape[0]
    dead = max(count, keep)
    if th_buf.shape[0] == n:
        th_buf[dead:] = float("nan")
    nu_buf[dead:] = float("nan")
    th, nu = view(th_buf, nu_buf)
    out = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    like.loglike_batch_sparse(th, nu, out, cnt, workspace=workspace)
    return out.cpu().numpy()


def assert_sparse(out, dense, count, what):
    live = min(count, len(dense))
    bad = np.flatnonzero(out[:live] != dense[:live])[:8]
    assert np.array_equal(out[:live], dense[:live]), \
        f"{what}, count {count}: live slots {bad} differ from the dense call by {(out[:live] - dense[:live])[bad]}"
    written = live + np.flatnonzero(out[live:] != SENTINEL)
    assert written.size == 0, f"{what}, count {count}: dead slots {written[:8]} written: {out[written[:8]]}"


@pytest.mark.parametrize("name", DATASETS)
def test_sparse_counts_match_dense(problems, name):
    """Every count around the 4-walker workgroup, the 64-walker tile and W:
    live slots have the dense call's bits, dead slots keep the sentinel, no
    NaN of a dead slot reaches an eigensolve, and a count beyond W is W.  The
    dense values are the oracles' at slots 0, 35 and 69."""
    p = problems(name)
    dense = p.dense()
    np.testing.assert_allclose(dense[list(SLOTS)], p.oracle_ref(), rtol=p.tol[0], atol=p.tol[1])
    for count in COUNTS:
        out = sparse_call(p.like, p.bufs(), count)
        assert_sparse(out, dense, count, name)
        if p.hl:
            assert p.like.status() == 0, f"{name}, count {count}: an HL eigensolve hit its sweep cap"


@pytest.mark.parametrize("name", SHARED_WS)
def test_sparse_on_a_stale_shared_workspace(problems, name):
    """The sampler hands every likelihood one workspace, so a sparse call finds
    the rows of its dead slots full of an earlier call's values: here a dense
    call on other finite inputs (the theory x 3, other nuisance rows) in every
    slot.  (Finite values only, written by the library itself: the split-K
    arrival tickets live in the workspace.)  The bytes behind the stated size
    stay untouched."""
    p = problems(name)
    dense = p.dense()
    nbytes = p.like.workspace_bytes(W)
    ws = torch.zeros(nbytes + 4096, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0xA5
    th, _ = p.bufs()
    other = torch.tensor(nuisance_rows(p.base[::-1], W, p.seed + 500), device="cuda")
    stale = p.like.loglike_batch(th * 3.0, other, workspace=ws).cpu().numpy()
    assert np.all(np.isfinite(stale)) and not np.any(stale == dense)
    p.like.status()
    for count in (1, 5, 64, 65):
        out = sparse_call(p.like, p.bufs(), count, workspace=ws)
        assert_sparse(out, dense, count, name + " (stale workspace)")
        if p.hl:
            assert p.like.status() == 0
    assert bool((ws[nbytes:] == 0xA5).all()), "written behind workspace_bytes(W)"


def layout_shared(p):
    """One theory row for every slot: expand, ld_walker = 0."""
    th, nu = p.bufs()
    return (th[:1].clone(), nu), lambda t, n: (t.expand(W, -1, -1), n)


def layout_padded(p):
    """Theory rows in a wider buffer: an odd ld_field (no 16-byte loads), two
    extra fields, NaN in all the padding."""
    th, nu = p.bufs()
    L = th.shape[2]
    big = torch.full((W, th.shape[1] + 2, (L + 6) | 1), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :th.shape[1], :L] = th
    return (big, nu), lambda t, n: (t[:, :th.shape[1], :L], n)


def layout_nuis_ld(p):
    """ld_nuis > n_nuis with NaN between the rows."""
    th, nu = p.bufs()
    nn = nu.shape[1]
    big = torch.full((W, nn + 3), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :nn] = nu
    return (th, big), lambda t, n: (t, n[:, :nn])


@pytest.mark.parametrize("layout", [layout_shared, layout_padded, layout_nuis_ld], ids=lambda f: f.__name__[7:])
@pytest.mark.parametrize("name", ["lensing_consext8", "bkplanck_3map_bins1to5"])
def test_sparse_layouts(problems, name, layout):
    """Strided inputs: the live slots have the bits of the dense call on the
    same layout.  That dense call agrees with the contiguous one to twice the
    dataset's oracle tolerance (each is the oracle's value to once), slot 0 of
    the shared row included: the layout is read as meant."""
    p = problems(name)
    bufs, view = layout(p)
    th, nu = view(*bufs)
    assert (th.stride(0) == 0) == (layout is layout_shared)
    dense = p.like.loglike_batch(th, nu).cpu().numpy()
    same = slice(0, 1) if layout is layout_shared else slice(None)
    np.testing.assert_allclose(dense[same], p.dense()[same], rtol=2 * p.tol[0], atol=2 * p.tol[1])
    assert np.all(np.isfinite(dense)) and len(np.unique(dense)) == W
    for count in (1, 65, 70):
        out = sparse_call(p.like, bufs, count, view=view)
        assert_sparse(out, dense, count, f"{name} ({layout.__name__})")
        if p.hl:
            assert p.like.status() == 0


@pytest.mark.parametrize("name", ["plik_lite_TTTEEE", "lensing_consext8", "bkplanck_3map_bins1to5"])
def test_sparse_eight_tiles(problems, name):
    """W = 512: tiles % 8 == 0 puts the quadratic form and the grouped windows
    on their XCD-remapped block order, and whole dead tiles exit without a
    ticket.  The 70 theories tiled (w % 70) with every slot's own nuisance row."""
    p = problems(name)
    n = 512
    th = p.bufs()[0][torch.arange(n, device="cuda") % W]
    nu = torch.tensor(nuisance_rows(p.base, n, p.seed + 8), device="cuda")
    dense = p.like.loglike_batch(th, nu).cpu().numpy()
    assert np.all(np.isfinite(dense)) and len(np.unique(dense)) == n
    assert p.like.status() == 0
    for count in (0, 1, 64, 449, 512):
        out = sparse_call(p.like, (th, nu), count)
        assert_sparse(out, dense, count, f"{name} (W = 512)")
        if p.hl:
            assert p.like.status() == 0


@pytest.mark.parametrize("name", SHARED_WS)
def test_sparse_back_to_back_counts(problems, name):
    """Counts 70, 1, 0, 70 on the handle's own workspace: a call leaves nothing
    behind (a ticket, a partial row) that the next count trips over, and count
    0 writes nothing.  (The count-0 call keeps slot 0 finite: a BK dataset
    reads nuisance row 0 for its T_dust table whatever the count.)"""
    p = problems(name)
    dense = p.dense()
    for count in (70, 1, 0, 70):
        out = sparse_call(p.like, p.bufs(), count, keep=1)
        assert_sparse(out, dense, count, f"{name} (after the previous count)")
        if p.hl:
            assert p.like.status() == 0


def _finite_inputs(like, n, lmax, n_fields):
    th = torch.tensor(syn.walker_theory(n, seed=3, lmax=lmax, n_fields=n_fields), device="cuda")
    return th, torch.ones((n, like.n_nuis), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("kind", ["exact", "sptpol"])
def test_sparse_unsupported_likelihoods_refuse(exact_data, sptpol_data, kind):
    """Exact CMBlikes and SPTpol have no sparse form: CMBL_ERR_UNSUPPORTED, nothing written."""
    from cosmomc_amd._native import NativeError
    from cosmomc_amd.likelihood import NativeCMBLikelihood
    if kind == "exact":
        like = NativeCMBLikelihood("exact", exact_data["exact_TE_lowl"])
        th, nu = _finite_inputs(like, 5, 29, 6)
    else:
        like = NativeCMBLikelihood("SPTPOL_TEEE", sptpol_data["SPTPOL_TEEE"], {})
        th, nu = _finite_inputs(like, 5, 8001, 3)
    out = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.tensor([3], dtype=torch.int32, device="cuda")
    with pytest.raises(NativeError) as e:
        like.loglike_batch_sparse(th, nu, out, cnt)
    assert e.value.code == ERR_UNSUPPORTED
    assert np.all(out.cpu().numpy() == SENTINEL)


def test_sparse_null_count_and_no_walkers(problems):
    """A null count pointer with W > 0 is CMBL_ERR_ARG; W = 0 returns 0; neither writes."""
    from cosmomc_amd import _native as N
    p = problems("plik_lite_TTTEEE")
    th, nu = p.bufs()
    out = torch.full((W,), SENTINEL, dtype=torch.float64, device="cuda")
    cnt = torch.tensor([W], dtype=torch.int32, device="cuda")
    args = (th.data_ptr(), th.stride(1), th.stride(0), nu.data_ptr(), nu.stride(0), out.data_ptr(), None, None)
    assert N.lib().cmbl_loglike_batch_sparse(p.like.handle, W, *args, None) == ERR_ARG
    assert N.lib().cmbl_loglike_batch_sparse(p.like.handle, 0, *args, cnt.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
