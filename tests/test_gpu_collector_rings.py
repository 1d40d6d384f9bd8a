"""The device sample collector (cmbs_collector_*, collector.hip, and
chain_moments_kernel's per-walker counts) where both of its rings wrap, at
every register width, on degenerate windows and on its error returns.

No test steps a sampler: a synthetic history (collector_fake.synth) is planted
block by block with history_restore, so the history ring wraps exactly as in
a run, and the whole history stays on the host for the restatement
(oracle/pyoracle.py collector_samples, pool_chain_statistics, confid_val;
collector_fake.FakeCollectorSampler keeps the per-walker lists).  Every edge a
scenario is there for is asserted from the restatement alone, so a test
cannot pass by not visiting it."""
import functools

import numpy as np
import pytest

import pyoracle as po
from collector_fake import LOGZERO, FakeCollectorSampler, ReplaySampler, synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FRACS = (0.0, 0.025, 0.3, 0.5)

MAIN = dict(W=150, n=5, seed=1, hist_cap=768, samp_cap=400, min_update=60, thin_limit=300,
            blocks=(37, 100, 1, 90, 64, 100) + (100,) * 10)


def _sampler(W, n):
    """A BatchedMCMC with no likelihood: only its history ring and collector are used."""
    from cosmomc_amd.sampler import BatchedMCMC
    used = list(range(1, n + 1))
    return BatchedMCMC(W, n, used, [used[:n // 2], used[n // 2:]], 1, -1e3 * np.ones(n), 1e3 * np.ones(n),
                       seed_ij=11, seed_kl=12)


def _planted(W, n, rows, hist_cap, samp_cap):
    """Sampler with `rows` in its history (restored in blocks of at most the ring) and the collector on."""
    s = ReplaySampler(_sampler(W, n), rows, hist_cap)
    s.collector_enable(samp_cap)
    s.step(len(rows))
    return s


def _snapshot(f, hist_cap):
    """The restatement's state now: what collector_state must return, each
    walker's list, and the ring facts the scenario's edges are read from."""
    start, count, burn, thin = f.collector_state()
    items = [list(st["items"]) for st in f.states]
    end = start.astype(int) + count
    first = np.array([it[len(it) // 2 - 1] if len(it) >= 2 else f.history_count() for it in items])
    return dict(T=f.history_count(), start=start, count=count, burn=burn, thin=thin, items=items,
                wrapped=end > f.cap,                                         # the list crosses the sample ring's seam
                win_wrapped=(end > f.cap) & (start.astype(int) + count // 2 - 1 < f.cap),
                in_ring=bool(np.all(f.history_count() - first <= hist_cap)))


_ORACLE_ARGS = ("W", "n", "seed", "hist_cap", "samp_cap", "min_update", "thin_limit", "blocks")


@functools.lru_cache(maxsize=None)
def _oracle_run(W, n, seed, hist_cap, samp_cap, min_update, thin_limit, blocks):
    """The restatement of a whole scenario, once: (rows, [(before thin, after thin) per block])."""
    rows = synth(W, n, sum(blocks), seed)
    rows.setflags(write=False)
    f = FakeCollectorSampler(W, n, rows=rows)
    f.collector_enable(samp_cap)
    snaps = []
    for blk in blocks:
        first = f.history_count()
        f.step(blk)
        f.collector_add(list(range(first, first + blk)), min_update)
        before = _snapshot(f, hist_cap)
        if thin_limit is not None:
            f.collector_thin(thin_limit)
        snaps.append((before, _snapshot(f, hist_cap)))
    return rows, snaps


def _assert_state(s, snap, what):
    start, count, burn, thin = s.collector_state()
    for name, got in (("count", count), ("burn", burn), ("thin", thin), ("start", start)):
        np.testing.assert_array_equal(got, snap[name], err_msg=f"{name} {what}")


def _pooled(rows, snap, n):
    return po.pool_chain_statistics([rows[it, :n, w] for w, it in enumerate(snap["items"])])


def _assert_moments(s, pooled, n, mean_tol, cov_tol, meanscov_tol, what):
    """collector_moments() and collector_moments(gmean) against the reference
    pooling, in test_gpu_collector's layout; *_tol = (rtol, atol)."""
    p1 = s.collector_moments().cpu().numpy()
    norm = p1[0]
    assert norm == pooled["counts"].sum(), what
    M = int(round(p1[-1]))
    assert M == len(pooled["counts"]), what
    np.testing.assert_allclose(p1[1:1 + n] / norm, pooled["mean"], rtol=mean_tol[0], atol=mean_tol[1], err_msg=what)
    np.testing.assert_allclose(p1[1 + n:1 + n + n * n].reshape(n, n) / norm, pooled["propose_cov"], rtol=cov_tol[0],
                               atol=cov_tol[1], err_msg=what)
    np.testing.assert_allclose(p1[1 + n + n * n:1 + n + 2 * n * n].reshape(n, n) / M, pooled["cov"], rtol=cov_tol[0],
                               atol=cov_tol[1], err_msg=what)
    p2 = s.collector_moments(p1[1:1 + n] / norm).cpu().numpy()
    np.testing.assert_allclose(p2.reshape(n, n) / norm * M / (M - 1), pooled["meanscov"], rtol=meanscov_tol[0],
                               atol=meanscov_tol[1], err_msg=what)
    return p1, p2


def _limit_refs(x, frac):
    """ConfidVal of one window column and what the device may differ by: nothing
    where no interpolation happens (pos an integer, or b == samps), else
    4 eps max(|x_b|, |x_b+1|) -- the GPU may contract v (1 - d) + d v1 into an fma."""
    ref = po.confid_val(x, frac)
    xs = np.sort(x)
    samps = xs.size
    tol = []
    for fr in (frac, 1.0 - frac):
        pos = (samps - 1) * fr + 1
        b = max(int(pos), 1)
        tol.append(4 * EPS * max(abs(xs[b - 1]), abs(xs[b])) if b < samps and pos > b else 0.0)
    return ref, tol


def _assert_limits(s, rows, snap, params, fracs, what, exact=False):
    for frac in fracs:
        lim = s.collector_limits(list(params), frac).cpu().numpy()
        for w, it in enumerate(snap["items"]):
            win = it[len(it) // 2 - 1:]
            for c, j in enumerate(params):
                ref, tol = _limit_refs(rows[win, j, w], frac)
                for side in (0, 1):
                    err = abs(lim[w, c, side] - ref[side])
                    assert err <= (0.0 if exact else tol[side]), (what, frac, w, j, side, lim[w, c, side], ref[side])
    return lim


def _main_edges(snaps, cfg):
    """Scenario 1's edges, from the restatement alone."""
    W = cfg["W"]
    ever_wrapped = np.zeros(W, dtype=bool)
    ever_win_wrapped = np.zeros(W, dtype=bool)
    thinned_wrapped = thinned_unburned = 0
    full = 0
    for b, (before, after) in enumerate(snaps):
        if b >= 3:                                            # the blocks whose windows are checked
            ever_wrapped |= before["wrapped"]
            ever_win_wrapped |= before["win_wrapped"]
        thinned_wrapped += int(np.sum(before["wrapped"] & (before["count"] > cfg["thin_limit"])))
        thinned_unburned += int(np.sum((before["burn"] == 0) & (before["count"] > cfg["thin_limit"])))
        full += int(np.sum(before["count"] == cfg["samp_cap"]))
        assert before["count"].max() <= cfg["samp_cap"]
        assert before["in_ring"] and after["in_ring"], f"a window left the history ring in block {b}"
    last = snaps[-1][1]
    return dict(wrapped=int(ever_wrapped.sum()), win_wrapped=int(ever_win_wrapped.sum()),
                thinned_wrapped=thinned_wrapped, thinned_unburned=thinned_unburned, full=full,
                thin=sorted(set(int(t) for t in last["thin"])),
                burned=int(last["burn"].sum()), never=int((last["burn"] == 0).sum()), T=last["T"])


def _drive_main(cfg, nblocks, check):
    """Scenario 1 on the device; check(s, b, before thin | None, after thin | None) after every block."""
    rows, snaps = _oracle_run(*(cfg[k] for k in _ORACLE_ARGS))
    s = ReplaySampler(_sampler(cfg["W"], cfg["n"]), rows, cfg["hist_cap"])
    s.collector_enable(cfg["samp_cap"])
    for b, blk in enumerate(cfg["blocks"][:nblocks]):
        first = s.history_count()
        s.step(blk)
        s.collector_add(list(range(first, first + blk)), cfg["min_update"])
        check(s, b, snaps[b][0], None)
        s.collector_thin(cfg["thin_limit"])
        check(s, b, None, snaps[b][1])
    return rows, snaps


def test_wrapped_rings_main_scenario():
    """150 walkers, 1392 planted steps in 16 blocks into a 768-row history ring
    and a 400-slot sample ring, Thin(2) above 300 items after every block.
    After every block count, burn, thin and start of every walker equal the
    restatement's, before and after the thinning; from the fourth block on the
    window moments (both passes) and the ConfidVal limits of every walker and
    parameter at limfrac 0, 0.025, 0.3 and 0.5 are compared before the
    thinning (the longest lists, the full ring) and the moments again after it.

    By the restatement alone (asserted below): 134 walkers burn in, the 14
    with a frozen parameter and 2 slow ones never do; 118 walkers have a list
    across the sample ring's seam at some check (114 a window across it); 269
    thinnings are of such a list; 3 lists fill the ring exactly (count 400);
    the thin factors end at 4 and 8; the history ring wraps from block 9 on and
    every window stays in it; 21 walkers have logZero rows."""
    cfg = MAIN
    n, W = cfg["n"], cfg["W"]
    rows, snaps = _oracle_run(*(cfg[k] for k in _ORACLE_ARGS))
    e = _main_edges(snaps, cfg)
    print("scenario 1 edges:", e)
    assert e["wrapped"] >= W // 3 and e["win_wrapped"] >= W // 3
    assert e["thinned_wrapped"] >= 1 and e["thinned_unburned"] >= 1
    assert max(e["thin"]) >= 4
    assert e["burned"] > 0 and e["never"] > 0
    assert e["T"] > cfg["hist_cap"]
    assert e["full"] >= 1
    logzero = np.any(rows[:, n, :] == LOGZERO, axis=0)
    assert logzero.sum() >= 1 and not logzero.all()
    frozen = [w for w in range(W) if w % 11 == 5]                # their last column is one value, windows included
    assert all(np.ptp(rows[snaps[-1][0]["items"][w], n - 1, w]) == 0 for w in frozen)
    assert not snaps[-1][1]["burn"][frozen].any()
    # a logZero row is skipped: those walkers' lists are shorter than the steps added before their burn-in
    assert np.any(snaps[0][0]["count"][logzero] < cfg["blocks"][0])

    tol = dict(mean_tol=(1e-11, 1e-13), cov_tol=(1e-10, 1e-13), meanscov_tol=(1e-8, 1e-13))

    def check(s, b, before, after):
        if before is not None:
            _assert_state(s, before, f"after block {b}")
            if b >= 3:
                _assert_moments(s, _pooled(rows, before, n), n, what=f"block {b}", **tol)
                _assert_limits(s, rows, before, range(n), FRACS, f"block {b}")
        else:
            _assert_state(s, after, f"after block {b}'s thin")
            if b >= 3:
                _assert_moments(s, _pooled(rows, after, n), n, what=f"block {b} thinned", **tol)

    _drive_main(cfg, len(cfg["blocks"]), check)


def test_side_stream_same_results():
    """Scenario 1's first 8 blocks under a torch side stream: every moment and
    limit is bit-identical to the default-stream run.  (The window check of
    collector_moments / collector_limits runs on the caller's stream, behind a
    pending collector_thin; a race there would not show reliably in a test.)"""
    def run():
        out = []

        def check(s, b, before, after):
            if b < 3:
                return
            if before is not None:
                _assert_state(s, before, f"after block {b}")
            p1 = s.collector_moments()
            out.append(p1.cpu().numpy())
            out.append(s.collector_moments(p1[1:1 + MAIN["n"]] / p1[0]).cpu().numpy())
            for frac in (0.025, 0.3):
                out.append(s.collector_limits(list(range(MAIN["n"])), frac).cpu().numpy())

        _drive_main(MAIN, 8, check)
        return out

    ref = run()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    assert len(ref) == len(got) and len(ref) > 0
    for k, (a, b) in enumerate(zip(ref, got)):
        np.testing.assert_array_equal(a, b, err_msg=f"output {k}")


WIDE = dict(W=300, hist_cap=384, samp_cap=640, min_update=60, thin_limit=None, blocks=(150,) * 4)


@pytest.mark.parametrize("n", [5, 12, 21, 40])
def test_every_width_more_walkers_than_threads(n):
    """coll_mean_kernel / coll_cov_kernel at their 8, 16, 32 and 64 widths and
    chain_moments_kernel's per-walker counts with W = 300 > its 256 threads,
    over a wrapped history ring (600 steps into 384 rows), no thinning.  By the
    restatement: about 230 walkers burn in, the lists hold 61 to 600 items,
    every window stays in the ring, and every walker from 256 on has another
    window (count or mean) than walker w - 256."""
    cfg = dict(WIDE, n=n, seed=n)
    W = cfg["W"]
    rows, snaps = _oracle_run(*(cfg[k] for k in _ORACLE_ARGS))
    last = snaps[-1][0]
    assert all(b["in_ring"] for b, _ in snaps) and last["T"] > cfg["hist_cap"]
    wcount = last["count"] - last["count"] // 2 + 1
    assert len(set(wcount.tolist())) >= 3
    wmean = np.array([rows[it[len(it) // 2 - 1:], :n, w].mean(axis=0) for w, it in enumerate(last["items"])])
    assert all(wcount[w] != wcount[w - 256] or np.all(wmean[w] != wmean[w - 256]) for w in range(256, W))
    assert np.sum(wcount[256:] != wcount[:W - 256]) >= 10
    print(f"n={n}: burned {int(last['burn'].sum())}, counts {last['count'].min()}..{last['count'].max()}, "
          f"{len(set(wcount.tolist()))} distinct window counts")

    s = ReplaySampler(_sampler(W, n), rows, cfg["hist_cap"])
    s.collector_enable(cfg["samp_cap"])
    for b, blk in enumerate(cfg["blocks"]):
        first = s.history_count()
        s.step(blk)
        s.collector_add(list(range(first, first + blk)), cfg["min_update"])
        _assert_state(s, snaps[b][0], f"after block {b}")
    _assert_moments(s, _pooled(rows, last, n), n, mean_tol=(1e-12, 1e-13), cov_tol=(1e-9, 1e-12),
                    meanscov_tol=(1e-9, 1e-12), what=f"n={n}")
    _assert_limits(s, rows, last, (0, n // 2, n - 1), (0.025, 0.3), f"n={n}")


def _plain_rows(T, n, W, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((T, n + 1, W))
    rows[:, n, :] = 0.5 * (rows[:, :n, :] ** 2).sum(axis=1)
    return rows


def test_windows_of_two_and_three():
    """Count 2 (window = items 1..2) and count 3 (window = items 1..3): moments
    and limits at limfrac 0, 0.3 and 0.5 (pos = 2 exactly at 0.5 of 3 items)."""
    W, n = 70, 3
    rows = _plain_rows(3, n, W, 21)
    s = _planted(W, n, rows, 16, 16)
    f = FakeCollectorSampler(W, n, rows=rows)
    f.collector_enable(16)
    f.step(3)
    for steps in ([0, 1], [2]):
        s.collector_add(steps, 60, check_burn=True)
        f.collector_add(steps, 60, True)
        snap = _snapshot(f, 16)
        assert np.all(snap["count"] == steps[-1] + 1)
        _assert_state(s, snap, f"{steps[-1] + 1} items")
        _assert_moments(s, _pooled(rows, snap, n), n, mean_tol=(1e-12, 1e-13), cov_tol=(1e-10, 1e-13),
                        meanscov_tol=(1e-8, 1e-13), what=f"{steps[-1] + 1} items")
        _assert_limits(s, rows, snap, range(n), (0.0, 0.3, 0.5), f"{steps[-1] + 1} items")


def test_limits_of_a_two_valued_column():
    """A column that only ever holds -2 or 0.5 (powers of two, so the
    interpolation is exact whether or not it is contracted): even walkers
    switch between them at random, the windows of walkers 1, 5, 9, ... are all
    -2 and those of walkers 3, 7, 11, ... all 0.5.  The radix select must land
    on the very values: limits equal ConfidVal exactly at every limfrac, with
    and without interpolation (40 items: a window of 21, pos = 11 at 0.5)."""
    W, n, T = 70, 3, 40
    rows = _plain_rows(T, n, W, 22)
    rng = np.random.default_rng(23)
    col = np.where(rng.random((T, W)) < 0.5, -2.0, 0.5)
    col[:, 1::4] = -2.0
    col[:, 3::4] = 0.5
    col[:T // 2 - 1, 1::2] = np.where(rng.random((T // 2 - 1, W // 2)) < 0.5, -2.0, 0.5)   # before the windows
    rows[:, 1, :] = col
    s = _planted(W, n, rows, 64, 64)
    f = FakeCollectorSampler(W, n, rows=rows)
    f.collector_enable(64)
    f.step(T)
    s.collector_add(list(range(T)), 60)
    f.collector_add(list(range(T)), 60, True)
    snap = _snapshot(f, 64)
    assert np.all(snap["count"] == T) and not snap["burn"].any()
    win = rows[T // 2 - 1:, 1, :]
    equal = np.all(win == win[0], axis=0)
    assert equal.sum() == W // 2 and set(np.unique(rows[:, 1, :])) == {-2.0, 0.5}
    assert {float(v) for v in win[0, equal]} == {-2.0, 0.5}
    assert all(len(np.unique(win[:, w])) == 2 for w in range(0, W, 2))
    _assert_state(s, snap, "two-valued column")
    _assert_limits(s, rows, snap, (1,), FRACS, "two-valued column", exact=True)
    _assert_limits(s, rows, snap, (0, 2), FRACS, "two-valued column's neighbours")
    _assert_moments(s, _pooled(rows, snap, n), n, mean_tol=(1e-12, 1e-13), cov_tol=(1e-10, 1e-13),
                    meanscov_tol=(1e-8, 1e-13), what="two-valued column")


def test_error_returns():
    """Every error return of the collector is a NativeError with the C message
    (host-side argument checks, or the in-bounds overflow flag of the add)."""
    from cosmomc_amd._native import NativeError
    W, n, hist_cap = 70, 3, 64
    rows = _plain_rows(3 * hist_cap, n, W, 31)
    rows[:, n, 17] = LOGZERO                                  # walker 17 is never anywhere else
    r = ReplaySampler(_sampler(W, n), rows, hist_cap)
    with pytest.raises(NativeError, match="collector not enabled"):
        r.collector_add([0], 60)
    r.collector_enable(50)
    r.step(60)
    with pytest.raises(NativeError, match="collector steps must increase"):
        r.collector_add([3, 3], 60)
    with pytest.raises(NativeError, match="collector steps must increase"):
        r.collector_add([5, 4], 60)
    with pytest.raises(NativeError, match=r"history step 60 is not in the ring \(count 60, capacity 64\)"):
        r.collector_add([59, 60], 60)
    with pytest.raises(NativeError, match=r"history step -1 is not in the ring"):
        r.collector_add([-1], 60)
    r.collector_add(list(range(10)), 60)
    _, count, _, _ = r.collector_state()
    assert count[17] == 0 and np.all(np.delete(count, 17) == 10)
    with pytest.raises(NativeError, match="a walker has 0 samples: too few for a window"):
        r.collector_moments()
    with pytest.raises(NativeError, match="a walker has 0 samples: too few for a window"):
        r.collector_limits([0], 0.025)
    with pytest.raises(NativeError, match="limit parameter 3 out of range"):
        r.collector_limits([3], 0.025)
    with pytest.raises(NativeError, match="sample list capacity 50 exceeded"):
        r.collector_add(list(range(10, 60)), 60)              # 60 items into 50 slots
    _, count, _, _ = r.collector_state()
    assert count[17] == 0 and np.all(np.delete(count, 17) == 50)
    r.step(10)                                                # step 0 left the ring of 64
    with pytest.raises(NativeError, match=r"history step 5 is not in the ring \(count 70, capacity 64\)"):
        r.collector_add([5], 60)

    # a window whose first step has left the history ring
    rows = _plain_rows(3 * hist_cap, n, W, 32)
    r = _planted(W, n, rows[:40], hist_cap, 64)
    r.planted = rows
    r.collector_add(list(range(40)), 60)
    assert np.isfinite(r.collector_moments().cpu().numpy()).all()
    r.step(hist_cap + 1)                                      # the window's first step, 19, is 86 rows back
    msg = r"a window starts at history step 19, no longer in the ring \(count 105, capacity 64\)"
    with pytest.raises(NativeError, match=msg):
        r.collector_moments()
    with pytest.raises(NativeError, match=msg):
        r.collector_limits([0, 1], 0.3)


# 240 slots: the longest list before its burn-in DeleteRange just fits (the fake raises if one does not)
REPLAY = dict(W=70, n=3, T=700, hist_cap=320, samp_cap=240, R_stop=0.07)


@functools.lru_cache(maxsize=None)
def _replay_rows():
    gen = FakeCollectorSampler(REPLAY["W"], REPLAY["n"], seed=11)
    gen.step(REPLAY["T"])
    rows = np.array(gen.rows)
    rows.setflags(write=False)
    return rows


def _run_chain_collector(sampler, cap):
    """ChainCollector over `sampler` until the planted rows run out or it is
    done: per exchange the history step, count0, R-1, the learnt proposal, the
    thin factors after it, and the lists (start, count) it windowed over --
    read just before its thinning."""
    from cosmomc_amd.converge import ChainCollector, CollectorSettings
    st = CollectorSettings(MPI_R_Stop=REPLAY["R_stop"], MPI_Sample_update_freq=10)
    with pytest.warns(UserWarning, match="lists are thinned at 120 items"):
        col = ChainCollector(sampler, st, num_slow=2, num_fast=1, sample_capacity=cap)
    seen = {}
    thin_lists = sampler.collector_thin

    def thin_and_record(limit):
        seen["start"], seen["count"], _, _ = sampler.collector_state()
        thin_lists(limit)

    sampler.collector_thin = thin_and_record
    log = []
    while sampler.history_count() + col.next_block() <= REPLAY["T"] and not col.done:
        sampler.step(col.next_block())
        r = col.process()
        if r is not None:
            _, _, _, thin = sampler.collector_state()
            log.append(dict(step=sampler.history_count(), count0=col.count0, R=r.R, propose_cov=r.propose_cov,
                            thin=thin.copy(), converged=r.converged, update=r.update_proposal,
                            start=seen["start"].copy(), count=seen.pop("count").copy()))
    return col, log


def test_chain_collector_on_wrapped_rings_device_against_host():
    """ChainCollector over a ReplaySampler (device collector) and over
    FakeCollectorSampler (the restatement) given the same 700 planted steps, a
    320-row history ring and 240-slot sample rings thinned at the default
    cap // 2: the same exchanges at the same steps, count0, update_freq,
    all_burn, done and thin factors, the same lists (start, count) under every
    exchange, R-1 within 1e-8 and the learnt proposal within 1e-10.  By the
    fake alone: 6 exchanges at steps 249 .. 576, every list thinned (factors
    up to 8), R-1 = 0.159, 0.121, 0.091, 0.073, 0.065, 0.051 against a stop at
    0.07 (converged at the sixth), and 70, 13, 3, 67, 0, 18 of the 70 lists
    across the sample ring's seam at the exchanges, 137 of them thinned there."""
    cfg = REPLAY
    rows = _replay_rows()
    fake = FakeCollectorSampler(cfg["W"], cfg["n"], rows=rows)
    colf, logf = _run_chain_collector(fake, cfg["samp_cap"])
    rstop = float(np.float32(cfg["R_stop"]))
    assert len(logf) >= 4
    assert max(int(e["thin"].max()) for e in logf) >= 2
    assert all(abs(e["R"] - rstop) > 1e-6 * rstop for e in logf)
    assert cfg["T"] > cfg["hist_cap"] and logf[-1]["step"] > cfg["hist_cap"]
    across = [e["start"].astype(int) + e["count"] > cfg["samp_cap"] for e in logf]
    wrapped = [int(a.sum()) for a in across]
    thinned_wrapped = sum(int(np.sum(a & (e["count"] > cfg["samp_cap"] // 2))) for a, e in zip(across, logf))
    assert sum(w >= cfg["W"] // 3 for w in wrapped) >= 2, wrapped
    assert thinned_wrapped >= cfg["W"] // 3
    print("replay:", [(e["step"], e["count0"], round(e["R"], 5), sorted(set(e["thin"].tolist()))) for e in logf],
          "wrapped", wrapped, "thinned while wrapped", thinned_wrapped, "done", colf.done)

    dev = ReplaySampler(_sampler(cfg["W"], cfg["n"]), rows, cfg["hist_cap"])
    cold, logd = _run_chain_collector(dev, cfg["samp_cap"])
    assert [e["step"] for e in logd] == [e["step"] for e in logf]
    for a, b in zip(logd, logf):
        assert a["count0"] == b["count0"] and a["converged"] == b["converged"] and a["update"] == b["update"]
        np.testing.assert_array_equal(a["thin"], b["thin"])
        np.testing.assert_array_equal(a["start"], b["start"])
        np.testing.assert_array_equal(a["count"], b["count"])
        assert a["R"] == pytest.approx(b["R"], rel=1e-8)
        np.testing.assert_allclose(a["propose_cov"], b["propose_cov"], rtol=1e-10, atol=1e-14)
    for k in ("count0", "update_freq", "all_burn", "done", "burn0", "min_count", "min_update"):
        assert getattr(cold, k) == getattr(colf, k), k
    for x, y in zip(dev.collector_state(), fake.collector_state()):
        np.testing.assert_array_equal(x, y)
