"""A host stand-in for BatchedMCMC's collector interface (history ring +
cmbs_collector_*), built on the oracle's item-by-item restatement, so that
ChainCollector's cross-rank logic runs on CPU with gloo, and the helpers that
plant a synthetic history into a real sampler's ring.  Test helpers only."""
import numpy as np

import pyoracle as po

LOGZERO = 1e30


def synth(W, n, T, seed):
    """A synthetic history [T, n + 1, W] (history_host's layout: the used
    parameters, then the like).  Walker w moves at a step with probability
    0.08 + 0.8 ((37 w) mod W) / W; a move adds 0.5 N(0,1) to parameters
    0 .. n//2-1 on even steps and to the rest on odd steps.  Parameter n-1 of
    the walkers with w % 11 == 5 never moves (they can never burn in, and the
    column is constant over their windows).  The like is |x|^2 / 2, except
    that the walkers with w % 7 == 3 are at logZero in their first 1 + w % 5
    rows and in 6 further random rows."""
    rng = np.random.default_rng(seed)
    w = np.arange(W)
    p = 0.08 + 0.8 * ((37 * w) % W) / W
    x = rng.standard_normal((W, n))
    cols = np.arange(n)
    frozen = (w % 11 == 5)[:, None] & (cols == n - 1)[None, :]
    rows = np.empty((T, n + 1, W))
    for t in range(T):
        move = rng.random(W) < p
        d = 0.5 * rng.standard_normal((W, n))
        half = cols < n // 2 if t % 2 == 0 else cols >= n // 2
        x = np.where(move[:, None] & half[None, :] & ~frozen, x + d, x)
        rows[t, :n, :] = x.T
        rows[t, n, :] = 0.5 * (x * x).sum(axis=1)
    for v in w[w % 7 == 3]:
        rows[:1 + v % 5, n, v] = LOGZERO
        rows[rng.choice(T, 6, replace=False), n, v] = LOGZERO
    return rows


class FakeCollectorSampler:
    """W synthetic chains (global walker ids first_walker ..): each step a
    chain moves (AR(1) step in a random subset of its parameters) with
    probability 0.6, else stays -- deterministic per global walker.  With
    `rows` ([T, n + 1, W], history_host's layout) the chains are those planted
    rows instead, and step(k) only advances through them."""

    def __init__(self, W, n=3, first_walker=0, seed=11, rows=None):
        self.W, self.n = W, n
        self.params_used = list(range(1, n + 1))
        self.first_walker = first_walker
        self.planted = None if rows is None else np.asarray(rows, dtype=np.float64)
        self.nrows = 0
        if self.planted is None:
            self.rngs = [np.random.default_rng([seed, first_walker + w]) for w in range(W)]
            self.cur = np.array([r.standard_normal(n) * 2 for r in self.rngs])
        self.rows = []
        self.states = None
        self.cap = 0

    def step(self, k):
        if self.planted is not None:
            assert self.nrows + k <= self.planted.shape[0], "no planted rows left"
            self.nrows += k
            return
        for _ in range(k):
            for w, r in enumerate(self.rngs):
                if r.random() < 0.6:
                    mask = r.random(self.n) < 0.7
                    self.cur[w] = np.where(mask, 0.5 * self.cur[w] + 0.87 * r.standard_normal(self.n), self.cur[w])
            row = np.concatenate([self.cur.T, 0.5 * (self.cur ** 2).sum(axis=1)[None, :]], axis=0)
            self.rows.append(row)
        self.nrows = len(self.rows)

    def _rows(self):
        return self.planted if self.planted is not None else np.array(self.rows)

    def history_count(self):
        return self.nrows

    def collector_enable(self, cap):
        self.states = [{"items": [], "sample_num": 0, "burn": False, "changes": None} for _ in range(self.W)]
        self.thin = np.ones(self.W, dtype=int)
        self.deleted = np.zeros(self.W, dtype=int)      # items the burn-in DeleteRange removed
        self.cap = cap

    def collector_add(self, steps, min_update, check_burn=True):
        rows = self._rows()
        for w in range(self.W):
            st = self.states[w]
            was_burned = st["burn"]
            if not was_burned:
                # the same items without the DeleteRange: the difference is what it removed
                keep = {"items": list(st["items"]), "sample_num": st["sample_num"], "burn": False,
                        "changes": None if st["changes"] is None else st["changes"].copy()}
                po.collector_samples(rows[:, :, w], steps, 1 << 60, check_burn, int(self.thin[w]), keep)
            po.collector_samples(rows[:, :, w], steps, min_update, check_burn, int(self.thin[w]), st)
            if st["burn"] and not was_burned:
                self.deleted[w] = len(keep["items"]) - len(st["items"])
            longest = len(st["items"]) if was_burned else len(keep["items"])     # before any DeleteRange
            if self.cap and longest > self.cap:
                raise OverflowError(f"walker {w}'s list reached {longest} items: over the ring's {self.cap}")

    def collector_state(self):
        """(start, count, burn, thin) as the device's: start is the ring slot
        of the first item, which only the burn-in DeleteRange moves."""
        count = np.array([len(s["items"]) for s in self.states], dtype=np.int32)
        burn = np.array([int(s["burn"]) for s in self.states], dtype=np.int32)
        start = (self.deleted % self.cap if self.cap else np.zeros(self.W)).astype(np.int32)
        return start, count, burn, self.thin.astype(np.int32)

    def collector_thin(self, limit):
        for w, s in enumerate(self.states):
            if len(s["items"]) > limit:
                s["items"] = s["items"][::2]
                self.thin[w] *= 2

    def _window(self, w):
        it = self.states[w]["items"]
        c = len(it)
        return self._rows()[it[c // 2 - 1:], :self.n, w]

    def collector_moments(self, gmean=None):
        import torch
        n = self.n
        if gmean is None:
            out = np.zeros(2 + n + 2 * n * n)
        else:
            out = np.zeros(n * n)
            g = np.asarray(gmean.cpu() if hasattr(gmean, "cpu") else gmean)
        for w in range(self.W):
            x = self._window(w)
            cw = x.shape[0]
            m = x.mean(axis=0)
            C = (x - m).T @ (x - m) / cw
            if gmean is None:
                out[0] += cw
                out[1:1 + n] += cw * m
                out[1 + n:1 + n + n * n] += cw * C.ravel()
                out[1 + n + n * n:1 + n + 2 * n * n] += C.ravel()
                out[-1] += 1
            else:
                out += cw * np.outer(m - g, m - g).ravel()
        return torch.tensor(out, dtype=torch.float64)

    def collector_limits(self, params, limfrac):
        import torch
        out = np.zeros((self.W, len(params), 2))
        for w in range(self.W):
            x = self._window(w)
            for c, j in enumerate(params):
                out[w, c] = po.confid_val(x[:, j], limfrac)
        return torch.tensor(out)

    def set_covariance(self, cov):
        pass

    device = "cpu"


class ReplaySampler:
    """A real BatchedMCMC whose step(k) puts the next k planted rows
    ([T, n + 1, W]) into its history ring (history_restore, in blocks of at
    most the ring's capacity) instead of sampling; everything else is the
    sampler's own."""

    def __init__(self, sampler, rows, hist_cap):
        self.s = sampler
        self.planted = np.asarray(rows, dtype=np.float64)
        self.hist_cap = hist_cap
        sampler.enable_history(hist_cap)

    def step(self, k):
        first = self.s.history_count()
        assert first + k <= self.planted.shape[0], "no planted rows left"
        while k > 0:
            b = min(k, self.hist_cap)
            self.s.history_restore(first, self.planted[first:first + b])
            first, k = first + b, k - b

    def set_covariance(self, cov):
        pass

    def __getattr__(self, name):
        return getattr(self.s, name)
