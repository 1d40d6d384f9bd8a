"""bench.py's command line: a plain run is the headline alone, every other leg
sits behind --full, and --dump-outputs writes the sampler state as float64
.npy files.  Host logic only (no GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_files(tmp_path):
    W, n = 5, 7
    state = (np.arange(W * n, dtype=np.float64).reshape(W, n), np.linspace(1.0, 2.0, W), np.ones(W),
             np.arange(W, dtype=np.int32))
    d = tmp_path / "out" / "dump"
    bench.dump_outputs(str(d), state, 0, 1)
    assert sorted(os.listdir(d)) == ["P.npy", "cur_like.npy", "mult.npy", "n_accept.npy"]
    for name, ref in zip(("P", "cur_like", "mult", "n_accept"), state):
        got = np.load(d / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.array_equal(got, ref)
    bench.dump_outputs(str(d), state, 1, 2)           # several ranks: one set of files each
    assert np.array_equal(np.load(d / "P_rank1.npy"), state[0])
