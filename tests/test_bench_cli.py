"""bench.py's command line and its --dump-outputs writer, without a device:
a plain run asks for none of the --full legs, and the dump is float64, keyed by
trial id, the same rows from call to call, and sampled past the row limit."""
import os
import sys

import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

import bench
from shrewd_amd.fi import HIST_DT, OUTCOME_DT


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_and_full_arguments(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    a = _parse(monkeypatch, "--full", "--dump-outputs", str(tmp_path))
    assert a.full and a.dump_outputs == str(tmp_path)
    assert a.workloads and not a.no_cpu_baseline      # what --full runs by default


def _fake_step(T):
    import torch
    rng = np.random.default_rng(7)
    out = np.zeros(T, OUTCOME_DT)
    out["cls"] = rng.integers(0, 6, T)
    out["sub"] = rng.integers(0, 16, T)
    out["exit_code"] = rng.integers(0, 256, T)
    out["flags"] = rng.integers(0, 4, T)
    out["detail"] = rng.integers(0, 1 << 32, T, dtype=np.uint64)
    out["ninst"] = rng.integers(0, 1 << 40, T, dtype=np.uint64)
    h = np.zeros(1, HIST_DT)[0]
    h["counts"][1, 2, 3] = 5
    h["crash_sub"][4] = 6
    h["escape_sub"][1] = 7
    h["trials"] = T
    h["guest_insts"] = int(out["ninst"].sum())
    h["device_insts"] = 99                             # a device counter, not a result: not dumped
    return out, torch.from_numpy(out.view(np.uint8).copy()), h


def test_dump_outputs_whole_and_sampled(tmp_path):
    T, first = 1000, 3000
    out, d_out, h = _fake_step(T)
    bench.dump_outputs(str(tmp_path / "a"), d_out, h, first, T)
    o, hist = np.load(tmp_path / "a" / "outcomes.npy"), np.load(tmp_path / "a" / "histogram.npy")
    assert sorted(os.listdir(tmp_path / "a")) == ["histogram.npy", "outcomes.npy"]
    assert o.dtype == np.float64 and o.shape == (T, 7) and hist.dtype == np.float64
    assert np.array_equal(o[:, 0], first + np.arange(T))
    for c, f in enumerate(("cls", "sub", "exit_code", "flags", "detail", "ninst"), 1):
        assert np.array_equal(o[:, c], out[f].astype(np.float64)), f
    n = h["counts"].size
    assert hist.size == n + 16 + 8 + 2 and hist.sum() == 5 + 6 + 7 + T + float(h["guest_insts"])
    assert hist[n + 4] == 6 and hist[n + 16 + 1] == 7 and hist[-2] == T and hist[-1] == float(h["guest_insts"])
    # past the row limit: a sample of that many rows, ascending, the same in every call
    bench.dump_outputs(str(tmp_path / "b"), d_out, h, first, T, max_rows=100)
    bench.dump_outputs(str(tmp_path / "c"), d_out, h, first, T, max_rows=100)
    s, s2 = np.load(tmp_path / "b" / "outcomes.npy"), np.load(tmp_path / "c" / "outcomes.npy")
    assert s.shape == (100, 7) and np.array_equal(s, s2)
    ids = s[:, 0].astype(int) - first
    assert np.all(np.diff(ids) > 0) and ids.min() >= 0 and ids.max() < T
    assert np.array_equal(s, o[ids])
    assert np.array_equal(np.load(tmp_path / "b" / "histogram.npy"), hist)
