"""bench.py --dump-outputs: the arrays of the last timed step as <name>.npy, float32 / float64, bounded in size."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def step_result():
    g = torch.Generator().manual_seed(0)
    return {"sample": torch.randn(4, 3, 8, 8, generator=g), "pred_xstart": torch.randn(4, 3, 8, 8, generator=g).bfloat16(),
            "t": torch.full((4,), 7, dtype=torch.long)}


def test_dump_writes_every_array_whole(tmp_path):
    out = step_result()
    written = bench.dump_outputs(out, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["pred_xstart.npy", "sample.npy", "t.npy"]
    s, x0, t = (np.load(tmp_path / "d" / f"{n}.npy") for n in ("sample", "pred_xstart", "t"))
    assert s.dtype == np.float32 and x0.dtype == np.float32 and t.dtype == np.float64
    assert np.array_equal(s, out["sample"].numpy())
    assert np.array_equal(x0, out["pred_xstart"].float().numpy())
    assert np.array_equal(t, np.full(4, 7.0))
    assert written["sample"] == [[4, 3, 8, 8], [4, 3, 8, 8]]


def test_dump_samples_the_same_elements_above_the_budget(tmp_path, monkeypatch):
    out = step_result()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1024)
    a = bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs({k: v.clone() for k, v in out.items()}, str(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 1024
    for name in ("sample", "pred_xstart", "t"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.ndim == 1 and 0 < x.size < out[name].numel() and np.array_equal(x, y)
        assert a[name][1] == list(out[name].shape)
    # the sample is a subset of the array, in flattened order
    s = np.load(tmp_path / "a" / "sample.npy")
    full = out["sample"].numpy().reshape(-1)
    pos = [int(np.flatnonzero(full == v)[0]) for v in s]
    assert pos == sorted(pos)
