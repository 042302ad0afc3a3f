"""CPU: the image-metrics entries' ABI and refusals, the float64 reference against closed forms, the host arithmetic of
flair_amd.metrics, evaluate_dirs' refusals and the evaluate / restore --ground-truth command lines."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def png(path, h, w, value=0):
    from PIL import Image
    arr = np.full((h, w, 3), value, dtype=np.uint8)
    Image.fromarray(arr, mode="RGB").save(path, format="PNG")


def test_library_exports_the_entries_at_abi_15():
    from flair_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "flair_image_metrics") and hasattr(lib, "flair_image_metrics_workspace")
    assert lib.flair_abi_version() >= 15
    header = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    assert "size_t flair_image_metrics_workspace(int N, int H, int W);" in header
    assert re.search(r"int flair_image_metrics\(const uint8_t\* a, const uint8_t\* b, int N, int H, int W, double\* out, void\* ws,"
                     r"\s+size_t ws_bytes,\s+hipStream_t stream\);", header)


def test_workspace_query_follows_the_tile():
    """One (SSIM sum, squared error) pair of doubles per workgroup: N x 3 channels x tiles of TILE_H x TILE_W map pixels; the
    Python mirror of the tile constants is the source's."""
    from flair_amd import _lib, metrics
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "metrics.hip")).read()
    tw, th = (int(re.search(rf"\b{n} = (\d+)", src).group(1)) for n in ("MT_TW", "MT_TH"))
    assert (metrics.TILE_H, metrics.TILE_W) == (th, tw)
    for N, H, W in [(1, 11, 11), (2, 12, 43), (1, th + 10, tw + 10), (3, th + 11, tw + 11), (2, 2 * th + 21, 2 * tw + 15), (10, 768, 1280)]:
        tiles = -(-(H - 10) // th) * -(-(W - 10) // tw)
        assert _lib.image_metrics_workspace(N, H, W) == N * 3 * tiles * 16
    for bad in [(0, 64, 64), (1, 10, 64), (1, 64, 10), (-1, 64, 64)]:
        assert _lib.image_metrics_workspace(*bad) == 0


def test_entry_refuses_before_any_launch():
    """Null pointer, H = 10, N = 0 and a short workspace: rc == -1 with the entry's name, on a machine without a GPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)
    need = _lib.image_metrics_workspace(1, 32, 32)
    assert need == 48
    cases = [((None, p, 1, 32, 32, p, p, need), b"null pointer"), ((p, p, 1, 32, 32, None, p, need), b"null pointer"),
             ((p, p, 1, 32, 32, p, None, need), b"null pointer"), ((p, p, 1, 10, 32, p, p, need), b"smaller than the 11x11"),
             ((p, p, 1, 32, 10, p, p, need), b"smaller than the 11x11"), ((p, p, 0, 32, 32, p, p, need), b"N = 0"),
             ((p, p, 1, 32, 32, p, p, need - 1), b"ws_bytes = 47")]
    for (a, b, N, H, W, out, ws, nbytes), what in cases:
        rc = lib.flair_image_metrics(a, b, N, H, W, out, ws, ctypes.c_size_t(nbytes), None)
        msg = lib.flair_last_error()
        assert rc == -1 and b"flair_image_metrics" in msg and what in msg, (rc, msg)


def test_ops_wrapper_refuses_wrong_tensors():
    from flair_amd import ops
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        ops.image_metrics(a, torch.zeros(1, 16, 17, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.image_metrics(a.float(), a.float())
    with pytest.raises(ValueError, match="dense"):
        ops.image_metrics(a.permute(0, 2, 1, 3), a.permute(0, 2, 1, 3))


# ------------------------------------------------------------------------------------------- the reference itself
def test_reference_window():
    g = mr.gaussian_window()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1]) and g.argmax() == 5
    assert abs(g[5] / g[4] - math.exp(1 / 4.5)) < 1e-12


@pytest.mark.parametrize("va,vb", [(0, 255), (127, 128), (10, 200), (255, 255)])
def test_reference_constant_frames_closed_form(va, vb):
    """x = a, y = b constant: the variances and the covariance vanish and SSIM = (2ab + C1) / (a^2 + b^2 + C1)."""
    a = np.full((2, 13, 17, 3), va, dtype=np.uint8)
    b = np.full((2, 13, 17, 3), vb, dtype=np.uint8)
    sse, sums, ssim, psnr = mr.reference(a, b)
    want = (2.0 * va * vb + mr.C1) / (va * va + vb * vb + mr.C1)
    assert np.abs(ssim - want).max() < 1e-9
    assert np.abs(sums / (3 * 7) - want).max() < 1e-9
    assert (sse == 13 * 17 * 3 * (va - vb) ** 2).all()
    if va == vb:
        assert np.isinf(psnr).all()
    else:
        assert np.abs(psnr - 20 * math.log10(255.0 / abs(va - vb))).max() < 1e-9


def test_reference_identical_frames_give_one():
    a = np.random.default_rng(0).integers(0, 256, (2, 23, 31, 3), dtype=np.uint8)
    sse, sums, ssim, psnr = mr.reference(a, a)
    assert (sse == 0).all() and np.isinf(psnr).all() and np.abs(ssim - 1).max() < 1e-12
    assert mr.ssim_map(a[0, :, :, 0], a[0, :, :, 0]).shape == (13, 21)


# ------------------------------------------------------------------------------------------- host arithmetic
def test_psnr_ssim_host_arithmetic(monkeypatch):
    """psnr_ssim turns the kernel's rows into PSNR over the 3 H W bytes, inf at sse = 0, and the mean SSIM of the three channels."""
    from flair_amd import metrics, ops
    H, W = 21, 31
    rows = torch.tensor([[0.0, 231.0, 231.0, 231.0], [3.0 * H * W, 100.0, 110.0, 121.0]], dtype=torch.float64)
    monkeypatch.setattr(ops, "image_metrics", lambda a, b: rows)
    got = metrics.psnr_ssim(torch.zeros(2, H, W, 3, dtype=torch.uint8), torch.zeros(2, H, W, 3, dtype=torch.uint8))
    assert got["sse"] == [0, 3 * H * W] and all(isinstance(v, int) for v in got["sse"])
    assert got["psnr"][0] == math.inf and abs(got["psnr"][1] - 20 * math.log10(255.0)) < 1e-12
    assert got["ssim"][0] == 1.0 and abs(got["ssim"][1] - 331.0 / (3 * 11 * 21)) < 1e-15


def test_format_report_four_decimals():
    from flair_amd import metrics
    res = dict(frames=[dict(name="0000.png", psnr=math.inf, ssim=1.0), dict(name="0001.png", psnr=31.23456, ssim=0.912349)],
               mean=dict(psnr=math.inf, ssim=0.9561745), count=2)
    lines = metrics.format_report(res)
    assert lines[0] == "0000.png  psnr inf  ssim 1.0000" and lines[1] == "0001.png  psnr 31.2346  ssim 0.9123"
    assert lines[2] == "mean of 2 frames  psnr inf  ssim 0.9562"


# ------------------------------------------------------------------------------------------- evaluate_dirs refusals
def test_evaluate_dirs_refusals(tmp_path):
    from flair_amd import metrics
    a, b, empty = tmp_path / "a", tmp_path / "b", tmp_path / "empty"
    for d in (a, b, empty):
        d.mkdir()
    for i in range(2):
        png(a / f"{i:04d}.png", 16, 20)
    png(b / "0000.png", 16, 20)
    with pytest.raises(ValueError, match=r"holds 2 frames and .* holds 1"):
        metrics.evaluate_dirs(str(a), str(b), "cpu")
    png(b / "0001.png", 16, 24)
    with pytest.raises(ValueError, match=r"0001\.png is 16x20 and .*0001\.png is 16x24"):
        metrics.evaluate_dirs(str(a), str(b), "cpu")
    png(a / "0001.png", 10, 20)
    png(b / "0001.png", 10, 20)
    with pytest.raises(ValueError, match=r"0001\.png .* 10x20.*at least 11 pixels"):
        metrics.evaluate_dirs(str(a), str(b), "cpu")
    for x, y in ((empty, a), (a, empty)):
        with pytest.raises(ValueError, match=f"no frame files in {re.escape(str(empty))}"):
            metrics.evaluate_dirs(str(x), str(y), "cpu")


def test_groups_break_at_a_size_change():
    from flair_amd import metrics
    sizes = [(16, 16)] * 5 + [(16, 32)] * 2 + [(16, 16)]
    assert metrics._groups(sizes, 4) == [(0, 4), (4, 1), (5, 2), (7, 1)]
    assert metrics._groups(sizes[:3], 8) == [(0, 3)]


def test_frame_batches_on_the_host(tmp_path):
    """io.iter_frame_batches without a GPU: HWC uint8 stacks of every list, group by group; metrics.json is no frame."""
    from flair_amd import io as fio
    for i in range(3):
        png(tmp_path / f"{i}.png", 12, 14, value=10 * i)
    (tmp_path / "metrics.json").write_text("{}")
    paths = fio.list_frames(str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["0.png", "1.png", "2.png"]
    assert fio.frame_size(paths[0]) == (12, 14)
    got = list(fio.iter_frame_batches([paths, paths[::-1]], [(0, 2), (2, 1)], "cpu"))
    assert [f for f, _ in got] == [0, 2]
    (x, y), (x2, y2) = got[0][1], got[1][1]
    assert x.shape == (2, 12, 14, 3) and x.dtype == torch.uint8 and x2.shape == (1, 12, 14, 3)
    assert all(t.is_contiguous() for t in (x, y, x2, y2))
    assert x[:, 0, 0, 0].tolist() == [0, 10] and y[:, 0, 0, 0].tolist() == [20, 10] and x2[0, 0, 0, 0] == 20 and y2[0, 0, 0, 0] == 0
    with pytest.raises(FileNotFoundError):
        list(fio.iter_frame_batches([[str(tmp_path / "missing.png")]], [(0, 1)], "cpu"))


# ------------------------------------------------------------------------------------------- command line
def test_evaluate_and_ground_truth_parse():
    from flair_amd.__main__ import make_parser
    ap = make_parser()
    e = ap.parse_args(["evaluate", "out", "truth", "--json", "m.json", "--device", "cuda:1"])
    assert (e.command, e.restored_dir, e.truth_dir, e.json, e.device) == ("evaluate", "out", "truth", "m.json", "cuda:1")
    e = ap.parse_args(["evaluate", "out", "truth"])
    assert e.json is None and e.device is None
    r = ap.parse_args(["restore", "gaussian", "in", "out", "--ground-truth", "clean"])
    assert r.ground_truth == "clean" and r.paths == ["in", "out"]
    assert ap.parse_args(["restore", "gaussian", "in", "out"]).ground_truth is None
    assert not hasattr(ap.parse_args(["jpeg-demo"]), "ground_truth")
    with pytest.raises(SystemExit):
        ap.parse_args(["evaluate", "only_one"])


def test_evaluate_main_reports_refusals(tmp_path):
    from flair_amd.__main__ import main
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    png(tmp_path / "a" / "0.png", 16, 16)
    with pytest.raises(SystemExit, match="no frame files"):
        main(["evaluate", str(tmp_path / "a"), str(tmp_path / "b")])


def test_restore_ground_truth_scores_every_video(tmp_path, monkeypatch, capsys):
    """restore --ground-truth with --output-root: evaluate_dirs runs once per video on (its output, ROOT/<its name>) after the
    video is written, the means are logged and metrics.json lands next to the frames."""
    from flair_amd import metrics, pipeline
    from flair_amd.__main__ import main
    vids, truth, out = tmp_path / "videos", tmp_path / "truth", tmp_path / "out"
    for name in ("a", "b"):
        for root in (vids, truth):
            (root / name).mkdir(parents=True)
            png(root / name / "0000.png", 16, 16)
    written, calls = [], []

    class Fake:
        def restore_video_files(self, v, o, **hp):
            os.makedirs(o, exist_ok=True)
            png(os.path.join(o, "0000.png"), 16, 16)
            written.append(o)
            return 1

    def evaluate(restored, truth_dir, device, batch=8):
        assert restored in written, "evaluated before the video was written"
        calls.append((restored, truth_dir))
        return dict(frames=[dict(name="0000.png", psnr=30.5, ssim=0.875)], mean=dict(psnr=30.5, ssim=0.875), count=1)

    monkeypatch.setattr(pipeline, "build_pipeline", lambda *a, **k: Fake())
    monkeypatch.setattr(metrics, "evaluate_dirs", evaluate)
    try:
        assert main(["restore", "gaussian", str(vids / "a"), str(vids / "b"), "--output-root", str(out),
                     "--ground-truth", str(truth)]) == 0
        assert calls == [(str(out / "a"), str(truth / "a")), (str(out / "b"), str(truth / "b"))]
        for name in ("a", "b"):
            got = json.load(open(out / name / "metrics.json"))
            assert got["count"] == 1 and got["mean"] == dict(psnr=30.5, ssim=0.875) and got["frames"][0]["name"] == "0000.png"
        text = capsys.readouterr().out
        assert text.count("psnr 30.5000  ssim 0.8750") == 2
        # one video: the directory itself
        calls.clear()
        assert main(["restore", "gaussian", str(vids / "a"), str(out / "single"), "--ground-truth", str(truth / "a")]) == 0
        assert calls == [(str(out / "single"), str(truth / "a"))] and os.path.isfile(out / "single" / "metrics.json")
        # without the option nothing is evaluated
        calls.clear()
        assert main(["restore", "gaussian", str(vids / "a"), str(out / "plain")]) == 0
        assert calls == [] and not os.path.exists(out / "plain" / "metrics.json")
        with pytest.raises(SystemExit, match="ground truth .* is not a directory"):
            main(["restore", "gaussian", str(vids / "a"), str(vids / "b"), "--output-root", str(out), "--ground-truth", str(vids / "a")])
    finally:
        torch.set_grad_enabled(True)
