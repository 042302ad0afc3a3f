"""CPU: scene cuts -- the ABI entry and its refusals, the rule on the fixture sequences of tests/scenes_ref.py (margins of the
restatement first, then flair_amd.scenes against it), window_plan, interpolation that does not cross a cut with a stand-in
network, the cuts file and the command line's refusals."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import scenes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ ABI
def test_library_exports_the_entry():
    from flair_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "flair_block_luma_sums")
    assert lib.flair_abi_version() >= 18
    header = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    assert re.search(r"int flair_block_luma_sums\(const uint8_t\* frames, int N, int H, int W, long long\* out, hipStream_t stream\);",
                     header)


def test_entry_refusals_need_no_gpu():
    """The C entry validates before it touches the stream: each refusal returns -1 with a message."""
    from flair_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)
    for frames, N, H, W, out, what in ((None, 1, 8, 8, p, b"null pointer"), (p, 1, 8, 8, None, b"null pointer"),
                                      (p, 0, 8, 8, p, b"N = 0"), (p, 1, 7, 8, p, b"7x8"), (p, 1, 8, 7, p, b"8x7"),
                                      (p, 1, 8, 8, ctypes.c_void_p(68), b"8-byte aligned")):
        rc = lib.flair_block_luma_sums(frames, N, H, W, out, None)
        msg = lib.flair_last_error()
        assert rc == -1 and b"flair_block_luma_sums" in msg and what in msg, (rc, msg)


def test_binding_refusals():
    from flair_amd import _lib, ops
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(_lib.FlairHipError, match="no CPU path"):
        ops.block_luma_sums(a)
    with pytest.raises(ValueError, match="uint8"):
        ops.block_luma_sums(a.float())
    with pytest.raises(ValueError, match="contiguous"):
        ops.block_luma_sums(a.permute(0, 2, 1, 3)[:, :, ::2])
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\)"):
        ops.block_luma_sums(torch.zeros(1, 16, 16, 4, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------ restatement
def test_restatement_weights_and_blocks():
    """Pure R, G, B at 255 give per-pixel luma 77, 149 and 29; white gives 255; blocks of a 13 x 29 frame partition it."""
    for c, want in ((0, 77), (1, 149), (2, 29)):
        px = np.zeros((1, 1, 1, 3), dtype=np.uint8)
        px[..., c] = 255
        assert R.luma(px).item() == want
    assert R.luma(np.full((1, 3), 255, dtype=np.uint8)).item() == 255
    from flair_amd import scenes
    for H, W in ((8, 8), (13, 29), (45, 70), (96, 1283)):
        cnt = R.block_counts(H, W)
        assert cnt.sum() == H * W and cnt.min() >= 1 and scenes.block_counts(H, W) == cnt.tolist()
        ones = np.full((1, H, W, 3), 255, dtype=np.uint8)
        assert np.array_equal(R.block_sums(ones)[0], 255 * cnt)
    with pytest.raises(ValueError, match="fewer than 8"):
        scenes.block_counts(7, 64)


# ------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("H,W", R.SIZES)
def test_find_cuts_on_the_cut_fixture(H, W):
    from flair_amd import scenes
    seq = R.cut_sequence(H, W)
    assert seq.shape == (19, H, W, 3)
    sums = R.block_sums(seq)
    dist = R.pair_distances(sums, H, W)
    print(f"{H}x{W} d = {[round(d, 2) for d in dist]}")
    R.margins(dist, {7, 13, 14})                                              # the restatement's own margins first
    assert R.candidates(dist) == [7, 13, 14] and R.find_cuts(dist) == [7, 13]
    got = scenes.pair_distances(torch.from_numpy(sums), H, W)
    assert got == dist and all(isinstance(d, float) for d in got)             # the same float64 operations: equal, not close
    assert scenes.candidates(got) == [7, 13, 14]
    assert scenes.find_cuts(got) == [7, 13]
    assert scenes.find_cuts(got, min_shot=1) == [7, 13, 14]
    assert scenes.find_cuts(got, min_shot=6) == [7, 13]
    assert scenes.find_cuts(got, min_shot=7) == [7]
    assert scenes.find_cuts(got, threshold=60.0) == [] and scenes.find_cuts(got, ratio=20.0) == []
    assert scenes.shots(19, [7, 13]) == [(0, 7), (7, 13), (13, 19)]


@pytest.mark.parametrize("H,W", R.SIZES)
@pytest.mark.parametrize("name", ["fast_pan", "fade", "noisy", "still"])
def test_no_cut_is_found_without_one(name, H, W):
    """A 9 px-per-frame pan, a 9 %-per-frame fade, uniform +-25 noise, six identical frames (d = 0, median 0)."""
    from flair_amd import scenes
    seq = getattr(R, name)(H, W)
    sums = R.block_sums(seq)
    dist = R.pair_distances(sums, H, W)
    print(f"{name} {H}x{W} d = {[round(d, 2) for d in dist]}")
    R.margins(dist, set())
    if name == "still":
        assert dist == [0.0] * 5
    if name in ("fast_pan", "fade"):
        assert min(dist) >= 6.0                                               # above the threshold: the ratio test rejects them
    got = scenes.pair_distances(sums, H, W)
    assert got == dist
    assert scenes.find_cuts(got) == [] and scenes.find_cuts(got, min_shot=1) == []


def test_rule_edge_cases():
    from flair_amd import scenes
    assert scenes.find_cuts([]) == []                                         # one frame
    assert scenes.find_cuts([50.0], min_shot=1) == [1]                        # two frames: empty neighbourhood, median 0
    assert scenes.find_cuts([50.0]) == []                                     # ... but no room for two shots of 4
    assert scenes.local_median([1.0, 9.0, 3.0, 5.0], 1, 4) == 3.0 and scenes.local_median([1.0, 2.0, 3.0, 4.0, 9.0], 4, 2) == 3.5
    for bad in (dict(radius=0), dict(min_shot=0), dict(threshold=-1.0), dict(ratio=float("nan")), dict(radius=1.5)):
        with pytest.raises(ValueError):
            scenes.find_cuts([1.0, 2.0], **bad)


def test_check_cuts_names_the_offender():
    from flair_amd import scenes
    assert scenes.check_cuts([3, 7], 9) == [3, 7] and scenes.check_cuts([], 1) == []
    for cuts, what in (([0], "cut 0 is outside 1..8"), ([9], "cut 9 is outside 1..8"), ([4, 4], "cut 4 does not follow cut 4"),
                       ([5, 3], "cut 3 does not follow cut 5"), ([2.5], "cut 2.5 is not an integer"), ([True], "cut True")):
        with pytest.raises(ValueError, match=re.escape(what)):
            scenes.check_cuts(cuts, 9)


# ------------------------------------------------------------------------------------------------------ window_plan
@pytest.mark.parametrize("length,overlap", [(10, 3), (4, 1), (5, 0)])
def test_window_plan(length, overlap):
    from flair_amd import scenes, video
    for n in range(0, 30):
        want = video.window_indices(n, length, overlap)
        for none in (None, []):
            plan = video.window_plan(n, none, length, overlap)
            assert [idx for idx, _ in plan] == want
            assert [s for _, s in plan] == [k == 0 for k in range(len(want))]
    min_shot = overlap + 1
    for n, cuts in ((19, [7, 13]), (9, [4]), (25, [1, 2, 24]), (40, [11, 12, 30]), (12, [min_shot]), (12, [12 - min_shot])):
        plan = video.window_plan(n, cuts, length, overlap)
        found = scenes.shots(n, cuts)
        contributed = []
        for idx, starts in plan:
            assert idx == list(range(idx[0], idx[-1] + 1))
            inside = [(a, b) for a, b in found if a <= idx[0] and idx[-1] < b]
            assert len(inside) == 1, (idx, cuts)                              # no window spans a cut
            a, b = inside[0]
            assert starts == (idx[0] == a)
            assert len(idx) >= min(min_shot, b - a)
            contributed += idx if starts else idx[overlap:]
        assert contributed == list(range(n)), (n, cuts)                       # every frame exactly once
        assert sum(s for _, s in plan) == len(found)
    with pytest.raises(ValueError, match="cut 9 is outside"):
        video.window_plan(9, [9], length, overlap)
    with pytest.raises(ValueError, match="does not follow"):
        video.window_plan(9, [5, 2], length, overlap)


def test_iter_windows_with_cuts_on_host(tmp_path):
    """The frame cache does not assume that consecutive windows overlap: the windows of a plan with cuts hold the right frames."""
    from flair_amd import io as fio
    from flair_amd import video
    rng = np.random.default_rng(2)
    for i in range(11):
        fio.write_frame(str(tmp_path / f"f_{i}.png"), rng.integers(0, 256, size=(6, 5, 3), dtype=np.uint8))
    paths = fio.list_frames(tmp_path)
    full = fio.read_frames(paths)
    got = list(fio.iter_windows(paths, "cpu", length=4, overlap=1, cuts=[2, 7]))
    assert [idx for idx, _ in got] == [idx for idx, _ in video.window_plan(11, [2, 7], 4, 1)]
    for idx, x in got:
        assert torch.equal(x, full[:, idx[0]:idx[-1] + 1])


# ------------------------------------------------------------------------------------------------------ interpolation
class _Recorder:
    """Stand-in interpolator: in-between k is a fixed blend of the pair; records the pairs it is called with."""
    MULTIPLE = 1

    def __init__(self):
        self.calls = []

    def __call__(self, a, b, factor):
        self.calls.append((a.clone(), b.clone()))
        t = [(k + 1) / factor for k in range(factor - 1)]
        return torch.stack([(1 - s) * a + s * b + 0.01 * a * b for s in t], 1)


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("batch", [1, 4])
def test_interpolate_frames_does_not_cross_a_cut(factor, batch):
    from flair_amd import interpolate as fi
    T, cuts = 9, [3, 4, 8]
    frames = torch.rand(T, 3, 6, 7, generator=torch.Generator().manual_seed(factor))
    plain_net, net = _Recorder(), _Recorder()
    plain = fi.interpolate_frames(plain_net, frames, factor, batch=batch)
    again = fi.interpolate_frames(_Recorder(), frames, factor, batch=batch, cuts=[])
    assert torch.equal(plain, again)
    got = fi.interpolate_frames(net, frames, factor, batch=batch, cuts=cuts)
    assert got.shape == plain.shape == (factor * (T - 1) + 1, 3, 6, 7)
    seen = set()
    for a, b in net.calls:
        for x, y in zip(a, b):
            p = [i for i in range(T) if torch.equal(x, frames[i] * 2 - 1)]
            q = [i for i in range(T) if torch.equal(y, frames[i] * 2 - 1)]
            assert len(p) == 1 and q == [p[0] + 1]
            seen.add(p[0])
    assert seen == {p for p in range(T - 1) if p + 1 not in cuts}              # never a pair across a cut, every other pair once
    for i, (kind, p, *k) in enumerate(fi.interleave_index(T, factor)):
        if kind == "mid" and p + 1 in cuts:
            src = p if (k[0] + 1) / factor < 0.5 else p + 1
            assert torch.equal(got[i], frames[src]), (i, p, k)                 # bit for bit, by the 0.5 rule
        else:
            assert torch.equal(got[i], plain[i]), (i, kind, p)
    with pytest.raises(ValueError, match="cut 9 is outside"):
        fi.interpolate_frames(net, frames, factor, cuts=[9])


# ------------------------------------------------------------------------------------------------------ cuts file, command line
def _frames_dir(path, n, h=16, w=24):
    from flair_amd import io as fio
    path.mkdir()
    for i in range(n):
        fio.write_frame(str(path / f"{i:03d}.png"), np.full((h, w, 3), 10 * i, dtype=np.uint8))
    return str(path)


def test_cuts_file_round_trip(tmp_path):
    from flair_amd import scenes
    result = dict(cuts=[7, 13], distances=[0.1 * i for i in range(18)], shots=[(0, 7), (7, 13), (13, 19)], frames=19)
    path = str(tmp_path / "cuts.json")
    scenes.write_cuts(path, result)
    obj = json.loads(open(path).read())
    assert sorted(obj) == ["cuts", "distances", "frames"] and obj["frames"] == 19 and obj["distances"] == result["distances"]
    assert scenes.read_cuts(path, 19) == [7, 13]
    with pytest.raises(ValueError, match="written for 19 frames; the video has 18"):
        scenes.read_cuts(path, 18)
    with pytest.raises(ValueError, match="not found"):
        scenes.read_cuts(str(tmp_path / "nope.json"), 19)
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(dict(cuts=[13, 7], distances=[], frames=19)))
    with pytest.raises(ValueError, match="cut 7 does not follow cut 13"):
        scenes.read_cuts(str(bad), 19)
    bad.write_text("[1, 2]")
    with pytest.raises(ValueError, match="expected"):
        scenes.read_cuts(str(bad), 19)
    bad.write_text("not json")
    with pytest.raises(ValueError, match="not JSON"):
        scenes.read_cuts(str(bad), 19)
    assert scenes.describe(dict(result, distances=[float(i) for i in range(18)])) == [
        "shot 0: frames 0..6 (7)", "shot 1: frames 7..12 (6), opened by d = 6.00", "shot 2: frames 13..18 (6), opened by d = 12.00"]
    assert scenes.resolve("off", ["a"] * 19, "cpu") == (None, None) and scenes.resolve(None, ["a"] * 19, "cpu") == (None, None)
    assert scenes.resolve([7, 13], ["a"] * 19, "cpu") == ([7, 13], None) and scenes.resolve(path, ["a"] * 19, "cpu") == ([7, 13], None)


def test_command_line_refusals_come_before_the_device(tmp_path, monkeypatch):
    """Every refusal is a SystemExit raised while torch has not been asked for a device."""
    from flair_amd import __main__ as cli
    from flair_amd import scenes

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    monkeypatch.setattr(scenes, "detect_cuts_files", no_device)
    a, b = _frames_dir(tmp_path / "a", 9), _frames_dir(tmp_path / "b", 9)
    cuts = str(tmp_path / "cuts.json")
    scenes.write_cuts(cuts, dict(cuts=[4], distances=[0.0] * 8, frames=9))
    ap = cli.make_parser()
    args = ap.parse_args(["restore", "gaussian", a, "out"])
    assert args.scene_cuts == "off" and cli.cuts_of(args, "restore", [a]) == dict(scene_cuts="off", cut_rule=scenes.RULE_DEFAULTS)
    args = ap.parse_args(["restore", "gaussian", a, "out", "--scene-cuts", "auto", "--cut-threshold", "8", "--cut-ratio", "2.5",
                          "--cut-radius", "3", "--min-shot", "5"])
    assert cli.cuts_of(args, "restore", [a]) == dict(scene_cuts="auto", cut_rule=dict(threshold=8.0, ratio=2.5, radius=3, min_shot=5))
    args = ap.parse_args(["restore", "gaussian", a, "out", "--scene-cuts", cuts])
    assert cli.cuts_of(args, "restore", [a])["scene_cuts"] == [4]
    for name in ("x8-bicubic-demo", "jpeg-demo"):
        assert ap.parse_args([name]).scene_cuts == "off" and ap.parse_args([name, "--scene-cuts", "auto"]).scene_cuts == "auto"
    with pytest.raises(SystemExit, match="cuts file of one video"):
        cli.main(["restore", "gaussian", a, b, "--output-root", str(tmp_path / "o"), "--scene-cuts", cuts])
    with pytest.raises(SystemExit, match="written for 9 frames; the video has 5"):
        cli.main(["restore", "gaussian", _frames_dir(tmp_path / "c", 5), "out", "--scene-cuts", cuts])
    with pytest.raises(SystemExit, match="not found"):
        cli.main(["restore", "gaussian", a, "out", "--scene-cuts", str(tmp_path / "missing.json")])
    with pytest.raises(SystemExit, match="min_shot=0"):
        cli.main(["restore", "gaussian", a, "out", "--scene-cuts", "auto", "--min-shot", "0"])
    with pytest.raises(SystemExit, match="interpolate: .*written for 9 frames; the video has 5"):
        cli.main(["interpolate", str(tmp_path / "c"), "out", "--factor", "2", "--scene-cuts", cuts])
    with pytest.raises(SystemExit, match="radius=0"):
        cli.main(["interpolate", a, "out", "--factor", "2", "--scene-cuts", "auto", "--cut-radius", "0"])
    # scenes: not a directory, no frames, differing sizes, fewer than 8 pixels a side, a bad rule
    with pytest.raises(SystemExit, match="is not a directory"):
        cli.main(["scenes", str(tmp_path / "nowhere")])
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit, match="no frame files"):
        cli.main(["scenes", str(tmp_path / "empty")])
    mixed = _frames_dir(tmp_path / "mixed", 3)
    from flair_amd import io as fio
    fio.write_frame(os.path.join(mixed, "003.png"), np.zeros((16, 20, 3), dtype=np.uint8))
    with pytest.raises(SystemExit, match="must share one size"):
        cli.main(["scenes", mixed])
    with pytest.raises(SystemExit, match="fewer than 8 pixels a side"):
        cli.main(["scenes", _frames_dir(tmp_path / "tiny", 3, h=7, w=24)])
    with pytest.raises(SystemExit, match="threshold=-1.0"):
        cli.main(["scenes", a, "--cut-threshold", "-1"])
    help_text = ap.format_help() + "".join(sp.format_help() for sp in ap._subparsers._group_actions[0].choices.values())
    assert "NOT been validated on real footage" in re.sub(r"\s+", " ", help_text)
