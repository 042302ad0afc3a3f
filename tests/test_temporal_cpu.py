"""CPU: the flow-warping error's definition (tests/temporal_ref.py) on hand cases and against its mutants, the data the GPU
tests stand on, the fifth header, the two entries' refusals, the flow loader on both file shapes, the host's arithmetic
(placement, cuts, missing values, means), the reports and the command line."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def png(path, h, w, value=0):
    from flair_amd import io as fio
    fio.write_frame(str(path), np.full((h, w, 3), value, dtype=np.uint8))


# ------------------------------------------------------------------------------------------- the definition
def test_reference_gives_the_known_answers():
    cases = R.known_answers()
    assert [c["frames"].shape[1:3] for c in cases] == [(37, 70), (1, 40), (40, 1), (37, 70), (37, 70)]
    for c in cases:
        mask, out = R.run_known_answer(c)
        assert R.check_known_answer(c, mask, out) == [], c["name"]
    shift = cases[0]                                # column W - 4 lands on W - 1 (inside), column W - 3 on W (outside)
    assert shift["mask"][0, 5, 70 - 4] == 1 and shift["mask"][0, 5, 70 - 3] == 0 and shift["mask"][0, 1, 10] == 0 and shift["mask"][0, 2, 10] == 1
    assert shift["N"] == (37 - 2) * (70 - 3) and R.warp_err(49.0, shift["N"]) == 49.0 / (255.0 ** 2 * shift["N"]) and R.warp_err(0.0, 0) is None


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_breaks_a_known_answer(mutant):
    broken = [c["name"] for c in R.known_answers() if R.check_known_answer(c, *R.run_known_answer(c, mutant))]
    print(f"{mutant}: breaks {broken}")
    assert broken


def test_generated_data_is_what_the_gpu_tests_assume():
    """Dyadic flows sit on the 1/4 grid within 8; the random case leaves at most 0.1 % of its pixels within 1e-9 relative of a
    threshold (asserted here on the reference alone, with the seed chosen here), and in both all three rules remove pixels
    and a good share stays."""
    for P in (1, 3):
        d = R.dyadic_case(P)
        for name in ("f", "g"):
            assert d[name].dtype == np.float32 and np.array_equal(d[name] * 4, np.round(d[name] * 4)) and np.abs(d[name]).max() <= 8
        assert d["frames"].shape == (P + 1, 37, 70, 3) and d["frames"].dtype == np.uint8
    assert np.array_equal(R.dyadic_case(1)["f"][0], R.dyadic_case(3)["f"][0])          # pair 0 is the same pair in both
    for d in (R.dyadic_case(3), R.random_case()):
        occluded = boundary = 0
        for i in range(d["f"].shape[0]):
            o = R.occlusion(d["f"][i], d["g"][i])
            share = o["mask"].mean()
            print(f"pair {i}: kept {share:.3f}, outside {1 - o['inside'].mean():.3f}, occluded {o['occluded'].mean():.3f}, "
                  f"boundary {o['boundary'].mean():.3f}, smallest margin {o['margin'].min():.3e}")
            assert 0.3 < share < 0.95 and not o["inside"].all()
            occluded, boundary = occluded + int(o["occluded"].sum()), boundary + int(o["boundary"].sum())
        assert occluded > 50 and boundary > 50      # (a pair that moves far has wide thresholds: the large-motion pair loses pixels at the frame's edge alone)
    d = R.random_case()
    close = np.concatenate([(R.occlusion(d["f"][i], d["g"][i])["margin"] <= 1e-9).ravel() for i in range(d["f"].shape[0])])
    assert close.mean() <= 1e-3
    e = R.batch(d["frames"], d["f"], d["g"])[1]
    assert (e[0, :, 0] > 1e6).all()                 # random bytes: S is large, so a relative 1e-12 is a real demand


# ------------------------------------------------------------------------------------------- the fifth header
def temporal_declared():
    text = open(os.path.join(ROOT, "include", "flair_temporal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_temporal_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib, ops
    assert temporal_declared() == sorted(_header.TEMPORAL_PROTOS) == ["flair_flow_occlusion", "flair_warp_error"]
    others = set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS) | set(_header.IDENT_PROTOS)
    assert not set(_header.TEMPORAL_PROTOS) & others and not set(_header.TEMPORAL_PROTOS) & set(_lib.ALL_PROTOS)
    assert len(_header.STRUCTS) == 7 and _header.parse(open(_header.TEMPORAL_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 21
    for name, (restype, params) in _header.TEMPORAL_PROTOS.items():
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and params[-1].name == "stream", name
        assert list(f.argtypes) == [p.ctype for p in params], name
    i, z, v = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    assert [tuple(p) for p in _header.TEMPORAL_PROTOS["flair_flow_occlusion"][1]] == [
        ("f", v, "float"), ("g", v, "float"), ("P", i, None), ("H", i, None), ("W", i, None), ("mask", v, "uint8_t"), ("stream", v, None)]
    assert [tuple(p) for p in _header.TEMPORAL_PROTOS["flair_warp_error"][1]] == [
        ("a", v, "uint8_t"), ("a2", v, "uint8_t"), ("f", v, "float"), ("mask", v, "uint8_t"), ("P", i, None), ("H", i, None), ("W", i, None),
        ("out", v, "double"), ("ws", v, "void"), ("ws_bytes", z, None), ("stream", v, None)]
    header = open(_header.TEMPORAL_HEADER_PATH).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "temporal.hip")).read()
    from flair_amd import metrics
    assert int(re.search(r"#define FLAIR_WARP_TILE_H (\d+)", header).group(1)) == ops.WARP_TILE_H == metrics.TILE_H
    assert int(re.search(r"#define FLAIR_WARP_TILE_W (\d+)", header).group(1)) == ops.WARP_TILE_W == metrics.TILE_W
    assert "TP_TH = FLAIR_WARP_TILE_H, TP_TW = FLAIR_WARP_TILE_W" in src and "atomic" not in src.replace("no atomics", "")
    assert not re.search(r"size_t\s+flair_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))     # the workspace is a closed form
    assert "NOT a reproduction of Lai" in header and "is 21 from this header on" in header
    make = open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read()
    assert "flair_temporal.h" in make and re.search(r"(?m)^temporal\.o: CXXFLAGS \+= -ffp-contract=off$", make)


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entries():
    from flair_amd import _lib
    call = _lib.call
    f32, f64, u8 = _device_tensor(torch.float32), _device_tensor(torch.float64), _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_flow_occlusion(torch.zeros(2), f32, 1, 1, 1, u8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_flow_occlusion: g must be float32, got float64$"):
        call.flair_flow_occlusion(f32, f64, 1, 1, 1, u8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_flow_occlusion: mask must be uint8, got float32$"):
        call.flair_flow_occlusion(f32, f32, 1, 1, 1, f32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_warp_error: a2 must be uint8, got float32$"):
        call.flair_warp_error(u8, f32, f32, u8, 1, 1, 1, f64, u8, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_warp_error: out must be float64, got float32$"):
        call.flair_warp_error(u8, None, f32, u8, 1, 1, 1, f32, u8, 16)
    with pytest.raises(TypeError, match="flair_warp_error takes 10 arguments"):
        call.flair_warp_error(u8, None)
    with pytest.raises(AttributeError, match="flair_warp_error_workspace is not an entry"):
        call.flair_warp_error_workspace


def test_entries_refuse_before_any_launch(monkeypatch):
    """Every refusal the header lists: status -1 and the entry's message, on a machine without a GPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    cases = R.entry_refusals()
    assert {n for n, _, _ in cases} == {"flair_flow_occlusion", "flair_warp_error"} and len(cases) >= 27
    for name, args, what in cases:
        R.assert_refused(lib, name, args, what)
    monkeypatch.setattr(_lib, "stream", lambda: None)
    f32, f64, u8 = _device_tensor(torch.float32), _device_tensor(torch.float64), _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_warp_error failed \(status -1\): flair_warp_error: ws_bytes = 8, sets \* P"):
        _lib.call.flair_warp_error(u8, None, f32, u8, 1, 8, 8, f64, u8, 8)


def test_ops_wrappers_refuse_wrong_tensors():
    from flair_amd import ops
    f = torch.zeros(2, 8, 9, 2)
    with pytest.raises(ValueError, match=r"flow_occlusion: f is a dense \(P, H, W, 2\) float32 tensor"):
        ops.flow_occlusion(f.double(), f)
    with pytest.raises(ValueError, match=r"flow_occlusion: f is a dense"):
        ops.flow_occlusion(f.permute(0, 2, 1, 3), f)
    with pytest.raises(ValueError, match=r"flow_occlusion: g is a dense \(2, 8, 9, 2\) float32 tensor like f"):
        ops.flow_occlusion(f, torch.zeros(2, 8, 8, 2))
    with pytest.raises(ValueError, match=r"flow_occlusion: out is a dense \(2, 8, 9\) uint8 tensor"):
        ops.flow_occlusion(f, f, out=torch.zeros(2, 8, 9))
    a, mask = torch.zeros(3, 8, 9, 3, dtype=torch.uint8), torch.zeros(2, 8, 9, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"warp_error: a is a dense \(3, 8, 9, 3\) uint8 tensor, one frame more than f has pairs, got \(2, 8, 9, 3\)"):
        ops.warp_error(a[:2], f, mask)
    with pytest.raises(ValueError, match=r"warp_error: a2 is a dense \(3, 8, 9, 3\) uint8 tensor"):
        ops.warp_error(a, f, mask, a2=a.float())
    with pytest.raises(ValueError, match=r"warp_error: mask is a dense \(2, 8, 9\) uint8 tensor"):
        ops.warp_error(a, f, mask.bool())
    with pytest.raises(ValueError, match=r"warp_error: out is a dense \(2, 2, 2\) float64 tensor"):
        ops.warp_error(a, f, mask, a2=a, out=torch.zeros(1, 2, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"warp_error: f is a dense"):
        ops.warp_error(a, f[:0], mask)


# ------------------------------------------------------------------------------------------- the flow weights
def test_load_flow_reads_both_file_shapes_and_refuses_the_rest(tmp_path):
    from flair_amd import temporal as ftm
    from flair_amd.guided_diffusion.sr3 import UNet
    from flair_amd.guided_diffusion.unet_new import SPyNet, UNetModel
    from tests.golden.weights import name_seeded_weights
    from tests.test_gpu_sr3 import SR3_SMALL
    from tests.test_gpu_unet import SMALL
    bare = name_seeded_weights(SPyNet()).state_dict()
    assert len(bare) == 62 and "basic_module.5.basic_module.4.conv.bias" in bare and "mean" in bare
    torch.save(bare, tmp_path / "spynet.pth")
    m = ftm.load_flow(str(tmp_path / "spynet.pth"), "cpu")
    assert isinstance(m, SPyNet) and len(m._pk["levels"]) == 6 and not m.training          # packed
    assert torch.equal(m.basic_module[3].basic_module[2].conv.weight, bare["basic_module.3.basic_module.2.conv.weight"])
    no_stats = {k: v for k, v in bare.items() if k not in ("mean", "std")}
    torch.save({"state_dict": no_stats}, tmp_path / "wrapped.pth")                            # mmedit's wrapping; mean / std optional
    m2 = ftm.load_flow(str(tmp_path / "wrapped.pth"), "cpu")
    assert torch.equal(m2.mean, SPyNet().mean) and torch.equal(m2.basic_module[0].basic_module[0].conv.bias, bare["basic_module.0.basic_module.0.conv.bias"])

    unet = name_seeded_weights(UNetModel(**SMALL))
    sd = unet.state_dict()
    assert sorted({re.match(r"(.*?spynet\.)", k).group(1) for k in sd if "spynet." in k}) == ["spynet."]
    torch.save(sd, tmp_path / "flair_task.pt")
    m3 = ftm.load_flow(str(tmp_path / "flair_task.pt"), "cpu")
    assert torch.equal(m3.basic_module[5].basic_module[4].conv.weight, sd["spynet.basic_module.5.basic_module.4.conv.weight"])

    sr3 = UNet(**SR3_SMALL)
    sd = dict(sr3.state_dict())
    prefixes = sorted({re.match(r"(.*?spynet\.)", k).group(1) for k in sd if "spynet." in k})
    assert len(prefixes) > 1 and all(p.endswith("vsrpp.wrapped_module.spynet.") for p in prefixes)      # one shared network, several names
    key = "basic_module.2.basic_module.1.conv.weight"
    sd[prefixes[0] + key] = torch.full_like(sd[prefixes[0] + key], 0.25)                      # the first prefix in sorted order is read
    sd[prefixes[1] + key] = torch.full_like(sd[prefixes[1] + key], 0.5)
    torch.save(sd, tmp_path / "flair_sr3.pt")
    m4 = ftm.load_flow(str(tmp_path / "flair_sr3.pt"), "cpu")
    assert bool((m4.basic_module[2].basic_module[1].conv.weight == 0.25).all())

    with pytest.raises(ValueError) as exc:
        ftm.flow_state_dict({"conv.weight": torch.zeros(1), "conv.bias": torch.zeros(1)}, "file.pt")
    text = str(exc.value)
    assert text.startswith("file.pt: no SPyNet weights among its 2 keys (conv.weight, conv.bias)")
    assert "basic_module.L.basic_module.J.conv.{weight,bias}" in text and "a prefix ending in spynet." in text and '"state_dict"' in text
    bad = dict(bare)
    del bad["basic_module.1.basic_module.0.conv.bias"]
    bad["basic_module.6.basic_module.0.conv.bias"] = torch.zeros(32)
    bad["basic_module.0.basic_module.0.conv.weight"] = torch.zeros(32, 8, 3, 3)
    with pytest.raises(ValueError) as exc:
        ftm.flow_state_dict(bad, "file.pth")
    text = str(exc.value)
    assert text.startswith("file.pth does not fit mmedit's SPyNet") and "unexpected keys: basic_module.6.basic_module.0.conv.bias" in text
    assert "missing keys: basic_module.1.basic_module.0.conv.bias" in text and "shapes: basic_module.0.basic_module.0.conv.weight (32, 8, 3, 3) for (32, 8, 7, 7)" in text
    for junk in ({}, {"a": 1}, [1, 2], {"state_dict": {}}):
        with pytest.raises(ValueError, match="holds no tensor state dict; looked for keys"):
            ftm.flow_state_dict(junk)
    with pytest.raises(FileNotFoundError, match="nope.pth not found"):
        ftm.load_flow(str(tmp_path / "nope.pth"), "cpu")
    (tmp_path / "text.pth").write_text("not a checkpoint")
    with pytest.raises(ValueError, match="not a tensor state dict"):
        ftm.load_flow(str(tmp_path / "text.pth"), "cpu")


# ------------------------------------------------------------------------------------------- the host's arithmetic
def row(*sets):
    return np.array(sets, dtype=np.float64)


def test_scores_place_values_on_the_later_frame_and_leave_out_what_has_none():
    from flair_amd import temporal as ftm
    u = 255.0 ** 2
    rows = [None, row((2 * u * 50, 50)), row((0.0, 0)), row((u * 100, 100)), row((4 * u * 25, 25))]
    values, mean = ftm.scores(rows, [100] * 5)
    assert values == [None, 2.0, None, 1.0, 4.0]                         # frame 0 has no pair; N = 0 has no value
    assert mean == dict(warp_err=7.0 / 3, warp_err_pairs=3, masked=(0.5 + 1.0 + 0.0 + 0.75) / 4) and list(mean) == ["warp_err", "warp_err_pairs", "masked"]
    values, mean = ftm.scores(rows, [100] * 5, skip=ftm.straddling([3]))                 # frame 3 starts a shot: pair (2, 3) is left out
    assert values == [None, 2.0, None, None, 4.0] and mean == dict(warp_err=3.0, warp_err_pairs=2, masked=(0.5 + 1.0 + 0.75) / 3)
    two = [None, row((u * 10, 10), (3 * u * 10, 10)), row((0.0, 0), (0.0, 0)), None, row((2 * u * 40, 40), (u * 40, 40))]      # a size change at frame 3
    values, mean = ftm.scores(two, [50, 50, 50, 80, 80])
    assert values == [None, 1.0, None, None, 2.0]
    assert mean == dict(warp_err=1.5, warp_err_truth=2.0, warp_err_pairs=2, masked=(0.8 + 1.0 + 0.5) / 3) and list(mean)[1] == "warp_err_truth"
    assert ftm.scores([None], [10]) == ([None], dict(warp_err=None, warp_err_pairs=0, masked=None))
    assert ftm.scores([], []) == ([], dict(warp_err=None, warp_err_pairs=0, masked=None))
    # cuts: a cut at k is the pair (k - 1, k); through interpolate --factor N every output pair between source frames k - 1 and k
    assert ftm.straddling(None) == set() and ftm.straddling([]) == set() and ftm.straddling([3, 7]) == {3, 7}
    assert ftm.straddling([3], factor=4) == {9, 10, 11, 12} and ftm.straddling([1, 2], factor=2) == {1, 2, 3, 4}
    assert ftm.format_value(0.0012345) == "  warp-err 1.2345" and ftm.format_value(None) == "  warp-err n/a"
    assert ftm.format_mean(dict(warp_err=0.0012345, warp_err_truth=0.0009876, warp_err_pairs=3, masked=0.07123)) == "  warp-err 1.2345 (truth 0.9876)  masked 0.0712"
    assert ftm.format_mean(dict(warp_err=None, warp_err_truth=None, warp_err_pairs=0, masked=None)) == "  warp-err n/a (truth n/a)  masked n/a"
    assert ftm.format_mean(dict(warp_err=0.002, warp_err_pairs=1, masked=0.5)) == "  warp-err 2.0000  masked 0.5000"
    with pytest.raises(ValueError, match=r"warp-error: out/0003.png is 31x64; the flow network needs frames of at least 32 pixels a side"):
        ftm.check_size(31, 64, what="out/0003.png")
    ftm.check_size(32, 32)
    with pytest.raises(ValueError, match="one frame pair must stay under 134217727 pixels"):
        ftm.check_size(16384, 8192)


class StubModel:
    """Stands in for WarpError: (S, N) of pair (i, i + 1) = (255^2 * first byte of frame i + 1, first byte of frame i); with truth
    the second set's S is doubled."""

    def __init__(self):
        self.calls = []

    def pairs(self, a, b=None):
        self.calls.append((a.shape[0], None if b is None else b.shape[0]))
        first = a[:, 0, 0, 0].double().numpy()
        one = np.stack([255.0 ** 2 * first[1:], first[:-1]], axis=1)
        return one[None] if b is None else np.stack([one, one * [2.0, 1.0]])


def test_pair_stream_measures_the_pair_across_two_batches():
    from flair_amd import temporal as ftm
    frame = lambda v, h=32, w=32: torch.full((1, h, w, 3), v, dtype=torch.uint8)            # noqa: E731
    m = StubModel()
    s = ftm.PairStream(m)
    s.push(torch.cat([frame(1), frame(2), frame(3)]))
    s.push(frame(4))                                # a batch of one frame still closes the pair (3, 4)
    s.push(torch.cat([frame(5, 32, 40), frame(6, 32, 40)]))          # another size: no pair with the frame before it
    assert m.calls == [(3, None), (2, None), (2, None)]
    assert [None if r is None else r.tolist() for r in s.rows] == [None, [[2 * 65025.0, 1.0]], [[3 * 65025.0, 2.0]], [[4 * 65025.0, 3.0]], None,
                                                                    [[6 * 65025.0, 5.0]]]
    assert s.pixels == [1024] * 4 + [1280] * 2
    values, mean = ftm.scores(s.rows, s.pixels)
    assert values == [None, 2.0, 1.5, 4.0 / 3, None, 1.2] and mean["warp_err_pairs"] == 4
    s = ftm.PairStream(StubModel())
    s.push(frame(1), frame(1))
    s.push(frame(2), frame(2))
    assert s.model.calls == [(2, 2)] and s.rows[0] is None and s.rows[1].tolist() == [[2 * 65025.0, 1.0], [4 * 65025.0, 1.0]]


# ------------------------------------------------------------------------------------------- evaluate_dirs / format_report
def test_report_and_json_with_and_without_the_option(tmp_path, monkeypatch):
    from flair_amd import metrics
    from flair_amd import temporal as ftm
    from flair_amd.__main__ import merge_results, warp_tail, write_json
    rows = dict(psnr=[math.inf, 31.23456, 30.0, 29.0], ssim=[1.0, 0.912349, 0.5, 0.25], sse=[0, 5, 6, 7])
    monkeypatch.setattr(metrics, "psnr_ssim", lambda a, b: {k: v[:a.shape[0]] for k, v in rows.items()})
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        for i in range(4):
            png(tmp_path / d / f"{i:04d}.png", 32, 32, value=i + 1)
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu")
    assert set(res["mean"]) == {"psnr", "ssim"} and set(res["frames"][1]) == {"name", "psnr", "ssim"}
    assert metrics.format_report(res)[1:] == ["0001.png  psnr 31.2346  ssim 0.9123", "0002.png  psnr 30.0000  ssim 0.5000",
                                              "0003.png  psnr 29.0000  ssim 0.2500", "mean of 4 frames  psnr inf  ssim 0.6656"]
    write_json(tmp_path / "plain.json", res)
    assert "warp_err" not in open(tmp_path / "plain.json").read() and "masked" not in open(tmp_path / "plain.json").read() and warp_tail(res) == ""

    model = StubModel()
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", batch=3, warp_error=model, warp_skip={2})
    assert model.calls == [(3, 3), (2, 2)]          # the second batch is one frame and the one kept from the first
    assert [f["warp_err"] for f in res["frames"]] == [None, 2.0, None, 4.0 / 3]
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", warp_error=StubModel(), warp_skip={2})      # one batch
    assert [f["warp_err"] for f in res["frames"]] == [None, 2.0, None, 4.0 / 3] and set(res["frames"][0]) == {"name", "psnr", "ssim", "warp_err"}
    assert set(res["mean"]) == {"psnr", "ssim", "warp_err", "warp_err_truth", "warp_err_pairs", "masked"}
    assert res["mean"]["warp_err"] == (2.0 + 4.0 / 3) / 2 and res["mean"]["warp_err_truth"] == 2 * res["mean"]["warp_err"] and res["mean"]["warp_err_pairs"] == 2
    assert res["mean"]["masked"] == ((1 - 1 / 1024) + (1 - 3 / 1024)) / 2
    masked = f"{res['mean']['masked']:.4f}"
    assert metrics.format_report(res) == ["0000.png  psnr inf  ssim 1.0000  warp-err n/a", "0001.png  psnr 31.2346  ssim 0.9123  warp-err 2000.0000",
                                          "0002.png  psnr 30.0000  ssim 0.5000  warp-err n/a", "0003.png  psnr 29.0000  ssim 0.2500  warp-err 1333.3333",
                                          f"mean of 4 frames  psnr inf  ssim 0.6656  warp-err 1666.6667 (truth 3333.3333)  masked {masked}"]
    assert warp_tail(res) == f"  warp-err 1666.6667 (truth 3333.3333)  masked {masked}"
    write_json(tmp_path / "warp.json", res)
    back = json.load(open(tmp_path / "warp.json"))
    assert back["frames"][0]["warp_err"] is None and back["frames"][1]["warp_err"] == 2.0 and back["mean"] == res["mean"]       # unscaled, null

    # a directory alone: its own flows, no truth value
    model = StubModel()
    alone = ftm.warp_error_dir(str(tmp_path / "a"), "cpu", model, skip={2})
    assert model.calls == [(4, None)] and alone["count"] == 4 and list(alone["mean"]) == ["warp_err", "warp_err_pairs", "masked"]
    assert alone["frames"] == [dict(name="0000.png", warp_err=None), dict(name="0001.png", warp_err=2.0), dict(name="0002.png", warp_err=None),
                               dict(name="0003.png", warp_err=4.0 / 3)]
    assert ftm.format_report(alone) == ["0000.png  warp-err n/a", "0001.png  warp-err 2000.0000", "0002.png  warp-err n/a", "0003.png  warp-err 1333.3333",
                                        f"mean of 2 pairs of 4 frames  warp-err 1666.6667  masked {masked}"]
    both = merge_results(dict(frames=[dict(name=f["name"], niqe=4.0) for f in alone["frames"]], mean=dict(niqe=4.0, niqe_frames=4), count=4), alone)
    assert both["frames"][1] == dict(name="0001.png", niqe=4.0, warp_err=2.0) and set(both["mean"]) == {"niqe", "niqe_frames", "warp_err", "warp_err_pairs", "masked"}
    with pytest.raises(ValueError, match="warp-error: no frame files in"):
        ftm.warp_error_dir(str(tmp_path), "cpu", model)
    # a small frame is refused on the file headers, with the other refusals: nothing is decoded
    png(tmp_path / "a" / "0004.png", 31, 40)
    png(tmp_path / "b" / "0004.png", 31, 40)
    monkeypatch.setattr(metrics.fio, "iter_frame_batches", lambda *a, **k: pytest.fail("decoded before the refusal"))
    with pytest.raises(ValueError, match=r"warp-error: evaluate: .*a.0004\.png is 31x40; the flow network needs frames of at least 32"):
        metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", warp_error=model)
    with pytest.raises(ValueError, match=r"warp-error: .*a.0004\.png is 31x40"):
        ftm.warp_error_dir(str(tmp_path / "a"), "cpu", model)


# ------------------------------------------------------------------------------------------- command line
def test_warp_error_options_parse_and_refuse(tmp_path):
    from flair_amd.__main__ import load_warp_of, main, make_parser, warp_of
    ap = make_parser()
    e = ap.parse_args(["evaluate", "out", "truth", "--warp-error", "f.pt", "--scene-cuts", "auto"])
    assert e.warp_error == "f.pt" and e.scene_cuts == "auto"
    e = ap.parse_args(["evaluate", "out", "truth"])
    assert e.warp_error is None and e.scene_cuts == "off" and warp_of(e, "evaluate") is None and load_warp_of(None, "cpu", "evaluate") is None
    assert ap.parse_args(["restore", "gaussian", "in", "out", "--warp-error", "f.pt"]).warp_error == "f.pt"             # with or without --ground-truth
    assert ap.parse_args(["interpolate", "in", "out", "--factor", "2", "--warp-error", "f.pt"]).warp_error == "f.pt"
    w = ap.parse_args(["warp-error", "frames", "--flow-weights", "f.pt", "--json", "o.json", "--scene-cuts", "cuts.json"])
    assert (w.frames_dir, w.flow_weights, w.json, w.scene_cuts) == ("frames", "f.pt", "o.json", "cuts.json")
    assert not hasattr(ap.parse_args(["jpeg-demo"]), "warp_error") and not hasattr(ap.parse_args(["niqe", "d"]), "warp_error")
    for command in ("evaluate", "restore", "interpolate"):
        text = re.sub(r"\s+", " ", ap._subparsers._group_actions[0].choices[command].format_help())
        assert "--warp-error FILE" in text and "at least 32 pixels a side" in text and "any FLAIR task checkpoint" in text

    with pytest.raises(SystemExit, match=r"evaluate: --warp-error .*nope\.pt is not a file"):
        main(["evaluate", "out", "truth", "--warp-error", str(tmp_path / "nope.pt")])
    with pytest.raises(SystemExit, match="evaluate: --scene-cuts only tells --warp-error FILE"):
        main(["evaluate", "out", "truth", "--scene-cuts", "auto"])
    with pytest.raises(SystemExit, match=r"warp-error: --flow-weights FILE is required"):
        main(["warp-error", str(tmp_path)])
    with pytest.raises(SystemExit, match=r"warp-error: --flow-weights .*nope\.pt is not a file"):
        main(["warp-error", str(tmp_path), "--flow-weights", str(tmp_path / "nope.pt")])
    torch.save({"a": torch.zeros(1)}, tmp_path / "f.pt")
    with pytest.raises(SystemExit, match=r"warp-error: .*missing is not a directory"):
        main(["warp-error", str(tmp_path / "missing"), "--flow-weights", str(tmp_path / "f.pt")])
    (tmp_path / "in").mkdir()
    with pytest.raises(SystemExit, match=r"warp-error: no frame files in"):
        main(["warp-error", str(tmp_path / "in"), "--flow-weights", str(tmp_path / "f.pt")])
    png(tmp_path / "in" / "0.png", 64, 64)
    png(tmp_path / "in" / "1.png", 64, 31)
    with pytest.raises(SystemExit, match=r"warp-error: .*1\.png is 64x31; the flow network needs frames of at least 32 pixels a side"):
        main(["warp-error", str(tmp_path / "in"), "--flow-weights", str(tmp_path / "f.pt")])
    with pytest.raises(SystemExit, match=r"restore: --warp-error .*nope\.pt is not a file"):
        main(["restore", "gaussian", str(tmp_path / "in"), str(tmp_path / "out"), "--warp-error", str(tmp_path / "nope.pt")])
    (tmp_path / "in2").mkdir()
    for i in range(2):
        png(tmp_path / "in2" / f"{i}.png", 32, 32)
    with pytest.raises(SystemExit, match=r"interpolate: --warp-error .*nope\.pt is not a file"):
        main(["interpolate", str(tmp_path / "in2"), str(tmp_path / "out"), "--factor", "2", "--warp-error", str(tmp_path / "nope.pt")])
    path = warp_of(ap.parse_args(["evaluate", "a", "b", "--warp-error", str(tmp_path / "f.pt")]), "evaluate")
    assert path == str(tmp_path / "f.pt")
    with pytest.raises(SystemExit, match=r"evaluate: .*f\.pt: no SPyNet weights among its 1 keys \(a\); looked for keys basic_module"):
        load_warp_of(path, "cpu", "evaluate")
    from flair_amd import metrics
    assert "flow-warping error" in metrics.__doc__ and "temporal metrics other than the identity drift and the flow-warping error" in metrics.__doc__
