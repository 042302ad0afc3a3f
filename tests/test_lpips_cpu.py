"""CPU: the LPIPS reference against a hand-computed tap and the misreadings it must tell apart, the loader, the second
header (include/flair_eval.h) and its binding, the entries' refusals without a device, the command line, and the report
without a model against a literal of what it printed before the option existed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import lpips_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_ENTRIES = ["flair_alexnet_stem", "flair_lpips_prepare", "flair_lpips_tap", "flair_maxpool_valid_s2_nhwc"]


def png(path, h, w, value=0):
    from PIL import Image
    Image.fromarray(np.full((h, w, 3), value, dtype=np.uint8), mode="RGB").save(path, format="PNG")


# ------------------------------------------------------------------------------------------- the reference itself
# Two pixels of C = 4.  Pixel 0: a = (3, 0, 4, 0), |a| = 5, a^ = (.6, 0, .8, 0); b = (0, 0, 0, 5), b^ = (0, 0, 0, 1);
# w = (1, 2, 0, .5): d = 1 * .36 + 2 * 0 + 0 * .64 + .5 * 1 = .86.  Pixel 1: a = (1e-10, 0, 0, 0), a^ = 1e-10 / (1e-10 + 1e-10)
# = .5; b = 0, b^ = 0 (an all-zero vector normalises to zeros): d = 1 * .25.  The tap is their mean.
HAND_A = torch.tensor([[[3.0, 0.0, 4.0, 0.0], [1e-10, 0.0, 0.0, 0.0]]], dtype=torch.float64)
HAND_B = torch.tensor([[[0.0, 0.0, 0.0, 5.0], [0.0, 0.0, 0.0, 0.0]]], dtype=torch.float64)
HAND_W = torch.tensor([1.0, 2.0, 0.0, 0.5], dtype=torch.float64)
HAND = (0.86 + 0.25) / 2
# eps inside the root: pixel 1's a^ = 1e-10 / sqrt(1e-20 + 1e-10) = 1e-5, d = 1e-10.  No weights: .36 + .64 + 1 = 2 and .25.
# Averaging over the channels before weighting: (2 / 4) * 3.5 and (.25 / 4) * 3.5.
MISREAD = {"eps_inside": (0.86 + 1e-10) / 2, "no_weights": (2.0 + 0.25) / 2, "mean_first": (1.75 + 0.21875) / 2}


def test_reference_equals_the_hand_computed_tap():
    got = lr.tap_distance(HAND_A, HAND_B, HAND_W).item()
    assert abs(got - HAND) < 1e-9, got
    assert torch.isfinite(lr.tap_distance(HAND_B * 0, HAND_B * 0, HAND_W)).all() and lr.tap_distance(HAND_B * 0, HAND_B * 0, HAND_W).item() == 0.0


@pytest.mark.parametrize("switch", sorted(MISREAD))
def test_each_misreading_moves_the_tap_beyond_the_gpu_bound(switch):
    """On the hand-computed tap every misreading gives its own hand-computed value, far from the definition's; on the random
    features of the GPU test it moves the value by more than that test's bound (4 x the float32 restatement's deviation)."""
    got = lr.tap_distance(HAND_A, HAND_B, HAND_W, **{switch: True}).item()
    assert abs(got - MISREAD[switch]) < 1e-9 and abs(got - HAND) > 1e-2, (switch, got)
    fa, fb, w = lr.random_tap_case(64, 323, 3)
    if switch == "eps_inside":              # random features have norms near 5: the eps only shows on faint ones
        fa, fb = fa * 1e-9, fb * 1e-9
    ref = lr.tap_distance(fa.double(), fb.double(), w.double())
    bound = lr.bound_4x(ref, lr.tap_distance(fa, fb, w))
    moved = (lr.tap_distance(fa.double(), fb.double(), w.double(), **{switch: True}) - ref).abs().min().item()
    assert 0 < bound < 1e-5 and moved > 10 * bound, (switch, bound, moved)


def test_dropping_the_minus_one_moves_the_metric_beyond_the_gpu_bound():
    """x = 2 byte / 255 without the -1 shifts every input by 1 / scale: the 16x16 VGG value moves by far more than 4 x the
    float32 restatement's deviation."""
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, 256, (1, 16, 16, 3), generator=g, dtype=torch.uint8)
    b = (a.int() + torch.randint(-64, 65, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    ref = lr.lpips("vgg", a, b)
    bound = lr.bound_4x(ref, lr.lpips("vgg", a, b, torch.float32))
    moved = (lr.lpips("vgg", a, b, minus_one=False) - ref).abs().item()
    assert ref.item() > 0 and 0 < bound < 1e-4 and moved > 10 * bound, (ref, bound, moved)
    assert lr.lpips("vgg", a, a).item() == 0.0


def test_reference_tap_shapes():
    for net, (h, w), want in (("vgg", (16, 16), [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
                              ("vgg", (37, 50), [(37, 50), (18, 25), (9, 12), (4, 6), (2, 3)]),
                              ("alex", (31, 31), [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]),
                              ("alex", (64, 48), [(15, 11), (7, 5), (3, 2), (3, 2), (3, 2)])):
        taps = lr.features(net, torch.zeros(1, 3, h, w, dtype=torch.float32), lr.state_dicts(net)[0])
        assert [tuple(t.shape[2:]) for t in taps] == want and tuple(t.shape[1] for t in taps) == lr.TAP_WIDTHS[net]


# ------------------------------------------------------------------------------------------- the model and its loader
def test_model_constants_are_the_references():
    from flair_amd import lpips as flp
    for net in ("vgg", "alex"):
        assert flp.TRUNKS[net]["taps"] == lr.TAP_WIDTHS[net] and flp.TRUNKS[net]["min_side"] == lr.MIN_SIDE[net]
        trunk, lin = lr.state_dicts(net)
        own = flp.LPIPS(net).state_dict()
        assert set(own) == set(trunk) | set(lin)
        assert all(own[k].shape == v.shape for k, v in {**trunk, **lin}.items())


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_loader_reads_torchvision_and_package_files(net, tmp_path):
    from flair_amd import lpips as flp
    trunk, lin = lr.state_dicts(net)
    names = flp.weight_files(net, tmp_path)
    assert [os.path.basename(p) for p in names] == {"vgg": ["vgg16.pth", "lpips_vgg.pth"], "alex": ["alexnet.pth", "lpips_alex.pth"]}[net]
    with pytest.raises(FileNotFoundError, match=os.path.basename(names[0])):
        flp.load_lpips(net, tmp_path, "cpu")
    # classifier.* of the trunk file and whatever else the package's file holds are ignored
    torch.save(dict(trunk, **{"classifier.1.weight": torch.zeros(3, 3)}), names[0])
    torch.save(dict(lin, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "net.slice1.0.weight": torch.zeros(2)}), names[1])
    model = flp.load_lpips(net, tmp_path, "cpu")
    sd = model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in {**trunk, **lin}.items())
    assert not model.training and not any(p.requires_grad for p in model.parameters())


def test_loader_names_every_misfit():
    from flair_amd import lpips as flp
    trunk, lin = (dict(d) for d in lr.state_dicts("vgg"))
    del trunk["features.5.bias"]
    del lin["lin3.model.1.weight"]
    trunk["features.3.weight"] = torch.zeros(1)
    lin["lin5.model.1.weight"] = torch.zeros(1, 8, 1, 1)
    trunk["avgpool.weight"] = torch.zeros(1)
    trunk["features.0.weight"] = torch.zeros(64, 3, 5, 5)
    lin["lin0.model.1.weight"] = torch.zeros(1, 32, 1, 1)
    with pytest.raises(ValueError) as exc:
        flp.lpips_state_dict("vgg", trunk, lin, "files")
    msg = str(exc.value)
    assert msg.startswith("files do not fit LPIPS('vgg'); unexpected keys: ")
    unexpected, missing, shapes = re.fullmatch(r".*unexpected keys: (.*); missing keys: (.*); shapes: (.*)", msg).groups()
    assert set(unexpected.split(", ")) == {"features.3.weight", "lin5.model.1.weight", "avgpool.weight"}
    assert set(missing.split(", ")) == {"features.5.bias", "lin3.model.1.weight"}
    assert "features.0.weight (64, 3, 5, 5) for (64, 3, 3, 3)" in shapes and "lin0.model.1.weight (1, 32, 1, 1) for (1, 64, 1, 1)" in shapes
    with pytest.raises(ValueError, match="holds no tensor state dict"):
        flp.lpips_state_dict("vgg", {"features.0.weight": 3}, lin)
    with pytest.raises(ValueError, match="lpips='squeeze': one of vgg, alex"):
        flp.LPIPS("squeeze")
    # an AlexNet file is no VGG-16
    with pytest.raises(ValueError, match="missing keys: .*features.28.bias"):
        flp.lpips_state_dict("vgg", *lr.state_dicts("alex"))


def test_small_frames_are_refused_by_name():
    from flair_amd import lpips as flp
    flp.check_size("vgg", 16, 16)
    flp.check_size("alex", 31, 200)
    with pytest.raises(ValueError, match=r"frames are 15x64; the vgg trunk needs frames of at least 16 pixels"):
        flp.check_size("vgg", 15, 64)
    with pytest.raises(ValueError, match=r"30x31; the alex trunk needs frames of at least 31 pixels"):
        flp.check_size("alex", 30, 31)
    with pytest.raises(ValueError, match="at least 16 pixels"):
        flp.LPIPS("vgg")(torch.zeros(1, 12, 16, 3, dtype=torch.uint8), torch.zeros(1, 12, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="fp32 only"):
        flp.LPIPS("alex").convert_to_bf16()


# ------------------------------------------------------------------------------------------- the second header
def eval_declared():
    text = open(os.path.join(ROOT, "include", "flair_eval.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_every_entry_of_the_eval_header_is_typed_and_exported():
    from flair_amd import _header, _lib
    from tests.test_abi_cpu import declared_symbols
    assert eval_declared() == sorted(_header.EVAL_PROTOS) == EVAL_ENTRIES
    assert sorted(_header.PROTOS) == declared_symbols() and not set(_header.PROTOS) & set(_header.EVAL_PROTOS)
    assert len(_header.STRUCTS) == 7
    lib = _lib.lib()
    for name, (restype, params) in _header.EVAL_PROTOS.items():
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and params[-1].name == "stream", name
        assert list(f.argtypes) == [p.ctype for p in params], name
    i, l, z, v = ctypes.c_int, ctypes.c_long, ctypes.c_size_t, ctypes.c_void_p
    assert [tuple(p) for p in _header.EVAL_PROTOS["flair_lpips_tap"][1]] == [
        ("fa", v, "float"), ("fa_ld", i, None), ("fb", v, "float"), ("fb_ld", i, None), ("F", i, None), ("HW", l, None), ("C", i, None),
        ("w", v, "float"), ("acc", v, "double"), ("ws", v, "void"), ("ws_bytes", z, None), ("stream", v, None)]
    assert [tuple(p) for p in _header.EVAL_PROTOS["flair_lpips_prepare"][1]] == [
        ("a", v, "uint8_t"), ("b", v, "uint8_t"), ("N", i, None), ("H", i, None), ("W", i, None), ("y", v, "float"), ("y_ld", i, None),
        ("stream", v, None)]


def test_the_workspace_is_the_headers_closed_form():
    from flair_amd import ops
    header = open(os.path.join(ROOT, "include", "flair_eval.h")).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "lpips.hip")).read()
    assert int(re.search(r"#define FLAIR_LPIPS_TAP_PARTS (\d+)", header).group(1)) == ops.LPIPS_TAP_PARTS
    assert "LP_PARTS = FLAIR_LPIPS_TAP_PARTS" in src and "atomic" not in src.replace("no floating-point atomics", "")
    assert not re.search(r"size_t\s+flair_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entries():
    from flair_amd import _lib
    call = _lib.call
    f32, f64, u8 = _device_tensor(torch.float32), _device_tensor(torch.float64), _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_lpips_prepare(torch.zeros(3, dtype=torch.uint8), u8, 1, 1, 1, f32, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_lpips_prepare: b must be uint8, got float32$"):
        call.flair_lpips_prepare(u8, f32, 1, 1, 1, f32, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_lpips_tap: acc must be float64, got float32$"):
        call.flair_lpips_tap(f32, 64, f32, 64, 1, 1, 64, f32, f32, u8, 8192)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_lpips_tap: fb must be float32, got float64$"):
        call.flair_lpips_tap(f32, 64, f64, 64, 1, 1, 64, f32, f64, u8, 8192)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_maxpool_valid_s2_nhwc: y must be float32, got uint8$"):
        call.flair_maxpool_valid_s2_nhwc(f32, 4, 1, 7, 7, 4, 3, u8, 4)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_alexnet_stem: bias must be float32, got float64$"):
        call.flair_alexnet_stem(f32, 16, 1, 31, 31, f32, f64, f32, 64)
    with pytest.raises(TypeError, match="flair_lpips_tap takes 11 arguments"):
        call.flair_lpips_tap(f32, 64)
    with pytest.raises(AttributeError, match="flair_lpips_tap_workspace is not an entry"):
        call.flair_lpips_tap_workspace


def test_entries_refuse_before_any_launch(monkeypatch):
    """Every refusal of the four entries: status -1 and the entry's message, on a machine without a GPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    P, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    parts = 1024 * 8

    def refused(name, args, what):
        rc = getattr(lib, name)(*args, None)
        msg = lib.flair_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)

    tap = lambda **k: tuple({**dict(fa=P, fa_ld=64, fb=P, fb_ld=64, F=1, HW=4, C=64, w=P, acc=P, ws=P, ws_bytes=parts), **k}.values())  # noqa: E731
    for k, what in [(dict(fa=None), "null pointer"), (dict(fb=None), "null pointer"), (dict(w=None), "null pointer"),
                    (dict(acc=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(F=0), "F = 0"), (dict(HW=0), "HW = 0"),
                    (dict(C=96), "C = 96 is not a tap width"), (dict(C=32), "C = 32 is not a tap width"),
                    (dict(fa_ld=60), "fa_ld = 60 must be >= C = 64"), (dict(fb_ld=66), "fb_ld = 66 must be >= C = 64 and a multiple of 4"),
                    (dict(fa=odd), "fa = "), (dict(w=odd), "16-byte aligned"), (dict(acc=odd), "hold doubles and must be 8-byte aligned"),
                    (dict(ws=odd), "8-byte aligned"), (dict(ws_bytes=parts - 1), f"ws_bytes = {parts - 1}, F * FLAIR_LPIPS_TAP_PARTS * 8 = {parts}"),
                    (dict(F=3, ws_bytes=2 * parts), f"= {3 * parts}"), (dict(F=1 << 22, ws_bytes=1 << 40), "exceed one launch")]:
        refused("flair_lpips_tap", tap(**k), what)
    prep = lambda **k: tuple({**dict(a=P, b=P, N=1, H=4, W=4, y=P, y_ld=16), **k}.values())  # noqa: E731
    for k, what in [(dict(a=None), "null pointer"), (dict(y=None), "null pointer"), (dict(N=0), "N = 0"), (dict(W=0), "W = 0"),
                    (dict(y_ld=12), "y_ld = 12 must be >= C = 16"), (dict(y_ld=18), "multiple of 4"), (dict(y=odd), "16-byte aligned")]:
        refused("flair_lpips_prepare", prep(**k), what)
    pool = lambda **k: tuple({**dict(x=P, x_ld=8, F=1, H=7, W=7, C=8, k=3, y=P, y_ld=8), **k}.values())  # noqa: E731
    for k, what in [(dict(x=None), "is null"), (dict(F=0), "F = 0"), (dict(k=4), "k = 4"), (dict(H=2), "hold no 3x3 window"),
                    (dict(k=2, W=1), "hold no 2x2 window"), (dict(C=6), "C = 6 is not a positive multiple of 4"),
                    (dict(x_ld=4), "x_ld = 4 must be >= C = 8"), (dict(y_ld=10), "y_ld = 10"), (dict(y=odd), "16-byte aligned")]:
        refused("flair_maxpool_valid_s2_nhwc", pool(**k), what)
    stem = lambda **k: tuple({**dict(x=P, x_ld=16, F=1, H=31, W=31, w=P, bias=P, y=P, y_ld=64), **k}.values())  # noqa: E731
    for k, what in [(dict(bias=None), "null pointer"), (dict(F=0), "F = 0"), (dict(H=6), "smaller than the 11x11 kernel"),
                    (dict(x_ld=2), "x_ld = 2"), (dict(y_ld=32), "y_ld = 32 must be >= C = 64"), (dict(w=odd), "16-byte aligned")]:
        refused("flair_alexnet_stem", stem(**k), what)
    # and through call(), which raises with the library's message
    monkeypatch.setattr(_lib, "stream", lambda: None)
    f32 = _device_tensor(torch.float32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_lpips_tap failed \(status -1\): flair_lpips_tap: C = 100 is not a tap width"):
        _lib.call.flair_lpips_tap(f32, 100, f32, 100, 1, 4, 100, f32, _device_tensor(torch.float64), f32, parts)


def test_ops_wrappers_refuse_wrong_tensors():
    from flair_amd import ops
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        ops.lpips_prepare(a, torch.zeros(1, 16, 17, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.lpips_prepare(a.float(), a.float())
    with pytest.raises(ValueError, match="dense"):
        ops.lpips_prepare(a.permute(0, 2, 1, 3), a.permute(0, 2, 1, 3))
    f = torch.zeros(2, 1, 4, 64)
    with pytest.raises(ValueError, match="one shape"):
        ops.lpips_tap(f, f[:1], torch.zeros(64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="the 64 weights"):
        ops.lpips_tap(f, f, torch.zeros(32), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"dense \(2,\) float64"):
        ops.lpips_tap(f, f, torch.zeros(64), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"w is \(363, 64\)"):
        ops.alexnet_stem(torch.zeros(1, 31, 31, 16), torch.zeros(64, 363), torch.zeros(64))


# ------------------------------------------------------------------------------------------- command line
def test_lpips_options_parse_and_refuse(tmp_path):
    from flair_amd.__main__ import lpips_of, main, make_parser
    ap = make_parser()
    e = ap.parse_args(["evaluate", "out", "truth", "--lpips", "alex", "--weights", "w"])
    assert (e.lpips, e.weights) == ("alex", "w")
    e = ap.parse_args(["evaluate", "out", "truth"])
    assert e.lpips is None and e.weights is None and lpips_of(e, "evaluate") is None
    assert ap.parse_args(["restore", "gaussian", "in", "out", "--ground-truth", "t", "--lpips", "vgg"]).lpips == "vgg"
    assert ap.parse_args(["interpolate", "in", "out", "--factor", "2", "--ground-truth", "t", "--lpips", "vgg"]).lpips == "vgg"
    assert not hasattr(ap.parse_args(["jpeg-demo"]), "lpips")
    with pytest.raises(SystemExit):
        ap.parse_args(["evaluate", "out", "truth", "--lpips", "squeeze"])
    with pytest.raises(SystemExit, match="evaluate: --lpips vgg reads its trunk and linear layers from --weights DIR"):
        main(["evaluate", "out", "truth", "--lpips", "vgg"])
    with pytest.raises(SystemExit, match=r"evaluate: --lpips alex needs .*alexnet\.pth and .*lpips_alex\.pth"):
        main(["evaluate", "out", "truth", "--lpips", "alex", "--weights", str(tmp_path)])
    (tmp_path / "in").mkdir()
    with pytest.raises(SystemExit, match="restore: --lpips scores the written frames against --ground-truth DIR"):
        main(["restore", "gaussian", str(tmp_path / "in"), str(tmp_path / "out"), "--lpips", "vgg", "--weights", str(tmp_path)])
    for i in range(2):
        png(tmp_path / "in" / f"{i}.png", 32, 32)
    with pytest.raises(SystemExit, match="interpolate: --lpips scores the written frames against --ground-truth DIR"):
        main(["interpolate", str(tmp_path / "in"), str(tmp_path / "out"), "--factor", "2", "--lpips", "alex", "--weights", str(tmp_path)])
    torch.save(lr.state_dicts("alex")[0], tmp_path / "alexnet.pth")
    torch.save(lr.state_dicts("vgg")[1], tmp_path / "lpips_alex.pth")
    spec = lpips_of(ap.parse_args(["evaluate", "a", "b", "--lpips", "alex", "--weights", str(tmp_path)]), "evaluate")
    assert spec == ("alex", str(tmp_path))
    from flair_amd.__main__ import load_lpips_of
    with pytest.raises(SystemExit, match=r"evaluate: .* do not fit LPIPS\('alex'\); shapes: lin1.model.1.weight \(1, 128, 1, 1\) for \(1, 192, 1, 1\)"):
        load_lpips_of(spec, "cpu", "evaluate")
    assert load_lpips_of(None, "cpu", "evaluate") is None


# ------------------------------------------------------------------------------------------- evaluate_dirs / format_report
def test_report_without_a_model_is_what_it_was(tmp_path, monkeypatch):
    """evaluate_dirs without a model returns the keys of before, and format_report prints the literal lines of before."""
    from flair_amd import metrics
    rows = dict(psnr=[math.inf, 31.23456], ssim=[1.0, 0.912349], sse=[0, 5])
    monkeypatch.setattr(metrics, "psnr_ssim", lambda a, b: rows)
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        for i in range(2):
            png(tmp_path / d / f"{i:04d}.png", 16, 20, value=i)
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu")
    assert res == dict(frames=[dict(name="0000.png", psnr=math.inf, ssim=1.0), dict(name="0001.png", psnr=31.23456, ssim=0.912349)],
                       mean=dict(psnr=math.inf, ssim=(1.0 + 0.912349) / 2), count=2)
    assert metrics.format_report(res) == ["0000.png  psnr inf  ssim 1.0000", "0001.png  psnr 31.2346  ssim 0.9123",
                                          "mean of 2 frames  psnr inf  ssim 0.9562"]

    class Model:                                # stands in for LPIPS: evaluate_dirs reads .net and calls it on the batch
        net = "vgg"

        def __call__(self, a, b):
            return [0.25 + 0.125 * i for i in range(a.shape[0])]
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", lpips=Model())
    assert [f["lpips"] for f in res["frames"]] == [0.25, 0.375] and res["mean"]["lpips"] == 0.3125
    assert metrics.format_report(res) == ["0000.png  psnr inf  ssim 1.0000  lpips 0.2500", "0001.png  psnr 31.2346  ssim 0.9123  lpips 0.3750",
                                          "mean of 2 frames  psnr inf  ssim 0.9562  lpips 0.3125"]
    # the trunk's minimum is checked on the file headers, with the other refusals: nothing is decoded
    monkeypatch.setattr(metrics.fio, "iter_frame_batches", lambda *a, **k: pytest.fail("decoded before the refusal"))
    Model.net = "alex"
    with pytest.raises(ValueError, match=r"evaluate: .*0000\.png and .*0000\.png are 16x20; the alex trunk needs frames of at least 31"):
        metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", lpips=Model())
