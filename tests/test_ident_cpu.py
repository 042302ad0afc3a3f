"""CPU: the ArcFace identity network's shape, its folded weights against the definition (tests/ident_ref.py), the calibrated
case the GPU tests stand on, the loader, the fourth header, the two entries' refusals, the command line, the report and the
host's cosine / drift arithmetic."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ident_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def png(path, h, w, value=0):
    from flair_amd import io as fio
    fio.write_frame(str(path), np.full((h, w, 3), value, dtype=np.uint8))


def loaded(sd):
    from flair_amd import identity as fid
    m = fid.ArcFace()
    m.load_state_dict(fid.identity_state_dict(sd))
    return m


# ------------------------------------------------------------------------------------------- the network
def test_parameter_and_key_counts():
    from flair_amd import identity as fid
    m = fid.ArcFace()
    own = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == R.PARAMETERS == 25627081
    assert len(own) == R.ENTRIES == 181
    assert {k: tuple(v.shape) for k, v in own.items()} == R.shapes() and list(own) == list(R.shapes())
    assert m.layer1[0].downsample is None and m.layer2[0].downsample is not None and m.layer2[1].downsample is None
    assert all(p.numel() == 1 for k, p in own.items() if k.endswith("prelu.weight"))
    with pytest.raises(ValueError, match="fp32 only"):
        m.convert_to_bf16()


def test_folded_weights_reproduce_the_definition_in_float64():
    """bn4 and bn5 folded into fc5 with its columns permuted to NHWC, and bn0 in the (x - sub) * mul form of the kernel that
    applies it: within 1e-12 relative of the unfolded float64 network."""
    from flair_amd import identity as fid
    c = R.case()
    m = loaded(c["sd"])
    w, b = fid.fold_head(m.bn4, m.fc5, m.bn5)
    assert w.dtype == torch.float64 and tuple(w.shape) == (512, 32768) and tuple(b.shape) == (512,)
    nhwc = c["feat64"].permute(0, 2, 3, 1).reshape(12, -1)
    got = (nhwc @ w.t() + b).numpy()
    err = np.abs(got - c["e64"]).max() / np.abs(c["e64"]).max()
    print(f"ident fold: head relative deviation {err:.3e}")
    assert err < 1e-12
    wrong = (c["feat64"].reshape(12, -1) @ w.t() + b).numpy()              # the columns left in (C, H, W) order
    assert np.abs(wrong - c["e64"]).max() > 0.1
    x = torch.randn(2, 64, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    sub, mul = fid.bn0_terms(m.layer1[0].bn0)
    want = R._bn(x, c["sd"], "layer1.0.bn0")
    got = (x - sub.view(1, -1, 1, 1)) * mul.view(1, -1, 1, 1)
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-12
    m.layer1[0].bn0.weight[3] = 0.0
    with pytest.raises(ValueError, match="zero scale in channel 3"):
        fid.bn0_terms(m.layer1[0].bn0)


def test_the_calibrated_case_is_not_blind():
    """The GPU tests compare cosines: the reference's must hold an exact 1 and span at least -0.1 .. 0.9, and none may sit so
    close to a rounding step of the four printed decimals that the printed text could differ for a correct result."""
    c = R.case()
    cos = R.cosines(c["e64"][:6], c["e64"][6:])
    cos32 = R.cosines(c["e32"][:6], c["e32"][6:])
    print(f"ident case: cosines {cos.tolist()}; f32 restatement deviates by {np.abs(c['e32'] - c['e64']).max():.3e} on embeddings of "
          f"magnitude {np.abs(c['e64']).max():.3f}, by {np.abs(cos32 - cos).max():.3e} on the cosines")
    assert cos[0] == 1.0 and cos.min() <= -0.1 and cos.max() >= 0.9
    assert np.sort(cos)[-2] > 0.9 and np.sort(cos)[-2] < 1.0 and ((cos > -0.1) & (cos < 0.9)).any()
    printed = np.concatenate([cos[1:], [cos.mean(), R.drift(c["e64"][:6]), R.drift(c["e64"][6:])]])     # what evaluate prints of the case
    room = np.abs(printed * 1e4 - np.floor(printed * 1e4) - 0.5) * 1e-4
    pairs = lambda e: np.concatenate([R.cosines(e[:6], e[6:]), R.cosines(e[1:6], e[:5]), R.cosines(e[7:], e[6:11])])     # noqa: E731
    bound = 4.0 * np.abs(pairs(c["e32"]) - pairs(c["e64"])).max()          # what tests/test_gpu_ident.py grants a cosine
    assert 0 < 2 * bound < room.min(), (room, bound)
    raw = R.embed(torch.cat([c["a"], c["b"]]), R.state_dict()).numpy()
    assert R.cosines(raw[:6], raw[6:]).min() > 0.7   # without the calibration even a frame and its negative look alike


def test_prepare_reference_on_hand_cases():
    u8 = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    assert torch.equal(R.prepare(u8), torch.full((1, 1, 128, 128), -(0.2989 + 0.5870 + 0.1140), dtype=torch.float64))
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 256, 256, 3).contiguous()
    got = R.prepare(u8)                              # exact 2:1 both weights 1/2: the mean of two neighbours
    x = (2.0 * torch.arange(256, dtype=torch.float64) / 255.0 - 1.0) * (0.2989 + 0.5870 + 0.1140)
    assert (got[0, 0, 5] - (x[0::2] + x[1::2]) / 2).abs().max() < 1e-15


# ------------------------------------------------------------------------------------------- the loader
def test_loader_accepts_both_spellings_and_names_every_fault(tmp_path):
    from flair_amd import identity as fid
    sd = R.case()["sd"]
    plain = fid.identity_state_dict(sd)
    prefixed = fid.identity_state_dict({"module." + k: v for k, v in sd.items()})
    no_counters = fid.identity_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    assert list(plain) == list(prefixed) == list(no_counters) == list(fid.ArcFace().state_dict())
    assert all(torch.equal(plain[k], prefixed[k]) for k in plain if not k.endswith("num_batches_tracked"))
    torch.save({"module." + k: v for k, v in sd.items()}, tmp_path / "arcface_resnet18.pth")
    m = fid.load_identity(str(tmp_path / "arcface_resnet18.pth"), "cpu")
    assert torch.equal(m.layer3[0].downsample[1].running_var, sd["layer3.0.downsample.1.running_var"])
    assert torch.equal(m.fc5.weight, sd["fc5.weight"]) and not m.training

    bad = dict(sd)
    del bad["layer2.0.downsample.0.weight"], bad["bn5.running_var"]
    bad["layer1.0.downsample.0.weight"] = torch.zeros(64, 64, 1, 1)
    bad["fc5.weight"] = torch.zeros(512, 512 * 7 * 7)
    with pytest.raises(ValueError) as exc:
        fid.identity_state_dict(bad, "file.pth")
    text = str(exc.value)
    assert text.startswith("file.pth does not fit ResNetArcFace")
    assert "unexpected keys: layer1.0.downsample.0.weight" in text
    assert "missing keys: layer2.0.downsample.0.weight, bn5.running_var" in text
    assert "shapes: fc5.weight (512, 25088) for (512, 32768)" in text
    with pytest.raises(ValueError, match=r"layer1\.0\.se\.fc\.0\.weight\); use_se=True is not built"):
        fid.identity_state_dict(dict(sd, **{"module.layer1.0.se.fc.0.weight": torch.zeros(4, 64)}))
    for junk in ({}, {"a": 1}, [1, 2], {"state_dict": dict(sd)}):
        with pytest.raises(ValueError, match="holds no tensor state dict"):
            fid.identity_state_dict(junk)
    with pytest.raises(FileNotFoundError, match="nope.pth not found"):
        fid.load_identity(str(tmp_path / "nope.pth"), "cpu")
    (tmp_path / "text.pth").write_text("not a checkpoint")
    with pytest.raises(ValueError, match="not a tensor state dict"):
        fid.load_identity(str(tmp_path / "text.pth"), "cpu")
    torch.save({"net": fid.ArcFace()}, tmp_path / "pickled.pth")          # a pickled module: weights_only refuses it
    with pytest.raises(ValueError, match="not a tensor state dict"):
        fid.load_identity(str(tmp_path / "pickled.pth"), "cpu")


# ------------------------------------------------------------------------------------------- the fourth header
def ident_declared():
    text = open(os.path.join(ROOT, "include", "flair_ident.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_ident_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib, ops
    assert ident_declared() == sorted(_header.IDENT_PROTOS) == ["flair_ident_embed", "flair_ident_prepare"]
    others = set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS)
    assert not set(_header.IDENT_PROTOS) & others
    assert set(_lib.ALL_PROTOS) == others and not set(_header.IDENT_PROTOS) & set(_lib.ALL_PROTOS)
    assert len(_header.STRUCTS) == 7 and _header.parse(open(_header.IDENT_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 20
    for name, (restype, params) in _header.IDENT_PROTOS.items():
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and params[-1].name == "stream", name
        assert list(f.argtypes) == [p.ctype for p in params], name
    i, z, v = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    assert [tuple(p) for p in _header.IDENT_PROTOS["flair_ident_prepare"][1]] == [
        ("a", v, "uint8_t"), ("b", v, "uint8_t"), ("N", i, None), ("H", i, None), ("W", i, None), ("y", v, "float"), ("y_ld", i, None),
        ("stream", v, None)]
    assert [tuple(p) for p in _header.IDENT_PROTOS["flair_ident_embed"][1]] == [
        ("x", v, "float"), ("x_ld", i, None), ("F", i, None), ("K", i, None), ("w", v, "float"), ("bias", v, "float"), ("O", i, None),
        ("out", v, "float"), ("out_ld", i, None), ("ws", v, "void"), ("ws_bytes", z, None), ("stream", v, None)]
    header = open(_header.IDENT_HEADER_PATH).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "ident.hip")).read()
    assert int(re.search(r"#define FLAIR_IDENT_SIDE (\d+)", header).group(1)) == ops.IDENT_SIDE == R.SIDE
    assert int(re.search(r"#define FLAIR_IDENT_EMBED_KCHUNK (\d+)", header).group(1)) == ops.IDENT_EMBED_KCHUNK
    assert "EM_KCHUNK = FLAIR_IDENT_EMBED_KCHUNK" in src and "atomic" not in src.replace("no atomics", "")
    assert not re.search(r"size_t\s+flair_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))     # the workspace is a closed form
    assert "flair_ident.h" in open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read()


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entries():
    from flair_amd import _lib
    call = _lib.call
    f32, f64, u8 = _device_tensor(torch.float32), _device_tensor(torch.float64), _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_ident_prepare(torch.zeros(3, dtype=torch.uint8), None, 1, 1, 1, f32, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_ident_prepare: b must be uint8, got float32$"):
        call.flair_ident_prepare(u8, f32, 1, 1, 1, f32, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_ident_prepare: y must be float32, got float64$"):
        call.flair_ident_prepare(u8, None, 1, 1, 1, f64, 16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_ident_embed: w must be float32, got float64$"):
        call.flair_ident_embed(f32, 2048, 1, 2048, f64, f32, 8, f32, 8, u8, 64)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_ident_embed: out must be float32, got float64$"):
        call.flair_ident_embed(f32, 2048, 1, 2048, f32, f32, 8, f64, 8, u8, 64)
    with pytest.raises(TypeError, match="flair_ident_embed takes 11 arguments"):
        call.flair_ident_embed(f32, 2048)
    with pytest.raises(AttributeError, match="flair_ident_embed_workspace is not an entry"):
        call.flair_ident_embed_workspace


def test_entries_refuse_before_any_launch(monkeypatch):
    """Every refusal the header lists: status -1 and the entry's message, on a machine without a GPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    cases = R.entry_refusals()
    assert {n for n, _, _ in cases} == {"flair_ident_prepare", "flair_ident_embed"} and len(cases) >= 29
    for name, args, what in cases:
        R.assert_refused(lib, name, args, what)
    monkeypatch.setattr(_lib, "stream", lambda: None)
    f32 = _device_tensor(torch.float32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_ident_embed failed \(status -1\): flair_ident_embed: K = 6 is not a multiple of 4"):
        _lib.call.flair_ident_embed(f32, 8, 1, 6, f32, f32, 8, f32, 8, f32, 64)


def test_ops_wrappers_refuse_wrong_tensors():
    from flair_amd import ops
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        ops.ident_prepare(a, torch.zeros(1, 16, 17, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.ident_prepare(a.float())
    with pytest.raises(ValueError, match="dense"):
        ops.ident_prepare(a.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match=r"out holds \(2, 128, 128\) pixels, not \(1, 128, 128\)"):
        ops.ident_prepare(a, out=torch.zeros(2, 128, 128, 16))
    x = torch.zeros(2, 2048)
    with pytest.raises(ValueError, match=r"w is a dense \(O, 2048\) tensor"):
        ops.ident_embed(x, torch.zeros(8, 1024), torch.zeros(8))
    with pytest.raises(ValueError, match="bias holds 8 values"):
        ops.ident_embed(x, torch.zeros(8, 2048), torch.zeros(4))
    with pytest.raises(ValueError, match=r"out is \(2, 8\) rows of floats"):
        ops.ident_embed(x, torch.zeros(8, 2048), torch.zeros(8), out=torch.zeros(2, 9))
    with pytest.raises(ValueError, match=r"x is \(F, K\) rows of floats"):
        ops.ident_embed(x.t(), torch.zeros(8, 2), torch.zeros(8))


# ------------------------------------------------------------------------------------------- the host's arithmetic
def test_cosine_drift_and_missing_values_on_hand_made_embeddings():
    from flair_amd import identity as fid
    e = lambda *v: np.array(v, dtype=np.float64)                         # noqa: E731
    assert fid.cosine(e(3, 4), e(3, 4)) == 1.0 and fid.cosine(e(1, 0), e(0, 2)) == 0.0 and fid.cosine(e(1, 0), e(-5, 0)) == -1.0
    assert fid.cosine(e(3, 4), e(4, 3)) == 24 / 25
    assert fid.cosine(e(0, 0), e(1, 0)) is None and fid.cosine(e(1, 0), e(0, 0)) is None
    v = np.random.default_rng(0).standard_normal((50, 512))
    assert all(fid.cosine(r, r.copy()) == 1.0 for r in v)                # one root: equal embeddings give exactly 1
    seq = [e(1, 0), e(0, 1), e(0, 2), e(-1, 0)]                          # cosines 0, 1, 0
    assert fid.drift(seq) == (1.0 + 0.0 + 1.0) / 3
    assert fid.drift([e(1, 0)]) is None and fid.drift([]) is None
    assert fid.drift([e(1, 0), e(0, 0), e(0, 3), e(0, 1)]) == 0.0        # two pairs with a zero embedding are left out
    assert fid.drift([e(1, 0), e(0, 0)]) is None
    ids, mean = fid.scores([e(1, 0), e(0, 0), e(3, 4)], [e(1, 0), e(1, 1), e(4, 3)])
    assert ids == [1.0, None, 24 / 25] and mean["ids"] == (1.0 + 24 / 25) / 2 and mean["id_drift"] is None
    assert mean["id_drift_truth"] == pytest.approx(((1 - 1 / math.sqrt(2)) + (1 - 7 / (5 * math.sqrt(2)))) / 2, abs=1e-15) and len(mean) == 3
    assert fid.scores([e(0, 0)], [e(0, 0)]) == ([None], dict(ids=None, id_drift=None, id_drift_truth=None))
    assert fid.format_value(0.81234) == "  ids 0.8123" and fid.format_value(None) == "  ids n/a"
    assert fid.format_mean(dict(ids=0.5, id_drift=0.03126, id_drift_truth=None)) == "  ids 0.5000  id-drift 0.0313 (truth n/a)"
    assert json.dumps(dict(ids=None)) == '{"ids": null}'
    with pytest.raises(ValueError, match=r"identity: out/0003.png is 64x96; the score takes aligned face crops, which are square"):
        fid.check_size(64, 96, what="out/0003.png")
    fid.check_size(37, 37)


# ------------------------------------------------------------------------------------------- command line
def test_identity_option_parses_and_refuses(tmp_path):
    from flair_amd.__main__ import identity_of, load_identity_of, main, make_parser
    ap = make_parser()
    assert ap.parse_args(["evaluate", "out", "truth", "--identity", "f.pth"]).identity == "f.pth"
    e = ap.parse_args(["evaluate", "out", "truth"])
    assert e.identity is None and identity_of(e, "evaluate") is None and load_identity_of(None, "cpu", "evaluate") is None
    assert ap.parse_args(["restore", "gaussian", "in", "out", "--ground-truth", "t", "--identity", "f.pth"]).identity == "f.pth"
    assert ap.parse_args(["interpolate", "in", "out", "--factor", "2", "--ground-truth", "t", "--identity", "f.pth"]).identity == "f.pth"
    assert not hasattr(ap.parse_args(["jpeg-demo"]), "identity") and not hasattr(ap.parse_args(["niqe", "d"]), "identity")
    for command in ("evaluate", "restore", "interpolate"):
        text = re.sub(r"\s+", " ", ap._subparsers._group_actions[0].choices[command].format_help())
        assert "--identity FILE" in text and "must be square" in text and "a cut shows up as drift" in text
    with pytest.raises(SystemExit, match=r"evaluate: --identity .*nope\.pth is not a file"):
        main(["evaluate", "out", "truth", "--identity", str(tmp_path / "nope.pth")])
    (tmp_path / "in").mkdir()
    torch.save({"a": torch.zeros(1)}, tmp_path / "f.pth")
    with pytest.raises(SystemExit, match="restore: --identity compares the written frames with --ground-truth DIR"):
        main(["restore", "gaussian", str(tmp_path / "in"), str(tmp_path / "out"), "--identity", str(tmp_path / "f.pth")])
    for i in range(2):
        png(tmp_path / "in" / f"{i}.png", 32, 32)
    with pytest.raises(SystemExit, match="interpolate: --identity compares the written frames with --ground-truth DIR"):
        main(["interpolate", str(tmp_path / "in"), str(tmp_path / "out"), "--factor", "2", "--identity", str(tmp_path / "f.pth")])
    path = identity_of(ap.parse_args(["evaluate", "a", "b", "--identity", str(tmp_path / "f.pth")]), "evaluate")
    assert path == str(tmp_path / "f.pth")
    with pytest.raises(SystemExit, match=r"evaluate: .*f\.pth does not fit ResNetArcFace.*unexpected keys: a; missing keys: conv1.weight"):
        load_identity_of(path, "cpu", "evaluate")


# ------------------------------------------------------------------------------------------- evaluate_dirs / format_report
def test_report_and_json_are_what_they_were_without_the_option(tmp_path, monkeypatch):
    from flair_amd import metrics
    from flair_amd.__main__ import write_json
    rows = dict(psnr=[math.inf, 31.23456, 30.0], ssim=[1.0, 0.912349, 0.5], sse=[0, 5, 6])
    monkeypatch.setattr(metrics, "psnr_ssim", lambda a, b: rows)
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        for i in range(3):
            png(tmp_path / d / f"{i:04d}.png", 20, 20, value=i)
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu")
    assert res == dict(frames=[dict(name="0000.png", psnr=math.inf, ssim=1.0), dict(name="0001.png", psnr=31.23456, ssim=0.912349),
                               dict(name="0002.png", psnr=30.0, ssim=0.5)],
                       mean=dict(psnr=math.inf, ssim=(1.0 + 0.912349 + 0.5) / 3), count=3)
    assert metrics.format_report(res) == ["0000.png  psnr inf  ssim 1.0000", "0001.png  psnr 31.2346  ssim 0.9123",
                                          "0002.png  psnr 30.0000  ssim 0.5000", "mean of 3 frames  psnr inf  ssim 0.8041"]
    write_json(tmp_path / "plain.json", res)
    assert "ids" not in open(tmp_path / "plain.json").read() and "id_drift" not in open(tmp_path / "plain.json").read()

    class Model:                                # stands in for ArcFace: evaluate_dirs calls .embed on a batch of both sets
        calls = 0

        def embed(self, a, b):
            Model.calls += 1
            ea = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])[:a.shape[0]]
            eb = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 2.0]])[:a.shape[0]]
            return np.concatenate([ea, eb])
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", identity=Model())
    half = math.sqrt(0.5)
    assert Model.calls == 1 and [f["ids"] for f in res["frames"]] == [1.0, pytest.approx(half, abs=1e-15), None]
    assert set(res["mean"]) == {"psnr", "ssim", "ids", "id_drift", "id_drift_truth"} and set(res["frames"][0]) == {"name", "psnr", "ssim", "ids"}
    assert res["mean"]["ids"] == pytest.approx((1.0 + half) / 2, abs=1e-15) and res["mean"]["id_drift"] == 1.0
    assert res["mean"]["id_drift_truth"] == pytest.approx(1.0 - half, abs=1e-15)
    assert metrics.format_report(res) == ["0000.png  psnr inf  ssim 1.0000  ids 1.0000", "0001.png  psnr 31.2346  ssim 0.9123  ids 0.7071",
                                          "0002.png  psnr 30.0000  ssim 0.5000  ids n/a",
                                          "mean of 3 frames  psnr inf  ssim 0.8041  ids 0.8536  id-drift 1.0000 (truth 0.2929)"]
    write_json(tmp_path / "ids.json", res)
    back = json.load(open(tmp_path / "ids.json"))
    assert back["frames"][2]["ids"] is None and back["mean"] == res["mean"]
    # a rectangular frame is refused on the file headers, with the other refusals: nothing is decoded
    png(tmp_path / "a" / "0003.png", 20, 30)
    png(tmp_path / "b" / "0003.png", 20, 30)
    monkeypatch.setattr(metrics.fio, "iter_frame_batches", lambda *a, **k: pytest.fail("decoded before the refusal"))
    with pytest.raises(ValueError, match=r"identity: evaluate: .*a.0003\.png is 20x30; the score takes aligned face crops"):
        metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", identity=Model())
