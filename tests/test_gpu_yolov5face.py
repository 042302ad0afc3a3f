"""YOLOv5-face detectors on the GPU: the five entries of csrc/detect.hip against torch on the CPU (outputs are views into
wider buffers whose sentinel must survive, inputs strided views where the model uses one), both networks against the
reference's own tensors (tests/golden/g16_yolov5face.npz), the detections, and FaceRestoreHelper driving the n detector.

Errors measured on an MI355X (f32 kernels, max |HIP - reference| / max |reference| per tensor; every test prints its
figure before it asserts; profiles/yolov5face_detect.txt keeps the run), and the bounds: min(cap, 8 x the worst measured),
rounded down.  The caps are 1e-5 for the decode and letterbox kernels alone and 2e-4 for network tensors.
  flair_yolo_face_decode (against float64, raw values in [-8, 8])
      12x20 stride 8: 4.367e-08   3x5 stride 32: 7.215e-08   1x1 stride 32: 5.494e-08      worst 7.215e-08 -> bound 5.7e-7
      (the longest chain, (2 sigmoid(v))^2 * anchor, is some 8 f32 roundings of 6.0e-8 each: the figure is of that size)
  flair_letterbox_nhwc (against F.interpolate in float64; copies are also bit-equal to the f32 evaluation)
      96x160, 90x160, 91x160 (copies): 5.914e-08   88x150 (bilinear to 94x160): 1.118e-07   worst 1.118e-07 -> bound 8.9e-7
  yolov5n against the fixture
      stem 5.663e-07  det0 3.538e-07  raw0 5.921e-07  det1 3.798e-07  raw1 3.641e-07  det2 4.409e-07  raw2 6.397e-07
      z 3.889e-07                                                                          worst 6.397e-07 -> bound 5.1e-6
  yolov5l against the fixture
      stem 7.647e-07  det0 3.721e-07  raw0 1.074e-06  det1 3.321e-07  raw1 9.384e-07  det2 3.814e-07  raw2 5.939e-07
      z 5.824e-07                                                                          worst 1.074e-06 -> bound 8.5e-6
  detections (frame pixels, gain 1): the network's bound times max |z| (1255.6 for n, 1676.8 for l), i.e. 6.4e-3 and 1.4e-2
      pixels; measured largest difference 6.9e-05 (n, 20 + 20 detections) and 1.6e-04 (l, 2 + 2 detections)
The kernels use no atomics and a fixed evaluation order, so a run repeats these figures.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden.weights import name_seeded_weights

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "g16_yolov5face.npz")
SENTINEL = -12345.0
# min(cap, 8 x measured), figures in the module docstring
DECODE_TOL = 5.7e-7
LETTERBOX_TOL = 8.9e-7
NET_TOL = {"yolov5n": 5.1e-6, "yolov5l": 8.5e-6}


def _yf():
    from flair_amd.guided_diffusion import yolov5face
    return yolov5face


def _guarded(shape, c, off, dtype, dev, total=None):
    """A (.., c) channel-slice view at channel offset ``off`` of a wider sentinel-filled buffer -> (buffer, view)."""
    total = total if total is not None else off + c + 8
    buf = torch.full((*shape, total), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[..., off:off + c]


def _guard_intact(buf, off, c):
    mask = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    mask[off:off + c] = False
    return bool((buf[..., mask] == SENTINEL).all())


def _nchw(x):
    return x.permute(0, 3, 1, 2).float().cpu()


# ------------------------------------------------------------------------------------------------- the five entries
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_maxpool2x2s2_is_bit_equal(dev, dtype):
    from flair_amd import ops
    g = torch.Generator().manual_seed(1)
    for H, W in ((7, 10), (1, 5), (6, 1), (8, 8)):
        for C in (16, 32, 64):
            src = torch.randn(2, H, W, C + 16, generator=g).to(dtype).to(dev)
            x = src[..., 8:8 + C]                                           # strided input view
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
            buf, y = _guarded((2, Ho, Wo), C, 16, dtype, dev)
            ops.maxpool2x2s2(x, out=y)
            ref = F.max_pool2d(_nchw(x), 2, 2, ceil_mode=True)
            assert torch.equal(_nchw(y), ref), (H, W, C)
            assert _guard_intact(buf, 16, C), (H, W, C)


@pytest.mark.parametrize("ks", [(3, 5, 7), (5, 9, 13)])
def test_spp_maxpool_is_bit_equal(dev, ks):
    from flair_amd import ops
    g = torch.Generator().manual_seed(2)
    for H, W in ((3, 5), (1, 1), (13, 20)):
        for C in (16, 64, 512):
            buf = torch.full((2, H, W, 4 * C + 8), SENTINEL, dtype=torch.float32, device=dev)
            x = torch.randn(2, H, W, C, generator=g)
            buf[..., :C] = x.to(dev)
            ops.spp_maxpool(buf[..., :4 * C], C, ks)
            assert torch.equal(buf[..., :C].cpu(), x) and bool((buf[..., 4 * C:] == SENTINEL).all()), (H, W, C)
            xn = x.permute(0, 3, 1, 2)
            for j, k in enumerate(ks):
                ref = F.max_pool2d(xn, k, 1, k // 2)
                assert torch.equal(_nchw(buf[..., (j + 1) * C:(j + 2) * C]), ref), (H, W, C, k)


def test_spp_maxpool_bf16_is_bit_equal(dev):
    from flair_amd import ops
    g = torch.Generator().manual_seed(3)
    C, ks = 32, (3, 5, 7)
    x = torch.randn(2, 6, 7, C, generator=g).bfloat16()
    buf = torch.full((2, 6, 7, 4 * C + 8), SENTINEL, dtype=torch.bfloat16, device=dev)
    buf[..., :C] = x.to(dev)
    ops.spp_maxpool(buf[..., :4 * C], C, ks)
    assert bool((buf[..., 4 * C:] == SENTINEL).all())
    for j, k in enumerate(ks):
        assert torch.equal(_nchw(buf[..., (j + 1) * C:(j + 2) * C]), F.max_pool2d(x.float().permute(0, 3, 1, 2), k, 1, k // 2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_channel_interleave_is_bit_equal(dev, dtype):
    from flair_amd import ops
    g = torch.Generator().manual_seed(4)
    for C in (16, 64, 256):
        wide = torch.randn(2, 5, 7, 2 * C, generator=g).to(dtype).to(dev)
        a = wide[..., :C]                                                   # the untouched half of a stride-1 unit's input
        b = torch.randn(2, 5, 7, C, generator=g).to(dtype).to(dev)
        buf, y = _guarded((2, 5, 7), 2 * C, 8, dtype, dev)
        ops.channel_interleave(a, b, out=y)
        cat = torch.cat((_nchw(a), _nchw(b)), 1)                            # channel_shuffle(cat, 2), common.py:25-34
        ref = cat.view(2, 2, C, 5, 7).transpose(1, 2).contiguous().view(2, -1, 5, 7)
        assert torch.equal(_nchw(y), ref), C
        assert _guard_intact(buf, 8, 2 * C), C


def _decode_ref(x, na, stride, anchor_grid):
    """Detect.forward's inference branch (yolo.py:52-86) in float64.  x: (B, ny, nx, na * 16) -> (B, na * ny * nx, 16)."""
    B, ny, nx, _ = x.shape
    v = x.double().view(B, ny, nx, na, 16).permute(0, 3, 1, 2, 4)             # (B, na, ny, nx, 16)
    yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
    grid = torch.stack((xv, yv), 2).view(1, 1, ny, nx, 2).double()
    ag = torch.tensor(anchor_grid, dtype=torch.float64).view(1, na, 1, 1, 2)
    y = torch.zeros_like(v)
    s = torch.sigmoid(v)
    y[..., 0:2] = (s[..., 0:2] * 2.0 - 0.5 + grid) * stride
    y[..., 2:4] = (s[..., 2:4] * 2) ** 2 * ag
    y[..., 4], y[..., 15] = s[..., 4], s[..., 15]
    for j in range(5, 15, 2):
        y[..., j:j + 2] = v[..., j:j + 2] * ag + grid * stride
    return y.reshape(B, -1, 16)


def test_yolo_face_decode(dev):
    from flair_amd import ops
    g = torch.Generator().manual_seed(5)
    yf = _yf()
    worst = 0.0
    for (ny, nx, stride), anchors in zip(((12, 20, 8.0), (3, 5, 32.0), (1, 1, 32.0)), (yf.ANCHORS[0], yf.ANCHORS[2], yf.ANCHORS[2])):
        ag = [(anchors[2 * a], anchors[2 * a + 1]) for a in range(3)]
        wide = ((torch.rand(2, ny, nx, 64, generator=g) * 16 - 8)).to(dev)
        x = wide[..., 8:56]                                                 # 48 of 64 channels
        rows, row0 = 3 * ny * nx, 7
        z = torch.full((2, rows + 20, 16), SENTINEL, dtype=torch.float32, device=dev)
        ops.yolo_face_decode(x, 3, stride, ag, z, row0)
        ref = _decode_ref(x.cpu(), 3, stride, ag)
        err = (z[:, row0:row0 + rows].cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        print(f"decode {ny}x{nx} stride {stride}: rel err {err:.3e}")
        worst = max(worst, err)
        assert bool((z[:, :row0] == SENTINEL).all()) and bool((z[:, row0 + rows:] == SENTINEL).all())
        assert err <= DECODE_TOL, (ny, nx, err)
    print(f"decode worst rel err {worst:.3e}")


# new_unpad (h, w), (top, bottom), (left, right) of utils/datasets.py:5-35 for imgsz = 160, derived by hand
LETTERBOX_CASES = {(96, 160): ((96, 160), (0, 0), (0, 0)), (90, 160): ((90, 160), (3, 3), (0, 0)), (91, 160): ((91, 160), (2, 3), (0, 0)),
                   (88, 150): ((94, 160), (1, 1), (0, 0))}


def _letterbox_ref(x, dtype):
    """clamp(127.5 x + 127.5, 0, 255), the new_unpad image, / 255 (times float32(1 / 255) in float32), 114 / 255 around it."""
    B, _, H, W = x.shape
    (nh, nw), (top, bottom), (left, right) = LETTERBOX_CASES[(H, W)]
    v = (x.to(dtype) * 127.5 + 127.5).clamp(0, 255)
    if (nh, nw) != (H, W):
        v = F.interpolate(v, size=(nh, nw), mode="bilinear", align_corners=False)
    v = v * (torch.tensor(1 / 255, dtype=torch.float32).to(dtype))
    out = torch.full((B, 3, nh + top + bottom, nw + left + right), 114 / 255, dtype=dtype)
    out[:, :, top:top + nh, left:left + nw] = v
    return out, (nh, nw), (top, left)


@pytest.mark.parametrize("hw", [(96, 160), (90, 160), (91, 160), (88, 150)])
def test_letterbox(dev, hw):
    from flair_amd import ops
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(2, 3, *hw, generator=g) * 2.2 - 1.1).half().float()      # fp16-exact, a little outside [-1, 1]: the clamp acts
    ref64, (nh, nw), (top, left) = _letterbox_ref(x, torch.float64)
    Ho, Wo = ref64.shape[2:]
    assert (Ho, Wo) == (96, 160)
    buf, y = _guarded((2, Ho, Wo), 16, 8, torch.float32, dev)
    ops.letterbox(x.to(dev), (nh, nw), (top, left), (Ho, Wo), pre=(127.5, 127.5, 0.0, 255.0), scale=1 / 255, out=y)
    assert _guard_intact(buf, 8, 16)
    got = _nchw(y)
    assert bool((got[:, 3:] == 0).all())
    err = (got[:, :3].double() - ref64).abs().max().item() / ref64.abs().max().item()
    print(f"letterbox {hw}: rel err {err:.3e}")
    assert err <= LETTERBOX_TOL, err
    if (nh, nw) == hw:                                                      # a copy: bit-equal to the float32 evaluation
        ref32, _, _ = _letterbox_ref(x, torch.float32)
        assert torch.equal(got[:, :3], ref32)


# ------------------------------------------------------------------------------------------------- the networks
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def nets(dev, gold):
    """Both detectors with the fixture's weights (name-seeded, Detect.m[i].weight times the recorded factors), loaded through
    load_state_dict like a checkpoint; built once for the module."""
    yf = _yf()
    out = {}

    def get(cfg):
        if cfg not in out:
            src = name_seeded_weights(yf.Model(cfg))
            with torch.no_grad():
                for mi, f in zip(src.model[-1].m, gold[cfg + "_factors"]):
                    mi.weight.mul_(float(f))
            det = yf.YoloDetector(cfg, device=dev)
            det.load_state_dict(src.state_dict(), strict=True)
            out[cfg] = det
        return out[cfg]
    return get


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("cfg", ["yolov5n", "yolov5l"])
def test_network_matches_reference(dev, gold, nets, cfg):
    det = nets(cfg)
    m = det.detector
    x = torch.from_numpy(gold["x"].astype(np.float32)).to(dev)
    head = m.model[-1]
    taps = {0: None, **{i: None for i in head.f}}
    z, raw = m.run_clip(m.to_clip(x), taps=taps)
    errs = {"stem": _rel(taps[0][..., torch.from_numpy(gold[cfg + "_stem_idx"]).to(dev)].permute(0, 3, 1, 2), gold[cfg + "_stem"])}
    for i, layer in enumerate(head.f):
        idx = torch.from_numpy(gold[f"{cfg}_det{i}_idx"]).to(dev)
        errs[f"det{i}"] = _rel(taps[layer][..., idx].permute(0, 3, 1, 2), gold[f"{cfg}_det{i}"])
        r = raw[i]
        assert r.shape[3] == head.na * 16
        errs[f"raw{i}"] = _rel(r.view(r.shape[0], r.shape[1], r.shape[2], head.na, 16).permute(0, 3, 1, 2, 4), gold[f"{cfg}_raw{i}"])
    errs["z"] = _rel(z, gold[cfg + "_z"])
    print(cfg, {k: f"{v:.3e}" for k, v in errs.items()})
    assert tuple(z.shape) == (2, 945, 16)
    for k, v in errs.items():
        assert v <= NET_TOL[cfg], (cfg, k, v)
    z2, xs = m(x)                                                            # forward(): the reference's (z, [x_i]) layout
    assert torch.equal(z2, z) and [tuple(t.shape) for t in xs] == [(2, 3, 12, 20, 16), (2, 3, 6, 10, 16), (2, 3, 3, 5, 16)]


@pytest.mark.parametrize("cfg", ["yolov5n", "yolov5l"])
def test_detections_match_reference(dev, gold, nets, cfg):
    """batched_detect_faces on the fixture's frames: per frame the reference's detections, all of them, in the reference's
    order (the fixture's score and IoU margins exist for this).  The frames have the network's size, so the reference's
    detections in frame pixels are its NMS rows clipped to the frame (gain 1, no padding)."""
    det = nets(cfg)
    conf, iou = (float(v) for v in gold["conf_iou"])
    frames = torch.from_numpy(gold["x"].astype(np.float32)).to(dev) * 255.0   # exact: fp16 values times 255
    dets = det.batched_detect_faces(frames, conf, iou, keep_empty=True)
    assert len(dets) == 2
    tol = NET_TOL[cfg] * float(np.abs(gold[cfg + "_z"]).max())                # the z tolerance, gain 1
    for b, d in enumerate(dets):
        ref = gold[f"{cfg}_nms{b}"][:, :15].copy()
        ref[:, [0, 2]] = ref[:, [0, 2]].clip(0, 160)
        ref[:, [1, 3]] = ref[:, [1, 3]].clip(0, 96)
        ref[:, 5:15:2] = ref[:, 5:15:2].clip(0, 160)
        ref[:, 6:15:2] = ref[:, 6:15:2].clip(0, 96)
        ref = ref[np.trunc(ref[:, 3]) - np.trunc(ref[:, 1]) >= det.min_face]
        assert d.shape == ref.shape and d.dtype == np.float32, (cfg, b, d.shape, ref.shape)
        print(cfg, b, len(d), "max |diff|", np.abs(d - ref).max(), "tol", tol)
        assert np.abs(d - ref).max() <= tol
    assert len(det.batched_detect_faces(frames, conf, iou)) == 2
    bgr = [np.ascontiguousarray((gold["x"][b].astype(np.float32) * 255.0).transpose(1, 2, 0)[:, :, ::-1]) for b in range(2)]
    out = det.detect_faces(bgr, conf, iou)                                    # the reference's entry: BGR arrays, int rows
    boxes = np.concatenate([gold[f"{cfg}_post96x160_boxes{b}"] for b in range(2)])
    assert out.shape == (len(boxes), 15) and np.array_equal(out[:, 4], out[:, 0])
    lms = np.concatenate([gold[f"{cfg}_post96x160_lms{b}"] for b in range(2)])
    assert np.abs(out[:, :4] - boxes).max() <= 1                              # truncation of values within tol of an integer
    assert np.abs(out[:, 5:] - lms).max() <= 1


def test_helper_with_the_n_detector(dev):
    """FaceRestoreHelper(face_det=<loaded YoloDetector>) has the contract test_helper_get_crop_face_with_the_mobile_detector
    checks.  Detector weights: the fixture's respond to their biases far more than to the image (every frame gives the same
    boxes), so this test picks others, for which a constant frame gives no detection and a structured one many: name-seeded,
    every convolution below Detect times 1.5 (the image then reaches the head), Detect.m[i].weight times (0.103, 0.064, 0.046)
    (raw standard deviation about 2), objectness bias - 5, class bias + 6.  On the CPU reference these give 67 and 20
    detections on the two block frames below and none on the constant frame (largest objectness 0.025)."""
    yf = _yf()
    import torch.nn as nn
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial, get_center_face
    src = name_seeded_weights(yf.Model("yolov5n"))
    head = src.model[-1]
    with torch.no_grad():
        for mod in src.modules():
            if isinstance(mod, nn.Conv2d) and all(mod is not d for d in head.m):
                mod.weight.mul_(1.5)
        for mi, f in zip(head.m, (0.103, 0.064, 0.046)):
            mi.weight.mul_(f)
            b = mi.bias.view(3, 16)
            b[:, 4] -= 5.0
            b[:, 15] += 6.0
    det = yf.YoloDetector("yolov5n", device=dev)
    det.load_state_dict(src.state_dict(), strict=True)
    helper = FaceRestoreHelper(face_size=128, det_model="YOLOv5n", device=dev, face_det=det)
    assert helper._detector() is det
    g = torch.Generator().manual_seed(9)
    blocks = (torch.rand(2, 3, 4, 4, generator=g) * 2 - 1).repeat_interleave(32, 2).repeat_interleave(32, 3).half().float()
    x = blocks.to(dev)
    faces, mats, idx = helper.get_crop_face(x, only_center_face=True)
    assert faces is not None and idx == [0, 1]
    assert tuple(faces.shape) == (len(idx), 3, 128, 128) and len(mats) == len(idx)
    assert faces.abs().max().item() <= 1.0 and all(np.asarray(M).shape == (2, 3) for M in mats)
    dets = det.batched_detect_faces(x, 0.5, pre=(127.5, 127.5, 0.0, 255.0))    # the helper's [-1, 1] -> [0, 255] mapping
    assert len(dets) == len(idx) and all(d.shape[1] == 15 and len(d) >= 2 for d in dets)
    for M, d in zip(mats, dets):
        assert np.all(np.diff(d[:, 4]) <= 0) and np.all(np.trunc(d[:, 3]) - np.trunc(d[:, 1]) >= det.min_face)
        _, k = get_center_face([b[0:5] for b in d], 128, 128)
        assert np.allclose(M, estimate_affine_partial(d[k, 5:15].reshape(5, 2), helper.face_template))
    assert torch.equal(faces, helper.get_crop_face_from_affine_matrices(x[idx].contiguous(), mats))
    # several faces per frame, and a frame without one: the constant 114 / 255 frame keeps its slot
    const = torch.full((1, 3, 128, 128), 2 * 114 / 255 - 1, device=dev)
    x3 = torch.cat([x[:1], const, x[1:]])
    per_frame = det.batched_detect_faces(x3, 0.5, pre=(127.5, 127.5, 0.0, 255.0), keep_empty=True)
    assert len(per_frame) == 3 and per_frame[1].shape == (0, 15) and len(per_frame[0]) and len(per_frame[2])
    assert len(det.batched_detect_faces(x3, 0.5, pre=(127.5, 127.5, 0.0, 255.0))) == 2
    crops, mats_all, face_frames = helper.get_crop_faces_all(x3, max_faces=3)
    assert face_frames == sorted(face_frames) and set(face_frames) == {0, 2} and len(mats_all) == len(face_frames)
    assert tuple(crops.shape) == (len(face_frames), 3, 128, 128)


def test_cli_restores_with_the_n_detector(dev, tmp_path):
    """python -m flair_amd restore gaussian FRAMES OUT --det-model YOLOv5n (its main(), in this process) builds from a weights
    directory that holds yolov5n-face.pth -- a name-seeded file written here, no released weights exist offline -- and runs
    the unaligned window loop with it (--faces all: with these weights no frame has a detection, which that mode allows)."""
    import json
    import scipy.io
    from PIL import Image
    yf = _yf()
    from flair_amd import __main__ as cli
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.unet_new import UNetModel
    S, s, N = 64, 16, 3
    kw = dict(num_res_blocks=1, attention_resolutions=[2, 4], channel_mult=[0.5, 1, 4], use_checkpoint=False)
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.manual_seed(0)
    cfg = pl.model_config("gaussian", S)
    cfg.update({k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()})
    m = UNetModel(**cfg)
    wl.randomize_zero_modules(m)
    torch.save(m.state_dict(), wdir / "flair_gaussian.pt")
    torch.save(name_seeded_weights(yf.Model("yolov5n")).state_dict(), wdir / "yolov5n-face.pth")
    torch.save(ParseNet(in_size=512, out_size=512, parsing_ch=19).state_dict(), wdir / "parsing_parsenet.pth")
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(tmp_path / "kernels_12.mat", {"kernels": kernels})
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(2)
    for i in range(N):
        Image.fromarray(rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8), mode="RGB").save(frames / f"{i}.png")
    built = []
    build = pl.build_pipeline

    def spy(*a, **k):
        built.append(build(*a, **k))
        return built[-1]
    grad = torch.is_grad_enabled()
    pl.build_pipeline = spy
    try:
        rc = cli.main(["restore", "gaussian", str(frames), str(tmp_path / "out"), "--det-model", "YOLOv5n", "--faces", "all", "--no-prior",
                       "--size", str(S), "--steps", "2", "--dtype", "fp32", "--no-graph", "--weights", str(wdir), "--kernels",
                       str(tmp_path / "kernels_12.mat"), "--model-kwargs", json.dumps(kw), "--seed", "11", "--device", str(dev)])
    finally:
        pl.build_pipeline = build
        torch.set_grad_enabled(grad)
    assert rc == 0 and sorted(os.listdir(tmp_path / "out")) == [f"{i:04d}.png" for i in range(N)]
    det = built[0].face_helper.face_det
    assert isinstance(det, yf.YoloDetector) and det.detector._loaded and next(det.detector.parameters()).is_cuda
    with pytest.raises(FileNotFoundError, match="yolov5l-face.pth"):
        pl.build_pipeline("gaussian", wdir, device=dev, size=S, steps=2, kernels_path=str(tmp_path / "kernels_12.mat"), prior=False,
                          det_model="YOLOv5l", model_kwargs=kw)
