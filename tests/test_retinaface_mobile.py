"""RetinaFace with the MobileNet-0.25 body (det_model="retinaface_mobile0.25") and its depthwise-separable kernel.

Pinned end to end by tests/golden/g12_retinaface_mobile.npz (make_golden_mobile.py: the reference's own MobileNetV1 / FPN / SSH /
heads / PriorBox / decode with name-seeded weights): configuration and parameter layout on the CPU, flair_dwconv_nhwc against
torch's grouped convolution and the whole HIP detector against the fixture on the GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.golden.weights import name_seeded_weights

GOLD = os.path.join(os.path.dirname(__file__), "golden", "g12_retinaface_mobile.npz")
VAR = [0.1, 0.2]
# (Cin, Cout, stride) of the 13 conv_dw blocks of MobileNetV1 (retinaface_net.py:100-135)
BLOCKS = [(8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2)] + [(128, 128, 1)] * 5 + \
         [(128, 256, 2), (256, 256, 1)]


def _model(device="cpu", tame=False):
    """Name-seeded weights; tame: box / landmark heads scaled down as in test_retinaface.py, so decoded boxes stay near the frame."""
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    m = RetinaFace(network_name="mobile0.25", device="cpu")
    name_seeded_weights(m)
    if tame:
        with torch.no_grad():
            for n, p_ in m.named_parameters():
                if n.startswith(("BboxHead", "LandmarkHead")):
                    p_.mul_(0.01)
    if device != "cpu":
        m = m.to(device)
        m.device = torch.device(device)
    return m.eval()


# ------------------------------------------------------------------------------------------------------ CPU
def test_generate_config_mobile():
    from flair_amd.guided_diffusion.retinaface import generate_config
    cfg = generate_config("mobile0.25")
    assert cfg["name"] == "mobilenet0.25"
    assert cfg["min_sizes"] == [[16, 32], [64, 128], [256, 512]] and cfg["steps"] == [8, 16, 32]
    assert cfg["variance"] == [0.1, 0.2] and cfg["clip"] is False
    assert cfg["return_layers"] == {"stage1": 1, "stage2": 2, "stage3": 3}
    assert cfg["in_channel"] == 32 and cfg["out_channel"] == 64
    assert generate_config("resnet50")["name"] == "Resnet50"


def test_parameter_layout_matches_reference_and_loads_strict():
    g = np.load(GOLD)
    m = _model()
    sd = m.state_dict()
    names = [str(n) for n in g["param_names"]]
    assert list(sd.keys()) == names
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["param_shapes"]]
    assert not any(".fc." in k or ".avg" in k for k in sd)
    assert sum(p.numel() for p in m.parameters()) == 426_608         # the small detector: ~0.4 M parameters
    # a checkpoint of the reference's layout ("module." already stripped, or not) loads strictly and replaces every value
    g_ = torch.Generator().manual_seed(1)
    ref = {n: (torch.randn(tuple(int(d) for d in str(s).split(";") if d), generator=g_) if "num_batches" not in n
               else torch.tensor(0)) for n, s in zip(names, g["param_shapes"])}
    m.load_state_dict(ref, strict=True)
    assert all(torch.equal(m.state_dict()[k].float(), ref[k].float()) for k in names)
    m.load_state_dict({"module." + k: v for k, v in ref.items()}, strict=True)


def test_unsupported_options_keep_raising():
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    with pytest.raises(NotImplementedError):
        RetinaFace(network_name="mobile0.25", half=True, device="cpu")
    m = _model()
    with pytest.raises(NotImplementedError):
        m.detect_faces(np.zeros((16, 16, 3), np.float32), use_origin_size=False)
    with pytest.raises(NotImplementedError):
        m.batched_detect_faces(torch.zeros(1, 3, 16, 16), use_origin_size=False)


def test_helper_builds_the_mobile_detector():
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface import _MobileNetV1Body
    det = FaceRestoreHelper(face_size=128, det_model="retinaface_mobile0.25", device="cpu")._detector()
    assert det.model_name == "retinaface_mobile0.25" and det.backbone == "mobilenet0.25"
    assert isinstance(det.body, _MobileNetV1Body)


def test_dwconv_argument_errors_without_a_gpu():
    from flair_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(1 << 20)                     # never dereferenced: validation precedes any launch

    def call(C=8, stride=1, x_ld=8, y_ld=16, pw=True, cout=16):
        return lib.flair_dwconv_nhwc(p, x_ld, 1, 4, 4, C, stride, p, p, p if pw else None, p, cout, _lib.ACT_LRELU01, p, y_ld, None)
    assert call(stride=3) == -1 and b"stride 3" in lib.flair_last_error()
    assert call(C=6, x_ld=8) == -1 and b"C = 6" in lib.flair_last_error()
    assert call(x_ld=6) == -1 and b"x_ld" in lib.flair_last_error()
    assert call(y_ld=12) == -1 and b"y_ld" in lib.flair_last_error()            # 1x1 stage writes Cout = 16 channels
    assert call(cout=10) == -1 and b"Cout = 10" in lib.flair_last_error()
    assert call(C=1024, x_ld=1024) == -1 and b"512" in lib.flair_last_error()


# ------------------------------------------------------------------------------------------------------ GPU
def _dw_ref(x, w_dw, b_dw, stride, w_pw=None, b_pw=None):
    """float64 CPU reference: F.conv2d(groups=C) + folded BatchNorm bias + LeakyReLU(0.1) [-> 1x1 -> bias -> LeakyReLU]."""
    import torch.nn.functional as F
    C = x.shape[1]
    d = F.leaky_relu(F.conv2d(x.double(), w_dw.double().t().reshape(C, 1, 3, 3), b_dw.double(), stride, 1, groups=C), 0.1)
    if w_pw is None:
        return d
    return F.leaky_relu(F.conv2d(d, w_pw.double()[:, :, None, None], b_pw.double()), 0.1)


def _close(got, ref, what):
    err = (got.double() - ref).abs().max().item()
    assert err <= 2e-5 * ref.abs().max().item() + 1e-6, f"{what}: max|err| {err:.3e}, max|ref| {ref.abs().max().item():.3e}"


@pytest.mark.gpu
def test_dwconv_depthwise_only(dev):
    from flair_amd import ops
    from tests.util import from_clip, to_clip
    g = torch.Generator().manual_seed(3)
    for C in (8, 16, 32, 64, 128, 256):
        w_dw = torch.randn(9, C, generator=g) / 3
        b_dw = 0.1 * torch.randn(C, generator=g)
        for T, (H, W) in ((1, (7, 10)), (3, (6, 1)), (1, (1, 5)), (3, (9, 8))):
            x = torch.randn(T, C, H, W, generator=g)
            for stride in (1, 2):
                Ho, Wo = -(-H // stride), -(-W // stride)
                ref = _dw_ref(x, w_dw, b_dw, stride)
                buf = torch.full((T, Ho, Wo, C + 8), 7.0, device=dev)                # out view with ld > C
                got = ops.dwconv(to_clip(x, torch.float32, dev), w_dw.to(dev), b_dw.to(dev), stride=stride, out=buf[..., :C])
                _close(from_clip(got), ref, f"C={C} T={T} {H}x{W} s={stride}")
                assert torch.all(buf[..., C:] == 7.0)


@pytest.mark.gpu
def test_dwconv_with_pointwise_every_mobilenet_block(dev):
    from flair_amd import ops
    from tests.util import from_clip, to_clip
    g = torch.Generator().manual_seed(4)
    for i, (cin, cout, stride) in enumerate(sorted(set(BLOCKS))):
        T, H, W = 2, 9 + i % 2, 11 - i % 2
        x = torch.randn(T, cin, H, W, generator=g)
        w_dw, b_dw = torch.randn(9, cin, generator=g) / 3, 0.1 * torch.randn(cin, generator=g)
        w_pw, b_pw = torch.randn(cout, cin, generator=g) / cin ** 0.5, 0.1 * torch.randn(cout, generator=g)
        ref = _dw_ref(x, w_dw, b_dw, stride, w_pw, b_pw)
        xd = to_clip(x, torch.float32, dev)
        got = ops.dwconv(xd, w_dw.to(dev), b_dw.to(dev), stride=stride, pw=(w_pw.to(dev), b_pw.to(dev)))
        _close(from_clip(got), ref, f"{cin}->{cout} s={stride}")
        buf = torch.full((T, -(-H // stride), -(-W // stride), cout + 4), 7.0, device=dev)
        ops.dwconv(xd, w_dw.to(dev), b_dw.to(dev), stride=stride, pw=(w_pw.to(dev), b_pw.to(dev)), out=buf[..., :cout])
        assert torch.equal(buf[..., :cout], got) and torch.all(buf[..., cout:] == 7.0)


@pytest.mark.gpu
def test_hip_mobile_detector_matches_reference_fixture(dev):
    from flair_amd import ops
    from flair_amd.guided_diffusion import retinaface_utils as ru
    from tests.util import parity_log
    g = np.load(GOLD)
    m = _model(dev)
    x = torch.from_numpy(g["x"]).float()
    clip = m._to_clip(x.to(dev))
    feats = m.body.run(clip)
    assert [f.shape[3] for f in feats] == [64, 128, 256]
    for i, f in enumerate(feats):
        ref = torch.from_numpy(g[f"body{i}"])
        err = (f.cpu().permute(0, 3, 1, 2) - ref).abs().max().item() / ref.abs().max().item()
        parity_log(f"g12 mobile body{i}: max|err|/max|ref| = {err:.2e}")
        assert err <= 1.1e-6, (i, err)                   # measured <= 7.0e-7
    bbox, cls, ldm = m._neck_heads(feats)
    got = {"bbox": bbox, "conf": torch.softmax(cls, dim=-1), "ldm": ldm}
    bounds = {"bbox": 1.5e-6, "conf": 8e-7, "ldm": 1.1e-6}          # ~1.5x the measured 1.0e-6 / 5.2e-7 / 7.4e-7
    for key, v in got.items():
        ref = torch.from_numpy(g[key])
        err = (v.cpu() - ref).abs().max().item() / ref.abs().max().item()
        parity_log(f"g12 mobile {key}: max|err|/max|ref| = {err:.2e}")
        assert err <= bounds[key], (key, err)
    # forward() is the same network; PriorBox / decode of frame 0 against the reference's
    fb, fc, fl = m(x.to(dev))
    assert torch.equal(fb, bbox) and torch.equal(fl, ldm)
    pri = ru.PriorBox(m.cfg, image_size=tuple(x.shape[2:])).forward()
    assert np.array_equal(pri, g["priors"])
    boxes = ru.decode(bbox[0].cpu().numpy(), pri, VAR)
    lms = ru.decode_landm(ldm[0].cpu().numpy(), pri, VAR)
    assert np.abs(boxes - g["boxes"]).max() <= 2e-5 * np.abs(g["boxes"]).max()
    assert np.abs(lms - g["landmarks"]).max() <= 2e-5 * np.abs(g["landmarks"]).max()
    assert ops.pad_channels(3, torch.float32) == clip.shape[3]


@pytest.mark.gpu
def test_helper_get_crop_face_with_the_mobile_detector(dev):
    """FaceRestoreHelper(det_model="retinaface_mobile0.25") through its own _detector(): the result has the resnet50 path's
    contract -- crops (n, 3, S, S) in [-1, 1], one 2 x 3 matrix per kept frame, the frames' indices -- and equals the landmark
    alignment of the detector's own detections followed by get_crop_face_from_affine_matrices."""
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial, get_center_face
    helper = FaceRestoreHelper(face_size=128, det_model="retinaface_mobile0.25", device=dev)
    det = helper._detector()
    det.load_state_dict(_model(tame=True).state_dict(), strict=True)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 3, 128, 128, generator=g) * 2 - 1).to(dev)
    faces, mats, idx = helper.get_crop_face(x, only_center_face=True)
    assert helper.face_det is det and faces is not None
    assert tuple(faces.shape) == (len(idx), 3, 128, 128) and len(mats) == len(idx) and idx == sorted(idx)
    assert faces.abs().max().item() <= 1.0 and all(np.asarray(M).shape == (2, 3) for M in mats)
    dets = det.batched_detect_faces(x, 0.5, pre=(127.5, 127.5, 0.0, 255.0))    # the helper's [-1, 1] -> [0, 255] mapping
    assert len(dets) == len(idx) and all(d.shape[1] == 15 for d in dets)
    for M, d in zip(mats, dets):
        _, k = get_center_face([b[0:5] for b in d], 128, 128)
        assert np.allclose(M, estimate_affine_partial(d[k, 5:15].reshape(5, 2), helper.face_template))
    assert torch.equal(faces, helper.get_crop_face_from_affine_matrices(x[idx].contiguous(), mats))
