"""GPU: flair_amd.facescore end to end on a stub detector with fixed detections: the per-face scores of evaluate_dirs and of the
command line are those of the byte metrics applied to the REFERENCE crops (tests/facecrop_ref.py), exactly; the whole-frame
values do not move; mode largest against mode all; the drift keys.

LPIPS and the ArcFace trunk run on flair_conv_nhwc, which picks its K split by launch size (tests/test_gpu_ident.py), so the models
are applied to the reference crops in the SAME batch as the scorer forms: all faces of a batch of frames at once."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import face_ref as F
from tests import facecrop_ref as R

pytestmark = pytest.mark.gpu

H, W, SIDE = 96, 128, 64
_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]])


def _det(cx, cy, size, score):
    lm = (_TPL / 512.0 - 0.5) * size + np.array([cx, cy])
    return np.concatenate([[cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, score], lm.reshape(-1)]).astype(np.float32)


# frame 0: two faces, the smaller one first in the detector's order; frame 1: none; frame 2: one that hangs over the right edge
# (clipped); frame 3: one
DETECTIONS = [[_det(96.0, 40.0, 30.0, 0.99), _det(40.0, 46.0, 50.0, 0.9)], [], [_det(112.0, 60.0, 40.0, 0.8)], [_det(60.0, 50.0, 44.0, 0.95)]]


@functools.lru_cache(maxsize=None)
def frames():
    """(restored, truth) (4, 96, 128, 3) uint8: smooth truth frames with noise, the restored ones a coarser, noisier copy."""
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    truth = np.stack([np.stack([127 + 90 * np.sin(xx / (7.0 + c) + t) * np.cos(yy / (5.0 + t) - c) for c in range(3)], axis=-1) for t in range(4)])
    truth = np.clip(truth + rng.normal(0, 6, truth.shape), 0, 255).astype(np.uint8)
    restored = np.clip(truth.astype(np.float64) * 0.9 + 10 + rng.normal(0, 9, truth.shape), 0, 255).astype(np.uint8)
    for a in (restored, truth):
        a.setflags(write=False)
    return restored, truth


class StubDetector:
    """batched_detect_faces with the fixed detections of the truth frame it is shown, found by the frame's bytes."""

    def __init__(self):
        self.calls = 0

    def batched_detect_faces(self, x, conf_threshold=0.8, nms_threshold=0.4, use_origin_size=True, pre=None, keep_empty=False):
        assert conf_threshold == 0.5 and pre == (127.5, 127.5, 0.0, 255.0) and keep_empty and x.dtype == torch.float32
        self.calls += 1
        u8 = torch.round(x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        truth = frames()[1]
        out = []
        for k in range(u8.shape[0]):
            t, = [t for t in range(len(truth)) if np.array_equal(truth[t], u8[k])]          # detection runs on the TRUTH alone
            out.append(np.stack(DETECTIONS[t]) if DETECTIONS[t] else np.zeros((0, 15), dtype=np.float32))
        return out


def scorer(dev, mode, max_faces=None):
    from flair_amd import facescore as ffs
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    return ffs.FaceScorer(FaceRestoreHelper(face_size=SIDE, device=dev, face_det=StubDetector()), mode, max_faces=max_faces)


@functools.lru_cache(maxsize=None)
def reference(max_faces=None):
    """The faces by the package's own selection rule and the REFERENCE crops of both sets: dict(M, minv, face_frames, a, b)."""
    from flair_amd.guided_diffusion.retinaface_utils import select_faces
    template = _TPL * (SIDE / 512.0)
    M, face_frames = select_faces([np.stack(d) if d else np.zeros((0, 15), dtype=np.float32) for d in DETECTIONS], H, W, template,
                                  eye_dist_threshold=0.1, max_faces=max_faces)
    minv = np.stack([F.invert(m).reshape(6) for m in M])
    restored, truth = frames()
    return dict(M=M, minv=minv, face_frames=face_frames, a=R.crop_batch(restored, minv, face_frames, (SIDE, SIDE)),
                b=R.crop_batch(truth, minv, face_frames, (SIDE, SIDE)))


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    from flair_amd import io as fio
    root = tmp_path_factory.mktemp("facescore")
    restored, truth = frames()
    for name, a in (("restored", restored), ("truth", truth)):
        os.makedirs(root / name)
        for t in range(a.shape[0]):
            fio.write_frame(str(root / name / f"{t:04d}.png"), a[t])
    return str(root / "restored"), str(root / "truth"), root


@functools.lru_cache(maxsize=None)
def lpips_model():
    from flair_amd import lpips as flp
    from tests import lpips_ref as lr
    m = flp.LPIPS("alex")
    m.load_state_dict(flp.lpips_state_dict("alex", *lr.state_dicts("alex")))
    return m.to("cuda:0")


@functools.lru_cache(maxsize=None)
def ident_model():
    from flair_amd import identity as fid
    from tests import ident_ref
    m = fid.ArcFace()
    m.load_state_dict(fid.identity_state_dict(dict(ident_ref.state_dict())))
    return m.to("cuda:0")


def on(dev, x):
    return torch.from_numpy(np.array(x)).to(dev)                   # a copy: the shared arrays are read-only


def test_the_crops_are_the_reference_crops(dev):
    ref = reference()
    assert list(ref["face_frames"]) == [0, 0, 2, 3] and not np.array_equal(ref["a"], ref["b"])
    s = scorer(dev, "all")
    restored, truth = frames()
    M, face_frames = s.detect(on(dev, truth))
    assert list(face_frames) == [0, 0, 2, 3] and all(np.array_equal(a, b) for a, b in zip(M, ref["M"]))
    ca, cb, minv = s.crops(on(dev, restored), on(dev, truth), M, face_frames)
    assert np.array_equal(minv, ref["minv"])
    assert np.array_equal(ca.cpu().numpy(), ref["a"]) and np.array_equal(cb.cpu().numpy(), ref["b"])
    # the larger face of frame 0 comes first although the detector listed it second
    assert abs(ref["M"][0][0, 0] - SIDE / 50.0) < 1e-3 and abs(ref["M"][1][0, 0] - SIDE / 30.0) < 1e-3


def test_per_face_scores_are_the_byte_metrics_of_the_reference_crops(dev, dirs):
    from flair_amd import identity as fid
    from flair_amd import metrics as fm
    rdir, tdir, _ = dirs
    ref = reference()
    lp, ident = lpips_model(), ident_model()
    got = fm.evaluate_dirs(rdir, tdir, dev, lpips=lp, identity=ident, faces=scorer(dev, "all"))
    ra, rb = on(dev, ref["a"]), on(dev, ref["b"])
    want = fm.psnr_ssim(ra, rb)
    want_lp = lp(ra, rb)
    e = ident.embed(ra, rb)
    K = len(ref["M"])
    faces = [f for fr in got["frames"] for f in fr["faces"]]
    assert [len(fr["faces"]) for fr in got["frames"]] == [2, 0, 1, 1] and len(faces) == K == 4
    for k, f in enumerate(faces):
        assert list(f) == ["psnr", "ssim", "lpips", "ids", "clipped", "matrix"]
        assert f["psnr"] == want["psnr"][k] and f["ssim"] == want["ssim"][k], k
        assert f["lpips"] == want_lp[k], k
        assert f["ids"] == fid.cosine(e[k], e[K + k]), k
        assert f["clipped"] == R.corners_outside(ref["minv"][k], (SIDE, SIDE), H, W)
        assert np.array_equal(np.array(f["matrix"]), ref["M"][k])
    assert [f["clipped"] for f in faces] == [False, False, True, False]
    assert 10 < min(want["psnr"]) and max(want["psnr"]) < 40 and len(set(want["psnr"])) == 4          # four different, finite scores
    mean = got["mean"]
    assert mean["face_count"] == 4 and mean["frames_with_faces"] == 3
    assert mean["face_psnr"] == sum(want["psnr"]) / 4 and mean["face_ssim"] == sum(want["ssim"]) / 4 and mean["face_lpips"] == sum(want_lp) / 4
    assert mean["face_ids"] == sum(f["ids"] for f in faces) / 4
    assert "ids" not in mean and "ids" not in got["frames"][0]                      # identity applies to the crops only
    assert not [k for k in mean if "drift" in k]                                    # mode all: no drift

    # the whole-frame values do not move, and without the scorer the result holds what it held
    base = fm.evaluate_dirs(rdir, tdir, dev, lpips=lp)
    assert [list(fr) for fr in base["frames"]] == [["name", "psnr", "ssim", "lpips"]] * 4 and list(base["mean"]) == ["psnr", "ssim", "lpips"]
    for fr, b in zip(got["frames"], base["frames"]):
        assert {k: v for k, v in fr.items() if k != "faces"} == b
    assert {k: v for k, v in mean.items() if not k.startswith(("face_", "frames_with"))} == base["mean"]
    lines = fm.format_report(got)
    assert len(lines) == 4 + 5 + 2 and lines[4] == "  faces 0" and lines[6].endswith("  (clipped)") and " (clipped)" not in lines[1]
    assert re.fullmatch(r"  face 1  psnr \d+\.\d{4}  ssim \d\.\d{4}  lpips \d\.\d{4}  ids -?\d\.\d{4}", lines[2])
    assert re.fullmatch(r"mean of 4 faces in 3 of 4 frames  psnr \d+\.\d{4}  ssim \d\.\d{4}  lpips \d\.\d{4}  ids -?\d\.\d{4}", lines[-1])
    assert fm.format_report(base) == [l for l in lines[:-1] if not l.startswith("  ")]


def test_largest_mode_keeps_one_face_and_reports_the_drift(dev, dirs):
    from flair_amd import facescore as ffs
    from flair_amd import metrics as fm
    rdir, tdir, _ = dirs
    ident = ident_model()
    every = fm.evaluate_dirs(rdir, tdir, dev, faces=scorer(dev, "all"))
    largest = fm.evaluate_dirs(rdir, tdir, dev, identity=ident, faces=scorer(dev, "largest", max_faces=4))
    assert [len(fr["faces"]) for fr in largest["frames"]] == [1, 0, 1, 1]
    for t in (2, 3):                                                                # frames with one face: the same face
        for key in ("psnr", "ssim", "clipped", "matrix"):
            assert largest["frames"][t]["faces"][0][key] == every["frames"][t]["faces"][0][key]
    for key in ("psnr", "ssim", "matrix"):                                          # frame 0: the larger of its two
        assert largest["frames"][0]["faces"][0][key] == every["frames"][0]["faces"][0][key]
    capped = fm.evaluate_dirs(rdir, tdir, dev, faces=scorer(dev, "all", max_faces=1))
    assert [[f["psnr"] for f in fr["faces"]] for fr in capped["frames"]] == [[f["psnr"] for f in fr["faces"]] for fr in largest["frames"]]
    # the drift: frames 2 and 3 are the one pair of consecutive frames that both have a face
    ref = reference(max_faces=1)
    assert list(ref["face_frames"]) == [0, 2, 3]
    e = ident.embed(on(dev, ref["a"]), on(dev, ref["b"]))
    from flair_amd.identity import cosine
    mean = largest["mean"]
    assert mean["face_id_drift"] == 1.0 - cosine(e[2], e[1]) and mean["face_id_drift_truth"] == 1.0 - cosine(e[5], e[4])
    assert [f["ids"] for fr in largest["frames"] for f in fr["faces"]] == [cosine(e[k], e[3 + k]) for k in range(3)]
    assert "face_id_drift" not in every["mean"] and "face_ids" not in every["mean"]
    assert ffs.format_mean(mean, 4).count("id-drift") == 1
    # mode all with the identity model: the score per face, no drift
    both = fm.evaluate_dirs(rdir, tdir, dev, identity=ident, faces=scorer(dev, "all"))
    assert "face_ids" in both["mean"] and not [k for k in both["mean"] if "drift" in k]


def test_evaluate_command_line(dev, dirs, monkeypatch, capsys):
    from flair_amd import facescore as ffs
    from flair_amd.__main__ import main
    rdir, tdir, root = dirs
    weights = root / "weights"
    os.makedirs(weights, exist_ok=True)
    with pytest.raises(SystemExit, match=re.escape(f"evaluate: --score-faces with --det-model retinaface_mobile0.25 needs {weights / 'detection_mobilenet0.25_Final.pth'}")):
        main(["evaluate", rdir, tdir, "--score-faces", "all", "--weights", str(weights), "--det-model", "retinaface_mobile0.25"])
    with pytest.raises(FileNotFoundError, match="detector checkpoint yolov5n-face.pth not found"):
        ffs.build_detector("YOLOv5n", str(weights), dev)
    (weights / "detection_mobilenet0.25_Final.pth").write_bytes(b"")
    built = []

    def factory(det_model, weights_dir, device):
        built.append((det_model, weights_dir))
        return StubDetector()
    monkeypatch.setattr(ffs, "build_detector", factory)
    plain_json, face_json = root / "plain.json", root / "faces.json"
    assert main(["evaluate", rdir, tdir, "--json", str(plain_json)]) == 0
    plain_lines = capsys.readouterr().out.splitlines()
    assert main(["evaluate", rdir, tdir, "--score-faces", "all", "--max-faces", "3", "--face-size", str(SIDE), "--weights", str(weights),
                 "--det-model", "retinaface_mobile0.25", "--json", str(face_json)]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert built == [("retinaface_mobile0.25", str(weights))]
    assert [l for l in lines if not l.startswith("  ")][:-1] == plain_lines and len(plain_lines) == 5
    assert [l.split("  psnr")[0] for l in lines if l.startswith("  ")] == ["  face 0", "  face 1", "  faces 0", "  face 0", "  face 0"]
    assert lines[-1].startswith("mean of 4 faces in 3 of 4 frames  psnr ")
    plain, got = json.load(open(plain_json)), json.load(open(face_json))
    assert list(plain["mean"]) == ["psnr", "ssim"] and all(list(fr) == ["name", "psnr", "ssim"] for fr in plain["frames"])
    assert list(got["mean"]) == ["psnr", "ssim", "face_psnr", "face_ssim", "face_count", "frames_with_faces"]
    assert all(list(fr) == ["name", "psnr", "ssim", "faces"] for fr in got["frames"])
    assert [list(f) for f in got["frames"][0]["faces"]] == [["psnr", "ssim", "clipped", "matrix"]] * 2
    assert {k: v for k, v in got["mean"].items() if k in plain["mean"]} == plain["mean"]
    ref = reference()
    from flair_amd import metrics as fm
    want = fm.psnr_ssim(on(dev, ref["a"]), on(dev, ref["b"]))
    assert [f["psnr"] for fr in got["frames"] for f in fr["faces"]] == want["psnr"]
