"""Generate tests/golden/g16_yolov5face.npz: the YOLOv5-face detectors (YOLOv5n, YOLOv5l), end to end, from the reference's
own modules.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_yolov5face.py

The reference's ``models/yolo.py::Model`` (with ``models/common.py``, ``models/experimental.py``, ``utils/autoanchor.py``,
``utils/torch_utils.py``), ``utils/general.py`` and ``face_detector.py::YoloDetector._postprocess`` run unmodified.  What is
absent here is stubbed:
  * the packages ``guided_diffusion.facelib.detection.yolov5face[.models|.utils]`` are given as path packages, so that their
    ``__init__`` files (which import cv2-bound code and download weights) do not run;
  * ``cv2`` is refimport's stub: nothing in the network or in ``_postprocess`` calls it; ``torch.__version__`` reads
    "2.0.0" while ``face_detector.py`` is imported (its version pattern does not match a local build suffix);
  * ``torchvision.ops.nms`` is the plain greedy restatement ``_nms`` below (decreasing score order, areas without ``+ 1``,
    suppression at IoU > threshold).  PARITY UNPINNED: torchvision is not importable here, as g11 declares for its NMS.

Weights are name-seeded (tests/golden/weights.py) in eval mode.  With them the head's raw outputs have a standard deviation
of about 0.08, every score is about 0.25 and nothing passes a threshold, so the three ``Detect.m[i].weight`` tensors are
multiplied by a recorded factor (``<cfg>_factors``, about 20) that scales the raw standard deviation of each level towards
the first entry of TARGET_STDS for which the margins below hold; the test applies the same factors.  The generator asserts the margins the detection test relies on before it saves.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import save  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402

H, W = 96, 160                  # levels 12 x 20, 6 x 10, 3 x 5: odd sizes, SPP windows larger than the frame; z is (2, 945, 16)
SEED = 16
TARGET_STDS = (1.75, 1.7, 1.8, 1.65, 1.85, 1.6, 1.9)      # raw standard deviation aimed at per level, tried in this order
CONF, IOU = 0.5, 0.5
ORIG_SHAPES = ((96, 160), (88, 150))       # no resize | gain 16 / 15 and one row of padding at the top and the bottom
STEM_CHANNELS, DET_CHANNELS = 8, 16        # channels kept of the stem output / of every Detect input (evenly spaced)


def _nms(boxes, scores, iou_threshold):
    order = torch.argsort(scores, descending=True, stable=True)
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead = torch.zeros(len(scores), dtype=torch.bool)
    keep = []
    for n, i in enumerate(order.tolist()):
        if dead[i]:
            continue
        keep.append(i)
        for j in order[n + 1:].tolist():
            iw = (torch.min(boxes[i, 2], boxes[j, 2]) - torch.max(boxes[i, 0], boxes[j, 0])).clamp(min=0)
            ih = (torch.min(boxes[i, 3], boxes[j, 3]) - torch.max(boxes[i, 1], boxes[j, 1])).clamp(min=0)
            inter = iw * ih
            if inter / (areas[i] + areas[j] - inter) > iou_threshold:
                dead[j] = True
    return torch.tensor(keep, dtype=torch.long)


def _install():
    import refimport
    refimport.install_stubs()
    root = os.path.join(refimport.REFERENCE_ROOT, "guided_diffusion", "facelib")
    for name, rel in (("guided_diffusion.facelib", ()), ("guided_diffusion.facelib.detection", ("detection",)),
                      ("guided_diffusion.facelib.detection.yolov5face", ("detection", "yolov5face")),
                      ("guided_diffusion.facelib.detection.yolov5face.models", ("detection", "yolov5face", "models")),
                      ("guided_diffusion.facelib.detection.yolov5face.utils", ("detection", "yolov5face", "utils"))):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__path__ = [os.path.join(root, *rel)]
        sys.modules[name] = m
    sys.modules["torchvision.ops"].nms = _nms
    sys.modules["cv2"].COLOR_BGR2RGB = 4
    return os.path.join(root, "detection", "yolov5face", "models")


def yolo_input():
    """Two frames in [0, 1], fp16-exact so that the fixture stores them as halves."""
    g = torch.Generator().manual_seed(SEED)
    return torch.rand(2, 3, H, W, generator=g).half().float()


def _pairwise_iou_margin(boxes):
    from guided_diffusion.facelib.detection.yolov5face.utils.general import box_iou
    if len(boxes) < 2:
        return 1.0
    iou = box_iou(boxes, boxes)
    iu = torch.triu_indices(len(boxes), len(boxes), 1)
    return float((iou[iu[0], iu[1]] - IOU).abs().min())


def one_config(cfg, models_dir, out):
    version, torch.__version__ = torch.__version__, "2.0.0"        # face_detector.py:18-26 parses it with a pattern a local
    try:                                                            # build suffix does not match
        from guided_diffusion.facelib.detection.yolov5face import face_detector as fd
    finally:
        torch.__version__ = version
    from guided_diffusion.facelib.detection.yolov5face.models.yolo import Model
    from guided_diffusion.facelib.detection.yolov5face.utils import general as G

    m = Model(cfg=os.path.join(models_dir, cfg + ".yaml"))
    name_seeded_weights(m)
    m.eval()
    x = yolo_input()
    det = m.model[-1]
    taps = {}
    m.model[0].register_forward_hook(lambda mod, inp, res: taps.__setitem__("stem", res))
    det.register_forward_pre_hook(lambda mod, inp: taps.__setitem__("det_in", list(inp[0])))
    _, raw0 = m(x)
    base = [mi.weight.data.clone() for mi in det.m]
    for target in TARGET_STDS:                       # the first target whose detections have the margins asserted below
        factors = [round(target / float(r.std()), 2) for r in raw0]
        for mi, w0, f in zip(det.m, base, factors):
            mi.weight.data = w0 * f
        z, raw = m(x)
        assert tuple(z.shape) == (2, 945, 16)
        obj = z[..., 4]
        score = obj * z[..., 15]
        margin_s = float(torch.min((obj - CONF).abs().min(), (score - CONF).abs().min()))
        nms_out = G.non_max_suppression_face(z.clone(), CONF, IOU)
        margin_i = 1.0
        for b in range(z.shape[0]):
            cand = z[b][(obj[b] > CONF) & (score[b] > CONF)]
            margin_i = min(margin_i, _pairwise_iou_margin(G.xywh2xyxy(cand[:, :4])))
        kept = [len(o) for o in nms_out]
        print(cfg, "target", target, "factors", factors, "raw std", [round(float(r.std()), 3) for r in raw], "kept", kept,
              "score margin %.4f IoU margin %.4f" % (margin_s, margin_i))
        if margin_s > 1e-3 and margin_i > 1e-3 and all(2 <= k <= 200 for k in kept):
            break
    # the margins the detection test relies on
    assert margin_s > 1e-3, (cfg, "score margin", margin_s)
    assert margin_i > 1e-3, (cfg, "IoU margin", margin_i)
    assert all(2 <= k <= 200 for k in kept), (cfg, "kept", kept)

    sd = m.state_dict()
    out[cfg + "_param_names"] = np.array(list(sd.keys()))
    out[cfg + "_param_shapes"] = np.array([";".join(map(str, v.shape)) for v in sd.values()])
    out[cfg + "_n_params"] = np.array(sum(p.numel() for p in m.parameters()))
    out[cfg + "_factors"] = np.array(factors, dtype=np.float64)
    out[cfg + "_stride"] = m.stride.numpy()
    out[cfg + "_anchors"] = det.anchors.numpy()
    stem = taps["stem"]
    sidx = np.linspace(0, stem.shape[1] - 1, STEM_CHANNELS).round().astype(np.int64)
    out[cfg + "_stem_idx"], out[cfg + "_stem"] = sidx, stem[:, sidx].numpy()
    for i, t in enumerate(taps["det_in"]):
        didx = np.linspace(0, t.shape[1] - 1, DET_CHANNELS).round().astype(np.int64)
        out[f"{cfg}_det{i}_idx"], out[f"{cfg}_det{i}"] = didx, t[:, didx].numpy()
    for i, r in enumerate(raw):                      # (bs, na, ny, nx, no)
        out[f"{cfg}_raw{i}"] = r.numpy()
    out[cfg + "_z"] = z.numpy()
    for b, o in enumerate(nms_out):
        out[f"{cfg}_nms{b}"] = o.numpy()
    helper = types.SimpleNamespace(min_face=10)
    for (h0, w0) in ORIG_SHAPES:
        origs = [np.zeros((h0, w0, 3), dtype=np.uint8)] * 2
        boxes, lms = fd.YoloDetector._postprocess(helper, x, origs, z.clone(), CONF, IOU)
        for b in range(2):
            out[f"{cfg}_post{h0}x{w0}_boxes{b}"] = np.array(boxes[b], dtype=np.int64).reshape(-1, 4)
            out[f"{cfg}_post{h0}x{w0}_lms{b}"] = np.array(lms[b], dtype=np.int64).reshape(-1, 10)


def main():
    models_dir = _install()
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    out = {"x": yolo_input().half(), "conf_iou": np.array([CONF, IOU])}
    for cfg in ("yolov5n", "yolov5l"):
        one_config(cfg, models_dir, out)
    save("g16_yolov5face", **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "g16_yolov5face.npz")))


if __name__ == "__main__":
    main()
