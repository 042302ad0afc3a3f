"""Detection forward of one 10-frame 512^2 window for the four detectors in one process, and the five entries of
csrc/detect.hip at the shapes YOLOv5l / YOLOv5n give them there.

Forward = what batched_detect_faces runs before its device-to-host copy and host decoding / NMS: for YOLOv5-face the
letterbox launch + network + the three decode launches, for RetinaFace the clip upload + mean subtraction + network.
Timed with device events on the launch stream: 2 warm-up iterations, then the median of 5.

    python tools/bench_yolov5face.py
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flair_amd import ops  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, iters=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def forwards(T, S, iters):
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    from flair_amd.guided_diffusion.yolov5face import YoloDetector, letterbox_geometry
    frames = torch.rand(T, 3, S, S, device=dev) * 2 - 1
    pre = (127.5, 127.5, 0.0, 255.0)
    (nw, nh), (top, bottom, left, right) = letterbox_geometry(S, S)

    def yolo(det):
        def run():
            x = ops.letterbox(frames, (nh, nw), (top, left), (nh + top + bottom, nw + left + right), pre=pre, scale=1 / 255)
            det.detector.run_clip(x)
        return run

    def retina(net):
        sub = torch.tensor(net.mean, dtype=torch.float32, device=dev)
        one = torch.ones(3, dtype=torch.float32, device=dev)

        def run():
            x = net._to_clip(frames)
            ops.affine_channels(x, 3, *pre, sub, one, x)
            net._run_clip(x)
        return run
    with torch.no_grad():
        for name, fn in (("YOLOv5n", yolo(YoloDetector("yolov5n", device=dev, allow_random_init=True))),
                         ("YOLOv5l", yolo(YoloDetector("yolov5l", device=dev, allow_random_init=True))),
                         ("retinaface_mobile0.25", retina(RetinaFace("mobile0.25", device=dev))),
                         ("retinaface_resnet50", retina(RetinaFace("resnet50", device=dev)))):
            med, best = timed(fn, iters)
            print(json.dumps({"detect_forward": name, "T": T, "size": S, "median_ms": round(med, 3), "min_ms": round(best, 3), "iters": iters}),
                  flush=True)


def entries(T, S, iters):
    """The five new entries at the largest shape each sees in a T-frame S^2 window (YOLOv5l's unless noted)."""
    f32 = dict(dtype=torch.float32, device=dev)
    frames = torch.rand(T, 3, S, S, device=dev) * 2 - 1
    s2, s4, s8, s32 = S // 2, S // 4, S // 8, S // 32
    stem = torch.randn(T, s2, s2, 64, **f32)
    cat = torch.empty(T, s4, s4, 128, **f32)
    spp = torch.randn(T, s32, s32, 2048, **f32)
    half = torch.randn(T, s8, s8, 128, **f32)                    # YOLOv5n: the first stride-1 ShuffleV2 unit (2 x 64 channels)
    branch = torch.randn(T, s8, s8, 64, **f32)
    mixed = torch.empty(T, s8, s8, 128, **f32)
    head = torch.randn(T, s8, s8, 48, **f32)
    z = torch.empty(T, 3 * (s8 * s8 + (s8 // 2) ** 2 + (s8 // 4) ** 2), 16, **f32)
    clip = torch.empty(T, S, S, 16, **f32)
    for name, fn in (("flair_letterbox_nhwc", lambda: ops.letterbox(frames, (S, S), (0, 0), (S, S), pre=(127.5, 127.5, 0.0, 255.0), scale=1 / 255, out=clip)),
                     ("flair_maxpool2x2s2_nhwc", lambda: ops.maxpool2x2s2(stem, out=cat[..., 64:])),
                     ("flair_spp_maxpool_nhwc", lambda: ops.spp_maxpool(spp, 512, (3, 5, 7))),
                     ("flair_channel_interleave_nhwc", lambda: ops.channel_interleave(half[..., :64], branch, out=mixed)),
                     ("flair_yolo_face_decode", lambda: ops.yolo_face_decode(head, 3, 8.0, [(4, 5), (8, 10), (13, 16)], z, 0))):
        med, best = timed(fn, iters)
        print(json.dumps({"entry": name, "T": T, "size": S, "median_us": round(med * 1e3, 1), "min_us": round(best * 1e3, 1), "iters": iters}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    forwards(a.frames, a.size, a.iters)
    entries(a.frames, a.size, a.iters)


if __name__ == "__main__":
    main()
