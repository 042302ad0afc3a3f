"""Isolated measurement of the face score's crop (flair_amd/facescore.py, csrc/facecrop.hip).

    python tools/bench_facescore.py [--out profiles/facescore_bench.json] [--kernels-only]

Eight faces of 512 x 512 cut from eight 720 x 1280 frames of seeded random bytes, one face per frame, under similarity
transforms of the kind face alignment gives (a face of 250 to 420 pixels, turned by up to 0.3 rad, wholly inside the frame):

  * ``flair_face_crop_u8`` with one frame set and with two, per call and per face;
  * a whole face-score batch -- the f32 copy of the truth frames for the detector, the alignment on the host, the crop of both
    sets, ``metrics.psnr_ssim`` on the crops -- beside the same batch's whole-frame ``metrics.psnr_ssim``, which is what
    evaluate does without ``--score-faces``.  The detector is a stub with fixed detections: no detector weights exist here, a
    random network finds thousands of boxes, and the detection's cost is that of ``restore``'s, not of this feature;
  * a device-to-device copy of 256 MiB in the same process, as the rate a streaming kernel can reach here.

Each kernel figure is taken twice: the median of 50 calls each bracketed by HIP events (which holds the host's enqueue of a
short launch), and one event pair around 50 calls back to back divided by 50 (the kernel's own pace).  Bytes per second are on
the algorithmic bytes: every crop byte written once and, for scale, read once from the source (the 16 taps of a pixel overlap
its neighbours'; at a magnification above 1 fewer source bytes than that are touched).  For the kernel alone run ``rocprofv3
--kernel-trace --stats -- python tools/bench_facescore.py --kernels-only``.  There is no earlier implementation to compare
against: reported, not gated.
"""
import json
import math
import statistics
import sys

import numpy as np
import torch

from flair_amd import facescore as ffs
from flair_amd import metrics as fm
from flair_amd import ops
from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper, invert_affine

K, HS, WS, SIDE = 8, 720, 1280, 512
CALLS = 50


def per_call_us(fn, iters=CALLS):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def back_to_back_us(fn, iters=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alignments(rng):
    """K frame -> crop similarity matrices: a face of `size` pixels centred at (cx, cy), turned by theta, onto the 512 crop."""
    mats = []
    for _ in range(K):
        size, theta = rng.uniform(250.0, 420.0), rng.uniform(-0.3, 0.3)
        cx, cy = rng.uniform(420.0, WS - 420.0), rng.uniform(320.0, HS - 320.0)
        s = SIDE / size
        c, d = s * math.cos(theta), s * math.sin(theta)
        mats.append(np.array([[c, -d, SIDE / 2 - (c * cx - d * cy)], [d, c, SIDE / 2 - (d * cx + c * cy)]]))
    return mats


_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043], [313.08905, 371.15118]])


class FixedDetector:
    """One detection per frame whose landmarks are the template under the inverse of alignments()'s matrix."""

    def __init__(self, mats):
        self.dets = []
        for m in mats:
            inv = invert_affine(m)
            lm = _TPL @ inv[:, :2].T + inv[:, 2]
            x0, y0, x1, y1 = lm[:, 0].min() - 60, lm[:, 1].min() - 90, lm[:, 0].max() + 60, lm[:, 1].max() + 60
            self.dets.append(np.concatenate([[x0, y0, x1, y1, 0.99], lm.reshape(-1)]).astype(np.float32)[None])

    def batched_detect_faces(self, frames, conf_threshold=0.8, nms_threshold=0.4, use_origin_size=True, pre=None, keep_empty=False):
        return list(self.dets[:frames.shape[0]])


def main(argv):
    if not torch.cuda.is_available():
        raise SystemExit("bench_facescore: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = dict(faces=K, frame_height=HS, frame_width=WS, face_size=SIDE, calls=CALLS)

    def log(key, **values):
        result[key] = values
        print(key + ": " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in values.items()), flush=True)

    a = torch.from_numpy(rng.integers(0, 256, (K, HS, WS, 3), dtype=np.uint8)).to(dev)
    b = torch.from_numpy(rng.integers(0, 256, (K, HS, WS, 3), dtype=np.uint8)).to(dev)
    mats = alignments(rng)
    minv_host = np.stack([invert_affine(m).reshape(6) for m in mats])
    assert not any(ffs.corners_outside(m, (SIDE, SIDE), HS, WS) for m in minv_host)
    minv = torch.from_numpy(minv_host).to(dev)
    index_host = list(range(K))
    index = torch.tensor(index_host, dtype=torch.int32).to(dev)
    out_a = torch.empty((K, SIDE, SIDE, 3), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    crop_bytes = float(K * SIDE * SIDE * 3)
    kernels = (("face_crop_one_set", lambda: ops.face_crop_u8(a, minv, minv_host, index, index_host, (SIDE, SIDE), out_a=out_a), 2.0 * crop_bytes),
               ("face_crop_two_sets", lambda: ops.face_crop_u8(a, minv, minv_host, index, index_host, (SIDE, SIDE), b=b, out_a=out_a, out_b=out_b),
                4.0 * crop_bytes))
    for name, fn, nbytes in kernels:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        if "--kernels-only" in argv:
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            continue
        each, b2b = per_call_us(fn), back_to_back_us(fn)
        log(name, us_per_call=each, us_per_call_back_to_back=b2b, us_per_face=b2b / K, megabytes=nbytes / 1e6, terabytes_per_s=nbytes / b2b / 1e6)
    if "--kernels-only" in argv:
        return 0

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(5):
        dst.copy_(src)
    us = back_to_back_us(lambda: dst.copy_(src), 20)
    log("copy_256MiB", us_per_call=us, terabytes_per_s=2.0 * src.numel() / us / 1e6)

    scorer = ffs.FaceScorer(FaceRestoreHelper(face_size=SIDE, device=dev, face_det=FixedDetector(mats)), "all", max_faces=4)
    for _ in range(3):
        fm.psnr_ssim(a, b)
        faces, _ = scorer.score(a, b)
    assert [len(f) for f in faces] == [1] * K
    whole = back_to_back_us(lambda: fm.psnr_ssim(a, b), 10)                      # ends in the copy of the sums to the host
    both = back_to_back_us(lambda: (fm.psnr_ssim(a, b), scorer.score(a, b)), 10)
    log("batch_of_8_frames", us_whole_frame_scores=whole, us_with_face_scores=both, us_added=both - whole, us_added_per_face=(both - whole) / K)
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as fh:
            json.dump(result, fh)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
