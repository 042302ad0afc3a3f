"""The RetinaFace MobileNet-0.25 body on a 10-frame 512^2 window.

--blocks: every conv_dw block of MobileNetV1 at the shape it sees for a 512^2 input, timed as one fused flair_dwconv_nhwc launch
          and as the depthwise-only launch followed by the existing 1x1 flair_conv_nhwc (event-timed, median of 20 launches
          after warm-up; same results checked).
--detect: the detector forward of both bodies in the same process (clip upload + mean subtraction + network: what
          batched_detect_faces runs before its host decoding / NMS), synchronised wall time per window.

    python tools/bench_dwconv.py --blocks --detect
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flair_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
# (Cin, Cout, stride, input side) of the 13 conv_dw blocks for a 512^2 frame (the stem conv_bn halves it to 256^2)
BLOCKS = [(8, 16, 1, 256), (16, 32, 2, 256), (32, 32, 1, 128), (32, 64, 2, 128), (64, 64, 1, 64), (64, 128, 2, 64)] + \
         [(128, 128, 1, 32)] * 5 + [(128, 256, 2, 32), (256, 256, 1, 16)]


def med_us(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


def blocks(T):
    g = torch.Generator().manual_seed(0)
    tot_f = tot_u = 0.0
    for cin, cout, s, S in BLOCKS:
        cp, op = ops.pad_channels(cin, torch.float32), ops.pad_channels(cout, torch.float32)
        x = torch.randn(T, S, S, cp, generator=g).to(dev)
        w_dw, b_dw = (torch.randn(9, cp, generator=g) / 3).to(dev), (0.1 * torch.randn(cp, generator=g)).to(dev)
        w_pw, b_pw = (torch.randn(op, cp, generator=g) / cp ** 0.5).to(dev), (0.1 * torch.randn(op, generator=g)).to(dev)
        wp = ops.pack_conv_weight(w_pw.view(op, cp, 1, 1), [(cp, cp)], torch.float32, op)
        So = (S + s - 1) // s
        y_f = torch.empty(T, So, So, op, device=dev)
        y_u = torch.empty_like(y_f)
        d = torch.empty(T, So, So, cp, device=dev)

        def fused():
            ops.dwconv(x, w_dw, b_dw, stride=s, pw=(w_pw, b_pw), out=y_f)

        def unfused():
            ops.dwconv(x, w_dw, b_dw, stride=s, out=d)
            ops.conv(d, wp, b_pw, op, (1, 1, 1), act=ops.ACT_LRELU01, out=y_u)
        tf, tu = med_us(fused), med_us(unfused)
        torch.cuda.synchronize()
        err = (y_f - y_u).abs().max().item() / max(y_u.abs().max().item(), 1e-30)
        tot_f += tf
        tot_u += tu
        print(json.dumps({"block": f"{cin}->{cout} s{s} {S}^2", "T": T, "fused_us": round(tf, 1), "dw_plus_conv1x1_us": round(tu, 1),
                          "rel_diff": float(f"{err:.1e}")}), flush=True)
    print(json.dumps({"all_13_blocks": True, "T": T, "fused_us": round(tot_f, 1), "dw_plus_conv1x1_us": round(tot_u, 1)}), flush=True)


def detect(T, S, iters):
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    torch.manual_seed(0)
    frames = (torch.rand(T, 3, S, S) * 255.0).to(dev)
    mean = torch.tensor([104.0, 117.0, 123.0], device=dev)
    ones = torch.ones(3, device=dev)
    models = {n: RetinaFace(network_name=n, device=dev) for n in ("mobile0.25", "resnet50")}

    def fwd(m):
        x = m._to_clip(frames)
        ops.affine_channels(x, 3, 1.0, 0.0, float("-inf"), float("inf"), mean, ones, x)
        return m._run_clip(x)
    for m in models.values():
        for _ in range(3):
            fwd(m)
    torch.cuda.synchronize()
    res = {n: [] for n in models}
    for _ in range(iters):                     # alternate the two bodies
        for n, m in models.items():
            t0 = time.perf_counter()
            fwd(m)
            torch.cuda.synchronize()
            res[n].append((time.perf_counter() - t0) * 1e3)
    for n, ts in res.items():
        ts.sort()
        print(json.dumps({"detect_forward": n, "T": T, "size": S, "median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3),
                          "iters": iters}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--detect", action="store_true")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.blocks:
        blocks(a.frames)
    if a.detect:
        detect(a.frames, a.size, a.iters)
