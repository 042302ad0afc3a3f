"""Isolated measurement of the flow-warping error (flair_amd/temporal.py, csrc/temporal.hip).

    python tools/bench_temporal.py [--out profiles/temporal_bench.json] [--kernels-only]

At 512 x 512 with P = 8 frame pairs per call (9 frames: what an evaluation batch of 8 and the frame kept from the batch before
give), seeded random frames and SPyNet weights (the cost does not depend on the weights' values):

  * SPyNet, both directions (``SPyNet.pair_flows``), per pair;
  * ``flair_flow_occlusion`` and ``flair_warp_error`` (one set and two), per pair, on smooth flows of a few pixels with a
    consistent backward flow, so that most pixels are gathered as on real footage;
  * a device-to-device copy of 256 MiB in the same process, as the rate a streaming kernel can reach here.

Each figure is taken twice: the median of 50 calls each bracketed by HIP events (which holds the host's enqueue of a short
launch), and one event pair around 50 calls back to back divided by 50 (the kernels' own pace).  Bytes per second are on the
algorithmic bytes: occlusion reads f and g once and writes the mask, 17 bytes per pixel; the error reads f, the mask and both
frames of every set once, 9 + 6 sets bytes per pixel.  For the kernels alone run ``rocprofv3 --kernel-trace --stats -- python
tools/bench_temporal.py --kernels-only``.  There is no earlier implementation to compare against: reported, not gated.
"""
import json
import statistics
import sys

import numpy as np
import torch

from flair_amd import ops
from flair_amd import temporal as ftm
from flair_amd.guided_diffusion.unet_new import SPyNet

P, H, W = 8, 512, 512
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


def smooth_flows(rng):
    """f: a few pixels, smooth; g: -f read where f points to, roughly (-f itself + a little noise)."""
    coarse = torch.from_numpy(rng.uniform(-4.0, 4.0, (P, 2, 9, 9)).astype(np.float32))
    f = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True).permute(0, 2, 3, 1).contiguous()
    g = -f + torch.from_numpy(rng.normal(0.0, 0.05, (P, H, W, 2)).astype(np.float32))
    return f, g


def main(argv):
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    result = dict(pairs=P, height=H, width=W, calls=CALLS)

    def log(key, **values):
        result[key] = values
        print(key + ": " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in values.items()), flush=True)

    frames = torch.from_numpy(rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8)).to(dev)
    frames2 = torch.from_numpy(rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8)).to(dev)
    f, g = (t.to(dev) for t in smooth_flows(rng))
    mask = ops.flow_occlusion(f, g)
    out1 = torch.empty((1, P, 2), dtype=torch.float64, device=dev)
    out2 = torch.empty((2, P, 2), dtype=torch.float64, device=dev)
    kept = float(mask.float().mean())
    pixels = float(P * H * W)
    kernels = (("flow_occlusion", lambda: ops.flow_occlusion(f, g, out=mask), 17.0 * pixels),
               ("warp_error_one_set", lambda: ops.warp_error(frames, f, mask, out=out1), 15.0 * pixels),
               ("warp_error_two_sets", lambda: ops.warp_error(frames, f, mask, a2=frames2, out=out2), 21.0 * pixels))
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
        log(name, us_per_call=each, us_per_call_back_to_back=b2b, us_per_pair=b2b / P, megabytes=nbytes / 1e6,
            terabytes_per_s=nbytes / b2b / 1e6, kept_share=kept)
    if "--kernels-only" in argv:
        return 0

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(5):
        dst.copy_(src)
    us = back_to_back_us(lambda: dst.copy_(src), 20)
    log("copy_256MiB", us_per_call=us, terabytes_per_s=2.0 * src.numel() / us / 1e6)

    torch.manual_seed(0)
    net = SPyNet()
    for p in net.parameters():
        torch.nn.init.normal_(p, std=0.02)
    net = net.requires_grad_(False).eval().to(dev)
    net.pack(torch.float32, dev)
    model = ftm.WarpError(net)
    for _ in range(3):
        model.flows(frames)
    torch.cuda.synchronize()
    each, b2b = per_call_us(lambda: model.flows(frames), 10), back_to_back_us(lambda: model.flows(frames), 10)
    log("spynet_both_directions", us_per_call=each, us_per_call_back_to_back=b2b, us_per_pair=b2b / P)
    for _ in range(2):
        model.pairs(frames, frames2)
    us = back_to_back_us(lambda: model.pairs(frames, frames2), 10)           # ends in the copy of (S, N) to the host
    log("pairs_two_sets_end_to_end", us_per_call=us, us_per_pair=us / P)
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as fh:
            json.dump(result, fh)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
