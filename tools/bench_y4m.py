"""Measurements of the .y4m path (csrc/yuv.hip, flair_amd/y4m.py, flair_amd/io.py).

    python tools/bench_y4m.py kernels [--json out.json] [--calls 50] [--repeats 5]
    python tools/bench_y4m.py commands [--json out.json] [--frames 64] [--size 512] [--repeats 5] [--dir DIR]

``kernels``: flair_yuv_to_rgb_u8 and flair_rgb_to_yuv_u8 on 8 frames of 1080 x 1920 in 420jpeg (and 444), bt709 limited; each is
warmed, then ``--calls`` back-to-back calls are bracketed by HIP events, ``--repeats`` times; the median is reported.  Bytes are
the algorithmic ones, payload + RGB, each moved once; a device-to-device copy of the same number of bytes is timed in the same
process for comparison.  Run it under ``rocprofv3 --kernel-trace --stats`` for the kernels' own times.

``commands``: the wall time of ``scenes.detect_cuts_files`` and ``interpolate.interpolate_video_files`` (factor 2, SuperSloMo with
seeded random weights: the cost, not the pictures, is what is measured) over the same ``--frames`` frames of ``--size`` squared,
once from and to a PNG directory and once from and to a .y4m stream: one warm-up of each, then ``--repeats`` runs in alternating
order, medians.  The frames are smooth seeded gradients with noise (PNG compresses them somewhat, as it does footage).
Prints one JSON line.
"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

from flair_amd import interpolate as fi
from flair_amd import io as fio
from flair_amd import ops, scenes, y4m


def opt(argv, name, default):
    return type(default)(argv[argv.index(name) + 1]) if name in argv else default


def time_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def median_us(fn, calls, repeats):
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    us = sorted(time_us(fn, calls) for _ in range(repeats))
    return us[len(us) // 2], us[0], us[-1]


def kernels(argv):
    calls, repeats = opt(argv, "--calls", 50), opt(argv, "--repeats", 5)
    dev = torch.device("cuda:0")
    N, H, W = 8, 1080, 1920
    rows = []
    g = torch.Generator(device=dev).manual_seed(1)
    for fmt in ("420jpeg", "444"):
        P = y4m.payload_bytes(fmt, H, W)
        payload = torch.randint(0, 256, (N, P), generator=g, device=dev, dtype=torch.uint8)
        rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        back = torch.empty((N, P), dtype=torch.uint8, device=dev)
        nbytes = N * (P + H * W * 3)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        for name, fn in (("yuv_to_rgb_u8", lambda: ops.yuv_to_rgb_u8(payload, (H, W), fmt, "bt709", "limited", out=rgb)),
                         ("yuv_to_rgb_u8 planar", lambda: ops.yuv_to_rgb_u8(payload, (H, W), fmt, "bt709", "limited", planar=True, out=rgb.view(N, 3, H, W))),
                         ("rgb_to_yuv_u8", lambda: ops.rgb_to_yuv_u8(rgb, fmt, "bt709", "limited", out=back)),
                         ("copy of as many bytes", lambda: dst.copy_(src))):
            med, lo, hi = median_us(fn, calls, repeats)
            rows.append(dict(kernel=name, format=fmt, shape=[N, H, W], us_per_call=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2),
                             algorithmic_bytes=nbytes, tbytes_per_s=round(nbytes / (med * 1e-6) / 1e12, 3)))
    return dict(bench="y4m kernels", calls=calls, repeats=repeats, device=torch.cuda.get_device_name(0), rows=rows)


def make_clip(root, n, size):
    """The same frames as a PNG directory and as a 420jpeg stream (made by the encode kernel, then decoded for the PNGs, so
    both hold the same pictures) -> (directory, stream path)."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    frames = []
    for i in range(n):
        base = np.stack([yy * 255, xx * 255, np.full_like(xx, 255.0 * i / n)], -1) * (0.4 if i >= n // 2 else 1.0)      # one cut in the middle
        frames.append(np.clip(base + rng.normal(0, 4, base.shape), 0, 255).astype(np.uint8))
    rgb = torch.from_numpy(np.stack(frames)).cuda()
    stream = os.path.join(root, "clip.y4m")
    w = fio._Writer(stream)
    w.submit_bytes(0, rgb)
    w.close()
    d = os.path.join(root, "clip")
    w = fio._Writer(d)
    for first, (u8,) in fio.iter_frame_batches([fio.list_frames(stream)], [(i, min(8, n - i)) for i in range(0, n, 8)], "cuda"):
        w.submit_bytes(first, u8)
    w.close()
    return d, stream


def commands(argv):
    n, size, repeats = opt(argv, "--frames", 64), opt(argv, "--size", 512), opt(argv, "--repeats", 5)
    root = tempfile.mkdtemp(prefix="bench_y4m_", dir=opt(argv, "--dir", tempfile.gettempdir()))
    try:
        from flair_amd.guided_diffusion.superslomo import SuperSloMo
        torch.manual_seed(0)
        net = SuperSloMo().eval().cuda()
        d, stream = make_clip(root, n, size)

        def run_scenes(src):
            return scenes.detect_cuts_files(fio.list_frames(src), "cuda")["cuts"]

        def run_interpolate(src, dst):
            if os.path.isdir(dst):
                shutil.rmtree(dst)
            elif os.path.exists(dst):
                os.remove(dst)
            return fi.interpolate_video_files(src, dst, 2, net=net, device="cuda")

        jobs = {"scenes png": lambda: run_scenes(d), "scenes y4m": lambda: run_scenes(stream),
                "interpolate png": lambda: run_interpolate(d, os.path.join(root, "out")),
                "interpolate y4m": lambda: run_interpolate(stream, os.path.join(root, "out.y4m"))}
        times = {k: [] for k in jobs}
        for rep in range(repeats + 1):                           # run 0 is the warm-up
            order = list(jobs) if rep % 2 == 0 else list(jobs)[::-1]
            for k in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jobs[k]()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        assert run_scenes(d) == run_scenes(stream)
        rows = {k: dict(median_s=round(sorted(v)[len(v) // 2], 4), min_s=round(min(v), 4), max_s=round(max(v), 4)) for k, v in times.items()}
        sizes = dict(png_bytes=sum(os.path.getsize(p) for p in fio.list_frames(d)), y4m_bytes=os.path.getsize(stream))
        return dict(bench="y4m commands", frames=n, size=size, repeats=repeats, device=torch.cuda.get_device_name(0), **sizes, rows=rows)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main(argv):
    if not argv or argv[0] not in ("kernels", "commands"):
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("bench_y4m: needs the GPU (nothing is measured without one)")
    torch.set_grad_enabled(False)
    y4m.set_defaults("bt601", "limited")
    line = json.dumps((kernels if argv[0] == "kernels" else commands)(argv[1:]))
    print(line)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
