"""Isolated measurement of flair_block_luma_sums (csrc/scenes.hip): one call = the zeroing of the output and one launch.

    python tools/bench_scenes.py [--json out.json] [--calls 50] [--repeats 5]

Sizes: 25 x 512 x 512 (the reference's 25-frame demo clips) and 10 x 768 x 1280 (one window of a rectangular video), as in
tools/bench_metrics.py.  Each size is warmed, then ``--calls`` back-to-back calls are bracketed by HIP events on the launch
stream, ``--repeats`` times; the median is reported with the spread.  Bytes are the algorithmic ones, N H W 3 read once (the
N x 64 result is noise beside them); the share is of the 8 TB/s data-sheet HBM rate.  There is no earlier implementation to
compare against, and the pre-pass that calls this kernel is bound by PNG decoding on the host, not by it.  Prints one JSON line.
"""
import json
import sys

import torch

from flair_amd import ops

HBM_BYTES_PER_S = 8.0e12
SIZES = [(25, 512, 512), (10, 768, 1280)]


def time_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main(argv):
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 50
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 5
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rows = []
    for N, H, W in SIZES:
        g = torch.Generator(device=dev).manual_seed(N + H + W)
        a = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        out = torch.empty((N, 64), dtype=torch.int64, device=dev)
        fn = lambda: ops.block_luma_sums(a, out=out)                                             # noqa: E731
        for _ in range(calls):                                                                  # warm-up
            fn()
        torch.cuda.synchronize()
        us = sorted(time_us(fn, calls) for _ in range(repeats))
        med = us[len(us) // 2]
        nbytes = 1.0 * N * H * W * 3
        rows.append(dict(shape=[N, H, W], us_per_call=round(med, 2), us_min=round(us[0], 2), us_max=round(us[-1], 2),
                         algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / (med * 1e-6), 1),
                         share_of_8TBps_hbm=round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4),
                         mpixels_per_s=round(N * H * W / med, 1)))
    line = json.dumps(dict(bench="block_luma_sums", calls=calls, repeats=repeats, device=torch.cuda.get_device_name(0), sizes=rows))
    print(line)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
