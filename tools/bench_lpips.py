"""Isolated measurement of LPIPS (flair_amd/lpips.py, csrc/lpips.hip): milliseconds per frame pair, and the tap kernel alone.

    python tools/bench_lpips.py [--json profiles/lpips_bench.json] [--calls 5] [--repeats 3]

Sizes: 512 x 512 (the reference's demo clips) and 768 x 1280 (a rectangular video), one pair per call (N = 1: the trunk sees
two frames), for both trunks, with freshly initialised weights (the cost does not depend on their values).  Each case is
warmed, then ``--calls`` back-to-back forwards are bracketed by HIP events on the launch stream, ``--repeats`` times; the
median is reported with the spread.  A forward ends with the copy of the result to the host, as evaluate's does.  The tap
kernel is timed alone on the five tap shapes of VGG-16 at 512 x 512 (two launches per call: the tap and the fixed-order sum),
with as many frames per call as make it read 512 MiB, twice the Infinity Cache, so that the rate is HBM's; its bytes are the
algorithmic ones, both feature tensors read once, to be read beside the 5.5-5.7 TB/s a copy reaches on this part (DESIGN.md
section 3).  There is no earlier implementation to compare against: the numbers are reported, not gated.
Prints one JSON line.
"""
import json
import sys

import torch

from flair_amd import lpips as flp
from flair_amd import ops

SIZES = [(512, 512), (768, 1280)]


def time_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def median_of(fn, calls, repeats):
    for _ in range(2):                                                                         # warm-up
        fn()
    torch.cuda.synchronize()
    ms = sorted(time_ms(fn, calls) for _ in range(repeats))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main(argv):
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 5
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    for net in ("vgg", "alex"):
        model = flp.LPIPS(net, dev)
        for H, W in SIZES:
            g = torch.Generator(device=dev).manual_seed(H + W)
            a = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
            b = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
            med, lo, hi = median_of(lambda: model(a, b), calls, repeats)
            rows.append(dict(net=net, shape=[H, W], ms_per_pair=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3)))
    taps = []
    for C, side in ((64, 512), (128, 256), (256, 128), (512, 64), (512, 32)):
        F_ = -(-(1 << 29) // (2 * side * side * C * 4))        # frames per call: 512 MiB read, twice the Infinity Cache
        fa = torch.rand(F_, side, side, C, device=dev)
        fb = torch.rand(F_, side, side, C, device=dev)
        w = torch.rand(C, device=dev)
        acc = torch.zeros(F_, dtype=torch.float64, device=dev)
        med, lo, hi = median_of(lambda: ops.lpips_tap(fa, fb, w, acc), 4 * calls, repeats)
        nbytes = 2.0 * F_ * side * side * C * 4
        taps.append(dict(C=C, F=F_, HW=side * side, us_per_call=round(med * 1e3, 2), us_min=round(lo * 1e3, 2), us_max=round(hi * 1e3, 2),
                         algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / (med * 1e-3), 1)))
    line = json.dumps(dict(bench="lpips", calls=calls, repeats=repeats, device=torch.cuda.get_device_name(0), pairs=rows, tap=taps))
    print(line)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
