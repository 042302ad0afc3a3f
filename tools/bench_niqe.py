"""Isolated measurement of NIQE (flair_amd/niqe.py, csrc/niqe.hip): milliseconds per frame, split into kernels and host part.

    python tools/bench_niqe.py [--json profiles/niqe_bench.json] [--calls 5] [--repeats 3]

Sizes: 512 x 512 (the reference's demo clips) and 768 x 1280 (a rectangular video), one frame per call (N = 1), with a synthetic
pristine model and the closed-form window (the cost does not depend on their values) on noise frames, where every block has a
fit.  Each case is warmed, then ``--calls`` back-to-back calls are bracketed by HIP events on the launch stream, ``--repeats``
times; the median is reported with the spread.  ``ms_per_frame`` is the whole call as evaluate makes it: three launches, the
copy of 50 doubles per block to the host, the AGGD fits and the distance in numpy.  ``kernels`` are the three launches alone
(and each of them alone), ``host`` the numpy part alone on moments already fetched, timed with the host's clock.  There is no
earlier implementation to compare against: the numbers are reported, not gated.
Prints one JSON line.
"""
import json
import sys
import time

import numpy as np
import torch

from flair_amd import niqe as fnq
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


def host_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def median_of(fn, calls, repeats, timer=time_ms):
    for _ in range(2):                                                                         # warm-up
        fn()
    torch.cuda.synchronize()
    ms = sorted(timer(fn, calls) for _ in range(repeats))
    return [round(v, 4) for v in (ms[len(ms) // 2], ms[0], ms[-1])]


def synthetic_model(dev):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((36, 36)) * 0.2
    x = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return fnq.NIQE(rng.standard_normal(36) * 0.5 + 1.0, a @ a.T + 0.01 * np.eye(36), g / g.sum(), dev)


def main(argv):
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 5
    repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else 3
    if not torch.cuda.is_available():
        raise SystemExit("bench_niqe: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    model = synthetic_model(dev)
    rows = []
    for H, W in SIZES:
        g = torch.Generator(device=dev).manual_seed(H + W)
        u8 = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        y1, y2 = ops.niqe_luma(u8)
        m = model.moments(u8).cpu().numpy()
        blocks = m.shape[2]

        def host():
            f = np.stack([fnq.features(m[0], 96 * 96), fnq.features(m[1], 48 * 48)], axis=2).reshape(1, blocks, 36)
            return fnq.score(f[0], model.mu, model.cov)
        assert not np.isnan(host())
        rows.append(dict(shape=[H, W], blocks=blocks,
                         ms_per_frame=median_of(lambda: model(u8), calls, repeats),
                         kernels_ms=median_of(lambda: model.moments(u8), calls, repeats),
                         luma_ms=median_of(lambda: ops.niqe_luma(u8, y1=y1, y2=y2), calls, repeats),
                         moments_96_ms=median_of(lambda: ops.niqe_moments(y1, 96, 1.0, model.window), calls, repeats),
                         moments_48_ms=median_of(lambda: ops.niqe_moments(y2, 48, ops.NIQE_HALF_UNIT, model.window), calls, repeats),
                         host_ms=median_of(host, calls, repeats, timer=host_ms)))
    line = json.dumps(dict(bench="niqe", calls=calls, repeats=repeats, device=torch.cuda.get_device_name(0),
                           columns="median, min, max", frames=rows))
    print(line)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
