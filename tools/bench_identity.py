"""Isolated measurement of the ArcFace identity score (flair_amd/identity.py, csrc/ident.hip).

    python tools/bench_identity.py [--out profiles/ident_bench.txt] [--embed-only]

``flair_ident_embed`` on the real network's sizes (F = 16 frames, K = 32768 inputs, O = 512 outputs; w is 67 MB): 60 warmed
calls, each bracketed by HIP events on the launch stream (both launches of the entry), median and minimum, once with one w
(which stays resident in the 256 MiB Infinity Cache) and once with six copies in rotation (403 MB, so the stream comes
from HBM); achieved bytes/s on the algorithmic bytes 4 (O K + F K).  Then one evaluation batch, 8 frame pairs = 16 frames
through the whole network with seeded random weights, from bytes on the device to embeddings on the host, with the host's
clock around calls that end in that copy.  An event pair around ONE call of two short launches measures the host's enqueue as
much as the kernels: for the kernels alone run ``rocprofv3 --kernel-trace --stats -- python tools/bench_identity.py --embed-only``,
which makes only the 78 calls of the rotation case (6 to warm up), so that the two kernels' averages in the statistics are that case's.
There is no earlier implementation to compare against: reported, not gated.
"""
import statistics
import sys
import time

import torch

from flair_amd import identity as fid
from flair_amd import ops

O, K, F = 512, 32768, 16


def event_us(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def main(argv):
    if not torch.cuda.is_available():
        raise SystemExit("bench_identity: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lines = []

    def log(line):
        print(line, flush=True)
        lines.append(line)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, K, generator=g).to(dev)
    bias = torch.randn(O, generator=g).to(dev)
    copies = [(torch.randn(O, K, generator=g) * 0.01).to(dev) for _ in range(6)]
    for w in copies:
        ops.ident_embed(x, w, bias)
    torch.cuda.synchronize()
    nbytes = 4.0 * O * K + 4.0 * F * K
    only = "--embed-only" in argv
    cases = (("one w, resident in the Infinity Cache", copies[:1]), ("six w in rotation, 403 MB, from HBM", copies))
    for label, ws in cases[1:] if only else cases:
        state = {"i": 0}

        def step():
            ops.ident_embed(x, ws[state["i"] % len(ws)], bias)
            state["i"] += 1
        event_us(step, 12)
        t = event_us(step, 60)
        med = statistics.median(t)
        log(f"flair_ident_embed F={F} K={K} O={O} ({label}): median {med:.1f} us, min {min(t):.1f} us over 60 calls (both launches); "
            f"{nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.2f} TB/s at the median")
    if only:
        return 0
    for Fr in (1, 2):
        t = event_us(lambda: ops.ident_embed(x[:Fr], copies[0], bias), 40)
        log(f"flair_ident_embed F={Fr}: median {statistics.median(t):.1f} us")
    m = fid.ArcFace().to(dev)
    for side in (512, 128):
        a = torch.randint(0, 256, (8, side, side, 3), generator=g).to(torch.uint8).to(dev)
        b = torch.randint(0, 256, (8, side, side, 3), generator=g).to(torch.uint8).to(dev)
        for _ in range(2):
            m.embed(a, b)
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            m.embed(a, b)
            ts.append((time.perf_counter() - t0) * 1e3)
        log(f"identity batch of 8 pairs (16 frames) of {side}x{side}: median {statistics.median(ts):.2f} ms, min {min(ts):.2f} ms host time "
            "from bytes on the device to embeddings on the host")
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
