"""VQFR v2 auxiliary prior (guided_diffusion/vqfr.py of the reference, the VQFR project's v2 release configuration) on one
window of aligned 512x512 faces: ms per call in f32 and bf16, the achieved FLOP/s of the whole call from the network's
shapes (flops_per_face) and the conv TFLOP/s from the per-call HIP events of ops.PROFILE; then one sampler step of the
gaussian task at 512x512 x 10 frames (bench.py's setup: bf16 UNet on hipGraphs, aligned=True, tau=5) with the VQFR,
RestoreFormer and CodeFormer priors (f32, the reference's precision) and with no prior, in the same process.
Kernel times: run it under ``rocprofv3 --kernel-trace --stats -- python tools/bench_vqfr.py --no-steps``.

    python tools/bench_vqfr.py [--frames 10] [--steps 3] [--no-steps] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_restoreformer import prior_alone, step_times  # noqa: E402
from flair_amd import pipeline as pl  # noqa: E402
from flair_amd import workload as wl  # noqa: E402
from flair_amd.guided_diffusion.vqfr import VQFRv2  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402


def flops_per_face(cfg):
    """Multiply-adds x 2 of one 512^2 face through the encoder, the code selection, the texture decoder (without its
    conv_out) and the main decoder, from the shapes: convolutions, attention products, the depthwise 7x7 and the
    deformable product (resizes, norms and activations not counted)."""
    base, mult = cfg["base_channels"], cfg["channel_multipliers"]
    n, G, cd, cc = len(mult), cfg["align_opt"]["deformable_groups"], cfg["code_dim"], cfg["inpfeat_dim"]

    def conv(hw, cin, cout, k):
        return 2.0 * hw * hw * cin * cout * k * k

    def res(hw, ci, co):
        return conv(hw, ci, co, 3) + conv(hw, co, co, 3) + (conv(hw, ci, co, 1) if ci != co else 0.0)

    def attn(hw, c):
        return 4 * conv(hw, c, c, 1) + 4.0 * (hw * hw) ** 2 * c

    tot = conv(512, 3, cc, 3) + conv(512, 3, base * mult[0], 3)
    hw = 512
    for i in range(n):                                         # encoder
        cp, c = base * mult[max(i - 1, 0)], base * mult[i]
        if i:
            hw //= 2
            tot += conv(hw, cp, cp, 3)
        for j in range(cfg["num_enc_blocks"]):
            tot += res(hw, cp if j == 0 else c, c) + (attn(hw, c) if i == n - 1 and cfg["use_enc_attention"] else 0.0)
    c = base * mult[-1]
    tot += 2 * res(hw, c, c) + (attn(hw, c) if cfg["use_enc_attention"] else 0.0) + conv(hw, c, cd, 3)
    if cfg["code_selection_mode"] == "Predict":
        tot += 2.0 * 256 * 256 * 1024
    tot += conv(hw, cd, c, 3) + 2 * res(hw, c, c) + (attn(hw, c) if cfg["use_dec_attention"] else 0.0)
    for i in reversed(range(n)):                               # texture decoder
        cp, c = base * mult[min(i + 1, n - 1)], base * mult[i]
        if i != n - 1:
            hw *= 2
            tot += conv(hw, cp, cp, 3)
        for j in range(cfg["num_dec_blocks"]):
            tot += res(hw, cp if j == 0 else c, c) + (attn(hw, c) if i == n - 1 and cfg["use_dec_attention"] else 0.0)
    for i in reversed(range(n)):                               # main decoder
        c, hw, cp = base * mult[i], 512 >> i, base * mult[min(i + 1, n - 1)]
        prev = 0 if i == n - 1 else cp
        tot += conv(hw, c + cc, c, 1) + 2.0 * hw * hw * c * 49 + conv(hw, c, c, 1) + conv(hw, c + prev, c, 3)
        tot += conv(hw, c, 27 * G, 3) + conv(hw, c, c, 3)      # conv_offset + the deformable product
        if i != n - 1:
            tot += conv(hw, cp, c, 3) + res(hw, 2 * c, c)
    return tot + conv(512, base * mult[0], 3, 3)               # decoder.conv_out on the main feature


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="faces per call (the reference's window is 10 frames)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="untimed sampler steps per prior")
    ap.add_argument("--steps", type=int, default=3, help="timed sampler steps per prior")
    ap.add_argument("--no-steps", action="store_true", help="the prior alone (kernel traces)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    cfg = pl.VQFR_CONFIG
    net = name_seeded_weights(VQFRv2(**cfg)).to(dev).eval()
    x = (torch.rand(a.frames, 3, 512, 512, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    fl = flops_per_face(cfg)
    res = {"workload": f"VQFRv2(**VQFR_CONFIG)(x0)['main_dec'] on {a.frames} aligned 512x512 faces", "frames": a.frames,
           "device": torch.cuda.get_device_name(dev), "gflop_per_face_from_shapes": fl / 1e9}
    print(f"{fl / 1e9:.1f} GFLOP per face from the shapes", flush=True)
    for name in ("f32", "bf16"):
        if name == "bf16":
            net.convert_to_bf16()
        r = prior_alone(net, x, a.iters)
        r["achieved_tflops_from_shapes"] = fl * a.frames / (r["ms_per_call"] * 1e-3) / 1e12
        res[name] = r
        print(name, json.dumps(r), flush=True)
    net.convert_to_fp32()
    if not a.no_steps:
        from flair_amd.guided_diffusion.codeformer import CodeFormer
        from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
        rf = name_seeded_weights(VQVAEGANMultiHeadTransformer()).to(dev).eval()
        cf = name_seeded_weights(CodeFormer()).to(dev).eval()
        res["step_ms"] = step_times(dev, a.frames, {"vqfrv2_f32": wl.vqfr_aux(net), "restoreformer_f32": wl.restoreformer_aux(rf),
                                                    "codeformer_f32": wl.codeformer_aux(cf), "none": wl.identity_aux},
                                    a.warmup, a.steps)
        print(json.dumps(res["step_ms"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
