"""Isolated measurement of the spatial QKVAttention kernel (north_star: >= 50 % MFMA utilisation target).

    python tools/bench_attn.py [--json out.json]
    python tools/bench_attn.py --head-dims 32,64,128 [--json out.json]
    python tools/bench_attn.py --wide-heads [--json out.json]
    python tools/bench_attn.py --unet-heads [--json out.json]

--head-dims times each listed head width at L = 256, 1024 and 4096 (16 frames, C = 256 channels, so 256/d heads:
the same FLOPs at every width), and flair_attention_wide once at L = 1024 for each width other than 64 for comparison.

--wide-heads times one head of d = 256, 512, 1024 at L = 256, 1024 and 4096 (16 frames, bf16) on flair_qkv_attention
(the channel-split kernel), on flair_attention_wide where it runs (d + L <= 2048) and on the d = 128 kernel over the
same data read as d/128 heads of width 128 (the same FLOPs: the same-box yardstick).

--unet-heads times one bf16 forward of UNetModel(**blur_unet_config(256, temporal_block=False)) over 16 frames with
one head per attention layer (num_heads=1, num_head_channels=-1: widths 256 and 512) and with the shipped
num_head_channels=64.  (With temporal blocks, one head per layer would give the middle temporal attention a width of
512, which flair_temporal_attention does not run.)

Shapes: the attention blocks of the 16-frame clips -- L = 256 tokens (256x256 clip at ds16; 512x512 at ds32),
L = 1024 (512x512 at ds16), L = 64; 16 frames x heads of width 64.  FLOPs = 4 * frames * heads * L^2 * 64
(QK^T + AV) over the mean launch time of 200 back-to-back launches bracketed by HIP events on the
launch stream; peak = 2.5 PFLOP/s dense bf16.  Also prints the grid (the kernel launches
(ceil(L/128), frames*heads) workgroups of 4 waves), which is what bounds it at these sizes.
"""
import json
import sys

import torch

from flair_amd import ops

PEAK_TFLOPS = 2500.0
SHAPES = [  # name, frames, L (= H*W), C, heads
    ("unet_new ds16 @256^2: L=256, C=256, 4 heads", 16, 256, 256, 4),
    ("unet_new ds32 @256^2: L=64, C=512, 8 heads", 16, 64, 512, 8),
    ("ds16 @512^2: L=1024, C=256, 4 heads", 16, 1024, 256, 4),
    ("ds16 @512^2, 32 frames: L=1024, C=256, 4 heads", 32, 1024, 256, 4),
    ("L=4096 (ds8 @512^2), C=128, 2 heads", 16, 4096, 128, 2),
]


def time_us(fn, n=200):
    """Mean launch time of n back-to-back launches bracketed by HIP events."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def head_dims(dims):
    dev = torch.device("cuda:0")
    F_, C = 16, 256
    rows = []
    for d in dims:
        heads = C // d
        for L in (256, 1024, 4096):
            side = int(L ** 0.5)
            qkv = torch.randn(F_, side, side, 3 * C, device=dev).to(torch.bfloat16)
            out = ops.qkv_attention(qkv, heads)
            kernels = [("flair_qkv_attention", lambda: ops.qkv_attention(qkv, heads, out=out))]
            if d != 64 and L == 1024:
                kernels.append(("flair_attention_wide", lambda: ops.attention_wide(
                    qkv, heads, d, q_off=0, k_off=d, v_off=2 * d, head_stride=3 * d, out=out)))
            for kname, fn in kernels:
                us = time_us(fn, 200 if kname == "flair_qkv_attention" else 20)
                flops = 4.0 * F_ * heads * L * L * d
                tf = flops / us / 1e6
                rows.append({"kernel": kname, "head_dim": d, "frames": F_, "L": L, "heads": heads, "us_per_launch": us,
                             "GFLOP": flops / 1e9, "TFLOP_s": tf, "frac_of_2.5PF": tf / PEAK_TFLOPS})
                print(f"{kname:22s} d={d:4d} L={L:5d} {heads:2d} heads x {F_} frames {us:9.1f} us  {tf:8.1f} TFLOP/s",
                      flush=True)
    return {"kernel": "flair_qkv_attention by head width (bf16)", "peak_TFLOP_s": PEAK_TFLOPS, "rows": rows}


def wide_heads():
    dev = torch.device("cuda:0")
    F_ = 16
    rows = []
    for d in (256, 512, 1024):
        for L in (256, 1024, 4096):
            side = int(L ** 0.5)
            qkv = torch.randn(F_, side, side, 3 * d, device=dev).to(torch.bfloat16)
            out = ops.qkv_attention(qkv, 1)
            kernels = [("flair_qkv_attention", lambda: ops.qkv_attention(qkv, 1, out=out)),
                       ("d=128 kernel, d/128 heads", lambda: ops.qkv_attention(qkv, d // 128, out=out))]
            row = {"head_dim": d, "frames": F_, "L": L, "heads": 1, "GFLOP": 4.0 * F_ * L * L * d / 1e9}
            if d + L <= 2048:
                kernels.append(("flair_attention_wide", lambda: ops.attention_wide(
                    qkv, 1, d, q_off=0, k_off=d, v_off=2 * d, head_stride=3 * d, out=out)))
                ref = ops.attention_wide(qkv, 1, d, q_off=0, k_off=d, v_off=2 * d, head_stride=3 * d).float()
                row["max_abs_diff_vs_attention_wide"] = (ops.qkv_attention(qkv, 1).float() - ref).abs().max().item()
            for kname, fn in kernels:
                us = time_us(fn, 20 if kname == "flair_attention_wide" else 100)
                tf = row["GFLOP"] * 1e3 / us
                row[kname] = {"us_per_launch": us, "TFLOP_s": tf}
                print(f"{kname:26s} d={d:5d} L={L:5d} x {F_} frames {us:10.1f} us  {tf:8.1f} TFLOP/s", flush=True)
            new = row["flair_qkv_attention"]["us_per_launch"]
            row["vs_d128_yardstick"] = row["d=128 kernel, d/128 heads"]["us_per_launch"] / new
            if "flair_attention_wide" in row:
                row["speedup_vs_attention_wide"] = row["flair_attention_wide"]["us_per_launch"] / new
            rows.append(row)
    return {"kernel": "flair_qkv_attention, one head of width d (bf16)", "peak_TFLOP_s": PEAK_TFLOPS, "rows": rows}


def unet_heads():
    from flair_amd.guided_diffusion.script_util import blur_unet_config
    from flair_amd.guided_diffusion.unet_new import UNetModel
    dev = torch.device("cuda:0")
    T, S = 16, 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, 3, S, S, generator=g).to(dev)
    lr = (torch.rand(1, T, 3, S, S, generator=g) * 2 - 1).to(dev)
    t = torch.full((T,), 371, dtype=torch.long, device=dev)
    rows = []
    for name, kw in (("num_heads=1, num_head_channels=-1", dict(num_heads=1, num_head_channels=-1)),
                     ("num_head_channels=64 (shipped)", dict(num_head_channels=64))):
        torch.manual_seed(0)
        m = UNetModel(**dict(blur_unet_config(S, use_fp16=True, temporal_block=False, use_checkpoint=False), **kw))
        m = m.to(dev).eval()
        m.convert_to_fp16()
        with torch.no_grad():
            ms = time_us(lambda: m(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0), 10) / 1e3
        rows.append({"config": name, "frames": T, "size": S, "ms_per_forward": ms})
        print(f"UNetModel blur_unet_config({S}, temporal_block=False) {name:36s} {ms:8.2f} ms / forward "
              f"({T} frames, bf16)", flush=True)
        del m
        torch.cuda.empty_cache()
    return {"model": "UNetModel(**blur_unet_config(256, temporal_block=False)), bf16 forward", "rows": rows}


def main():
    for flag, fn in (("--wide-heads", wide_heads), ("--unet-heads", unet_heads)):
        if flag in sys.argv:
            res = fn()
            if "--json" in sys.argv:
                with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
                    json.dump(res, f, indent=1)
            return
    if "--head-dims" in sys.argv:
        res = head_dims([int(x) for x in sys.argv[sys.argv.index("--head-dims") + 1].split(",")])
        if "--json" in sys.argv:
            with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
                json.dump(res, f, indent=1)
        return
    dev = torch.device("cuda:0")
    rows = []
    for name, F_, L, C, heads in SHAPES:
        side = int(L ** 0.5)
        qkv = torch.randn(F_, side, side, 3 * C, device=dev).to(torch.bfloat16)
        out = ops.qkv_attention(qkv, heads)
        torch.cuda.synchronize()
        n = 200
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ops.qkv_attention(qkv, heads, out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        flops = 4.0 * F_ * heads * L * L * 64
        tf = flops / us / 1e6
        rows.append({"shape": name, "frames": F_, "L": L, "heads": heads, "workgroups": ((L + 127) // 128) * F_ * heads if ((L + 127) // 128) * F_ * heads >= 256 else ((L + 63) // 64) * F_ * heads,
                     "us_per_launch": us, "GFLOP": flops / 1e9, "TFLOP_s": tf, "frac_of_2.5PF": tf / PEAK_TFLOPS})
        print(f"{name:52s} {us:8.1f} us  {tf:8.1f} TFLOP/s = {tf / PEAK_TFLOPS:6.3f} of peak "
              f"({rows[-1]['workgroups']} workgroups)", flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump({"kernel": "attn_mfma_bf16_v2_kernel", "peak_TFLOP_s": PEAK_TFLOPS, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
