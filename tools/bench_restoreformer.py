"""RestoreFormer auxiliary prior (guided_diffusion/restoreformer.py of the reference) on one window of aligned 512x512
faces: ms per call in f32 and bf16 with the conv TFLOP/s from the per-call HIP events of ops.PROFILE; then one sampler
step of the gaussian task at 512x512 x 10 frames (bench.py's setup: bf16 UNet on hipGraphs, aligned=True, tau=5) with
the RestoreFormer prior, with the CodeFormer prior (both f32, the reference's precision) and with no prior.

    python tools/bench_restoreformer.py [--frames 10] [--steps 3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flair_amd import ops  # noqa: E402
from flair_amd import workload as wl  # noqa: E402
from flair_amd.guided_diffusion.codeformer import CodeFormer  # noqa: E402
from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402


def prior_alone(model, x, iters):
    for _ in range(2):
        model(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        model(x)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    ops.PROFILE = []
    model(x)
    torch.cuda.synchronize()
    prof, ops.PROFILE = ops.PROFILE, None
    fam = {}
    for f, _dt, flops, _nbytes, e0, e1, *_rest in prof:
        d = fam.setdefault(f[0], [0, 0.0, 0.0])
        d[0] += 1
        d[1] += flops
        d[2] += e0.elapsed_time(e1)
    conv = fam.get("conv", [0, 0.0, 1e-9])
    n = x.shape[0]
    return {"ms_per_call": ms, "ms_per_face": ms / n, "conv_launches": conv[0], "conv_gflop_per_face": conv[1] / n / 1e9,
            "conv_ms_event_sum": conv[2], "conv_tflops": conv[1] / (conv[2] * 1e-3) / 1e12,
            "whole_call_tflops": conv[1] / (ms * 1e-3) / 1e12, "families_ms": {k: round(v[2], 3) for k, v in fam.items()}}


def step_times(dev, frames, aux_models, warmup, steps):
    """ms per denoising step of bench.py's gaussian-task chain (bf16 UNet, hipGraphs) with each aux model."""
    from flair_amd.guided_diffusion import pseudoSR as psr
    from flair_amd.guided_diffusion.unet_new import UNetModel
    S, T, hp = 512, frames, wl.TASKS["gaussian"]
    torch.manual_seed(0)
    model = UNetModel(**wl.blur_config(S, use_fp16=True))
    wl.randomize_zero_modules(model)
    model = model.to(dev).eval()
    model.convert_to_fp16()
    model.enable_hip_graph()
    degraded, init, rnn = (v.to(dev) for v in wl.clip_inputs("gaussian", 0, T, S))
    lr = degraded[0].contiguous()
    diffusion = wl.diffusion_for(250)
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(),
                     kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    g = torch.Generator(device=dev).manual_seed(4321)
    tt = torch.full((T,), diffusion.num_timesteps - 1, device=dev, dtype=torch.long)
    x_T = diffusion.q_sample(init[0].contiguous(), tt, noise=torch.randn(T, 3, S, S, device=dev, generator=g))
    kwargs = dict(low_res_input=init, num_frames=T, enable_cross_frames=True, vsrpp_weights=1.0, rnn_input=rnn)
    out = {}
    for name, aux in aux_models.items():
        gen = diffusion.p_sample_loop_progressive(
            model, x_T.shape, noise=x_T, clip_denoised=True, model_kwargs=kwargs, device=dev,
            restore_fn=lambda x0: A.A_pinv(lr, x0), aux_model=aux, w=hp["w"], tau=5, aligned=True, rho=hp["rho"],
            noise_level=hp["noise_level"], zeta=hp["zeta"])
        for _ in range(warmup):
            next(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            next(gen)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) * 1e3 / steps
        print("step", name, f"{out[name]:.2f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="faces per call (the reference's window is 10 frames)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2, help="untimed sampler steps per prior")
    ap.add_argument("--steps", type=int, default=3, help="timed sampler steps per prior")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    net = name_seeded_weights(VQVAEGANMultiHeadTransformer()).to(dev).eval()
    x = (torch.rand(a.frames, 3, 512, 512, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    res = {"workload": f"VQVAEGANMultiHeadTransformer()(x0) on {a.frames} aligned 512x512 faces", "frames": a.frames,
           "device": torch.cuda.get_device_name(dev)}
    for name in ("f32", "bf16"):
        if name == "bf16":
            net.convert_to_bf16()
        res[name] = prior_alone(net, x, a.iters)
        print(name, json.dumps(res[name]), flush=True)
    net.convert_to_fp32()
    cf = name_seeded_weights(CodeFormer()).to(dev).eval()
    res["step_ms"] = step_times(dev, a.frames, {"restoreformer_f32": wl.restoreformer_aux(net),
                                                "codeformer_f32": wl.codeformer_aux(cf), "none": wl.identity_aux},
                                a.warmup, a.steps)
    print(json.dumps(res["step_ms"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
