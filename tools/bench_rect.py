"""Cost of rectangular frames: one sampler step of the gaussian task and the JPEG codec alone, random weights.

    python tools/bench_rect.py                       # every case below, each in a fresh process under its own time limit;
                                                     # stops at the first case that fails; prints one JSON line per case
                                                     # and a table (ms per step, ms per megapixel relative to 512 x 512)
    python tools/bench_rect.py --case step:512x768   # one case in this process: one JSON line

Cases: ``step:HxW`` -- one denoising step (network in the literal 512 layout, bf16, hipGraph; blur data consistency; fused
sampler update) of a 10-frame window; ``codec:HxW:hw|square`` -- flair_jpeg_roundtrip_hw or the three-launch
flair_jpeg_roundtrip on 10 x 3 x H x W.  Device events, median of 5 timed repetitions after 2 warm-up ones.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_CASES = ["step:512x512", "step:512x768", "step:768x1280"]
CODEC_CASES = ["codec:128x128:square", "codec:128x128:hw", "codec:192x320:hw"]
FRAMES = 10


def median_ms(fn, reps=5, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def run_step(H, W):
    import torch
    from flair_amd import pipeline as pl
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    from flair_amd.guided_diffusion.unet_new import UNetModel
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    pl.check_frame_size("gaussian", (H, W), frames=FRAMES)
    torch.manual_seed(0)
    model = UNetModel(**pl.model_config("gaussian", (H, W)))
    wl.randomize_zero_modules(model)
    model = model.to(dev).eval()
    model.convert_to_fp16()
    model.enable_hip_graph()
    hp = wl.TASKS["gaussian"]
    g = torch.Generator(device=dev).manual_seed(7)
    base = torch.rand(1, 3, H // 4, W // 4, device=dev, generator=g)
    deg = torch.cat([torch.roll(base, shifts=(i, 2 * i), dims=(2, 3)) for i in range(FRAMES)])
    deg = (deg + 0.02 * torch.randn(deg.shape, device=dev, generator=g)).clamp(0, 1)
    init = video.init_frames("gaussian", deg, (H, W))[None]
    deg_n, deg_clip = video.normalise(deg)
    rnn = video.rnn_input(deg_clip, (H, W))[None]
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(),
                     kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    diffusion = wl.diffusion_for(100)
    tt = torch.full((FRAMES,), diffusion.num_timesteps - 1, device=dev, dtype=torch.long)
    x_T = diffusion.q_sample(init[0].contiguous(), tt, noise=torch.randn(FRAMES, 3, H, W, device=dev, generator=g))
    kwargs = dict(low_res_input=init, num_frames=FRAMES, enable_cross_frames=True, vsrpp_weights=1.0, rnn_input=rnn)
    gen = diffusion.p_sample_loop_progressive(
        model, x_T.shape, noise=x_T, clip_denoised=True, model_kwargs=kwargs, device=dev,
        restore_fn=lambda x0: A.A_pinv(deg_n, x0), aux_model=wl.identity_aux, w=hp["w"], tau=5, aligned=True,
        rho=hp["rho"], noise_level=hp["noise_level"], zeta=hp["zeta"])
    out = {}

    def step():
        out["o"] = next(gen)
    med, lo, hi = median_ms(step)          # the warm-up steps hold the chain's first (SPyNet, graph capture)
    finite = bool(torch.isfinite(out["o"]["sample"]).all().item())
    return dict(case=f"step:{H}x{W}", frames=FRAMES, H=H, W=W, ms_per_step=med, ms_min=lo, ms_max=hi,
                ms_per_megapixel=med / (FRAMES * H * W / 1e6), finite=finite, device=torch.cuda.get_device_name(0))


def run_codec(H, W, entry):
    import torch
    from flair_amd import ops
    from flair_amd.guided_diffusion.jpeg import dct8_matrix, general_quant_matrix
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    x = (torch.rand(FRAMES, 3, H, W, device=dev, generator=g) * 2 - 1).contiguous()
    q1, q2 = general_quant_matrix(60)
    d = dct8_matrix().reshape(-1)

    def twenty():
        for _ in range(20):
            ops.jpeg_roundtrip(x, q1, q2, d, entry=entry)
    med, lo, hi = median_ms(twenty)
    return dict(case=f"codec:{H}x{W}:{entry}", frames=FRAMES, H=H, W=W, us_per_call=1e3 * med / 20, us_min=1e3 * lo / 20,
                us_max=1e3 * hi / 20, device=torch.cuda.get_device_name(0))


def run_case(case):
    kind, hw, *rest = case.split(":")
    H, W = (int(v) for v in hw.split("x"))
    return run_step(H, W) if kind == "step" else run_codec(H, W, rest[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None, help="run one case in this process")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds per case (driver mode)")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case)), flush=True)
        return 0
    rows = []
    for case in CODEC_CASES + STEP_CASES:
        r = subprocess.run(["timeout", "-k", "10", str(a.time_limit), sys.executable, os.path.abspath(__file__), "--case", case],
                           cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:            # nothing more is started on the GPU after a failure
            print(f"{case}: exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}", flush=True)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    base = next(r for r in rows if r["case"] == "step:512x512")["ms_per_megapixel"]
    print(f"{'case':<24}{'ms/step':>10}{'min':>9}{'max':>9}{'ms/Mpx':>9}{'rel.':>7}")
    for r in rows:
        if r["case"].startswith("step"):
            print(f"{r['case']:<24}{r['ms_per_step']:>10.2f}{r['ms_min']:>9.2f}{r['ms_max']:>9.2f}"
                  f"{r['ms_per_megapixel']:>9.2f}{r['ms_per_megapixel'] / base:>7.3f}")
    print(f"{'case':<24}{'us/call':>10}{'min':>9}{'max':>9}")
    for r in rows:
        if r["case"].startswith("codec"):
            print(f"{r['case']:<24}{r['us_per_call']:>10.1f}{r['us_min']:>9.1f}{r['us_max']:>9.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
