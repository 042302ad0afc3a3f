#!/usr/bin/env python3
"""Headline benchmark: restored frames/s of FLAIR's sampling hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

Workload (BASELINE.json configs[1]): gaussian-demo, one clip of 16 frames at 256x256 per
GPU, 250-step generalised-DDIM chain (space_timesteps(1000,"250"), rho=0.25), bf16 UNet
(unet_new.UNetModel, 405.6 M parameters, random init), Gaussian-blur x4 data-consistency
operator on the GPU, identity aux prior with aligned=True.  A "step" is one denoising step
of the clip = one UNet forward + restore_fn + fused sampler update.  W warm-up steps, then
exactly K steps are timed between barrier + synchronize; frames/s for the whole 250-step
job is  n_gpus * frames / (250 * mean step time)  (with the default K = 250 - W - 2 the timed
region is the whole chain but the warm-up steps and the two steps of the instrumented pass).
When W + K + 2 exceeds the chain, the chain starts over from the same x_T, as the next job on
the clip would (its first step recomputes the SPyNet flows and re-captures the UNet's graph).
Inputs are resident in HBM before timing; every input is seeded, so runs with the same
arguments see the same inputs.

--dump-outputs DIR writes what the timed path handed its caller in the last timed step (rank 0)
as DIR/<name>.npy: the sample x_{t-1} and pred_xstart (float32, the sampler's (B*T, 3, S, S)
layout) and the timestep t (float64).  Above DUMP_BUDGET_BYTES in all, every array is replaced by
the same fixed, seeded sample of its flattened elements (see dump_outputs).

The JSON line also carries
  roofline     -- the dominant kernel (implicit-GEMM conv on MFMA): algorithmic FLOPs of its
                  launches / their summed HIP-event durations in one extra instrumented step;
  cpu_baseline -- the CPU oracle (oracle/, torch fp32) on this host's cores on a bounded
                  sample of the same workload (rank 0, N=1 only).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOTAL_STEPS = 250
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}   # dense, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0
DUMP_BUDGET_BYTES = 60 * 10 ** 6                     # --dump-outputs: array data written in all (< 64 MB with headers)
# rocprofv3 kernel names of the conv variants (keys of profiles/*_hbm_traffic_pmc.json)
CONV_ROCPROF = {0: "conv_igemm_kernel<{E}, 128, 128, 2, 2>", 1: "conv_igemm_kernel<{E}, 64, 128, 1, 4>",
                2: "conv_igemm_kernel<{E}, 64, 64, 2, 2>", 3: "conv3x3_halo_kernel<{E}, 8, 1, 1>",
                4: "conv3x3_halo_kernel<{E}, 4, 1, 1>", 5: "conv3x3_halo_kernel<{E}, 2, 1, 1>",
                6: "conv3x3_halo_ks_kernel<{E}, 8, 1, 2>", 7: "conv3x3_halo_ks_kernel<{E}, 4, 1, 2>",
                8: "conv3x3_dma_kernel<8, 2, 2>", 9: "conv3x3_dma_kernel<8, 1, 2>", 10: "conv3x3_dma_kernel<4, 1, 3>"}
CONV_VARIANTS = {0: "conv_igemm_kernel<128co x 128px>", 1: "conv_igemm_kernel<64co x 128px>",
                 2: "conv_igemm_kernel<64co x 64px>", 3: "conv3x3_halo_kernel<8 rows>",
                 4: "conv3x3_halo_kernel<4 rows>", 5: "conv3x3_halo_kernel<2 rows>",
                 6: "conv3x3_halo_ks_kernel<8 rows>", 7: "conv3x3_halo_ks_kernel<4 rows>",
                 8: "conv3x3_dma_kernel<16 rows, persistent>", 9: "conv3x3_dma_kernel<8 rows>", 10: "conv3x3_dma_kernel<4 rows>",
                 11: "conv3x3_dma_kernel<4 rows, K split>"}


def pmc_traffic_for(kernel_fmt, dkey):
    """HBM bytes per launch of `kernel` from the newest committed PMC table (profiles/*_hbm_traffic_pmc.json,
    written by tools/pmc_traffic.py from two separate rocprofv3 --pmc passes of this same command: counters
    cannot be read from inside the process).  Returns (bytes or None, source file or None)."""
    import glob
    name = kernel_fmt.format(E="bf16" if dkey == "bf16" else "float")
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_hbm_traffic_pmc.json")), reverse=True):
        try:
            with open(path) as f:
                tab = json.load(f)
        except (OSError, ValueError):
            continue
        ent = tab.get("kernels", {}).get(name)
        if ent:
            return ent["read_bytes_per_launch"] + ent["write_bytes_per_launch"], os.path.relpath(path, ROOT)
    return None, None


def cpu_baseline_prior():
    """cpu_baseline leg of `--aux codeformer`: the oracle's CodeFormer (port, torch CPU fp32) on ONE aligned 512x512 face,
    as the sampler calls it (w = 1, AdaIN), with the same default-initialised weights as the benched HIP module."""
    from flair_amd.guided_diffusion.codeformer import CodeFormer
    from oracle import codeformer as ocf
    torch.manual_seed(1)
    sd = {k: v.detach().float() for k, v in CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                                                        connect_list=["32", "64", "128", "256"]).state_dict().items()}
    x = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(0)) * 2 - 1
    ocf.codeformer_forward(sd, x, w=1.0, adain=True)
    t0 = time.time()
    ocf.codeformer_forward(sd, x, w=1.0, adain=True)
    return {"kind": "port", "cores": torch.get_num_threads(), "s_per_face": time.time() - t0,
            "sample": "oracle/codeformer.py, one 512x512 face, fp32"}


def dump_outputs(out, path):
    """--dump-outputs: write the tensors of one sampler step's result `out` as <path>/<name>.npy (floating point as
    float32, integers as float64).  When they exceed DUMP_BUDGET_BYTES together, each array is cut to the same share of
    its flattened elements, at sorted indices drawn by numpy's default_rng(0): a fixed sample for a fixed shape, so two
    runs with the same arguments stay comparable element for element.  Returns {name: [shape written, full shape]}."""
    import numpy as np
    arrays = {}
    for name, v in out.items():
        if torch.is_tensor(v):
            dt = torch.float32 if v.is_floating_point() else torch.float64
            arrays[name] = v.detach().to("cpu", dt).numpy()
    total = sum(x.nbytes for x in arrays.values())
    os.makedirs(path, exist_ok=True)
    written = {}
    for name, x in arrays.items():
        full = list(x.shape)
        if total > DUMP_BUDGET_BYTES:
            n = max(1, x.size * DUMP_BUDGET_BYTES // total)
            x = x.reshape(-1)[np.sort(np.random.default_rng(0).choice(x.size, size=n, replace=False))]
        np.save(os.path.join(path, name + ".npy"), x)
        written[name] = [list(x.shape), full]
    return written


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps, exactly (default: the whole chain minus the warm-up and the two instrumented steps)")
    ap.add_argument("--total-steps", type=int, default=None,
                    help="length of the sampling chain (default 250; 1000 for x16_bicubic = BASELINE config 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--task", default="gaussian", choices=["gaussian", "jpeg", "x8_bicubic", "x16_bicubic"])
    ap.add_argument("--aux", default="identity", choices=["identity", "codeformer"],
                    help="auxiliary prior inside the step: identity (BASELINE configs; the reference's demos at 256^2 "
                         "cannot run CodeFormer, which is fixed to 512^2) or the HIP CodeFormer (needs --size 512)")
    ap.add_argument("--aux-dtype", default="f32", choices=["f32", "bf16"],
                    help="CodeFormer arithmetic: the reference keeps the prior in fp32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--attention-resolutions", default=None,
                    help="comma-separated downsample rates that get spatial attention (unet_new.UNetModel). Default: the "
                         "reference's 512-pixel tuple scaled with the clip side, (S//32, S//16, S//8) = 8,16,32 at 256 "
                         "(attention over 1024 / 256 / 64 tokens, as in the 512-pixel network); 16,32,64 = the tuple "
                         "taken literally (scripts/video_sample.py:122-126; 256 / 64 / 16 tokens at 256, SURVEY.md section 3.2)")
    ap.add_argument("--graph", dest="graph", action="store_true", default=True,
                    help="replay a captured hipGraph of the UNet forward (default): bit-identical to eager launches and "
                         "as fast on one GPU (the step is GPU-bound), but the host spends ~5 ms instead of ~60 ms per "
                         "step, which keeps 8 rank processes on one node from competing for CPU time")
    ap.add_argument("--no-graph", dest="graph", action="store_false", help="launch every kernel eagerly")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's sample / pred_xstart / t as DIR/<name>.npy")
    return ap.parse_args()


def cpu_baseline(size, frames):
    """Oracle (port) timed on this host's cores on BASELINE config 1's own geometry: ONE full denoising step
    (UNet forward incl. SPyNet + blur restore_fn + generalised-DDIM update) of the 8-frame 128x128 gaussian-demo
    clip with the full-width network, fp32.  `value` converts that to the metric's unit for the benched job
    (frames x size^2, TOTAL_STEPS steps): conv work is linear in frames x pixels."""
    from flair_amd import workload as wl
    from oracle import degrade as odeg
    from oracle import diffusion as odiff
    from oracle.unet import UNetModel as Oracle
    T, S, STEPS = 8, 128, 50
    n_threads = torch.get_num_threads()
    torch.manual_seed(0)
    t0 = time.time()
    o = Oracle(**wl.blur_config(S, use_fp16=False)).eval()
    wl.randomize_zero_modules(o)
    build = time.time() - t0
    degraded, init, rnn = wl.clip_inputs("gaussian", 0, T, S)
    hp = wl.TASKS["gaussian"]
    tab = odiff.Spaced(odiff.spaced_steps(1000, str(STEPS)), odiff.named_betas("face_blur", 1000))
    g = torch.Generator().manual_seed(4321)
    x_T = odiff.q_sample(tab, init[0], torch.full((T,), STEPS - 1), torch.randn(T, 3, S, S, generator=g))
    z = torch.randn(T, 3, S, S, generator=g)
    oblur = odeg.BlurOperator(wl.synthetic_blur_kernel(), 4)
    calls = []

    class Stop(Exception):
        pass

    def model(x, t, **kw):
        if calls:
            raise Stop()
        calls.append(1)
        return o(x, t, **kw)
    trace = []
    t0 = time.time()
    with torch.no_grad():
        try:
            odiff.sample_loop(tab, model, x_T,
                              model_kwargs=dict(low_res_input=init, num_frames=T, rnn_input=rnn, vsrpp_weights=1.0),
                              restore_fn=lambda x0: oblur.a_pinv(degraded[0], x0), aux_model=wl.identity_aux,
                              w=hp["w"], tau=5, rho=hp["rho"], noise_level=hp["noise_level"], zeta=hp["zeta"],
                              step_noise=[z] * STEPS, trace=trace)
        except Stop:
            pass
    dt = time.time() - t0                      # one full step (the second model call stops the loop at once)
    scale = (frames / T) * (size / S) ** 2
    return {"value": frames / (TOTAL_STEPS * dt * scale), "unit": "frames/s", "cores": n_threads, "kind": "port",
            "config1_frames_per_s": T / (STEPS * dt),
            "sample": f"oracle/ (torch CPU fp32, {n_threads} threads): ONE full denoising step of BASELINE config 1 "
                      f"(gaussian-demo, {T} frames x {S}x{S}, full-width network): {dt:.1f} s (model build {build:.0f} s) "
                      f"= {T / (STEPS * dt):.2e} frames/s for config 1's 50-step job; `value` scales the step by "
                      f"frames x pixels (x{scale:.0f}) to the benched {frames} x {size}x{size}, {TOTAL_STEPS}-step job"}


def visible_gpu_count():
    """GPUs this process may use, counted WITHOUT touching the HIP runtime (the parent only spawns the rank processes and
    must never initialise the GPU): KFD topology nodes with SIMDs, narrowed by *_VISIBLE_DEVICES.  None if unknown."""
    import glob
    n = 0
    try:
        for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
            with open(path) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except (OSError, ValueError):
        return None
    if n == 0:
        return None
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([d for d in v.split(",") if d.strip() != ""]))
    return n


def spawn_ranks(n, wall_limit_s=None):
    """`python bench.py --gpus N` without a launcher: start N rank processes (one per GPU) from this
    process, which never touches the GPU, and relay rank 0's JSON line.  Children get the same
    environment torch.distributed.run would give them.  All children are polled: when one exits non-zero,
    or the wall limit passes, the others are terminated and this process exits non-zero with the tail of
    the failing rank's stderr (a rank that dies inside RCCL initialisation must not leave rank 0 hanging)."""
    import socket
    import subprocess
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    wall_limit_s = wall_limit_s or float(os.environ.get("FLAIR_BENCH_WALL_LIMIT_S", "1500"))
    procs, logs = [], []
    tmp = tempfile.mkdtemp(prefix="flair_bench_")
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out = open(os.path.join(tmp, f"rank{r}.out"), "w+b")
        err = open(os.path.join(tmp, f"rank{r}.err"), "w+b")
        logs.append((out, err))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out, stderr=err, start_new_session=True))

    def tail(f, nbytes=4000):
        f.flush()
        f.seek(0, 2)
        size = f.tell()
        f.seek(max(0, size - nbytes))
        return f.read().decode("utf-8", "replace")

    def stop_all(sig=None):
        """Every child leads its own session (start_new_session above), so a kill of this process's group misses them:
        signal each child's process group explicitly, then reap."""
        import signal as _sg
        for q in procs:
            if q.poll() is None:
                try:
                    os.killpg(q.pid, sig or _sg.SIGTERM)
                except (ProcessLookupError, PermissionError):
                    pass
        t_end = time.time() + 10
        for q in procs:
            try:
                q.wait(timeout=max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(q.pid, _sg.SIGKILL)
                except (ProcessLookupError, PermissionError):
                    pass
                q.wait()

    def cleanup():
        import shutil
        for out, err in logs:
            out.close()
            err.close()
        shutil.rmtree(tmp, ignore_errors=True)

    class _Stopped(Exception):
        pass

    def on_signal(signum, _frame):
        raise _Stopped(signum)

    import signal
    old_handlers = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP)}
    t0 = time.time()
    failed = None
    rc = 1
    try:
        while True:
            codes = [q.poll() for q in procs]
            bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                failed = (bad[0], f"rank {bad[0]} exited with status {codes[bad[0]]}")
                break
            if all(c == 0 for c in codes):
                break
            if time.time() - t0 > wall_limit_s:
                failed = (0, f"wall limit of {wall_limit_s:.0f} s passed (ranks still running: "
                             f"{[r for r, c in enumerate(codes) if c is None]})")
                break
            time.sleep(0.2)
        if failed is not None:
            r, why = failed
            sys.stderr.write(f"bench.py --gpus {n}: {why}; stderr tail of rank {r}:\n{tail(logs[r][1])}\n")
            sys.stderr.flush()
        else:
            sys.stdout.write(tail(logs[0][0], 1 << 20))
            sys.stdout.flush()
            sys.stderr.write(tail(logs[0][1]))
            rc = 0
    except _Stopped as e:
        sys.stderr.write(f"bench.py --gpus {n}: signal {e.args[0]} received, stopping the rank processes\n")
        rc = 128 + int(e.args[0])
    finally:
        # whatever ended the loop (a failing rank, the wall limit, a signal from the driver, an exception): no rank process
        # outlives this one, the per-rank log files are closed and the temporary directory removed
        for sg, h in old_handlers.items():
            signal.signal(sg, h)
        stop_all()
        cleanup()
    return rc


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        n_dev = visible_gpu_count()             # sysfs only: the parent never loads the HIP runtime
        if n_dev is not None and n_dev < a.gpus:
            raise SystemExit(f"--gpus {a.gpus} requested but only {n_dev} GPU(s) are visible")
        raise SystemExit(spawn_ranks(a.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)

    from flair_amd import ops, parallel
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    from flair_amd.guided_diffusion.jpeg import jpeg_decode, jpeg_encode
    from flair_amd.guided_diffusion.unet_new import UNetModel

    S, T = a.size, a.frames
    global TOTAL_STEPS
    TOTAL_STEPS = a.total_steps or (1000 if a.task == "x16_bicubic" else 250)
    W = max(0, a.warmup)
    if a.steps is None:
        a.steps = max(1, TOTAL_STEPS - W - 2)
    if a.steps < 1:
        raise SystemExit(f"--steps {a.steps}: at least one step must be timed")
    K = a.steps
    hp = wl.TASKS[a.task]
    bicubic = "bicubic" in a.task
    torch.manual_seed(0)
    if bicubic:
        from flair_amd.guided_diffusion.restore_util import SRConv
        from flair_amd.guided_diffusion.sr3 import UNet as BicubicUNet
        model = BicubicUNet(**wl.sr3_config(S, use_fp16=(a.dtype == "bf16")))
    else:
        cfg_ = wl.blur_config(S, use_fp16=(a.dtype == "bf16"))
        if a.attention_resolutions:
            cfg_["attention_resolutions"] = tuple(int(v) for v in a.attention_resolutions.split(","))
        model = UNetModel(**cfg_)
        attn_res = tuple(cfg_["attention_resolutions"])
    if rank == 0:
        wl.randomize_zero_modules(model)
    n_params = sum(p_.numel() for p_ in model.parameters())
    model = model.to(dev).eval()
    if a.dtype == "bf16":
        model.convert_to_fp16()
    # one kernel-native (bf16-packed) weight blob from rank 0 over RCCL; the other ranks never repack
    t_bcast, bcast_bytes = parallel.broadcast_packed_weights(model, src=0) if world > 1 else (0.0, 0)
    bcast_per_rank = [{"rank": 0, "s": t_bcast, "bytes": bcast_bytes}]
    if world > 1:       # every rank's own view of the start-up weight distribution (seconds, bytes received)
        mine = torch.tensor([t_bcast, float(bcast_bytes)], device=dev, dtype=torch.float64)
        allv = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allv, mine)
        bcast_per_rank = [{"rank": r, "s": float(v[0]), "bytes": int(v[1])} for r, v in enumerate(allv)]
    use_graph = a.graph and hasattr(model, "enable_hip_graph")
    if use_graph:
        model.enable_hip_graph()          # one hipGraph per clip shape: ~3300 launches become one replay
    clip_id = rank                                     # weak scaling: one clip per GPU
    degraded, init, rnn = (v.to(dev) for v in wl.clip_inputs(a.task, clip_id, T, S))
    lr_flat = degraded[0].contiguous()
    qf = hp["jpeg_qf"]
    if bicubic:
        diffusion = wl.bicubic_diffusion_for(TOTAL_STEPS)
        A_func = SRConv(wl.bicubic_taps(hp["factor"]), 3, S, dev, stride=hp["factor"])
        d_flat = lr_flat.reshape(T, -1)

        def restore_fn(x0):                            # bicubic_restore, scripts/video_sample.py:177-181
            return A_func.A_pinv(ops.axpby(A_func.A(x0.reshape(T, -1)), d_flat, 1.0, -1.0)).reshape(x0.shape)
    else:
        diffusion = wl.diffusion_for(TOTAL_STEPS)
        conf = psr.Get_pseudoSR_Conf(4)
        A_func = psr.pseudoSR(conf, upscale_kernel=wl.synthetic_blur_kernel(),
                              kernel_indx=10).WrapArchitecture_PyTorch().to(dev)

        def restore_fn(x0):
            return A_func.A_pinv(lr_flat, x0,
                                 jpeg_encode=(lambda im: jpeg_encode(im, qf)) if qf != -1 else None,
                                 jpeg_decode=(lambda im: jpeg_decode(im, qf)) if qf != -1 else None)

    g = torch.Generator(device=dev).manual_seed(4321 + clip_id)
    tt = torch.full((T,), diffusion.num_timesteps - 1, device=dev, dtype=torch.long)
    x_T = diffusion.q_sample(init[0].contiguous(), tt, noise=torch.randn(T, 3, S, S, device=dev, generator=g))
    if bicubic:
        kwargs = dict(low_res_input=init, num_frames=T, enable_cross_frames=True,
                      vsrpp_weights=wl.face_weight_map(T, S, hp["face_weight"]).to(dev))
    else:
        kwargs = dict(low_res_input=init, num_frames=T, enable_cross_frames=True, vsrpp_weights=1.0, rnn_input=rnn)

    aux_model = wl.identity_aux
    if a.aux == "codeformer":
        if S != 512:
            raise SystemExit("--aux codeformer needs --size 512 (codeformer.py:730 reshapes to a 16x16 code grid)")
        from flair_amd.guided_diffusion.codeformer import CodeFormer
        torch.manual_seed(1)
        gan = CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                         connect_list=["32", "64", "128", "256"]).to(dev).eval()
        if a.aux_dtype == "bf16":
            gan.convert_to_bf16()
        aux_model = wl.codeformer_aux(gan)

    def chains():
        """The timed path: the denoising steps of the clip's chain, and of the same chain again when a run outlasts it."""
        while True:
            yield from diffusion.p_sample_loop_progressive(
                model, x_T.shape, noise=x_T, clip_denoised=True, model_kwargs=kwargs, device=dev,
                restore_fn=restore_fn, aux_model=aux_model, w=hp["w"], tau=5, aligned=True, rho=hp["rho"],
                noise_level=hp["noise_level"], zeta=hp["zeta"])
    gen = chains()

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(W):
        next(gen)
    sync()
    t0 = time.perf_counter()
    for _ in range(K):
        out = next(gen)
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    finite = bool(torch.isfinite(out["sample"]).all().item())
    dumped = dump_outputs(out, a.dump_outputs) if a.dump_outputs and rank == 0 else None
    # the instrumented pass below wants steady-state steps (not a chain's first: SPyNet, graph re-capture) within one
    # chain; a run that ended at a chain boundary steps on, untimed (never with the default K: W + K + 2 <= the chain)
    for _ in range({0: 1, TOTAL_STEPS - 1: 2}.get((W + K) % TOTAL_STEPS, 0)):
        next(gen)

    # ---- roofline leg.  One more (eagerly launched, steady-state) step records every conv / GroupNorm / alignment / warp /
    # attention call together with a closure that re-issues the identical library call (same tensors, same arguments).
    # Every DISTINCT launch shape is then timed on the launch stream: a hipGraph of REPLAY_N back-to-back launches of that
    # call between two HIP events, minimum of three replays / REPLAY_N.  A family's time is sum(count x per-launch time).
    # Nothing is subtracted: the figure includes the ~1.6 us launch boundary of a replayed graph (tools/probes/launch_probe),
    # so it reads up to ~3 % BELOW rocprofv3's kernel-only average duration of the same kernel (profiles/r03*_kernel_stats.csv;
    # dominant kernel: 71.2 us here against 69.1 us under rocprofv3), never above it.  Bracketing each launch of the eager step
    # itself with events is not usable: the eager step is host-bound for short kernels (the event pairs time host gaps, up to
    # 10x for the fused chains) -- those raw in-situ times are reported for the dominant kernel only, as a cross-check.
    if use_graph:
        # the instrumented step launches eagerly.  The eager path keys its optical-flow cache on the caller's tensors, not
        # on the graph's static copies: one un-instrumented eager step first, so that the measured step is a steady-state
        # one (no SPyNet, second-order flows already composed) like the timed steps
        model.enable_hip_graph(False)
        next(gen)
        torch.cuda.synchronize()
    c0_, c1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0_.record()
    torch.cuda._sleep(20_000_000)
    c1_.record()
    torch.cuda.synchronize()
    spin_cycles_per_ms = 20_000_000 / max(c0_.elapsed_time(c1_), 1e-3)
    torch.cuda._sleep(int(spin_cycles_per_ms * 250))          # the host queues the step behind ~250 ms of spinning
    ops.PROFILE = []
    next(gen)
    torch.cuda.synchronize()
    prof, ops.PROFILE = ops.PROFILE, None
    REPLAY_N = 10
    # FLAIR_BENCH_REPLAY: "pad" (default) replays with the padding described in replay_us; "plain" without it; "off" no isolated
    # replays at all -- the in-situ event times stand in (counter-collection passes of rocprofv3, where every launch is
    # serialised and costs milliseconds: the process then launches exactly what the steps launch)
    REPLAY_MODE = os.environ.get("FLAIR_BENCH_REPLAY", "pad")

    def replay_us(fn, count=1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            fn()
            with torch.cuda.graph(g_, stream=side, capture_error_mode="thread_local"):
                for _ in range(REPLAY_N):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        g_.replay()
        torch.cuda.synchronize()
        best = None
        for _ in range(3):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            g_.replay()
            c1.record()
            torch.cuda.synchronize()
            us_ = c0.elapsed_time(c1) * 1e3 / REPLAY_N
            best = us_ if best is None else min(best, us_)
        # Untimed padding so that a profiler's per-kernel AVERAGE over this process is comparable with the figures below:
        # a shape has been launched 1 + 4 * REPLAY_N times so far whatever its share of a step; launching it that often
        # per launch it has in a step makes rocprofv3's average of a kernel the launch-count-weighted average over its
        # shapes, which is what `avg_launch_us` is (profiles/*_bench_steps6_kernel_stats.csv).
        if REPLAY_MODE == "pad":
            for _ in range(round((1 + 4 * REPLAY_N) * (count - 1) / REPLAY_N)):
                g_.replay()
            torch.cuda.synchronize()
        return best

    sig_events = {}
    for fam, dt_name, flops_, nbytes, e0, e1, replay, sig in prof:
        d = sig_events.setdefault((fam, dt_name, sig), [0, 0.0, flops_, replay, 0.0, nbytes])
        d[0] += 1
        d[1] += e0.elapsed_time(e1) * 1e3              # raw in-situ events (cross-check only)
    for k_, d in sig_events.items():
        d[4] = replay_us(d[3], d[0]) if REPLAY_MODE != "off" else d[1] / d[0]      # isolated per-launch time of this shape
    per = {}
    for (fam, dt_name, sig), (n_, ev_us, fl_, replay, us_, nb_) in sig_events.items():
        d = per.setdefault((fam, dt_name), [0, 0.0, 0.0, 0.0, 0.0])
        d[0] += n_
        d[1] += fl_ * n_
        d[3] += us_ * n_ * 1e-6
        d[4] += ev_us * 1e-6
    for fam, dt_name, flops_, nbytes, e0, e1, replay, sig in prof:
        per[(fam, dt_name)][2] += nbytes
    conv_keys = [k for k in per if k[0][0] == "conv"]
    key = max(conv_keys, key=lambda k: per[k][3])
    calls, flops, _, secs, secs_events = per[key]
    achieved = flops / secs / 1e12
    dkey = "bf16" if "bfloat16" in key[1] else "f32"
    peak = MFMA_PEAK_TFLOPS[dkey]
    all_flops = sum(per[k][1] for k in conv_keys)
    all_secs = sum(per[k][3] for k in conv_keys)
    step_s = elapsed / K
    by_shape = []
    for (fam, dt_name, sig), (n_, ev_us, fl_, replay, us_, nb_) in sig_events.items():
        if (fam, dt_name) != key:
            continue
        by_shape.append({"shape": {"T": sig[1], "H": sig[2], "W": sig[3], "cin": list(sig[4]), "cout": sig[5], "kernel": list(sig[6]),
                                   "act": sig[8], "residuals": int(sig[9]) + int(sig[10])},
                         "launches": n_, "us_per_launch": us_, "us_per_launch_in_situ_events": ev_us / n_,
                         "TFLOP/s": fl_ / us_ / 1e6, "frac": fl_ / us_ / 1e6 / peak})
    by_shape.sort(key=lambda e_: -e_["launches"] * e_["us_per_launch"])

    def family(pred, bound, label):
        """pred(fam, sig) over the distinct launch shapes; time = sum(count x isolated per-launch time)."""
        ks = [k for k in sig_events if pred(k[0], k[2])]
        if not ks:
            return None
        n = sum(sig_events[k][0] for k in ks)
        fl = sum(sig_events[k][0] * sig_events[k][2] for k in ks)
        by = sum(sig_events[k][0] * sig_events[k][5] for k in ks)
        se = sum(sig_events[k][0] * sig_events[k][4] for k in ks) * 1e-6
        ent = {"family": label, "bound": bound, "launches": n, "ms_per_step": 1e3 * se, "share_of_step": se / step_s}
        if bound == "mfma":
            pk = MFMA_PEAK_TFLOPS["bf16" if "bfloat16" in ks[0][1] else "f32"]
            ent.update(achieved=fl / se / 1e12, peak=pk, unit="TFLOP/s", frac=fl / se / 1e12 / pk)
        else:
            ent.update(achieved=by / se / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / se / 1e9 / HBM_PEAK_GBS,
                       algorithmic_MB_per_launch=by / n / 1e6, TFLOP_per_s=fl / se / 1e12)
        return ent

    def is_1x1(sig):          # a convolution that only moves bytes: 1x1x1 taps, stride 1 (sig: ops.conv's signature)
        return tuple(sig[6]) == (1, 1, 1) and sig[7] == 1

    def big_level(sig):       # >= 64 x 64 pixels per frame: activations far beyond the L2s, arithmetic intensity <= 2*Cin*Cout/(Cin+Cout)/esz
        return sig[2] * sig[3] >= 64 * 64
    fams = [
        family(lambda f, sg: f[0] == "conv" and f[1] in (6, 7, 9, 10), "mfma",
               "per-frame 3x3 convs of the BasicVSR++ recurrence (conv3x3_dma_kernel<8|4 rows> / conv3x3_halo_ks_kernel)"),
        family(lambda f, sg: f[0] == "conv" and f[1] in (3, 4, 5, 8), "mfma",
               "clip-level 3x3 / 3x3x3 convs + c->432 offset convs (conv3x3_dma_kernel<16 rows> / conv3x3_halo_kernel)"),
        family(lambda f, sg: f[0] == "conv" and f[1] in (0, 1, 2) and is_1x1(sg) and big_level(sg), "hbm",
               "1x1 convs on the >= 64x64 levels (conv_igemm_kernel): skip / qkv / proj / conv_last, <= 64 FLOP per byte moved; "
               "bytes = esz*(Cin+Cout*(1+residuals))*T*H*W"),
        family(lambda f, sg: f[0] == "conv" and f[1] in (0, 1, 2) and not (is_1x1(sg) and big_level(sg)), "mfma",
               "strided / 7x7 / deep-K small-spatial convs and 1x1 convs of the <= 32x32 levels (conv_igemm_kernel, split-K)"),
        family(lambda f, sg: f[0] == "chain", "mfma", "fused per-frame conv chains (conv_chain_kernel)"),
        family(lambda f, sg: f[0] == "gn", "hbm", "GroupNorm+SiLU+FiLM(+resample): gn_partial/finalize/apply, bytes = esz*3*numel"),
        family(lambda f, sg: f[0] == "dcn" and f[1] <= 64, "hbm", "deformable alignment c=64 (dcn_kernel), bytes = esz*(3c+432)*H*W"),
        family(lambda f, sg: f[0] == "dcn" and f[1] > 64, "hbm", "deformable alignment c=128 (dcn_kernel), bytes = esz*(3c+432)*H*W"),
        family(lambda f, sg: f[0] == "prep", "hbm", "flow warp + compose of one propagation step (vsrpp_prep_kernel)"),
        family(lambda f, sg: f[0] == "attn", "mfma", "spatial QKVAttention in situ (attn_mfma_bf16_kernel; isolated: attention_isolated)"),
    ]
    fams = [f for f in fams if f]

    # ---- north_star target 1: the ResBlock conv path against the HBM roofline.  One level-0 2-D ResBlock (GroupNorm+SiLU ->
    # conv3x3 -> GroupNorm*(1+scale)+shift+SiLU -> conv3x3 + skip on the (T, S, S, c0) tensor): SURVEY 8a/8d's minimum
    # traffic = 7 passes over the activation (statistics read + normalise-on-load read + write, twice, + the residual read
    # = 0.94 GB at 16 x 256^2 x 64 bf16) over the measured time of its two norms and two convolutions.
    resblock_path = None
    esz_act = 2 if a.dtype == "bf16" else 4
    sig_mean = {(fam, sig): d[4] for (fam, dt_name, sig), d in sig_events.items()}

    def pick(pred):
        v = [us_ for (fam, sig), us_ in sig_mean.items() if pred(fam, sig)]
        return sum(v) / len(v) if v else None
    conv2 = [sig for (fam, sig) in sig_mean if fam[0] == "conv" and sig[1:4] == (T, S, S) and len(sig[4]) == 1
             and sig[4][0] == sig[5] and tuple(sig[6]) == (1, 3, 3) and sig[7] == 1 and sig[9] and not sig[10]]
    if conv2:
        c0 = min(sig[5] for sig in conv2)            # level 0 is the narrowest level
        conv2_us = pick(lambda fam, sig: fam[0] == "conv" and sig in conv2 and sig[5] == c0)
        conv1_us = pick(lambda fam, sig: fam[0] == "conv" and sig[1:4] == (T, S, S) and sig[4] == (c0,) and sig[5] == c0
                        and tuple(sig[6]) == (1, 3, 3) and not sig[9] and sig[8] == 0 and not sig[11])
        gn1_us = pick(lambda fam, sig: fam[0] == "gn" and sig[1:5] == (T, S, S, c0) and sig[5] == c0 and sig[9] == 0
                      and not sig[10] and not sig[11] and sig[8] != 0)
        gn2_us = pick(lambda fam, sig: fam[0] == "gn" and sig[1:5] == (T, S, S, c0) and sig[5] == c0 and sig[9] == 0
                      and not sig[10] and sig[11])
        if None not in (conv1_us, gn1_us, gn2_us):
            act_bytes = esz_act * T * S * S * c0
            tot_us = conv1_us + conv2_us + gn1_us + gn2_us
            resblock_path = {"block": f"level-0 2-D ResBlock, ({T},{S},{S},{c0}) {a.dtype}", "bound": "hbm",
                             "algorithmic_bytes": 7 * act_bytes, "us": {"gn1": gn1_us, "conv1": conv1_us, "gn2": gn2_us,
                                                                        "conv2": conv2_us, "total": tot_us},
                             "achieved": 7 * act_bytes / tot_us / 1e3, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": 7 * act_bytes / tot_us / 1e3 / HBM_PEAK_GBS, "target_frac": 0.70,
                             "bytes_actually_moved": 11 * act_bytes,
                             "note": "isolated replay times; 7 activation passes = SURVEY 8d minimum (0.94 GB at 16x256^2x64 bf16); "
                                     "the unfused pipeline moves 11 (two-pass norm x2, conv read+write x2, residual read)"}

    # ---- north_star target 2: QKVAttention against the MFMA peak, isolated (replay-timed) at L = 256, 1024 and 4096 tokens;
    # 16 frames, heads of width 64; FLOPs = 4 * frames * heads * L^2 * 64.  The benched network (attention_resolutions scaled
    # with the clip: 8,16,32 at 256) runs its attention blocks at L = 1024 / 256 / 64 like the 512-pixel reference network;
    # L = 256 is also the LARGEST block of the literal 16,32,64 layout (--attention-resolutions 16,32,64): 1.07 GFLOP, launch-bound
    attention_isolated = []
    if a.dtype == "bf16":
        for L_, C_, heads_ in ((256, 256, 4), (1024, 256, 4), (4096, 128, 2)):
            side_ = int(L_ ** 0.5)
            qkv_ = torch.randn(16, side_, side_, 3 * C_, device=dev).to(torch.bfloat16)
            out_ = ops.qkv_attention(qkv_, heads_)
            us_ = replay_us(lambda: ops.qkv_attention(qkv_, heads_, out=out_))
            fl_ = 4.0 * 16 * heads_ * L_ * L_ * 64
            attention_isolated.append({"L": L_, "frames": 16, "heads": heads_, "us_per_launch": us_, "GFLOP": fl_ / 1e9,
                                       "achieved": fl_ / us_ / 1e6, "peak": MFMA_PEAK_TFLOPS["bf16"], "unit": "TFLOP/s",
                                       "frac": fl_ / us_ / 1e6 / MFMA_PEAK_TFLOPS["bf16"], "target_frac": 0.50})
            del qkv_, out_
    # ---- what THIS device sustains with nothing in the way (calibration launches of the library, include/flair_hip.h): independent
    # bf16 MFMA chains out of registers in a launch of per-frame length (~80 us, replayed back to back like every shape above) and
    # in one ~7 ms launch; read / write / copy of 1 GiB.  Fractions above stay against the data-sheet peaks; this block says how
    # much of those peaks the silicon reaches at the clock it holds under load (profiles/r04_attainable_peaks.txt).
    attainable = None
    if a.dtype == "bf16":
        sink_ = torch.zeros(4, dtype=torch.float32, device=dev)
        fl_short = ops.probe_matrix_rate(250, 1, sink_)
        us_short = replay_us(lambda: ops.probe_matrix_rate(250, 1, sink_))
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fl_long = ops.probe_matrix_rate(25000, 1, sink_)
        torch.cuda.synchronize()
        c0.record()
        ops.probe_matrix_rate(25000, 1, sink_)
        c1.record()
        torch.cuda.synchronize()
        us_long = c0.elapsed_time(c1) * 1e3
        buf_a = torch.empty(1 << 30, dtype=torch.uint8, device=dev).fill_(1)
        buf_b = torch.empty(1 << 30, dtype=torch.uint8, device=dev).fill_(2)
        stream_rates = {}
        for name_, mode_ in (("read", 0), ("write", 1), ("copy", 2)):
            moved_ = ops.probe_stream_rate(buf_a, buf_b, mode_)
            torch.cuda.synchronize()
            best_ = None
            for _ in range(3):
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0.record()
                ops.probe_stream_rate(buf_a, buf_b, mode_)
                c1.record()
                torch.cuda.synchronize()
                t_ = c0.elapsed_time(c1) * 1e3
                best_ = t_ if best_ is None else min(best_, t_)
            stream_rates[name_ + "_1GiB_GB/s"] = moved_ / best_ / 1e3
        del buf_a, buf_b
        attainable = {"matrix_TFLOP/s_80us_launches": fl_short / us_short / 1e6, "matrix_TFLOP/s_7ms_launch": fl_long / us_long / 1e6,
                      "matrix_frac_of_peak": [fl_short / us_short / 1e6 / MFMA_PEAK_TFLOPS["bf16"], fl_long / us_long / 1e6 / MFMA_PEAK_TFLOPS["bf16"]],
                      **stream_rates, "copy_frac_of_peak": stream_rates["copy_1GiB_GB/s"] / HBM_PEAK_GBS,
                      "note": "measured on this device in this process: v_mfma_f32_32x32x16_bf16 chains out of registers on every CU; "
                              "16-byte grid-stride streaming kernels; the data-sheet peaks assume 2.4 GHz and 8 TB/s"}

    # ---- the whole step against the MFMA peak: every FLOP the instrumented steady-state step issued on the matrix cores
    # (convolutions, fused chains, alignment GEMM + bilinear blends, QK^T / AV) over the timed mean step; SPyNet is not in it
    # (its flows are cached per clip: not executed in a steady-state step), GroupNorm / warps / sampler count as zero FLOPs.
    step_flops = sum(d[0] * d[2] for d in sig_events.values())
    whole_step = {"TFLOP": step_flops / 1e12, "ms": 1e3 * step_s, "achieved": step_flops / step_s / 1e12,
                  "peak": MFMA_PEAK_TFLOPS[a.dtype if a.dtype in MFMA_PEAK_TFLOPS else "bf16"], "unit": "TFLOP/s",
                  "frac": step_flops / step_s / 1e12 / MFMA_PEAK_TFLOPS[a.dtype if a.dtype in MFMA_PEAK_TFLOPS else "bf16"],
                  "launches_profiled": sum(d[0] for d in sig_events.values()),
                  "sum_of_isolated_family_ms": sum(f["ms_per_step"] for f in fams)}
    traffic, traffic_src = pmc_traffic_for(CONV_ROCPROF.get(key[0][1], ""), dkey)
    ms_per_step = 1e3 * elapsed / K
    value = world * T / (TOTAL_STEPS * elapsed / K)
    line = {
        "metric": f"restored frames/sec at {S}x{S}, {T}-frame clip, {TOTAL_STEPS}-step DDIM",
        "value": value, "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": f"{a.task}-demo, {world} clip(s) x {T} frames x {S}x{S}, "
                               f"{TOTAL_STEPS}-step generalised DDIM (rho={hp['rho']}), "
                               + (f"sr3.UNet {n_params / 1e6:.1f}M params random init, SRConv bicubic restore_fn on GPU" if bicubic else
                                  f"unet_new.UNetModel {n_params / 1e6:.1f}M params random init, attention_resolutions="
                                  f"{','.join(str(v) for v in attn_res)} (spatial attention over "
                                  f"{'/'.join(str((S // v) ** 2) for v in attn_res)} tokens), blur x4 restore_fn on GPU")
                               + ", one clip per GPU",
                   "steps_per_clip": TOTAL_STEPS, "value_definition": f"n_gpus*frames/({TOTAL_STEPS}*mean timed step)",
                   "finite_output": finite, "dumped_outputs": dumped, "weight_broadcast_s": max(b["s"] for b in bcast_per_rank),
                   "weight_broadcast_bytes": bcast_bytes, "weight_broadcast_per_rank": bcast_per_rank,
                   "hip_graph": use_graph, "params_M": n_params / 1e6,
                   "attention_resolutions": None if bicubic else list(attn_res),
                   "aux_prior": "identity" if a.aux == "identity" else f"CodeFormer (HIP, {a.aux_dtype}) every step t >= tau"},
        "roofline": {"bound": "mfma", "kernel": CONV_VARIANTS.get(key[0][1], str(key[0][1])) + " " + key[1],
                     "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                     "traffic": traffic, "traffic_unit": "HBM bytes per launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE)",
                     "traffic_source": traffic_src, "algorithmic_bytes_per_launch": per[key][2] / calls,
                     "launches": calls, "avg_launch_us": 1e6 * secs / calls,
                     "avg_launch_us_in_situ_events": 1e6 * secs_events / calls,
                     "timing": f"every distinct launch shape of one steady-state step re-issued alone: hipGraph of {REPLAY_N} back-to-back "
                               "launches between HIP events on the launch stream, min of 3 replays; nothing subtracted (includes the "
                               "~1.6 us launch boundary: reads <= 3 % below rocprofv3's kernel-only average in profiles/)",
                     "by_shape": by_shape,
                     "all_conv_achieved": all_flops / all_secs / 1e12,
                     "all_conv_share_of_step": all_secs / (ms_per_step * 1e-3),
                     "whole_step": whole_step,
                     "resblock_path": resblock_path,
                     "attention_isolated": attention_isolated,
                     "attainable_on_this_device": attainable,
                     "families": fams},
    }
    if rank == 0:
        if world == 1 and not a.no_cpu_baseline:
            try:
                line["cpu_baseline"] = cpu_baseline(S, T)
                if a.aux == "codeformer":
                    line["cpu_baseline"]["aux_prior"] = cpu_baseline_prior()
            except Exception as exc:  # the baseline must never hide the measurement
                line["cpu_baseline"] = {"value": None, "error": repr(exc)}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
