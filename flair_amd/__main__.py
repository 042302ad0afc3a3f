"""Command line: ``python -m flair_amd restore TASK VIDEO_DIR OUTPUT_DIR [options]`` and the four demo presets.

The options of the reference's ``main()`` keep their names and defaults (``scripts/video_sample.py:249-263``); the
presets are its ``x8_bicubic_demo`` ... ``jpeg_demo`` commands (:500-556).  Several videos go through one call with
``--output-root DIR`` (each to ``DIR/<video dir name>``); ``--frame-size HxW`` (or ``auto``) restores rectangular frames; under ``torch.distributed.run`` the videos are split over the
ranks (flair_amd.pipeline.restore_many) and rank 0 reads the checkpoints once and ships them to the others.
"""
import argparse
import json
import os
import sys

from . import pipeline as pl


def _add_common(p):
    p.add_argument("--weights", default="./checkpoints", metavar="DIR",
                   help="directory with flair_<task>.pt, the prior's checkpoint (codeformer.pth, RestoreFormer.ckpt or VQFR_v2.pth), "
                        "the detector and the parser's parsing_parsenet.pth / parsing_bisenet.pth")
    p.add_argument("--kernels", default=pl.DEFAULT_KERNELS, metavar="PATH",
                   help="the blur kernels .mat file (MATLAB v5) of the gaussian and jpeg tasks")
    p.add_argument("--device", default=None, help="default: cuda (cuda:LOCAL_RANK under torch.distributed.run)")
    p.add_argument("--size", type=int, default=512, help="frame side of the restored video")
    p.add_argument("--frame-size", default=None, metavar="HxW|auto",
                   help="rectangular frames of height H and width W (multiples of the task's frame multiple); the degraded "
                        "frames must be exactly H/f x W/f and are not resized; auto: the first frame's size times the "
                        "task's factor f.  Excludes a non-default --size")
    p.add_argument("--steps", type=int, default=100, help="sampler steps (respacing of the diffusion)")
    p.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("--det-model", choices=tuple(pl.DETECTOR_FILES), default="retinaface_resnet50")
    p.add_argument("--parser", choices=tuple(pl.PARSER_FILES), default="parsenet",
                   help="face parser of the unaligned branch and the bicubic tasks' weights (parsenet reads "
                        "parsing_parsenet.pth, bisenet parsing_bisenet.pth)")
    p.add_argument("--prior", choices=tuple(pl.PRIOR_FILES), default=None,
                   help="auxiliary face prior (default: codeformer, reading codeformer.pth; restoreformer reads "
                        "RestoreFormer.ckpt, vqfrv2 VQFR_v2.pth)")
    p.add_argument("--prior-kwargs", default=None, metavar="JSON", help="overrides of the prior's constructor arguments")
    p.add_argument("--no-prior", action="store_true", help="identity prior instead of CodeFormer (no codeformer.pth)")
    p.add_argument("--model-kwargs", default=None, metavar="JSON", help="overrides of the task's model configuration")
    p.add_argument("--no-graph", action="store_true", help="run the network eagerly instead of replaying hipGraphs")
    p.add_argument("--seed", type=int, default=None, help="seed torch's generators before every video")


def _add_hparams(p, d):
    p.add_argument("--t-start", type=int, default=d["t_start"])
    p.add_argument("--jpeg-qf", type=int, default=d["jpeg_qf"])
    p.add_argument("--w", type=float, default=d["w"])
    p.add_argument("--tau", type=int, default=d["tau"])
    p.add_argument("--aligned", action="store_true", default=d["aligned"],
                   help="frames are aligned 512 x 512 faces: run the prior on whole frames, no face detection")
    p.add_argument("--faces", choices=("largest", "all"), default="largest",
                   help="unaligned frames: run the prior on the largest face of every frame, each of which needs one "
                        "(largest), or on every detected face, where frames may have none (all)")
    p.add_argument("--max-faces", type=int, default=4, metavar="N",
                   help="with --faces all: at most N faces per frame, largest first (bounds the prior's cost)")
    p.add_argument("--rho", type=float, default=d["rho"])
    p.add_argument("--noise-level", type=float, default=d["noise_level"])
    p.add_argument("--zeta", type=float, default=d["zeta"])


def make_parser():
    ap = argparse.ArgumentParser(prog="python -m flair_amd", description="FLAIR face video restoration on MI355X")
    sub = ap.add_subparsers(dest="command", required=True)
    r = sub.add_parser("restore", help="restore one video (VIDEO_DIR OUTPUT_DIR) or several (VIDEO_DIR... --output-root)")
    r.add_argument("task", choices=pl.TASK_NAMES)
    r.add_argument("paths", nargs="+", metavar="PATH", help="VIDEO_DIR OUTPUT_DIR, or VIDEO_DIR... with --output-root")
    r.add_argument("--output-root", default=None, metavar="DIR", help="write every VIDEO_DIR to DIR/<its name>")
    _add_hparams(r, pl.MAIN_DEFAULTS)
    _add_common(r)
    for name, demo in pl.DEMOS.items():
        d = sub.add_parser(name, help=f"{demo['task']}: {demo['video_path']} -> {demo['output_path']}")
        _add_hparams(d, dict(pl.MAIN_DEFAULTS, **{k: v for k, v in demo.items() if k in pl.MAIN_DEFAULTS}))
        _add_common(d)
    return ap


def jobs_of(args):
    """The (video_dir, output_dir) pairs of a parsed command line."""
    if args.command in pl.DEMOS:
        demo = pl.DEMOS[args.command]
        return demo["task"], [(demo["video_path"], demo["output_path"])]
    if args.output_root is None:
        if len(args.paths) != 2:
            raise SystemExit("restore: give VIDEO_DIR OUTPUT_DIR, or several VIDEO_DIRs with --output-root DIR")
        jobs = [tuple(args.paths)]
    else:
        jobs = [(v, os.path.join(args.output_root, os.path.basename(os.path.normpath(v)))) for v in args.paths]
    for v, _ in jobs:
        if not os.path.isdir(v):
            raise SystemExit(f"restore: {v} is not a directory")
    return args.task, jobs


def prior_of(args):
    """The ``prior`` argument of build_pipeline for a parsed command line."""
    if args.no_prior and args.prior is not None:
        raise SystemExit("restore: --no-prior and --prior exclude each other")
    if args.no_prior:
        return False
    return args.prior or "codeformer"


def faces_of(args):
    """The ``faces`` / ``max_faces`` arguments of restore_video_files for a parsed command line (--max-faces is only read
    with --faces all)."""
    if args.faces != "all":
        return {}
    if args.aligned:
        raise SystemExit("restore: --faces all belongs to unaligned frames (drop --aligned)")
    if args.max_faces < 1:
        raise SystemExit("restore: --max-faces must be at least 1")
    return dict(faces="all", max_faces=args.max_faces)


def size_of(args, task, jobs):
    """The ``size`` argument of build_pipeline for a parsed command line: --size S (an int, the reference's square
    frames) or --frame-size HxW / auto (a pair; auto reads the first frame of the first video)."""
    if args.frame_size is None:
        return args.size
    if args.size != 512:
        raise SystemExit("restore: --frame-size and --size exclude each other")
    try:
        size = pl.parse_frame_size(args.frame_size)
        if size == "auto":
            size = pl.auto_frame_size(task, jobs[0][0])
        return pl.check_frame_size(task, size)
    except ValueError as exc:
        raise SystemExit(f"restore: {exc}")


def main(argv=None):
    args = make_parser().parse_args(argv)
    task, jobs = jobs_of(args)
    prior = prior_of(args)
    faces = faces_of(args)
    size = size_of(args, task, jobs)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
        dist.init_process_group("nccl" if torch.cuda.is_available() else "gloo")
        device = args.device or (f"cuda:{local}" if torch.cuda.is_available() else "cpu")
    else:
        device = args.device or "cuda"
    try:
        torch.set_grad_enabled(False)
        p = pl.build_pipeline(task, args.weights, device=device, size=size, dtype=args.dtype, steps=args.steps,
                              kernels_path=args.kernels, prior=prior, det_model=args.det_model,
                              model_kwargs=json.loads(args.model_kwargs) if args.model_kwargs else None,
                              graph=not args.no_graph,
                              prior_kwargs=json.loads(args.prior_kwargs) if args.prior_kwargs else None,
                              parser=args.parser)
        hp = dict(aligned=args.aligned, t_start=args.t_start, jpeg_qf=args.jpeg_qf, w=args.w, tau=args.tau,
                  rho=args.rho, noise_level=args.noise_level, zeta=args.zeta, seed=args.seed)
        hp.update(faces)
        pl.restore_many(jobs, lambda v, o: p.restore_video_files(v, o, **hp))
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
