"""Command line: ``python -m flair_amd restore TASK VIDEO_DIR OUTPUT_DIR [options]`` and the four demo presets, plus the two
ends of the loop around it: ``degrade TASK CLEAN_DIR OUT_DIR`` makes a task's degraded frames from clean ones with the exact
operator the restoration assumes (flair_amd.degrade), and ``evaluate RESTORED_DIR TRUTH_DIR`` scores written frames with PSNR
and SSIM (flair_amd.metrics) and, with ``--lpips {vgg,alex} --weights DIR``, LPIPS (flair_amd.lpips); ``restore --ground-truth
DIR`` scores every video as soon as it is written.  ``niqe FRAMES_DIR --params FILE`` scores frames that have no ground truth
(flair_amd.niqe); ``--niqe FILE`` adds that score to evaluate, restore and interpolate, the last two with or without ground truth.
``--identity FILE`` adds the ArcFace identity similarity and drift (flair_amd.identity) wherever there is ground truth.
``--warp-error FILE`` adds the flow-warping error, the temporal consistency of the written frames (flair_amd.temporal), to
evaluate, restore and interpolate, and ``warp-error FRAMES_DIR --flow-weights FILE`` scores footage that has no ground truth.
``--score-faces largest|all`` adds the same scores over the face regions of unaligned frames (flair_amd.facescore) to evaluate and
restore --ground-truth.
``interpolate SRC_DIR OUT_DIR --factor N`` changes the frame rate of written frames with SuperSloMo or AMT-G (flair_amd.interpolate).
``scenes SRC_DIR --json PATH`` finds the hard cuts of a video (flair_amd.scenes); ``restore`` / ``interpolate --scene-cuts
auto|PATH`` then treat every shot on its own.

The options of the reference's ``main()`` keep their names and defaults (``scripts/video_sample.py:249-263``); the
presets are its ``x8_bicubic_demo`` ... ``jpeg_demo`` commands (:500-556).  Several videos go through one call with
``--output-root DIR`` (each to ``DIR/<video dir name>``); a YUV4MPEG2 stream (a path ending ``.y4m``, flair_amd.y4m) stands
wherever a directory of frames does, as input of every command and as output of restore, degrade and interpolate; ``--frame-size HxW`` (or ``auto``) restores rectangular frames; under ``torch.distributed.run`` the videos are split over the
ranks (flair_amd.pipeline.restore_many) and rank 0 reads the checkpoints once and ships them to the others.
"""
import argparse
import json
import os
import sys

from . import pipeline as pl
from . import scenes
from .tiling import DEFAULT_OVERLAP, DEFAULT_TILE


def _add_yuv(p, writes=False):
    """The options of .y4m streams: what a stream's header leaves open and, for the commands that write one, its format."""
    p.add_argument("--yuv-matrix", choices=("bt601", "bt709"), default=None,
                   help="colour matrix of .y4m streams, read and written; their header cannot say (default: bt601)")
    p.add_argument("--yuv-range", choices=("limited", "full"), default=None,
                   help="range of .y4m streams whose header has no XCOLORRANGE tag, and of written ones that follow no input "
                        "stream (default: limited)")
    if writes:
        p.add_argument("--y4m-chroma", choices=("420jpeg", "420mpeg2", "422", "444"), default=None,
                       help="chroma format of a written .y4m stream (default: the input stream's, else 420jpeg)")
        p.add_argument("--fps", default=None, metavar="N[:D]",
                       help="frame rate in a written .y4m stream's header (default: the input stream's, else 25:1)")


def apply_yuv(args):
    """Make a parsed command line's stream options the process-wide ones of flair_amd.y4m (a command line is complete: what it
    does not say is the default, not what an earlier one said)."""
    from . import y4m
    try:
        y4m.set_defaults(args.yuv_matrix or "bt601", args.yuv_range or "limited")
        y4m.set_output(getattr(args, "y4m_chroma", None), getattr(args, "fps", None))
    except ValueError as exc:
        raise SystemExit(f"{args.command}: {exc}")


def frames_exist(path):
    """A directory of frame files, or a .y4m file."""
    from .y4m import is_y4m
    return os.path.isfile(path) if is_y4m(path) else os.path.isdir(path)


def metrics_path(output):
    """Where restore writes a video's scores: metrics.json in a directory of frames, <output>.metrics.json next to a stream."""
    from .y4m import is_y4m
    return output + ".metrics.json" if is_y4m(output) else os.path.join(output, "metrics.json")


def _add_common(p):
    _add_yuv(p, writes=True)
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
    p.add_argument("--tile", default="off", metavar="off|auto|HxW",
                   help="tiled denoising (needs --frame-size): at every step the network runs on overlapping tiles of H x W pixels, "
                        "clipped per axis to the frame, and the tile outputs are blended with feathered weights; everything else "
                        "of a step stays on whole frames.  off (default): whole frames, with today's size rules; HxW: always "
                        "tile; auto: tile at 512x512 only where the frame is refused whole (not a multiple of the task's frame "
                        "multiple, or beyond the kernels' 32-bit limits, e.g. 1080x1920).  The frame's H and W must still be "
                        "multiples of the task's factor (of 64 for jpeg) and hold one tile; frames are not padded.  Tiling costs "
                        "work (the overlaps are denoised twice), faces cut by a seam get per-tile propagation weights in the "
                        "bicubic tasks, and 512 with overlap 64 is a heuristic that has NOT been validated on real footage")
    p.add_argument("--tile-overlap", type=int, default=DEFAULT_OVERLAP, metavar="P",
                   help="with --tile: neighbouring tiles share at least P pixels, over which the blend ramps from one to the "
                        "other (a multiple of the task's factor; default 64, a heuristic)")
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
    _add_cut_options(p, "restore every shot on its own: no window spans a cut and a shot's first window is not pinned to "
                        "the shot before it")


def _add_cut_rule(p):
    d = scenes.RULE_DEFAULTS
    p.add_argument("--cut-threshold", type=float, default=d["threshold"], metavar="D",
                   help="a cut needs a block-luma distance d of at least D between its two frames (0..255 scale)")
    p.add_argument("--cut-ratio", type=float, default=d["ratio"], metavar="R",
                   help="... and of at least R times the median d of the neighbouring pairs (rejects motion, noise and fades)")
    p.add_argument("--cut-radius", type=int, default=d["radius"], metavar="K", help="pairs on either side in that median")
    p.add_argument("--min-shot", type=int, default=d["min_shot"], metavar="N",
                   help="shortest shot in frames; flash frames are folded into a neighbouring shot")


def _add_cut_options(p, what):
    p.add_argument("--scene-cuts", default="off", metavar="off|auto|PATH",
                   help=f"{what}.  off (default): the frames are one shot; auto: detect the cuts first (hard cuts only, no "
                        "fades or dissolves; the rule's defaults are heuristics chosen on synthetic sequences and have NOT "
                        "been validated on real footage); PATH: a cuts file written by the scenes command or by hand")
    _add_cut_rule(p)


def _add_lpips(p, what, where):
    p.add_argument("--lpips", choices=("vgg", "alex"), default=None,
                   help=f"{what} LPIPS on a VGG-16 trunk (vgg16.pth + lpips_vgg.pth; what BasicSR-style evaluation reports) or "
                        f"an AlexNet trunk (alexnet.pth + lpips_alex.pth; the lpips package's default){where}")


def _add_niqe(p, what):
    p.add_argument("--niqe", default=None, metavar="FILE",
                   help=f"{what} the no-reference NIQE of the written frames (lower is better); FILE is BasicSR's "
                        "niqe_pris_params.npz (mu_pris_param, cov_pris_param, gaussian_window).  Needs no ground truth; frames "
                        "must hold at least two 96x96 blocks")


def _add_identity(p, what):
    p.add_argument("--identity", default=None, metavar="FILE",
                   help=f"{what} the ArcFace identity similarity of every frame with its truth (ids, a cosine: higher is closer) "
                        "and the identity drift from frame to frame of both sets; FILE is GFPGAN's / VQFR's arcface_resnet18.pth.  "
                        "Frames are taken as aligned face crops and must be square: faces are not detected.  Scene cuts are not "
                        "consulted: a cut shows up as drift")


WARP_FILE = "a bare mmedit SPyNet state dict or any FLAIR task checkpoint (flair_<task>.pt), which holds one"


def _add_warp_error(p, what):
    p.add_argument("--warp-error", default=None, metavar="FILE",
                   help=f"{what} the flow-warping error of every two consecutive written frames (warp-err, printed x 10^3: lower "
                        "is steadier; Lai et al. 2018 with the occlusion mask of Ruder et al. 2016, on SPyNet flows) and the "
                        f"masked-out share; FILE is {WARP_FILE}.  With ground truth the flows and the mask come from the truth "
                        "and the truth's own value is printed in brackets; without it they come from the written frames.  "
                        "Frames must be at least 32 pixels a side; pairs across a scene cut are left out")


def warp_of(args, command, option="--warp-error"):
    """The flow weights of a parsed command line's --warp-error (--flow-weights of the warp-error command), or None without
    it; refused before any GPU work where it is not a file."""
    path = getattr(args, "warp_error" if option == "--warp-error" else "flow_weights", None)
    if path is None:
        return None
    if not os.path.isfile(path):
        raise SystemExit(f"{command}: {option} {path} is not a file ({WARP_FILE})")
    return path


def load_warp_of(path, device, command):
    """The WarpError model of warp_of's result on ``device`` (None for None)."""
    if path is None:
        return None
    from . import temporal as ftm
    try:
        return ftm.WarpError(ftm.load_flow(path, device))
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"{command}: {exc}")


def warp_tail(result):
    """``  warp-err X (truth Y)  masked Z`` of a result's mean where it holds them ('' without --warp-error)."""
    if "warp_err" not in result["mean"]:
        return ""
    from .temporal import format_mean
    return format_mean(result["mean"])


def warp_skip_of(scene_cuts, cut_rule, paths, device, command, factor=1):
    """The ``warp_skip`` argument of evaluate_dirs: the later frames of the pairs that straddle a cut of ``paths`` (``factor``:
    the frames scored are interpolate's output at that multiple of ``paths``' rate)."""
    from . import temporal as ftm
    try:
        cuts, _ = scenes.resolve(scene_cuts, paths, device, **cut_rule)
    except (ValueError, OSError) as exc:
        raise SystemExit(f"{command}: {exc}")
    return ftm.straddling(cuts, factor)


def _add_score_faces(p, what, own_detector):
    p.add_argument("--score-faces", choices=("largest", "all"), default=None,
                   help=f"{what} PSNR / SSIM (and --lpips, --identity) of the face regions: the faces are found on the ground-truth "
                        "frames and one alignment cuts both frame sets; largest: at most one face per frame, with the identity "
                        "drift; all: every face, at most --max-faces per frame.  --identity then scores the face crops only")
    p.add_argument("--face-size", type=int, default=512, metavar="S", help="with --score-faces: the side of the aligned face crops")
    if own_detector:
        p.add_argument("--max-faces", type=int, default=4, metavar="N", help="with --score-faces all: at most N faces per frame, largest first")
        p.add_argument("--det-model", choices=tuple(pl.DETECTOR_FILES), default="retinaface_resnet50",
                       help="with --score-faces: the face detector, read from --weights DIR")


def face_scorer_of(args, command):
    """dict(mode, max_faces, face_size, det_model, weights) of a parsed command line's --score-faces, or None without it;
    refused before any GPU work where there is no ground truth, a number is out of range or (evaluate, which builds the
    detector itself) the detector's file is missing."""
    mode = getattr(args, "score_faces", None)
    if mode is None:
        return None
    if command != "evaluate" and not args.ground_truth:
        raise SystemExit(f"{command}: --score-faces compares the written frames with --ground-truth DIR; give one")
    if args.max_faces < 1:
        raise SystemExit(f"{command}: --max-faces must be at least 1")
    from .metrics import SSIM_WINDOW
    if args.face_size < SSIM_WINDOW:
        raise SystemExit(f"{command}: --face-size must be at least {SSIM_WINDOW} (SSIM's window)")
    if command == "evaluate":
        if not args.weights:
            raise SystemExit(f"{command}: --score-faces reads the {args.det_model} detector from --weights DIR; give one")
        path = os.path.join(args.weights, pl.DETECTOR_FILES[args.det_model][1])
        if not os.path.isfile(path):
            raise SystemExit(f"{command}: --score-faces with --det-model {args.det_model} needs {path}")
    return dict(mode=mode, max_faces=args.max_faces, face_size=args.face_size, det_model=args.det_model, weights=args.weights)


def load_face_scorer_of(spec, device, command, face_det=None):
    """The FaceScorer of face_scorer_of's result on ``device`` (None for None); ``face_det``: a loaded detector to reuse
    (restore's) instead of reading one from the weights directory."""
    if spec is None:
        return None
    from . import facescore as ffs
    try:
        if face_det is None:
            return ffs.load_face_scorer(spec["det_model"], spec["weights"], device, spec["mode"], spec["max_faces"], spec["face_size"])
        from .guided_diffusion.face_restoration_helper import FaceRestoreHelper
        helper = FaceRestoreHelper(face_size=spec["face_size"], det_model=spec["det_model"], device=device, face_det=face_det)
        return ffs.FaceScorer(helper, spec["mode"], max_faces=spec["max_faces"])
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"{command}: {exc}")


def identity_of(args, command):
    """The checkpoint of a parsed command line's --identity, or None without it; refused before any GPU work where there is no
    ground truth to compare with or it is not a file."""
    path = getattr(args, "identity", None)
    if path is None:
        return None
    if command != "evaluate" and not args.ground_truth:
        raise SystemExit(f"{command}: --identity compares the written frames with --ground-truth DIR; give one")
    if not os.path.isfile(path):
        raise SystemExit(f"{command}: --identity {path} is not a file (GFPGAN's / VQFR's arcface_resnet18.pth)")
    return path


def load_identity_of(path, device, command):
    """The ArcFace model of identity_of's result on ``device`` (None for None)."""
    if path is None:
        return None
    from . import identity as fid
    try:
        return fid.load_identity(path, device)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"{command}: {exc}")


def identity_tail(result):
    """``  ids X  id-drift Y (truth Z)`` of a result's mean where it holds them ('' without --identity)."""
    if "ids" not in result["mean"]:
        return ""
    from .identity import format_mean
    return format_mean(result["mean"])


def niqe_of(args, command, option="--niqe"):
    """The parameter file of a parsed command line's --niqe (--params of the niqe command), or None without it; refused
    before any GPU work where it is not a file."""
    path = getattr(args, "niqe" if option == "--niqe" else "params", None)
    if path is None:
        return None
    if not os.path.isfile(path):
        raise SystemExit(f"{command}: {option} {path} is not a file (BasicSR's niqe_pris_params.npz)")
    return path


def load_niqe_of(path, device, command):
    """The NIQE model of niqe_of's result on ``device`` (None for None)."""
    if path is None:
        return None
    from . import niqe as fnq
    try:
        return fnq.load_niqe(path, device)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"{command}: {exc}")


def lpips_of(args, command):
    """(net, weights directory) of a parsed command line's --lpips, or None without it; refusals before any GPU work."""
    net = getattr(args, "lpips", None)
    if net is None:
        return None
    if command != "evaluate" and not args.ground_truth:
        raise SystemExit(f"{command}: --lpips scores the written frames against --ground-truth DIR; give one")
    if not args.weights:
        raise SystemExit(f"{command}: --lpips {net} reads its trunk and linear layers from --weights DIR; give one")
    from . import lpips as flp
    missing = [p for p in flp.weight_files(net, args.weights) if not os.path.isfile(p)]
    if missing:
        raise SystemExit(f"{command}: --lpips {net} needs {' and '.join(missing)}")
    return net, args.weights


def load_lpips_of(spec, device, command):
    """The LPIPS model of lpips_of's result on ``device`` (None for None)."""
    if spec is None:
        return None
    from . import lpips as flp
    try:
        return flp.load_lpips(spec[0], spec[1], device)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"{command}: {exc}")


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
    r.add_argument("paths", nargs="+", metavar="PATH", help="VIDEO_DIR OUTPUT_DIR, or VIDEO_DIR... with --output-root; either may be a .y4m stream")
    r.add_argument("--output-root", default=None, metavar="DIR", help="write every VIDEO_DIR to DIR/<its name>")
    r.add_argument("--ground-truth", default=None, metavar="DIR",
                   help="clean frames of the video (with --output-root: a root holding one directory per video name): "
                        "after a video is written, log its mean PSNR / SSIM and write metrics.json next to the frames")
    _add_lpips(r, "with --ground-truth: also score", "; the files are read from --weights")
    _add_niqe(r, "after a video is written, log its mean and write into metrics.json")
    _add_identity(r, "with --ground-truth: also score")
    _add_warp_error(r, "after a video is written, log and write into metrics.json")
    _add_score_faces(r, "with --ground-truth: also score", own_detector=False)
    _add_hparams(r, pl.MAIN_DEFAULTS)
    _add_common(r)
    for name, demo in pl.DEMOS.items():
        d = sub.add_parser(name, help=f"{demo['task']}: {demo['video_path']} -> {demo['output_path']}")
        _add_hparams(d, dict(pl.MAIN_DEFAULTS, **{k: v for k, v in demo.items() if k in pl.MAIN_DEFAULTS}))
        _add_common(d)
    g = sub.add_parser("degrade", help="clean frames -> the task's degraded frames, with the operator restore assumes")
    g.add_argument("task", choices=pl.TASK_NAMES)
    g.add_argument("clean_dir", metavar="CLEAN_DIR", help="directory or .y4m stream of clean frames of one size valid for the task (--frame-size's rule)")
    g.add_argument("out_dir", metavar="OUT_DIR", help="receives {i:04d}.png at 1/f of the size; a path ending .y4m receives a stream")
    g.add_argument("--kernels", default=pl.DEFAULT_KERNELS, metavar="PATH",
                   help="the blur kernels .mat file (MATLAB v5) of the gaussian and jpeg tasks")
    g.add_argument("--jpeg-qf", type=int, default=None, metavar="Q", help="jpeg only: the codec's quality factor (default 60)")
    g.add_argument("--noise-sigma", type=float, default=0.0, metavar="S",
                   help="add white Gaussian noise of standard deviation S on the 0..255 scale before quantisation")
    g.add_argument("--seed", type=int, default=None, help="seed of the noise")
    g.add_argument("--device", default=None, help="default: cuda")
    _add_yuv(g, writes=True)
    e = sub.add_parser("evaluate", help="PSNR / SSIM of written frames against ground truth")
    e.add_argument("restored_dir", metavar="RESTORED_DIR")
    e.add_argument("truth_dir", metavar="TRUTH_DIR", help="frames are paired with RESTORED_DIR's in natural order")
    e.add_argument("--json", default=None, metavar="PATH", help="also write the per-frame values and the means as JSON")
    e.add_argument("--device", default=None, help="default: cuda")
    _add_lpips(e, "also score", "")
    e.add_argument("--weights", default=None, metavar="DIR", help="with --lpips or --score-faces: the directory that holds those files")
    _add_niqe(e, "also report")
    _add_identity(e, "also report")
    _add_warp_error(e, "also report")
    _add_cut_options(e, "with --warp-error: leave out the frame pairs that straddle a cut of TRUTH_DIR")
    _add_score_faces(e, "also report", own_detector=True)
    _add_yuv(e)
    w = sub.add_parser("warp-error", help="flow-warping error (temporal consistency) of written frames without ground truth: one "
                                          "line per frame and the means")
    w.add_argument("frames_dir", metavar="FRAMES_DIR", help="frames of at least 32 pixels a side")
    w.add_argument("--flow-weights", default=None, metavar="FILE", help=f"{WARP_FILE} (required)")
    w.add_argument("--json", default=None, metavar="PATH", help="also write the per-frame values and the means as JSON")
    w.add_argument("--device", default=None, help="default: cuda")
    _add_cut_options(w, "leave out the frame pairs that straddle a cut")
    _add_yuv(w)
    q = sub.add_parser("niqe", help="no-reference NIQE of written frames: one line per frame and the mean")
    q.add_argument("frames_dir", metavar="FRAMES_DIR", help="frames of at least two 96x96 blocks each")
    q.add_argument("--params", default=None, metavar="FILE", help="BasicSR's niqe_pris_params.npz (required)")
    q.add_argument("--json", default=None, metavar="PATH", help="also write the per-frame values and the mean as JSON")
    q.add_argument("--device", default=None, help="default: cuda")
    _add_yuv(q)
    i = sub.add_parser("interpolate", help="factor - 1 new frames between every two frames of a video (SuperSloMo or AMT-G)",
                       description="With a .y4m output the header's frame rate is the input's (or --fps) times --factor.  With .y4m in "
                                   "and out the original frames are re-encoded from their RGB bytes: payloads are not passed "
                                   "through byte for byte.")
    i.add_argument("src_dir", metavar="SRC_DIR", help="frames of one size")
    i.add_argument("out_dir", metavar="OUT_DIR", help="receives {i:04d}.png, factor * (T - 1) + 1 of them; a path ending .y4m receives a stream")
    i.add_argument("--factor", type=int, required=True, metavar="N", help="frame-rate multiplier, >= 2")
    i.add_argument("--interpolator", choices=("superslomo", "amt-g"), default="superslomo",
                   help="the network: SuperSloMo (default) or AMT-G (fp32 only; frames whose coarsest correlation level is "
                        "at least 2x2 or exactly 1x1)")
    i.add_argument("--weights", default="./checkpoints", metavar="DIR", help="directory with SuperSloMo.ckpt / amt-g.pth")
    i.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32", help="bf16: SuperSloMo only")
    i.add_argument("--device", default=None, help="default: cuda")
    i.add_argument("--ground-truth", default=None, metavar="DIR",
                   help="frames at the new rate: score the written frames against them (PSNR / SSIM)")
    i.add_argument("--json", default=None, metavar="PATH", help="with --ground-truth, --niqe or --warp-error: also write the values as JSON")
    _add_lpips(i, "with --ground-truth: also score", "; the files are read from --weights")
    _add_niqe(i, "also report")
    _add_identity(i, "with --ground-truth: also report")
    _add_warp_error(i, "also report")
    _add_cut_options(i, "synthesise nothing between the two frames of a cut: the in-betweens there are copies of the nearer "
                        "frame (--min-shot keeps its default of 4 here too)")
    _add_yuv(i, writes=True)
    s = sub.add_parser("scenes", help="find the hard cuts of a video (block-luma distances; heuristic defaults, not validated "
                                      "on real footage) and write the cuts file restore / interpolate --scene-cuts PATH read",
                       description="Print one line per shot and, with --json, write the cuts file that restore / interpolate "
                                   "--scene-cuts PATH read.  Hard cuts only: fades and dissolves are not detected.  The rule's "
                                   "defaults are heuristics chosen on synthetic sequences; they have NOT been validated on real "
                                   "footage, so check the shots it prints, tune the options below, or edit the cuts file.")
    s.add_argument("src_dir", metavar="SRC_DIR", help="frames of one size, at least 8 pixels a side")
    s.add_argument("--json", default=None, metavar="PATH", help='write {"cuts": [...], "distances": [...], "frames": n}')
    _add_cut_rule(s)
    s.add_argument("--device", default=None, help="default: cuda")
    _add_yuv(s)
    return ap


def rule_of(args, command):
    """find_cuts' keywords of a parsed command line (refused before any GPU work)."""
    rule = dict(threshold=args.cut_threshold, ratio=args.cut_ratio, radius=args.cut_radius, min_shot=args.min_shot)
    try:
        scenes.check_rule(**rule)
    except ValueError as exc:
        raise SystemExit(f"{command}: {exc}")
    return rule


def cuts_of(args, command, video_dirs):
    """The ``scene_cuts`` / ``cut_rule`` arguments of the drivers for a parsed command line: "off", "auto", or the checked
    cuts of --scene-cuts PATH (one file describes one video).  Refusals come before any GPU work."""
    rule = rule_of(args, command)
    mode = args.scene_cuts
    if mode in ("off", "auto"):
        return dict(scene_cuts=mode, cut_rule=rule)
    if len(video_dirs) != 1:
        raise SystemExit(f"{command}: --scene-cuts {mode} is the cuts file of one video; with --output-root and "
                         f"{len(video_dirs)} videos use --scene-cuts auto, or restore them one by one")
    from . import io as fio
    try:
        cuts = scenes.read_cuts(mode, len(fio.list_frames(video_dirs[0])))
    except (ValueError, OSError) as exc:
        raise SystemExit(f"{command}: {exc}")
    return dict(scene_cuts=cuts, cut_rule=rule)


def scenes_of(args):
    """The refusals of a parsed ``scenes`` command line, before any GPU work -> (frame paths, rule)."""
    rule = rule_of(args, "scenes")
    if not frames_exist(args.src_dir):
        raise SystemExit(f"scenes: {args.src_dir} is not a directory")
    from . import io as fio
    try:
        paths = fio.list_frames(args.src_dir)
        scenes.check_frames(paths)
    except ValueError as exc:
        raise SystemExit(f"scenes: {args.src_dir}: {exc}")
    return paths, rule


def _scenes(args):
    paths, rule = scenes_of(args)
    import torch
    torch.set_grad_enabled(False)
    try:
        result = scenes.detect_cuts_files(paths, args.device or "cuda", **rule)
    except ValueError as exc:
        raise SystemExit(f"scenes: {exc}")
    for line in scenes.describe(result):
        print(line)
    if args.json:
        scenes.write_cuts(args.json, result)
    return 0


def interpolate_of(args):
    """The refusals of a parsed ``interpolate`` command line, before any GPU work -> the frame paths."""
    from . import interpolate as fi
    try:
        paths, size = fi.check_source(args.src_dir, args.factor)
        fi.check_interpolator(args.interpolator, args.dtype, size)
    except ValueError as exc:
        raise SystemExit(f"interpolate: {exc}")
    if args.json and not args.ground_truth and not args.niqe and not args.warp_error:
        raise SystemExit("interpolate: --json writes the scores of --ground-truth DIR")
    if args.ground_truth and not frames_exist(args.ground_truth):
        raise SystemExit(f"interpolate: ground truth {args.ground_truth} is not a directory")
    lpips_of(args, "interpolate")
    niqe_of(args, "interpolate")
    identity_of(args, "interpolate")
    warp_of(args, "interpolate")
    return paths


def _interpolate(args):
    paths = interpolate_of(args)
    how = cuts_of(args, "interpolate", [args.src_dir])
    import torch
    from . import interpolate as fi
    torch.set_grad_enabled(False)
    device = args.device or "cuda"
    try:
        cuts, _ = scenes.resolve(how["scene_cuts"], paths, device, **how["cut_rule"])
        if cuts is not None:
            found = scenes.shots(len(paths), cuts)
            print(f"{args.src_dir}: {len(found)} shot{'s' if len(found) != 1 else ''} " + ", ".join(f"{a}..{b - 1}" for a, b in found))
        net = fi.load_interpolator(args.weights, device, args.dtype, name=args.interpolator)
        n = fi.interpolate_video_files(args.src_dir, args.out_dir, args.factor, net=net, device=device, cuts=cuts)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"interpolate: {exc}")
    print(f"wrote {n} frames to {args.out_dir} ({args.factor}x the rate of {args.src_dir})")
    niqe = load_niqe_of(niqe_of(args, "interpolate"), device, "interpolate")
    niqe_kw = {} if niqe is None else dict(niqe=niqe)
    warp = load_warp_of(warp_of(args, "interpolate"), device, "interpolate")
    if args.ground_truth:
        from . import metrics as fm
        from . import temporal as ftm
        model = load_lpips_of(lpips_of(args, "interpolate"), device, "interpolate")
        ident = load_identity_of(identity_of(args, "interpolate"), device, "interpolate")
        warp_kw = {} if warp is None else dict(warp_error=warp, warp_skip=ftm.straddling(cuts, args.factor))
        try:
            result = fm.evaluate_dirs(args.out_dir, args.ground_truth, device, **({} if model is None else dict(lpips=model)), **niqe_kw,
                                      **({} if ident is None else dict(identity=ident)), **warp_kw)
        except ValueError as exc:
            raise SystemExit(str(exc))
        for line in fm.format_report(result):
            print(line)
        if args.json:
            write_json(args.json, result)
    elif niqe is not None or warp is not None:
        result = None
        if niqe is not None:
            result = _report_niqe(args.out_dir, device, niqe, None, "interpolate")
        if warp is not None:
            from . import temporal as ftm
            got = _report_warp(args.out_dir, device, warp, ftm.straddling(cuts, args.factor), None, "interpolate")
            result = got if result is None else merge_results(result, got)
        if args.json:
            write_json(args.json, result)
    return 0


def merge_results(first, second):
    """Two results of one directory (frames in the same order) as one: every frame dict and the means hold both's keys."""
    return dict(frames=[dict(a, **b) for a, b in zip(first["frames"], second["frames"])], mean=dict(first["mean"], **second["mean"]),
                count=first["count"])


def _report_warp(frames_dir, device, model, skip, json_path, command):
    """Score a directory by its own flows: one line per frame, the means, and the JSON file where one is asked for.  ``skip``:
    the later frames of the pairs to leave out."""
    from . import temporal as ftm
    try:
        result = ftm.warp_error_dir(frames_dir, device, model, skip=skip)
    except ValueError as exc:                               # the messages name warp-error themselves
        raise SystemExit(str(exc) if command == "warp-error" else f"{command}: {exc}")
    for line in ftm.format_report(result):
        print(line)
    if json_path:
        write_json(json_path, result)
    return result


def warp_error_of(args):
    """The refusals of a parsed ``warp-error`` command line, before any GPU work -> (flow weights path, frame paths)."""
    if args.flow_weights is None:
        raise SystemExit(f"warp-error: --flow-weights FILE is required ({WARP_FILE}); nothing is shipped or downloaded")
    path = warp_of(args, "warp-error", option="--flow-weights")
    if not frames_exist(args.frames_dir):
        raise SystemExit(f"warp-error: {args.frames_dir} is not a directory")
    from . import io as fio
    from . import temporal as ftm
    try:
        paths = fio.list_frames(args.frames_dir)
    except ValueError as exc:
        raise SystemExit(f"warp-error: {exc}")
    if not paths:
        raise SystemExit(f"warp-error: no frame files in {args.frames_dir}")
    try:
        for p in paths:
            ftm.check_size(*fio.frame_size(p), what=p)
    except ValueError as exc:
        raise SystemExit(str(exc))
    return path, paths


def _warp_error(args):
    path, paths = warp_error_of(args)
    how = cuts_of(args, "warp-error", [args.frames_dir])
    import torch
    torch.set_grad_enabled(False)
    device = args.device or "cuda"
    skip = warp_skip_of(how["scene_cuts"], how["cut_rule"], paths, device, "warp-error")
    _report_warp(args.frames_dir, device, load_warp_of(path, device, "warp-error"), skip, args.json, "warp-error")
    return 0


def _report_niqe(frames_dir, device, model, json_path, command):
    """Score a directory without ground truth: one line per frame, the mean, and the JSON file where one is asked for."""
    from . import niqe as fnq
    try:
        result = fnq.niqe_dir(frames_dir, device, model)
    except ValueError as exc:                               # the messages name niqe themselves
        raise SystemExit(str(exc) if command == "niqe" else f"{command}: {exc}")
    for line in fnq.format_report(result):
        print(line)
    if json_path:
        write_json(json_path, result)
    return result


def _niqe(args):
    if args.params is None:
        raise SystemExit("niqe: --params FILE is required (BasicSR's niqe_pris_params.npz); nothing is shipped or downloaded")
    path = niqe_of(args, "niqe", option="--params")
    if not frames_exist(args.frames_dir):
        raise SystemExit(f"niqe: {args.frames_dir} is not a directory")
    import torch
    torch.set_grad_enabled(False)
    device = args.device or "cuda"
    _report_niqe(args.frames_dir, device, load_niqe_of(path, device, "niqe"), args.json, "niqe")
    return 0


def degrade_of(args):
    """The keyword arguments of degrade_video_files for a parsed ``degrade`` command line (refusals before any GPU work)."""
    if args.jpeg_qf is not None and args.task != "jpeg":
        raise SystemExit(f"degrade: --jpeg-qf belongs to the jpeg task, not {args.task}")
    if args.jpeg_qf is not None and not 1 <= args.jpeg_qf <= 100:
        raise SystemExit("degrade: --jpeg-qf is a quality factor in 1..100")
    if not args.noise_sigma >= 0:
        raise SystemExit("degrade: --noise-sigma must not be negative")
    if not frames_exist(args.clean_dir):
        raise SystemExit(f"degrade: {args.clean_dir} is not a directory")
    return dict(jpeg_qf=args.jpeg_qf, noise_sigma=args.noise_sigma, seed=args.seed)


def truth_of(args, jobs):
    """{output_dir: ground-truth directory} for the jobs of a parsed ``restore`` command line (with --output-root the
    directory of the video's name under --ground-truth), or None without --ground-truth."""
    root = getattr(args, "ground_truth", None)
    if root is None:
        return None
    if args.output_root is None:
        truth = [root]
    else:
        truth = [os.path.join(root, os.path.basename(os.path.normpath(v))) for v, _ in jobs]
    for t in truth:
        if not frames_exist(t):
            raise SystemExit(f"restore: ground truth {t} is not a directory")
    return {o: t for (_, o), t in zip(jobs, truth)}


def _degrade(args):
    kw = degrade_of(args)
    import torch
    from . import degrade as dg
    torch.set_grad_enabled(False)
    kernel = pl.load_blur_kernel(args.kernels) if "bicubic" not in args.task else None
    try:
        n = dg.degrade_video_files(args.task, args.clean_dir, args.out_dir, device=args.device or "cuda", kernel=kernel, **kw)
    except ValueError as exc:
        raise SystemExit(f"degrade: {exc}")
    print(f"degraded {n} frames of {args.clean_dir} ({args.task}) to {args.out_dir}")
    return 0


def write_json(path, result):
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def _evaluate(args):
    spec = lpips_of(args, "evaluate")
    niqe_path = niqe_of(args, "evaluate")
    ident_path = identity_of(args, "evaluate")
    warp_path = warp_of(args, "evaluate")
    face_spec = face_scorer_of(args, "evaluate")
    if warp_path is None and args.scene_cuts != "off":
        raise SystemExit("evaluate: --scene-cuts only tells --warp-error FILE which frame pairs to leave out; give one")
    how = cuts_of(args, "evaluate", [args.truth_dir]) if warp_path is not None else None
    import torch
    from . import metrics as fm
    torch.set_grad_enabled(False)
    model = load_lpips_of(spec, args.device or "cuda", "evaluate")
    niqe = load_niqe_of(niqe_path, args.device or "cuda", "evaluate")
    ident = load_identity_of(ident_path, args.device or "cuda", "evaluate")
    scorer = load_face_scorer_of(face_spec, args.device or "cuda", "evaluate")
    warp_kw = {}
    if warp_path is not None:
        from . import io as fio
        skip = warp_skip_of(how["scene_cuts"], how["cut_rule"], fio.list_frames(args.truth_dir), args.device or "cuda", "evaluate")
        warp_kw = dict(warp_error=load_warp_of(warp_path, args.device or "cuda", "evaluate"), warp_skip=skip)
    try:
        result = fm.evaluate_dirs(args.restored_dir, args.truth_dir, args.device or "cuda", **({} if model is None else dict(lpips=model)),
                                  **({} if niqe is None else dict(niqe=niqe)), **({} if ident is None else dict(identity=ident)), **warp_kw,
                                  **({} if scorer is None else dict(faces=scorer)))
    except ValueError as exc:
        raise SystemExit(str(exc))
    for line in fm.format_report(result):
        print(line)
    if args.json:
        write_json(args.json, result)
    return 0


def face_tail(result):
    """The face scores of a result's mean for restore's one-line log ('' without --score-faces)."""
    if "face_count" not in result["mean"]:
        return ""
    from .facescore import face_tail as tail
    return tail(result)


def niqe_tail(result):
    """``  niqe X`` of a result's mean where it holds one ('' without --niqe)."""
    if "niqe" not in result["mean"]:
        return ""
    from .niqe import format_value
    return format_value(result["mean"]["niqe"])


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
        if not frames_exist(v):
            raise SystemExit(f"restore: {v} is not a directory")
        if os.path.isfile(v):                           # a stream: its header's refusals come before any GPU work
            from . import io as fio
            try:
                fio.list_frames(v)
            except ValueError as exc:
                raise SystemExit(f"restore: {exc}")
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
        if getattr(args, "tile", "off") != "off":               # tile_of holds the tiled frame's refusals
            from .video import frame_hw
            return frame_hw(size)
        return pl.check_frame_size(task, size)
    except ValueError as exc:
        raise SystemExit(f"restore: {exc}")


def tile_of(args, task, size):
    """build_pipeline's ``tile`` / ``tile_overlap`` keywords for a parsed command line ({} for --tile off, the default: the
    call of before).  --tile HxW tiles; --tile auto tiles at 512x512 only where the frame is refused whole.  The refusals
    of the tiled frame come here, before any GPU work."""
    if getattr(args, "tile", "off") == "off":
        return {}
    try:
        tile = pl.parse_tile(args.tile)
        if tile is None:
            return {}
        if args.frame_size is None:
            raise ValueError("--tile needs --frame-size HxW or auto (tiles are cut from rectangular frames that are not resized)")
        if tile == "auto":
            from .video import FRAME_SLICE_LEN
            if not pl.needs_tiling(task, size, frames=FRAME_SLICE_LEN, parser=args.parser, dtype=args.dtype):
                return {}
            tile = DEFAULT_TILE
        _, tile = pl.check_tiled_frame_size(task, size, tile, args.tile_overlap, parser=args.parser, dtype=args.dtype)
        return dict(tile=tile, tile_overlap=args.tile_overlap)
    except ValueError as exc:
        raise SystemExit(f"restore: {exc}")


def main(argv=None):
    args = make_parser().parse_args(argv)
    apply_yuv(args)
    if args.command == "degrade":
        return _degrade(args)
    if args.command == "evaluate":
        return _evaluate(args)
    if args.command == "interpolate":
        return _interpolate(args)
    if args.command == "scenes":
        return _scenes(args)
    if args.command == "niqe":
        return _niqe(args)
    if args.command == "warp-error":
        return _warp_error(args)
    task, jobs = jobs_of(args)
    truth = truth_of(args, jobs)
    lpips_spec = lpips_of(args, "restore")
    niqe_path = niqe_of(args, "restore")
    ident_path = identity_of(args, "restore")
    warp_path = warp_of(args, "restore")
    face_spec = face_scorer_of(args, "restore")
    prior = prior_of(args)
    faces = faces_of(args)
    size = size_of(args, task, jobs)
    tiling = tile_of(args, task, size)
    how = cuts_of(args, "restore", [v for v, _ in jobs])
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
                              parser=args.parser, **tiling)
        hp = dict(aligned=args.aligned, t_start=args.t_start, jpeg_qf=args.jpeg_qf, w=args.w, tau=args.tau,
                  rho=args.rho, noise_level=args.noise_level, zeta=args.zeta, seed=args.seed)
        hp.update(faces)
        hp.update(how)
        lpips_model = load_lpips_of(lpips_spec, device, "restore")
        score_kw = {} if lpips_model is None else dict(lpips=lpips_model)      # without the option, the call of before
        niqe_model = load_niqe_of(niqe_path, device, "restore")
        if niqe_model is not None:
            score_kw["niqe"] = niqe_model
        ident_model = load_identity_of(ident_path, device, "restore")
        if ident_model is not None:
            score_kw["identity"] = ident_model
        warp_model = load_warp_of(warp_path, device, "restore")
        if face_spec is not None:                       # the detector restore built is the one that scores
            score_kw["faces"] = load_face_scorer_of(face_spec, device, "restore", face_det=p.face_helper.face_det)

        def warp_skip(v):
            """The pairs across the cuts restore_video_files worked with: the same rule on the same degraded frames."""
            from . import io as fio
            return warp_skip_of(how["scene_cuts"], how["cut_rule"], fio.list_frames(v), device, "restore")

        def restore_one(v, o):
            n = p.restore_video_files(v, o, **hp)
            if truth is not None:
                from . import metrics as fm
                warp_kw = {} if warp_model is None else dict(warp_error=warp_model, warp_skip=warp_skip(v))
                result = fm.evaluate_dirs(o, truth[o], device, **score_kw, **warp_kw)
                print(f"{o}: mean of {result['count']} frames  psnr {result['mean']['psnr']:.4f}  "
                      f"ssim {result['mean']['ssim']:.4f}" + (f"  lpips {result['mean']['lpips']:.4f}" if lpips_model is not None else "")
                      + niqe_tail(result) + identity_tail(result) + warp_tail(result) + face_tail(result))
                write_json(metrics_path(o), result)
            elif niqe_model is not None or warp_model is not None:      # footage without a clean original: the no-reference scores alone
                from . import niqe as fnq
                from . import temporal as ftm
                try:
                    result = fnq.niqe_dir(o, device, niqe_model) if niqe_model is not None else None
                    if warp_model is not None:
                        got = ftm.warp_error_dir(o, device, warp_model, skip=warp_skip(v))
                        result = got if result is None else merge_results(result, got)
                except ValueError as exc:               # frames too small for a score: the video is written, only the score is not
                    print(f"{o}: no score: {exc}")
                    return n
                head = (f"{o}: mean of {result['mean']['niqe_frames']} of {result['count']} frames" if niqe_model is not None
                        else f"{o}: mean of {result['mean']['warp_err_pairs']} pairs of {result['count']} frames")
                print(head + niqe_tail(result) + warp_tail(result))
                write_json(metrics_path(o), result)
            return n
        pl.restore_many(jobs, restore_one)
    finally:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
