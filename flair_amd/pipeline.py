"""A restoration task wired end to end: what ``main()`` of the reference's ``scripts/video_sample.py`` builds.

``build_pipeline(task, weights_dir, device=...)`` returns a ``Pipeline`` holding the diffusion (``DIFFUSION_CONFIG``,
:35-75, respaced ``"100"`` uniform, :266-283), the network (``MODEL_CONFIG``, :77-156, bf16 through
``convert_to_fp16``), the task operator (``get_A_func``, :190-247) and its data-consistency step (``RESTORE_FUNC``,
:174-199), the CodeFormer prior (:405-414, :450-452) or, on request, the reference's RestoreFormer or VQFR v2 prior
(guided_diffusion/restoreformer.py, guided_diffusion/vqfr.py), the face-parsing weights of the bicubic tasks (:427-444) and a
``FaceRestoreHelper`` built on a loaded RetinaFace and face parser (ParseNet or BiSeNet, :351).  Every network reads its checkpoint from
``weights_dir`` under the reference's file names; a missing file is an error, never a randomly initialised network.

Everything per step runs on the HIP kernels the pieces already use; this module is host-side wiring only.  The
command line (``python -m flair_amd``) is ``flair_amd.__main__``.
"""
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import io as fio
from . import ops
from . import parallel
from . import scenes
from . import tiling
from . import video
from . import workload as wl
from .guided_diffusion import gaussian_diffusion as gd

TASK_NAMES = ("x8_bicubic", "x16_bicubic", "gaussian", "jpeg")

# scripts/video_sample.py:35-75
_BICUBIC_DIFFUSION = dict(diffusion_steps=2000, noise_schedule="face_bicubic", model_mean_type=gd.ModelMeanType.EPSILON,
                          model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE, rescale_timesteps=False)
_BLUR_DIFFUSION = dict(diffusion_steps=1000, noise_schedule="face_blur", model_mean_type=gd.ModelMeanType.EPSILON,
                       model_var_type=gd.ModelVarType.LEARNED_RANGE, loss_type=gd.LossType.RESCALED_MSE,
                       rescale_timesteps=False)
DIFFUSION_CONFIG = {"x8_bicubic": dict(_BICUBIC_DIFFUSION), "x16_bicubic": dict(_BICUBIC_DIFFUSION),
                    "gaussian": dict(_BLUR_DIFFUSION), "jpeg": dict(_BLUR_DIFFUSION)}

# scripts/video_sample.py:77-156 (the 512 x 512 networks of the released checkpoints)
_SR3_CONFIG = dict(image_size=512, in_channel=6, out_channel=3, inner_channel=64, norm_groups=16,
                   channel_mults=(1, 2, 4, 8, 16), attn_res=(64, 32), vsrpp_res=(512, 256), spatial_attn=False,
                   temporal_attn=True, res_blocks=1, dropout=0.0, dtype=torch.float16, cross_frame_module=True,
                   use_checkpoint=True, num_frames=7, head_dim=64)
_BLUR_CONFIG = dict(image_size=512, in_channels=6, model_channels=128, out_channels=6, num_res_blocks=2,
                    attention_resolutions=(512 // 32, 512 // 16, 512 // 8), rnn_resolutions=(1, 2),
                    channel_mult=(0.5, 1, 1, 2, 2, 4, 4), use_fp16=True, num_head_channels=64, resblock_updown=True,
                    use_scale_shift_norm=True, temporal_block=True, use_checkpoint=True)
MODEL_CONFIG = {"x8_bicubic": dict(_SR3_CONFIG), "x16_bicubic": dict(_SR3_CONFIG),
                "gaussian": dict(_BLUR_CONFIG), "jpeg": dict(_BLUR_CONFIG)}

# main()'s defaults (scripts/video_sample.py:249-263) and the four demo commands (:500-556)
MAIN_DEFAULTS = dict(t_start=-1, jpeg_qf=-1, w=0.5, tau=5, aligned=False, rho=0.5, noise_level=12.75, zeta=-1.0)
DEMOS = {
    "x8-bicubic-demo": dict(task="x8_bicubic", video_path="./data/x8_bicubic", output_path="./output/x8_bicubic",
                            w=0.85, rho=0.85, noise_level=0.0),
    "x16-bicubic-demo": dict(task="x16_bicubic", video_path="./data/x16_bicubic", output_path="./output/x16_bicubic",
                             w=0.7, rho=0.85, noise_level=0.0),
    "gaussian-demo": dict(task="gaussian", video_path="./data/gaussian", output_path="./output/gaussian",
                          w=0.75, rho=0.25, noise_level=2.55, zeta=1.0),
    "jpeg-demo": dict(task="jpeg", video_path="./data/jpeg", output_path="./output/jpeg",
                      w=0.5, rho=0.5, noise_level=12.75, zeta=1.0, jpeg_qf=60),
}

# checkpoint file names of the reference (CKPT_PATH, :165-171; the facelib downloads, facelib/detection/__init__.py,
# facelib/parsing/__init__.py)
DETECTOR_FILES = {"retinaface_resnet50": ("resnet50", "detection_Resnet50_Final.pth"),
                  "retinaface_mobile0.25": ("mobile0.25", "detection_mobilenet0.25_Final.pth"),
                  "YOLOv5l": ("yolov5l", "yolov5l-face.pth"), "YOLOv5n": ("yolov5n", "yolov5n-face.pth")}
PARSER_FILE = "parsing_parsenet.pth"
# the face parsers build_pipeline(parser=...) offers (facelib/parsing/__init__.py:8-25), with their checkpoint files
PARSER_FILES = {"parsenet": PARSER_FILE, "bisenet": "parsing_bisenet.pth"}
CODEFORMER_FILE = "codeformer.pth"
# the auxiliary face priors build_pipeline(prior=...) offers, with their checkpoint files (RestoreFormer: the RestoreFormer
# project's release name; guided_diffusion/restoreformer.py of the reference)
PRIOR_FILES = {"codeformer": CODEFORMER_FILE, "restoreformer": "RestoreFormer.ckpt", "vqfrv2": "VQFR_v2.pth"}
PRIOR_LABELS = {"codeformer": "CodeFormer", "restoreformer": "RestoreFormer", "vqfrv2": "VQFR"}
# frame interpolation (flair_amd.interpolate): the published SuperSloMo checkpoint, or the flat state dict of the reference module
INTERPOLATOR_FILES = {"superslomo": "SuperSloMo.ckpt"}
# the second interpolator, AMT-G: the file the reference's authors load, {"state_dict": ...} (or the flat state dict)
AMT_INTERPOLATOR_FILES = {"amt-g": "amt-g.pth"}
# VQFRv2's constructor arguments in the VQFR project's published v2 release configuration (its options file for VQFR v2:
# base_channels 64, channel_multipliers [1, 2, 2, 4, 4, 8], two encoder and two decoder blocks with attention, code_dim
# 256, inpfeat_dim 32, align_opt cond_channels 32 / deformable_groups 4, "Predict" code selection).  The reference tree
# does not record them and they cannot be checked offline; a wrong value fails loudly in the strict load of
# VQFR_v2.pth, and prior_kwargs overrides any of them.
VQFR_CONFIG = dict(base_channels=64, channel_multipliers=(1, 2, 2, 4, 4, 8), num_enc_blocks=2, use_enc_attention=True,
                   num_dec_blocks=2, use_dec_attention=True, code_dim=256, inpfeat_dim=32, code_selection_mode="Predict",
                   align_opt={"cond_channels": 32, "deformable_groups": 4})
DEFAULT_KERNELS = "./miscs/kernels_12.mat"


def model_file(task):
    return f"flair_{task}.pt"


def _check_task(task):
    if task not in TASK_NAMES:
        raise ValueError(f"unknown task {task!r}: one of {', '.join(TASK_NAMES)}")


# the face parsers run on whole frames for the bicubic tasks' propagation weights: ParseNet(in_size=512) halves the frame
# four times, BiSeNet's ResNet-18 five times
PARSER_MULTIPLE = {"parsenet": 16, "bisenet": 32}
JPEG_MCU = 16                       # the codec works on whole 16 x 16 MCUs of the degraded (low-resolution) frames
SR3_MIN_FLOW_SIDE = 64              # sr3's propagation levels estimate flows on frames of at least 64 pixels a side


def frame_multiple(task):
    """What H and W of a rectangular frame must be multiples of: the least common multiple of the network's deepest
    level (one halving per entry of channel_mult(s) after the first: the layout is the checkpoint's, whatever the
    frame), the operator's factor, and -- for the blur tasks, whose operator may run the codec -- the 16-pixel MCU on the
    low-resolution grid.  64 for gaussian / jpeg, 16 for the bicubic tasks with the shipped configurations."""
    import math
    _check_task(task)
    cfg = MODEL_CONFIG[task]
    factor = wl.TASKS[task]["factor"]
    if "bicubic" in task:
        return math.lcm(2 ** (len(cfg["channel_mults"]) - 1), factor)
    return math.lcm(2 ** (len(cfg["channel_mult"]) - 1), factor, JPEG_MCU * factor)


def frame_minimum(task):
    """The smallest side of a rectangular frame: sr3's coarsest propagation level (image_size / vsrpp_res halvings)
    still needs SR3_MIN_FLOW_SIDE pixels; the blur tasks need one multiple."""
    m = frame_multiple(task)
    if "bicubic" in task:
        cfg = MODEL_CONFIG[task]
        deepest = max(cfg["image_size"] // r for r in cfg["vsrpp_res"])
        return -(-SR3_MIN_FLOW_SIDE * deepest // m) * m
    return m


def parse_frame_size(text):
    """``"HxW"`` (also ``H,W``) -> (H, W); ``"auto"`` -> ``"auto"`` (the first frame's (h*f, w*f), resolved by
    auto_frame_size)."""
    t = str(text).strip().lower()
    if t == "auto":
        return "auto"
    parts = t.replace(",", "x").split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts) or min(int(p) for p in parts) <= 0:
        raise ValueError(f"frame size {text!r}: HxW with positive integers (height first), or auto")
    return int(parts[0]), int(parts[1])


def auto_frame_size(task, video_path):
    """--frame-size auto: (h*f, w*f) of the first frame file of ``video_path`` (only its header is read)."""
    _check_task(task)
    paths = fio.list_frames(video_path)
    if not paths:
        raise ValueError(f"{video_path}: no frame files to take the frame size from")
    h, w = fio.frame_size(paths[0])
    f = wl.TASKS[task]["factor"]
    return h * f, w * f


def check_frame_size(task, size, frames=None, parser=None, dtype="bf16"):
    """Refuse a rectangular frame size the task cannot restore: not a multiple of frame_multiple(task) (the two
    nearest valid sizes are named), below frame_minimum(task), not a multiple of the parser's own stride (bicubic
    tasks: the parser sees whole frames), or -- given the window length ``frames`` -- beyond the kernels' 32-bit
    offsets (video.check_clip_elements)."""
    _check_task(task)
    H, W = video.frame_hw(size)
    m, lo = frame_multiple(task), frame_minimum(task)
    bad = [(n, v) for n, v in (("H", H), ("W", W)) if v % m or v < lo]
    if bad:
        near = lambda v: (max(lo, v // m * m), max(lo, -(-v // m) * m))                    # noqa: E731
        (h0, h1), (w0, w1) = near(H), near(W)
        raise ValueError(f"{task}: frame size {H}x{W} is not valid: H and W must be multiples of {m} and at least {lo}; "
                         f"the nearest valid sizes are {h0}x{w0} and {h1}x{w1} (frames are not padded or cropped for you)")
    if parser is not None and "bicubic" in task:
        pm = PARSER_MULTIPLE[parser]
        if H % pm or W % pm:
            raise ValueError(f"{task}: the {parser} parser reads whole frames for the propagation weights and needs H and W "
                             f"to be multiples of {pm}; {H}x{W} is not")
    if frames is not None:
        video.check_clip_elements(frames, H, W, torch.float32 if dtype == "fp32" else torch.bfloat16)
    return H, W


def tile_multiple(task, parser=None):
    """What a tile's sides must be multiples of: frame_multiple(task) and, for the bicubic tasks, the parser's stride (the parser
    reads every tile's init frames for the propagation weights)."""
    import math
    m = frame_multiple(task)
    return math.lcm(m, PARSER_MULTIPLE[parser]) if parser is not None and "bicubic" in task else m


def parse_tile(text):
    """--tile: ``"off"`` -> None, ``"auto"`` -> ``"auto"``, ``"HxW"`` -> (H, W)."""
    t = str(text).strip().lower()
    if t == "off":
        return None
    if t == "auto":
        return "auto"
    try:
        return parse_frame_size(t)
    except ValueError:
        raise ValueError(f"tile {text!r}: off, auto or HxW with positive integers (height first)") from None


def check_tiled_frame_size(task, size, tile, tile_overlap=tiling.DEFAULT_OVERLAP, frames=None, parser=None, dtype="bf16"):
    """Refuse a frame size tiled denoising cannot restore, and choose the tile: per axis min(requested, the largest multiple of
    tile_multiple(task, parser) the axis holds).  The frame's H and W must be multiples of the task's factor (tile origins lie on
    the low-resolution grid) and hold at least one tile of frame_minimum(task); the jpeg task keeps frame_multiple(task) for the
    FRAME, because the codec's MCU grid is the frame's and not the tile's.  The tile itself then passes check_frame_size: its
    multiples, the parser's stride and -- given ``frames`` -- the window's 32-bit limits hold for the tile, and
    video.check_tiled_frame_elements for the frame.  Returns ((H, W), (th, tw))."""
    _check_task(task)
    H, W = video.frame_hw(size)
    f = wl.TASKS[task]["factor"]
    if H % f or W % f:
        raise ValueError(f"{task}: tiled frames of {H}x{W}: H and W must be multiples of the factor {f} (the degraded frames are "
                         f"{H // f}x{W // f} at best; frames are not padded or cropped for you)")
    if task == "jpeg" and (H % frame_multiple(task) or W % frame_multiple(task)):
        raise ValueError(f"jpeg: tiled frames of {H}x{W}: H and W must stay multiples of {frame_multiple(task)}, because the codec's "
                         "16x16 MCU grid on the degraded frames is the frame's, not the tile's")
    m, lo = tile_multiple(task, parser), frame_minimum(task)
    req = video.frame_hw(tile)
    th, tw = tiling.tile_side(H, req[0], m), tiling.tile_side(W, req[1], m)
    if min(th, tw) < lo or min(th, tw) < m:
        raise ValueError(f"{task}: frames of {H}x{W} with tiles of {req[0]}x{req[1]}: a tile's sides are multiples of {m} and at least "
                         f"{lo}, and the frame must hold one; frames smaller than a tile are not padded")
    check_frame_size(task, (th, tw), frames=frames, parser=parser, dtype=dtype)
    p = int(tile_overlap)
    if p < f or p % f or p >= min(th, tw):
        raise ValueError(f"{task}: tile overlap {tile_overlap}: a positive multiple of the factor {f} below the tile's sides {th}x{tw}")
    if frames is not None:
        video.check_tiled_frame_elements(task, frames, H, W, tiling.make_plan((H, W), (th, tw), p, f))
    return (H, W), (th, tw)


def needs_tiling(task, size, frames=None, parser=None, dtype="bf16"):
    """--tile auto: True when check_frame_size refuses the frame whole."""
    try:
        check_frame_size(task, size, frames=frames, parser=parser, dtype=dtype)
    except ValueError:
        return True
    return False


def model_config(task, size=512):
    """MODEL_CONFIG[task] for clips of ``size`` x ``size``: the attention / propagation resolutions scale with the size
    as in workload.sr3_config / script_util.blur_unet_config (at 512 this is the reference's table).  A pair (H, W)
    returns the literal 512 layout: which levels carry attention and BasicVSR++ is a property of the checkpoint, not of
    the frame, and both networks take their flow resolutions from the clip at run time."""
    _check_task(task)
    cfg = dict(MODEL_CONFIG[task])
    if video.is_pair(size):
        return cfg
    cfg["image_size"] = size
    if "bicubic" in task:
        cfg["attn_res"] = (size // 8, size // 16)
        cfg["vsrpp_res"] = (size, size // 2)
    else:
        cfg["attention_resolutions"] = (size // 32, size // 16, size // 8)
    return cfg


def create_diffusion(task, steps=100):
    """The SpacedDiffusion of main() (video_sample.py:266-283): DIFFUSION_CONFIG[task] respaced ``str(steps)``, uniform."""
    from .guided_diffusion.respace import SpacedDiffusion, space_timesteps
    _check_task(task)
    cfg = dict(DIFFUSION_CONFIG[task])
    n = cfg.pop("diffusion_steps")
    cfg["use_timesteps"] = space_timesteps(n, str(steps), "uniform")
    cfg["betas"] = gd.get_named_beta_schedule(cfg["noise_schedule"], n)
    return SpacedDiffusion(**cfg)


def load_blur_kernel(path):
    """``kernels[0, 3]`` of the reference's ``miscs/kernels_12.mat`` (video_sample.py:231-242) as a float32 array.
    Read with scipy.io.loadmat, which reads MATLAB v5 files (the reference's is one); a v7.3 (HDF5) file is refused
    with a message that says so."""
    import scipy.io
    from scipy.io.matlab import matfile_version
    if not os.path.isfile(path):
        raise FileNotFoundError(f"blur kernel file {path} not found (the reference's miscs/kernels_12.mat; --kernels PATH)")
    with open(path, "rb") as f:
        try:
            major, minor = matfile_version(f)
        except Exception as exc:
            raise ValueError(f"{path}: not a MATLAB .mat file ({exc})") from exc
    if major == 2:
        raise ValueError(f"{path}: a MATLAB v7.3 (HDF5) .mat file; only v5 .mat files are read (scipy.io.loadmat): "
                         "save the kernels with MATLAB's save(..., '-v7') or scipy.io.savemat")
    if major != 1:
        raise ValueError(f"{path}: a MATLAB v{4 if major == 0 else major} .mat file; only v5 .mat files are read")
    mat = scipy.io.loadmat(path)
    if "kernels" not in mat:
        raise ValueError(f"{path}: no 'kernels' variable")
    return np.asarray(mat["kernels"][0, 3], dtype=np.float32)


def prior_name(prior):
    """build_pipeline's ``prior`` argument -> a key of PRIOR_FILES, or None for the identity prior: True means
    "codeformer" and False / None the identity, as before a second prior existed."""
    if prior is True:
        return "codeformer"
    if prior is False or prior is None:
        return None
    if isinstance(prior, str) and prior in PRIOR_FILES:
        return prior
    raise ValueError(f"prior={prior!r}: one of {', '.join(map(repr, PRIOR_FILES))}, True (= 'codeformer'), False or None")


def _required_files(task, weights_dir, det_model, prior, parser="parsenet"):
    files = [model_file(task)]
    name = prior_name(prior)
    if name is not None:
        files.append(PRIOR_FILES[name])
    files += [DETECTOR_FILES[det_model][1], PARSER_FILES[parser]]
    return [os.path.join(str(weights_dir), f) for f in files]


class Pipeline:
    """One task's networks and operators on one device; ``restore_video_files`` runs the reference's window loop over a
    directory of frames (flair_amd.io.restore_video_files)."""

    def __init__(self, task, model, diffusion, A_func, face_helper, aux_model, vsrpp_weights_fn, size, device, prior=None,
                 tile=None, tile_overlap=tiling.DEFAULT_OVERLAP):
        self.task, self.model, self.diffusion, self.A_func = task, model, diffusion, A_func
        self.face_helper, self.aux_model, self.vsrpp_weights_fn = face_helper, aux_model, vsrpp_weights_fn
        self.size, self.device, self.prior = size, torch.device(device), prior
        self.tile, self.tile_overlap = tile, tile_overlap          # tiled denoising (flair_amd.tiling): None = whole frames

    def check_aligned(self, aligned):
        """aligned=True hands whole frames to the prior, which restores 512 x 512 faces: with a size pair and a prior the
        frames must be exactly that."""
        if aligned and self.prior is not None and video.is_pair(self.size) and video.frame_hw(self.size) != (512, 512):
            H, W = video.frame_hw(self.size)
            raise ValueError(f"aligned=True runs the {PRIOR_LABELS[self.prior]} prior on whole frames, which must be 512x512 "
                             f"aligned faces; frames of {H}x{W} need aligned=False (faces are detected and cropped) or "
                             "prior=False")

    def restore_fn_for(self, jpeg_qf=-1):
        """RESTORE_FUNC[task] bound to the window's normalised degraded frames (video_sample.py:174-199, :455-459).
        As in the reference only the jpeg task passes ``jpeg_qf`` on (:456-457)."""
        A = self.A_func
        if "bicubic" in self.task:
            def for_window(deg_n):                        # bicubic_restore: A_pinv(A(x) - d)
                T = deg_n.shape[1]
                d_flat = deg_n[0].contiguous().reshape(T, -1)
                return lambda x0: A.A_pinv(ops.axpby(A.A(x0.reshape(T, -1)), d_flat, 1.0, -1.0)).reshape(x0.shape)
            return for_window
        from .guided_diffusion.jpeg import jpeg_decode, jpeg_encode
        qf = jpeg_qf if self.task == "jpeg" else -1

        def for_window(deg_n):                            # gaussian_restore
            lr = deg_n[0].contiguous()
            return lambda x0: A.A_pinv(lr, x0, jpeg_encode=(lambda im: jpeg_encode(im, qf)) if qf != -1 else None,
                                       jpeg_decode=(lambda im: jpeg_decode(im, qf)) if qf != -1 else None)
        return for_window

    def restore_video_files(self, video_path, output_path, *, aligned=MAIN_DEFAULTS["aligned"], t_start=-1, jpeg_qf=-1,
                            w=MAIN_DEFAULTS["w"], tau=5, rho=MAIN_DEFAULTS["rho"],
                            noise_level=MAIN_DEFAULTS["noise_level"], zeta=MAIN_DEFAULTS["zeta"], seed=None,
                            faces="largest", max_faces=None, scene_cuts="off", cut_rule=None, log=print):
        """Frame files of ``video_path`` -> ``output_path/{i:04d}.png`` (video_sample.py:334-492).  ``seed`` seeds
        torch's generators first (the reference does not seed).  ``faces="all"`` (aligned=False only): the prior runs on
        every detected face, at most ``max_faces`` per frame, and frames may have none (video.restore_window).
        ``scene_cuts`` (ours): "off" restores the directory as one shot, like the reference; "auto" finds the cuts of
        the degraded input frames first (scenes.detect_cuts_files with ``cut_rule``, find_cuts' keywords: heuristic
        defaults, not validated on real footage); a list of cuts or the path of a cuts file is used as given.  Every
        shot is then restored on its own (io.restore_video_files' ``cuts``), and one line with the shots is logged.
        Returns the number of frames written."""
        self.check_aligned(aligned)
        paths = fio.list_frames(video_path)
        cuts, _ = scenes.resolve(scene_cuts, paths, self.device, **(cut_rule or {}))
        if cuts is not None:
            found = scenes.shots(len(paths), cuts)
            log(f"{video_path}: {len(found)} shot{'s' if len(found) != 1 else ''} "
                + ", ".join(f"{a}..{b - 1}" for a, b in found))
        if seed is not None:
            torch.manual_seed(int(seed))
        hp = dict(w=w, rho=rho, noise_level=noise_level, zeta=zeta)
        return fio.restore_video_files(
            self.task, video_path, output_path, self.model, self.diffusion, self.restore_fn_for(jpeg_qf), size=self.size,
            device=self.device, aligned=aligned, face_helper=self.face_helper, aux_model=self.aux_model,
            vsrpp_weights_fn=self.vsrpp_weights_fn, hp=hp, tau=tau, t_start=t_start, faces=faces, max_faces=max_faces,
            cuts=cuts, **({} if self.tile is None else dict(tile=self.tile, tile_overlap=self.tile_overlap)))


def build_operator(task, size, device, kernel=None):
    """The task operator (get_A_func, video_sample.py:190-247) on ``device``: SRConv with the 4f-tap bicubic kernel and
    reflect padding for the bicubic tasks (``size``: an int or a pair (H, W)); the pseudoSR operator of ``kernel`` (the
    25 x 25 blur array of load_blur_kernel) at factor 4 for gaussian and jpeg.  build_pipeline's data-consistency step and
    flair_amd.degrade.Degrader apply the same object."""
    _check_task(task)
    if "bicubic" in task:
        from .guided_diffusion.restore_util import SRConv
        factor = wl.TASKS[task]["factor"]
        return SRConv(wl.bicubic_taps(factor), 3, size, device, stride=factor)
    from .guided_diffusion import pseudoSR as psr
    if kernel is None:
        raise ValueError(f"{task}: the blur operator needs the 25 x 25 blur kernel (load_blur_kernel)")
    conf = psr.Get_pseudoSR_Conf(4)
    conf.sigmoid_range_limit = False
    conf.input_range = np.array(None)
    return psr.pseudoSR(conf, upscale_kernel=kernel, kernel_indx=10).WrapArchitecture_PyTorch().to(device)


def build_pipeline(task, weights_dir, *, device, size=512, dtype="bf16", steps=100, kernels_path=None, prior=True,
                   det_model="retinaface_resnet50", model_kwargs=None, graph=True, prior_kwargs=None, parser="parsenet",
                   tile=None, tile_overlap=tiling.DEFAULT_OVERLAP):
    """Build ``task``'s Pipeline from the checkpoints in ``weights_dir``: ``flair_{task}.pt``, the prior's checkpoint,
    the detector's ``detection_Resnet50_Final.pth`` / ``detection_mobilenet0.25_Final.pth`` / ``yolov5l-face.pth`` /
    ``yolov5n-face.pth`` (``det_model``: the RetinaFace bodies or the YOLOv5-face detectors) and the parser's
    ``parsing_parsenet.pth`` (``parser="parsenet"``, the default) or ``parsing_bisenet.pth`` (``parser="bisenet"``),
    all loaded strictly with ``weights_only=True``.  ``size``: an int S restores S x S frames as the reference does (every
    input is resized to S x S; a prior needs S = 512); a pair (H, W) restores rectangular frames: H and W multiples of
    frame_multiple(task), degraded frames of exactly (H/f, W/f), the network in its literal 512 layout, and the face
    helper at face size 512 whenever a prior is configured, whatever the frame size (check_frame_size holds the
    refusals).  ``tile`` = (th, tw) (needs a size pair; None, the default, restores whole frames exactly as before): the network
    runs on overlapping tiles sharing at least ``tile_overlap`` pixels, clipped per axis to the frame, and the tile outputs are
    blended at every step (flair_amd.tiling); check_tiled_frame_size holds the refusals, and check_frame_size then applies to
    the tile.  ``model_kwargs`` overrides entries of MODEL_CONFIG[task]
    (checkpoints of other widths).  ``kernels_path``: the reference's ``miscs/kernels_12.mat`` (gaussian and jpeg tasks).

    ``prior``: ``"codeformer"`` (or True, the default) reads ``codeformer.pth`` (its ``params_ema``);
    ``"restoreformer"`` reads ``RestoreFormer.ckpt`` (a plain state dict, or a training checkpoint whose ``state_dict``
    holds the network under ``vqvae.``); ``"vqfrv2"`` reads ``VQFR_v2.pth`` (a state dict, or BasicSR's
    ``params_ema`` / ``params``) into VQFRv2 built with VQFR_CONFIG; False / None selects the identity prior and reads
    none of them.  ``prior_kwargs`` overrides the prior's constructor arguments (RestoreFormer's ``head_size`` is not
    recorded in a checkpoint); for VQFR it may also hold ``fidelity_ratio`` (default 1.0, the reference forward's),
    which is passed to every call of the prior instead of the constructor.

    In an initialised torch.distributed world only rank 0 reads the files; the other ranks receive its weights (the
    flagship network in its kernel-native packed form, parallel.broadcast_packed_weights; the small networks as fp32
    parameters, parallel.broadcast_weights)."""
    from .checkpoint import load_reference_checkpoint
    from .guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from .guided_diffusion.parsenet import ParseNet
    from .guided_diffusion.retinaface import RetinaFace
    _check_task(task)
    if det_model not in DETECTOR_FILES:
        raise ValueError(f"det_model={det_model!r}: one of {', '.join(DETECTOR_FILES)}")
    if parser not in PARSER_FILES:
        raise ValueError(f"parser={parser!r}: one of {', '.join(PARSER_FILES)}")
    if dtype not in ("bf16", "fp32"):
        raise ValueError(f"dtype={dtype!r}: 'bf16' or 'fp32'")
    prior = prior_name(prior)
    pair = video.is_pair(size)
    if tile is not None:
        if not pair:
            raise ValueError(f"tile={tile!r} needs a size pair (H, W): size={size!r} resizes every frame to a square")
        size, tile = check_tiled_frame_size(task, size, tile, tile_overlap, frames=video.FRAME_SLICE_LEN, parser=parser, dtype=dtype)
    elif pair:
        size = check_frame_size(task, size, frames=video.FRAME_SLICE_LEN, parser=parser, dtype=dtype)
    if prior is not None and not pair and size != 512:
        raise ValueError(f"the {PRIOR_LABELS[prior]} prior restores 512 x 512 faces (its code grid is 16 x 16): size={size} needs "
                         "prior=False")
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    reads = not distributed or dist.get_rank() == 0
    files = _required_files(task, weights_dir, det_model, prior, parser)
    if reads:
        for f in files:
            if not os.path.isfile(f):
                raise FileNotFoundError(f"checkpoint {os.path.basename(f)} not found in {weights_dir} ({f})")
    kernel = None
    if "bicubic" not in task:
        kernel = load_blur_kernel(kernels_path if kernels_path is not None else DEFAULT_KERNELS)
    device = torch.device(device)

    def load(net, path):
        if reads:
            load_reference_checkpoint(net, path, strict=True)
        return net

    # the network (video_sample.py:285-289)
    cfg = model_config(task, size)
    cfg.update({k: tuple(v) if isinstance(v, list) else v for k, v in (model_kwargs or {}).items()})   # JSON lists
    if "bicubic" in task:
        from .guided_diffusion.sr3 import UNet as Net
    else:
        from .guided_diffusion.unet_new import UNetModel as Net
    model = load(Net(**cfg), files[0]).to(device).eval()
    if dtype == "bf16":
        model.convert_to_fp16()
    else:
        model.convert_to_fp32()
    # the face helper's networks (facelib/detection/__init__.py, facelib/parsing/__init__.py)
    det_path, parser_path = files[-2], files[-1]
    if det_model.startswith("YOLOv5"):                  # init_yolov5face_model, facelib/detection/__init__.py:51-81
        from .guided_diffusion.yolov5face import YoloDetector
        det = YoloDetector(DETECTOR_FILES[det_model][0], device="cpu", allow_random_init=not reads)
        det_net = det.detector = load(det.detector, det_path).to(device).eval()
    else:
        det = det_net = load(RetinaFace(network_name=DETECTOR_FILES[det_model][0], half=False, device="cpu"), det_path).to(device).eval()
    det.device = device
    if parser == "bisenet":
        from .guided_diffusion.bisenet import BiSeNet
        parser = load(BiSeNet(num_class=19), parser_path).to(device).eval()
    else:
        parser = load(ParseNet(in_size=512, out_size=512, parsing_ch=19), parser_path).to(device).eval()
    gan = None
    pkw = {k: tuple(v) if isinstance(v, list) else v for k, v in (prior_kwargs or {}).items()}   # JSON lists
    if prior == "codeformer":
        from .guided_diffusion.codeformer import CodeFormer
        gan = CodeFormer(**dict(dict(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                                     connect_list=["32", "64", "128", "256"]), **pkw))
        gan = load(gan, files[1]).to(device).eval()
    elif prior == "restoreformer":
        from .guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
        gan = load(VQVAEGANMultiHeadTransformer(**pkw), files[1]).to(device).eval()
    elif prior == "vqfrv2":
        from .guided_diffusion.vqfr import VQFRv2
        fidelity_ratio = float(pkw.pop("fidelity_ratio", 1.0))
        gan = load(VQFRv2(**dict(VQFR_CONFIG, **pkw)), files[1]).to(device).eval()
    if distributed:
        parallel.broadcast_packed_weights(model, src=0)
        for net in (det_net, parser, gan):
            if net is not None:
                parallel.broadcast_weights(net, src=0)
    if graph and hasattr(model, "enable_hip_graph") and device.type == "cuda":
        model.enable_hip_graph()
    A_func = build_operator(task, size, device, kernel)
    weights_fn = wl.parsenet_weights_fn(parser, task) if "bicubic" in task else None
    # with a size pair the face size is the prior's 512, not the frame's
    helper = FaceRestoreHelper(face_size=512 if pair else size, det_model=det_model, device=device, face_det=det, face_parse=parser)
    aux = wl.identity_aux
    if prior == "codeformer":
        aux = wl.codeformer_aux(gan)
    elif prior == "restoreformer":
        aux = wl.restoreformer_aux(gan)
    elif prior == "vqfrv2":
        aux = wl.vqfr_aux(gan, fidelity_ratio)
    diffusion = create_diffusion(task, steps)
    return Pipeline(task, model, diffusion, A_func, helper, aux, weights_fn, size, device, prior=prior, tile=tile,
                    tile_overlap=tile_overlap)


def restore_many(jobs, restore_one, *, log=print):
    """Restore independent videos: ``jobs`` is a list of (video_dir, output_dir); rank r of an initialised
    torch.distributed world takes ``parallel.clips_for_rank(len(jobs), r, world)`` (every video is written by exactly
    one rank), ``restore_one(video_dir, output_dir) -> frames written``.  Rank 0 logs one summary line.
    Returns this rank's (video_dir, frames) list."""
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
    outs = [os.path.abspath(str(o)) for _, o in jobs]
    if len(set(outs)) != len(outs):
        raise ValueError("two videos would be written to the same output directory")
    if distributed:
        dist.barrier()
    t0 = time.perf_counter()
    done = []
    for k in parallel.clips_for_rank(len(jobs), rank, world):
        video_dir, out_dir = jobs[k]
        done.append((str(video_dir), int(restore_one(video_dir, out_dir))))
    every = parallel.gather_results(done, dst=0)
    secs = time.perf_counter() - t0
    if rank == 0:
        frames = sum(n for part in every for _, n in part)
        videos = sum(len(part) for part in every)
        log(f"restored {videos} videos, {frames} frames in {secs:.2f} s ({frames / max(secs, 1e-9):.2f} frames/s) "
            f"on {world} process{'es' if world > 1 else ''}")
    return done
