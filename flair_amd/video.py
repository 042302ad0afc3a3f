"""Sliding-window restoration of a whole video: the caller side of the sampling hot path.

Mirror of the window loop of the reference's ``scripts/video_sample.py:334-492`` (SURVEY.md section
8f, "next" row 2) without its file I/O: the frames are cut into windows of ``FRAME_SLICE_LEN`` with
``OVERLAP`` frames shared between neighbours (``more_itertools.windowed`` semantics,
video_sample.py:361-368), every window is initialised by the task's ``INIT_FUNC`` (:158-163),
sampled with ``diffusion.sample`` and stitched: all but the first window pin their first ``OVERLAP``
frames to the previous window's result (``prev_recon``, gaussian_diffusion.py:497-505) and
contribute only the frames after them (:481-485).

Everything tensor-valued runs through the HIP kernels (resize / clamp / sampler); the face-parsing
weights and the CodeFormer prior are passed in as callables (``vsrpp_weights_fn`` / ``aux_model``; the HIP
versions are ``workload.parsenet_weights_fn(ParseNet(...), task)`` and ``workload.codeformer_aux(CodeFormer(...))``).
"""
import numbers

import torch

from . import ops
from . import scenes
from . import tiling
from . import workload as wl

FRAME_SLICE_LEN = 10   # scripts/video_sample.py:202
OVERLAP = 3            # scripts/video_sample.py:203


def window_indices(n_frames, length=FRAME_SLICE_LEN, overlap=OVERLAP):
    """Frame indices of every window: ``more_itertools.windowed(range(n), length, step=length-overlap)``
    with the ``None`` padding of the last window dropped (video_sample.py:361-368)."""
    if length <= 0 or not 0 <= overlap < length:
        raise ValueError("need 0 <= overlap < length")
    step = length - overlap
    if n_frames <= 0:
        return []
    if n_frames <= length:
        return [list(range(n_frames))]
    return [list(range(s, min(s + length, n_frames))) for s in range(0, n_frames - length + step, step)]


def window_plan(n_frames, cuts=None, length=FRAME_SLICE_LEN, overlap=OVERLAP):
    """[(indices, starts_shot)] of every window of a video with scene cuts (flair_amd.scenes; ours, the reference restores one
    continuous clip): ``window_indices`` applied to every shot and shifted to video indices, so that no window spans a
    cut.  The first window of a shot has ``starts_shot`` True: it gets no ``prev_recon`` and contributes all its frames.
    Without cuts the plan is window_indices with only the first window starting a shot."""
    plan = []
    for start, stop in (scenes.shots(n_frames, cuts) if n_frames > 0 else []):
        for k, idx in enumerate(window_indices(stop - start, length, overlap)):
            plan.append(([start + i for i in idx], k == 0))
    if not plan:
        window_indices(n_frames, length, overlap)                 # its refusals hold for an empty video too
    return plan


_consts = {}


def _const(dev, value):
    """Cached 4-element device constant for flair_affine_channels_f32's per-channel terms."""
    key = (dev, float(value))
    if key not in _consts:
        _consts[key] = torch.full((4,), float(value), device=dev)
    return _consts[key]


def _to_clip(x):
    N, C, h, w = x.shape
    clip = torch.zeros((N, h, w, 4), dtype=torch.float32, device=x.device)
    return ops.nchw_to_clip(x.float().contiguous(), clip, 0)


def _affine(clip, a, b, lo, hi, sub=0.0, mul=1.0):
    """(clamp(x*a + b, lo, hi) - sub) * mul on the 3 image channels of an f32 clip tensor -> (N,3,H,W)."""
    out = torch.zeros_like(clip)
    ops.affine_channels(clip, 3, a, b, lo, hi, _const(clip.device, sub), _const(clip.device, mul), out)
    return ops.clip_to_nchw(out, 3)


def is_pair(size):
    """A frame size is an int S (the reference's square frames: every input is resized to S x S) or a pair (H, W)
    (rectangular mode: degraded frames must be exactly (H/f, W/f); nothing is resized on the user's behalf)."""
    return not isinstance(size, numbers.Integral)


def frame_hw(size):
    """(H, W) of a frame size given as an int or a pair."""
    if not is_pair(size):
        return int(size), int(size)
    hw = tuple(int(v) for v in size)
    if len(hw) != 2 or min(hw) <= 0:
        raise ValueError(f"size={size!r}: an int or a pair (H, W) of positive ints")
    return hw


def check_degraded(task, degraded_hw, size):
    """Pair mode: data consistency needs y = A(x) on the pixel grid, so the degraded frames must be exactly
    (H/f, W/f) for the task's factor f.  Raised before anything is launched, naming both sizes."""
    H, W = frame_hw(size)
    f = wl.TASKS[task]["factor"]
    h, w = (int(v) for v in degraded_hw)
    if H % f or W % f or (h, w) != (H // f, W // f):
        raise ValueError(f"{task} restores {H}x{W} frames from degraded frames of {H // f}x{W // f} (factor {f}), got "
                         f"{h}x{w}: with a size pair nothing is resized; give size=({h * f}, {w * f}) or frames of the right size")


# Size limits of a window ("Rectangular frames").  The element-wise kernels index with 64 bits; the
# convolution, chain, alignment and warp entries address single frames (or SPyNet's small clips) through buffer
# descriptors with 32-bit byte offsets and refuse what does not fit.  Two of those checks bound a window:
#   * one frame of the alignment branch's offset / mask tensor (27 * deform_groups = 432 channels) must stay below the
#     convolution entry's 1 GiB per frame: H * W * 432 * bytes-per-element < 2^30;
#   * SPyNet warps the T - 1 frame pairs of a clip in one call over a 4-channel f32 clip that must stay below 2 GiB:
#     (T - 1) * H * W * 16 < 2^31.
# The Python layer refuses a window beyond either before anything is launched, so no entry is ever asked to wrap.
OFFSET_CHANNELS = 27 * 16           # deform_groups = 16: the shipped layouts; offset_channels(model) reads a network's own
FRAME_BYTES_LIMIT = 2 ** 30
FLOW_CLIP_BYTES_LIMIT = 2 ** 31


def offset_channels(model):
    """27 * deform_groups of the widest alignment module of ``model`` (a network built with other groups through
    model_kwargs has another per-frame limit); OFFSET_CHANNELS for an object without such modules (test stand-ins)."""
    mods = model.modules() if hasattr(model, "modules") else ()
    groups = [int(m.deform_groups) for m in mods if hasattr(m, "deform_groups")]
    return 27 * max(groups) if groups else OFFSET_CHANNELS


def max_frame_pixels(dtype=torch.bfloat16, channels=OFFSET_CHANNELS):
    """Largest H*W of one frame: with the shipped 432 offset channels 1 242 756 pixels in bf16 (e.g. 960 x 1280),
    621 378 in f32 (e.g. 640 x 960)."""
    esz = 4 if dtype == torch.float32 else 2
    return (FRAME_BYTES_LIMIT - 1) // (channels * esz)


def max_clip_pixels():
    """Largest (T - 1) * H * W of one window (SPyNet's flow clip), whatever the network's dtype."""
    return (FLOW_CLIP_BYTES_LIMIT - 1) // 16


def check_clip_elements(T, H, W, dtype=torch.bfloat16, channels=OFFSET_CHANNELS):
    name = "f32" if dtype == torch.float32 else "bf16"
    if H * W > max_frame_pixels(dtype, channels):
        raise ValueError(f"frames of {H}x{W} are {H * W} pixels; the {name} kernels address one frame of the alignment "
                         f"offsets ({channels} channels) with 32-bit byte offsets below 1 GiB: at most "
                         f"{max_frame_pixels(dtype, channels)} pixels a frame")
    if (T - 1) * H * W > max_clip_pixels():
        raise ValueError(f"a window of {T} frames of {H}x{W} gives SPyNet a clip of {(T - 1) * H * W} pixels; its warp "
                         f"addresses at most {max_clip_pixels()} (2 GiB): use shorter windows")


# Tiled denoising (flair_amd.tiling; DESIGN section 7, "Tiled denoising").  With ``tile=`` the two limits above bound the TILE, and
# the frame is bounded only by the whole-frame consumers of the sampler path.  All of them index with 64 bits; what is left:
#   * ops.resize (init_frames, rnn_input), flair_warp_affine_cubic_indexed and paste_faces compute pixel coordinates in f32, where
#     integers + 0.5 are exact below 2^23: a side of at most 2^23 - 1 pixels;
#   * the blur tasks' operator: flair_depthwise_filter's inverse filter on the low-resolution grid counts its T * 3 * ceil(h / 32) *
#     ceil(w / 32) workgroups in an int, the codec (flair_jpeg_roundtrip_hw) one workgroup per 10 MCUs of 16 x 16: below 2^31,
#     which the blend's limit below implies (it launches 5 and 40 times as many workgroups on the same window);
#   * the bicubic tasks' operator: flair_matmul_f32 puts ceil(H / 16) row blocks and the T * 3 planes on grid axes of at most 65535;
#   * flair_tile_gather_f32 / flair_tile_blend_f32: one launch of at most 2^31 - 1 workgroups of 256 threads, 4 pixels a thread
#     (the blend's counted per frame, the gather's per plane of a tile: check_tiled_frame_elements checks both);
#   * nchw_to_clip / clip_to_nchw, affine_channels and the sampler's element-wise kernels are grid-stride loops over 64-bit
#     counts: no limit of their own.
MAX_TILED_SIDE = 2 ** 23 - 1
MAX_WORKGROUPS = 2 ** 31 - 1
MATMUL_GRID_AXIS = 65535


def check_tiled_frame_elements(task, T, H, W, plan=None):
    """Refuse, by the consumer's name, a window of ``T`` whole frames of H x W that a whole-frame kernel of the tiled sampler path
    cannot index (the list above).  ``plan`` (a tiling.TilePlan): also the gather's launch, whose workgroups are counted per
    plane of a tile (three channels: x, low_res_input, rnn_input).  Raised before the first launch."""
    if plan is not None and plan.n_tiles * T * 3 * -(-plan.th * -(-plan.tw // 4) // 256) > MAX_WORKGROUPS:
        raise ValueError(f"a window of {T} frames in {plan.n_tiles} tiles of {plan.th}x{plan.tw} exceeds one launch of "
                         f"flair_tile_gather_f32 ({MAX_WORKGROUPS} workgroups): use shorter windows or larger tiles")
    if max(H, W) > MAX_TILED_SIDE:
        raise ValueError(f"frames of {H}x{W}: ops.resize and the face warps (flair_warp_affine_cubic_indexed, paste_faces) compute "
                         f"pixel coordinates in f32, exact up to {MAX_TILED_SIDE} pixels a side")
    if T * -(-H * -(-W // 4) // 256) > MAX_WORKGROUPS:
        raise ValueError(f"a window of {T} frames of {H}x{W} exceeds one launch of flair_tile_blend_f32 ({MAX_WORKGROUPS} workgroups "
                         "of 1024 pixels): use shorter windows")
    if "bicubic" in task and (-(-H // 16) > MATMUL_GRID_AXIS or T * 3 > MATMUL_GRID_AXIS):
        raise ValueError(f"a window of {T} frames of {H}x{W}: the bicubic operator's flair_matmul_f32 takes at most "
                         f"{MATMUL_GRID_AXIS * 16} rows and {MATMUL_GRID_AXIS} planes")


def tiled_model(task, model, size, tile, tile_overlap, frames, vsrpp_weights_fn=None):
    """``model`` wrapped for tiled denoising of ``size`` = (H, W) frames with tiles of ``tile`` = (th, tw) sharing at least
    ``tile_overlap`` pixels (flair_amd.tiling.TiledModel).  Origins are multiples of the task's factor, so H, W, th, tw and the
    overlap must be.  The window limits of check_clip_elements hold for the tile, check_tiled_frame_elements for the frame; a
    frame smaller than one tile is refused (frames are not padded)."""
    if not is_pair(size):
        raise ValueError(f"tile={tile!r} needs a size pair (H, W); size={size!r} resizes every frame to a square")
    (H, W), (th, tw) = frame_hw(size), frame_hw(tile)
    if th > H or tw > W:
        raise ValueError(f"{task}: frames of {H}x{W} are smaller than one tile of {th}x{tw}; frames are not padded: use a smaller tile")
    try:
        plan = tiling.make_plan((H, W), (th, tw), tile_overlap, wl.TASKS[task]["factor"])
    except ValueError as exc:
        raise ValueError(f"{task}: tiles of {th}x{tw} with overlap {tile_overlap} on frames of {H}x{W}: {exc}") from exc
    check_clip_elements(frames, th, tw, dtype=getattr(model, "dtype", torch.bfloat16), channels=offset_channels(model))
    check_tiled_frame_elements(task, frames, H, W, plan)
    return tiling.TiledModel(model, plan, vsrpp_weights_fn)


def init_frames(task, degraded01, size):
    """INIT_FUNC (video_sample.py:158-163) followed by the (x - 0.5) / 0.5 of :372-373: bicubic for the
    bicubic tasks, ``area`` (= block replication when upscaling by an integer factor) for the blur tasks,
    clamped to [0, 1], returned in [-1, 1].  ``size``: an int S -> (S, S), or a pair (H, W) with degraded frames of
    exactly (H/f, W/f): the same resize modes, the blur tasks' replication being by exactly f."""
    H, W = frame_hw(size)
    if is_pair(size):
        check_degraded(task, degraded01.shape[-2:], size)
    clip = _to_clip(degraded01)
    if "bicubic" in task:
        mode = ops.RESIZE_BICUBIC
    else:
        if W % degraded01.shape[-1] or H % degraded01.shape[-2]:
            raise ValueError("area initialisation needs an integer upscaling factor")
        mode = ops.RESIZE_NEAREST
    big = ops.resize(clip, (H, W), mode, channels=3)
    return _affine(big, 1.0, 0.0, 0.0, 1.0, sub=0.5, mul=2.0)


def normalise(degraded01):
    """(x - 0.5) / 0.5 (video_sample.py:372); returns the NCHW images and their clip form."""
    clip = _to_clip(degraded01)
    out = torch.zeros_like(clip)
    ops.affine_channels(clip, 3, 2.0, -1.0, float("-inf"), float("inf"), _const(clip.device, 0.0),
                        _const(clip.device, 1.0), out)
    return ops.clip_to_nchw(out, 3), out


def rnn_input(degraded_norm_clip, size):
    """The flow-network input of the blur tasks (video_sample.py:406-425): the two ``VF.normalize`` calls
    cancel around the bicubic resize, what remains is resize + clamp to [-1, 1].  ``size``: an int or a pair (H, W)."""
    big = ops.resize(degraded_norm_clip, frame_hw(size), ops.RESIZE_BICUBIC, channels=3)
    return _affine(big, 1.0, 0.0, -1.0, 1.0)


FACES = ("largest", "all")


def window_faces(face_helper, init_n, window_index=0, frame_indices=None, faces="largest", max_faces=None,
                 any_frame_size=False):
    """Affine matrices of the window's faces (video_sample.py:446-448): one per frame, estimated on the normalised init
    frames ((T, 3, S, S) in [-1, 1]) with the largest face of every frame kept.  A frame without a face is a
    ValueError naming the window and the frame's index in the video (the reference fails later, inside the sampler).
    ``faces="all"`` (extension) returns (matrices, face_frames) instead: every face of every frame, largest first and at
    most ``max_faces`` per frame, face k in frame face_frames[k] of the window; frames without a face are simply absent
    from the list, and a window without any gives ([], []).
    ``any_frame_size`` (the pair mode of restore_window): the frames need not have the helper's face size -- the faces
    are cropped to it and pasted back through FaceRestoreHelper.paste_faces, for which the caller passes face_frames."""
    if faces not in FACES:
        raise ValueError(f"faces={faces!r}: one of {', '.join(FACES)}")
    T = init_n.shape[0]
    frames = list(frame_indices) if frame_indices is not None else list(range(T))
    if not any_frame_size and (init_n.shape[-1] != face_helper.face_size[0] or init_n.shape[-2] != face_helper.face_size[1]):
        raise ValueError(f"aligned=False pastes faces at the helper's face size {face_helper.face_size}: frames of "
                         f"{tuple(init_n.shape[-2:])} must match it (video_sample.py restores 512 x 512 frames)")
    if faces == "all":
        _, mats, face_frames = face_helper.get_crop_faces_all(init_n, eye_dist_threshold=0.1, max_faces=max_faces)
        return mats, face_frames
    _, mats, idx = face_helper.get_crop_face(init_n, only_keep_largest=True, eye_dist_threshold=0.1)
    if mats is None or len(idx) < T:
        # the helper pairs the detector's per-frame lists with the frames in order, so a frame without a detection
        # shifts the indices it returns: find the faceless frames one by one (this path only raises)
        missing = [frames[k] for k in range(T)
                   if face_helper.get_crop_face(init_n[k:k + 1].contiguous(), only_keep_largest=True,
                                                eye_dist_threshold=0.1)[1] is None]
        raise ValueError(f"aligned=False: window {window_index} (frames {frames[0]}..{frames[-1]}) has no face in "
                         f"frame(s) {missing or 'unknown'} of the video; every frame of an unaligned window needs one")
    return mats


def restore_window(task, degraded01, model, diffusion, restore_fn_for, *, size, prev_recon=None, overlap=OVERLAP,
                   window_index=0, aux_model=wl.identity_aux, vsrpp_weights_fn=None, hp=None, tau=5, t_start=-1,
                   noise_fn=None, q_noise_fn=None, aligned=True, face_helper=None, frame_indices=None, faces="largest",
                   max_faces=None, tile=None, tile_overlap=tiling.DEFAULT_OVERLAP):
    """One window of the loop (video_sample.py:371-485).  degraded01: (1, T, 3, h, w) in [0, 1] on the GPU;
    prev_recon: the previous window's last ``overlap`` results ((1, <=overlap, 3, S, S), [-1, 1] domain) or None.
    ``aligned=False`` (the reference's default, :275) detects the faces of the window's init frames with
    ``face_helper`` before the first step (:446-448) and runs the prior on their crops (:460-479); frame_indices
    (the window's frames in the video) only name frames in its errors.  ``faces="all"`` (with aligned=False) runs the
    prior on every detected face, at most ``max_faces`` per frame, and lets frames -- or the whole window -- have none.
    ``size``: an int S (every frame is resized to S x S, as in the reference) or a pair (H, W): the degraded frames must
    be exactly (H/f, W/f), and aligned=False crops the faces to the helper's face size -- which is then independent of
    the frame size -- and pastes them back with paste_faces (faces="largest" passes face_frames = 0..T-1 itself).
    ``tile`` = (th, tw) (ours; needs a size pair): the network runs on overlapping th x tw tiles sharing at least ``tile_overlap``
    pixels and the tile outputs are blended into the whole-frame model output at every step (tiled_model); everything else of
    the step stays on whole frames.  The window limits then hold for the tile, and ``vsrpp_weights_fn`` is applied per tile.
    Returns (frames01 of the frames this window contributes, (T', 3, H, W) in [0, 1]; next prev_recon)."""
    hp = hp or wl.TASKS[task]
    dev = degraded01.device
    wi = window_index
    pair = is_pair(size)
    if pair:                                                                      # refusals come before the first launch
        check_degraded(task, degraded01.shape[-2:], size)
        if tile is None:
            check_clip_elements(degraded01.shape[1], *frame_hw(size), dtype=getattr(model, "dtype", torch.bfloat16),
                                channels=offset_channels(model))
    if tile is not None:
        model = tiled_model(task, model, size, tile, tile_overlap, degraded01.shape[1], vsrpp_weights_fn)
    deg = degraded01[0].float().contiguous()                                      # (T,3,h,w) in [0,1]
    T = deg.shape[0]
    init_n = init_frames(task, deg, size)[None]                                   # (1,T,3,S,S) in [-1,1]
    mats, face_frames = None, None
    if faces not in FACES:
        raise ValueError(f"faces={faces!r}: one of {', '.join(FACES)}")
    if not aligned:
        if face_helper is None:
            raise ValueError("aligned=False needs face_helper (a FaceRestoreHelper with a detector and a face parser)")
        if faces == "all":
            mats, face_frames = window_faces(face_helper, init_n[0], wi, frame_indices, faces="all", max_faces=max_faces,
                                             any_frame_size=pair)
        else:
            mats = window_faces(face_helper, init_n[0], wi, frame_indices, any_frame_size=pair)
            if pair:
                face_frames = list(range(T))
    deg_n, deg_n_clip = normalise(deg)
    deg_n = deg_n[None]
    t0 = diffusion.num_timesteps - 1 if t_start == -1 else t_start
    tt = torch.full((T,), t0, device=dev, dtype=torch.long)
    qn = q_noise_fn(wi, init_n[0]) if q_noise_fn is not None else None
    noise = diffusion.q_sample(init_n[0].contiguous(), tt, noise=qn)
    if tile is not None:                          # the tiled model parses every tile's init frames itself
        weights = None if vsrpp_weights_fn is not None else 1.0
    else:
        weights = vsrpp_weights_fn(init_n) if vsrpp_weights_fn is not None else 1.0
    kwargs = dict(low_res_input=init_n, num_frames=T, enable_cross_frames=True, vsrpp_weights=weights)
    if "bicubic" not in task:
        kwargs["rnn_input"] = rnn_input(deg_n_clip, size)[None]
    sample = diffusion.sample(
        model, noise, model_kwargs=kwargs, device=dev, progress=False, clip_denoised=True,
        restore_fn=restore_fn_for(deg_n), post_fn=None, face_restore_helper=None if aligned else face_helper,
        aux_model=aux_model, w=hp["w"], tau=tau, affine_matrices=mats, aligned=aligned, sample_mode="ddpm", rho=hp["rho"],
        noise_level=hp["noise_level"], prev_recon=prev_recon, zeta=hp["zeta"], t_start=t_start,
        noise_fn=(lambda it, like, _wi=wi: noise_fn(_wi, it, like)) if noise_fn is not None else None,
        **({} if face_frames is None else dict(face_frames=face_frames)))
    keep = sample if prev_recon is None else sample[overlap:]                    # (T',3,S,S), [-1,1] domain
    nxt = keep[-overlap:].clone()[None] if overlap > 0 else None                 # (1,<=overlap,3,S,S), :481-483
    frames01 = _affine(_to_clip(keep.contiguous()), 0.5, 0.5, 0.0, 1.0)          # (clamp(x,-1,1)+1)/2
    return frames01, nxt


def restore_video(task, degraded01, model, diffusion, restore_fn_for, *, size, aux_model=wl.identity_aux,
                  vsrpp_weights_fn=None, hp=None, tau=5, t_start=-1, length=FRAME_SLICE_LEN, overlap=OVERLAP,
                  noise_fn=None, q_noise_fn=None, aligned=True, face_helper=None, faces="largest", max_faces=None, cuts=None,
                  tile=None, tile_overlap=tiling.DEFAULT_OVERLAP):
    """degraded01: (1, N, 3, h, w) frames in [0, 1] on the GPU.  Returns (N, 3, H, W) in [0, 1] for ``size`` = an int
    S (H = W = S) or a pair (H, W) (see restore_window).

    restore_fn_for(degraded_norm_window (1,T,3,h,w)) -> restore_fn(x0) is the data-consistency
    operator of the window (video_sample.py:455-459); vsrpp_weights_fn(init_norm (1,T,3,S,S)) supplies
    the per-pixel propagation weights of the bicubic tasks (face parsing, :427-444) and defaults to 1.0;
    noise_fn / q_noise_fn(window_index, like) let tests share one noise tape with the oracle; aligned / face_helper /
    faces / max_faces / tile / tile_overlap: see restore_window.  ``cuts`` (ours; None = one shot, exactly the reference's loop): frames that start
    a new shot (flair_amd.scenes).  Every shot is windowed on its own (window_plan): its first window gets no prev_recon and
    contributes all its frames, while window_index keeps counting over the whole video (noise_fn / q_noise_fn are keyed by it).
    (File-to-file form with decode / upload / encode overlapped: flair_amd.io.restore_video_files.)"""
    dev = degraded01.device
    n_frames = degraded01.shape[1]
    prev_recon = None
    if is_pair(size):
        check_degraded(task, degraded01.shape[-2:], size)
    out = torch.empty((n_frames, 3, *frame_hw(size)), dtype=torch.float32, device=dev)
    filled = 0
    for wi, (idx, starts_shot) in enumerate(window_plan(n_frames, cuts, length, overlap)):
        frames01, prev_recon = restore_window(
            task, degraded01[:, idx[0]:idx[-1] + 1], model, diffusion, restore_fn_for, size=size,
            prev_recon=None if starts_shot else prev_recon, overlap=overlap, window_index=wi, aux_model=aux_model,
            vsrpp_weights_fn=vsrpp_weights_fn, hp=hp, tau=tau, t_start=t_start, noise_fn=noise_fn, q_noise_fn=q_noise_fn,
            aligned=aligned, face_helper=face_helper, frame_indices=idx, faces=faces, max_faces=max_faces,
            **({} if tile is None else dict(tile=tile, tile_overlap=tile_overlap)))
        out[filled:filled + frames01.shape[0]].copy_(frames01)
        filled += frames01.shape[0]
    return out[:filled]
