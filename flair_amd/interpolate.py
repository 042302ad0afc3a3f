"""Change the frame rate of a video: ``python -m flair_amd interpolate SRC_DIR OUT_DIR --factor N``.

The reference ships the networks (``guided_diffusion/superslomo.py``, ``guided_diffusion/amt.py``) and no driver for them;
this is the driver.  Every pair of neighbouring frames gets ``factor - 1`` frames between them from ``SuperSloMo`` (the
default) or ``AMT`` (``--interpolator amt-g``) on the HIP kernels, so ``T`` frames become ``factor * (T - 1) + 1``.  The
original frames pass through untouched: files are written from their decoded bytes.  With ``cuts`` (flair_amd.scenes,
``--scene-cuts``) nothing is synthesised between the two frames of a cut: the in-betweens there are copies of the nearer one.

``load_interpolator`` returns a module with ``forward(frame0, frame1, factor) -> (B, factor - 1, 3, H, W)`` on frames in
[-1, 1] and a ``MULTIPLE`` attribute (32 for SuperSloMo; 1 for AMT, which pads to multiples of 16 itself, centred).
"""
import os

import torch
import torch.nn.functional as F

from . import io as fio
from . import pipeline as pl
from . import scenes

_PARTS = (("state_dictFC", "flow_estimator."), ("state_dictAT", "interp."))
# name -> checkpoint file under the weights directory
INTERPOLATORS = {**pl.INTERPOLATOR_FILES, **pl.AMT_INTERPOLATOR_FILES}


def amt_state_dict(obj, what="checkpoint"):
    """The two forms of an AMT checkpoint -> the flat state dict of the module: the published file's {"state_dict": ...}
    (what the reference's ``AMT(pretrained=...)`` loads), or the flat dict itself."""
    if not isinstance(obj, dict):
        raise ValueError(f"{what}: not a state dict")
    if "state_dict" in obj:
        obj = obj["state_dict"]
        if not isinstance(obj, dict):
            raise ValueError(f"{what}: holds no state dict under state_dict")
    if not all(isinstance(v, torch.Tensor) for v in obj.values()):
        raise ValueError(f"{what}: not a tensor state dict")
    return obj


def check_interpolator(name, dtype="fp32", size=None):
    """What an interpolator refuses, before any GPU work: its name, its dtype and (AMT) the frame size (h, w)."""
    if name not in INTERPOLATORS:
        raise ValueError(f"interpolator={name!r}: one of {', '.join(INTERPOLATORS)}")
    if dtype not in ("fp32", "bf16"):
        raise ValueError(f"dtype={dtype!r}: fp32 or bf16")
    if name == "amt-g":
        from .guided_diffusion import amt
        if dtype != "fp32":
            raise ValueError("interpolator='amt-g' runs in fp32 only (--dtype bf16 is SuperSloMo's)")
        if size is not None and not amt.supported_size(*size)[0]:
            raise ValueError(amt.size_error(*size))


def superslomo_state_dict(obj, what="checkpoint"):
    """The two forms of a SuperSloMo checkpoint -> the flat state dict of the module: the flat dict itself (what the
    reference's ``SuperSloMo(pretrained=...)`` loads), or the published file's dict with ``state_dictFC`` (flow
    computation) and ``state_dictAT`` (arbitrary-time interpolation), whose keys get the ``flow_estimator.`` / ``interp.``
    prefix."""
    if not isinstance(obj, dict):
        raise ValueError(f"{what}: not a state dict")
    if any(k in obj for k, _ in _PARTS):
        missing = [k for k, _ in _PARTS if not isinstance(obj.get(k), dict)]
        if missing:
            raise ValueError(f"{what}: holds no state dict under {', '.join(missing)}")
        obj = {prefix + k: v for part, prefix in _PARTS for k, v in obj[part].items()}
    if not all(isinstance(v, torch.Tensor) for v in obj.values()):
        raise ValueError(f"{what}: not a tensor state dict")
    return obj


def load_state(net, sd, what="checkpoint"):
    """Strict load that names every unexpected or missing key (and every shape that differs)."""
    own = net.state_dict()
    unexpected = [k for k in sd if k not in own]
    missing = [k for k in own if k not in sd]
    shapes = [f"{k} {tuple(sd[k].shape)} for {tuple(own[k].shape)}" for k in sd if k in own and sd[k].shape != own[k].shape]
    if unexpected or missing or shapes:
        parts = [f"{name}: {', '.join(keys)}" for name, keys in (("unexpected keys", unexpected), ("missing keys", missing),
                                                                ("shapes", shapes)) if keys]
        raise ValueError(f"{what} does not fit {type(net).__name__}; " + "; ".join(parts))
    net.load_state_dict(sd, strict=True)
    return net


def load_interpolator(weights_dir, device, dtype="fp32", name="superslomo"):
    """``name`` "superslomo": SuperSloMo with ``weights_dir/SuperSloMo.ckpt``, dtype "fp32" (default) or "bf16";
    "amt-g": AMT with ``weights_dir/amt-g.pth``, fp32 only.  On ``device``, eval mode."""
    check_interpolator(name, dtype)
    path = os.path.join(str(weights_dir), INTERPOLATORS[name])
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found")
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if name == "amt-g":
        from .guided_diffusion.amt import AMT
        return load_state(AMT(), amt_state_dict(obj, path), path).eval().to(device)
    from .guided_diffusion.superslomo import SuperSloMo
    net = load_state(SuperSloMo(), superslomo_state_dict(obj, path), path).eval().to(device)
    return net.convert_to_bf16() if dtype == "bf16" else net


def padded_size(h, w, multiple=32):
    """(h, w) rounded up to the network's multiple."""
    return -(-h // multiple) * multiple, -(-w // multiple) * multiple


def pad_frames(x, multiple=32):
    """(N, 3, h, w) -> (N, 3, H, W) with H, W the next multiples: edge replication at the bottom and the right.  (Ours: the
    reference has no padding for this network; the bicubic tasks' frames are multiples of 16.)"""
    h, w = x.shape[2:]
    H, W = padded_size(h, w, multiple)
    return x if (H, W) == (h, w) else F.pad(x, (0, W - w, 0, H - h), mode="replicate")


def interleave_index(T, factor):
    """Where the frames of the result come from, in time order: [("orig", i) | ("mid", pair, k)] of length
    factor * (T - 1) + 1; ("mid", p, k) is the frame at t = (k + 1) / factor between originals p and p + 1."""
    order = []
    for i in range(T - 1):
        order.append(("orig", i))
        order += [("mid", i, k) for k in range(factor - 1)]
    order.append(("orig", T - 1))
    return order


def interpolate_pairs(net, first01, second01, factor):
    """(P, 3, h, w) x 2 in [0, 1] on the device -> (P, factor - 1, 3, h, w) in [0, 1]: padded, run, cropped, clamped."""
    h, w = first01.shape[2:]
    m = getattr(net, "MULTIPLE", 32)
    a = pad_frames(first01.float(), m) * 2 - 1
    b = pad_frames(second01.float(), m) * 2 - 1
    mid = net(a.contiguous(), b.contiguous(), factor)
    return ((mid[..., :h, :w] + 1) / 2).clamp(0, 1)


def nearest_original(k, factor):
    """Across a cut nothing is synthesised: in-between k (at t = (k + 1) / factor) of a pair (p, p + 1) is a copy of frame
    p + nearest_original(k, factor), i.e. of p where t < 0.5 and of p + 1 otherwise (2 (k + 1) < factor, in integers)."""
    return 0 if 2 * (k + 1) < factor else 1


def _pairs_of_group(p, q, cutset):
    """Pairs p .. q - 1 split into those the network interpolates and those that straddle a cut."""
    keep = [i for i in range(p, q) if i + 1 not in cutset]
    return keep, [i for i in range(p, q) if i + 1 in cutset]


def _run_pairs(net, frames01, keep, base, factor):
    """interpolate_pairs on the pairs ``keep`` (video indices; frames01[i - base] is frame i) of a group with a cut in it."""
    idx = torch.tensor([i - base for i in keep], device=frames01.device)
    return interpolate_pairs(net, frames01[idx], frames01[idx + 1], factor)


def interpolate_frames(net, frames01, factor, batch=4, cuts=None):
    """(T, 3, H, W) in [0, 1] -> (factor * (T - 1) + 1, 3, H, W): originals (untouched) and intermediates interleaved in
    time order.  Pairs go through the network ``batch`` at a time.  ``cuts`` (flair_amd.scenes: frames that start a new
    shot): the network is not called for a pair (p, p + 1) with p + 1 in cuts; its in-betweens are copies of the nearer
    original (nearest_original), so the count and the timing of the result stay the same."""
    if frames01.dim() != 4 or frames01.shape[1] != 3:
        raise ValueError(f"interpolate: (T, 3, H, W) frames, got {tuple(frames01.shape)}")
    T = frames01.shape[0]
    if T < 2:
        raise ValueError("interpolate: at least two frames")
    if isinstance(factor, bool) or int(factor) != factor or factor < 2:
        raise ValueError(f"interpolate: factor={factor!r}; an integer >= 2")
    factor = int(factor)
    cutset = set(scenes.check_cuts(cuts or [], T))
    out = frames01.new_empty((factor * (T - 1) + 1, *frames01.shape[1:]), dtype=torch.float32)
    out[::factor] = frames01
    for p in range(0, T - 1, max(1, int(batch))):
        q = min(T - 1, p + max(1, int(batch)))
        keep, across = _pairs_of_group(p, q, cutset)
        if not across:
            mid = interpolate_pairs(net, frames01[p:q], frames01[p + 1:q + 1], factor)
            for k in range(factor - 1):
                out[p * factor + 1 + k:q * factor:factor] = mid[:, k]
            continue
        if keep:
            mid = _run_pairs(net, frames01[p:q + 1], keep, p, factor)
            for j, i in enumerate(keep):
                out[i * factor + 1:(i + 1) * factor] = mid[j]
        for i in across:
            for k in range(factor - 1):
                out[i * factor + 1 + k] = frames01[i + nearest_original(k, factor)]
    return out


def check_source(src_dir, factor):
    """The refusals of the command line, before any GPU work: ValueError -> the frame paths and their (h, w)."""
    if isinstance(factor, bool) or int(factor) != factor or factor < 2:
        raise ValueError(f"--factor {factor} makes no frame: an integer >= 2")
    if fio.is_y4m(src_dir):
        if not os.path.isfile(src_dir):
            raise ValueError(f"{src_dir} is not a file")
    elif not os.path.isdir(src_dir):
        raise ValueError(f"{src_dir} is not a directory")
    paths = fio.list_frames(src_dir)
    if len(paths) < 2:
        raise ValueError(f"{src_dir} holds {len(paths)} frame file(s); two or more are needed")
    sizes = [fio.frame_size(p) for p in paths]
    for p, s in zip(paths, sizes):
        if s != sizes[0]:
            raise ValueError(f"{p} is {s[0]}x{s[1]} and {paths[0]} is {sizes[0][0]}x{sizes[0][1]}; the frames of a video "
                             "must share one size")
    return paths, sizes[0]


def interpolate_video_files(src_dir, out_dir, factor, *, net, device, batch=4, cuts=None):
    """Frame files of ``src_dir`` (flair_amd.io's listing and order) -> ``out_dir/{i:04d}.png``, factor * (T - 1) + 1 of
    them.  Original frames are written from their decoded bytes (never re-quantised from floats), intermediates through
    ``io.to_bytes``.  At most ``batch`` pairs are on the device at a time; decoding and PNG encoding overlap the network
    (the reader and writer threads of flair_amd.io).  ``cuts``: as in interpolate_frames; the copies that stand between the
    two frames of a cut are written from the decoded bytes too.  Returns the number of frames written."""
    paths, _ = check_source(src_dir, factor)
    factor = int(factor)
    T = len(paths)
    batch = max(1, int(batch))
    cutset = set(scenes.check_cuts(cuts or [], T))
    # group g holds frames first .. first + n - 1: its pairs and the frame that closes the last of them
    groups = [(p, min(batch, T - 1 - p) + 1) for p in range(0, T - 1, batch)]
    writer = fio._Writer(out_dir, y4m=fio.y4m.output_params(fio.y4m.stream_of(paths), rate=factor))
    try:
        for first, (u8,) in fio.iter_frame_batches([paths], groups, device):
            frames01 = u8.permute(0, 3, 1, 2).float() / 255.0
            n = u8.shape[0] - 1
            keep, across = _pairs_of_group(first, first + n, cutset)
            block = torch.empty((n * factor, *u8.shape[1:]), dtype=torch.uint8, device=u8.device)
            block[::factor] = u8[:-1]
            if not across:
                mid = fio.to_bytes(interpolate_pairs(net, frames01[:-1], frames01[1:], factor).flatten(0, 1))
                mid = mid.view(n, factor - 1, *u8.shape[1:])
                for k in range(factor - 1):
                    block[1 + k::factor] = mid[:, k]
            else:
                if keep:
                    mid = fio.to_bytes(_run_pairs(net, frames01, keep, first, factor).flatten(0, 1))
                    mid = mid.view(len(keep), factor - 1, *u8.shape[1:])
                    for j, i in enumerate(keep):
                        block[(i - first) * factor + 1:(i - first + 1) * factor] = mid[j]
                for i in across:
                    for k in range(factor - 1):
                        block[(i - first) * factor + 1 + k] = u8[i - first + nearest_original(k, factor)]
            writer.submit_bytes(first * factor, block)
        last = torch.from_numpy(fio.decode_frame_hwc(paths[-1]).copy())[None]
        writer.submit_bytes((T - 1) * factor, last)
    finally:
        writer.close()
    return factor * (T - 1) + 1
