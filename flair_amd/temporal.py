"""The flow-warping error of written frames, on the GPU: ``--warp-error FILE`` of evaluate, restore and interpolate, and the
``warp-error`` command for footage without ground truth.

Every other score of this package judges one frame; this one says whether a restored VIDEO holds together over time.  It is
``E_warp`` of Lai et al. ("Learning Blind Video Temporal Consistency", ECCV 2018) with the occlusion and motion-boundary rule
of Ruder et al. 2016, as restated in include/flair_temporal.h: frame t + 1 is warped back onto frame t along the optical
flow, pixels that leave the frame, are occluded or lie on a motion boundary are masked out, and the mean squared difference
of the rest is taken.  It is the definition computed here, not a reproduction of Lai's script (FlowNet2 flows, its own
occlusion code); the reference ships no scoring tool.

  * the flows are SPyNet's (``unet_new.SPyNet``: ``flair_conv_nhwc`` in f32), both directions per pair; its weights are the
    user's: a bare mmedit SPyNet state dict, or any FLAIR task checkpoint, which holds one (``load_flow``);
  * ``flair_flow_occlusion`` makes the mask and ``flair_warp_error`` the masked sums (S, N) per pair, in float64, in a fixed
    order and without atomics: for given flows a pair's (S, N) is the same bits in every run, batch size and batch position;
  * ``warp_err = S / (255^2 N)`` and the means are float64 here.

With ground truth, the flows and the mask come from the TRUTH frames and both frame sets are judged by them, so the restored
frames' value and the truth's (``warp_err_truth``: what the flow's own error and real appearance change leave) are comparable.
Without it they come from the scored frames themselves.

The convolution entry picks its K split by launch size, so a pair's FLOW may differ in the last bits between batch sizes (as
the ArcFace trunk's embeddings do); only the two kernels above promise equal bits.
"""
import os
import re

import torch

from . import ops
from .guided_diffusion.unet_new import SPyNet
from .video import max_clip_pixels

MIN_SIDE = 32                                   # SPyNet's coarsest pyramid level is 1/32 of the frame
PRINT_SCALE = 1e3                               # reports print warp_err x 10^3, the scale papers print; JSON is unscaled


def check_size(h, w, what="frames"):
    """ValueError where a frame is under 32 pixels a side, or too large for one SPyNet call."""
    if min(h, w) < MIN_SIDE:
        raise ValueError(f"warp-error: {what} is {h}x{w}; the flow network needs frames of at least {MIN_SIDE} pixels a side")
    if h * w > max_clip_pixels():
        raise ValueError(f"warp-error: {what} is {h}x{w}; one frame pair must stay under {max_clip_pixels()} pixels")


# ------------------------------------------------------------------------------------------- the checkpoint
def flow_state_dict(sd, what="checkpoint"):
    """The state dict of ``SPyNet()`` from either file shape: a bare mmedit SPyNet state dict (``basic_module.L.basic_module.J.
    conv.{weight,bias}``, ``mean`` / ``std`` optional), or a FLAIR task checkpoint, of which the keys under the first prefix in
    sorted order that ends in ``spynet.`` are taken; either may sit under ``"state_dict"``.  ValueError for anything else,
    naming what was looked for, and for missing keys, stray keys and shapes that differ."""
    looked = ("looked for keys basic_module.L.basic_module.J.conv.{weight,bias} (a bare mmedit SPyNet state dict) or keys under "
              "a prefix ending in spynet. (a FLAIR task checkpoint), plain or under \"state_dict\"")
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict) or not sd or not all(isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in sd.items()):
        raise ValueError(f"{what}: the file holds no tensor state dict; {looked}")
    own = SPyNet().state_dict()
    if any(k.startswith("basic_module.") for k in sd):
        got = dict(sd)
    else:
        prefixes = sorted({m.group(1) for m in (re.match(r"(.*?spynet\.)basic_module\.", k) for k in sd) if m})
        if not prefixes:
            some = ", ".join(list(sd)[:3])
            raise ValueError(f"{what}: no SPyNet weights among its {len(sd)} keys ({some}{', ...' if len(sd) > 3 else ''}); {looked}")
        got = {k[len(prefixes[0]):]: v for k, v in sd.items() if k.startswith(prefixes[0])}
    need = [k for k in own if k not in ("mean", "std")]
    stray = [k for k in got if k not in own]
    missing = [k for k in need if k not in got]
    shapes = [f"{k} {tuple(got[k].shape)} for {tuple(own[k].shape)}" for k in own if k in got and got[k].shape != own[k].shape]
    if stray or missing or shapes:
        parts = [f"{name}: {', '.join(keys)}" for name, keys in (("unexpected keys", stray), ("missing keys", missing),
                                                                ("shapes", shapes)) if keys]
        raise ValueError(f"{what} does not fit mmedit's SPyNet; " + "; ".join(parts))
    return {k: got.get(k, own[k]) for k in own}


def load_flow(path, device):
    """A packed ``SPyNet`` on ``device`` with the weights of ``path`` (see flow_state_dict for the two file shapes)."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found")
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as exc:            # not a checkpoint at all, or one that needs code to unpickle
        raise ValueError(f"{path}: not a tensor state dict ({type(exc).__name__}: {str(exc).splitlines()[0] if str(exc) else ''})")
    model = SPyNet()
    model.load_state_dict(flow_state_dict(sd, str(path)), strict=True)
    model = model.requires_grad_(False).eval().to(device)
    model.pack(torch.float32, device)
    return model


# ------------------------------------------------------------------------------------------- the GPU's part
class WarpError:
    """``WarpError(flow_model)``: a packed SPyNet.  ``pairs(frames_u8, truth_u8=None)``: (T, H, W, 3) uint8 frame sets on the
    device -> numpy float64 (sets, T - 1, 2) of (S, N) per consecutive pair; set 0 = ``frames_u8``, set 1 = ``truth_u8``."""

    def __init__(self, flow_model):
        self.flow = flow_model

    @torch.no_grad()
    def flows(self, u8):
        """(T, H, W, 3) uint8 -> (f, g), each (T - 1, H, W, 2) f32: f[i] the flow frame i -> i + 1, g[i] the flow i + 1 -> i."""
        T, H, W, _ = u8.shape
        raw = torch.zeros((T, H, W, 4), dtype=torch.float32, device=u8.device)     # [-1, 1], channel 3 zero: pair_flows' input
        raw[..., :3] = u8.float().mul_(2.0 / 255.0).sub_(1.0)
        g, f = self.flow.pair_flows(raw)        # (flows_forward, flows_backward): flows_backward = run(ref=a, supp=b) = a -> b
        return f, g

    @torch.no_grad()
    def pairs(self, frames_u8, truth_u8=None, max_pairs=None):
        if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8 or (
                truth_u8 is not None and (tuple(truth_u8.shape) != tuple(frames_u8.shape) or truth_u8.dtype != torch.uint8)):
            raise ValueError(f"warp-error: (T, H, W, 3) uint8 frame sets of one shape, got {tuple(frames_u8.shape)} {frames_u8.dtype}"
                             + ("" if truth_u8 is None else f" and {tuple(truth_u8.shape)} {truth_u8.dtype}"))
        T, H, W, _ = frames_u8.shape
        check_size(H, W, what="a frame")
        sets = 1 if truth_u8 is None else 2
        out = torch.empty((sets, max(T - 1, 0), 2), dtype=torch.float64, device=frames_u8.device)
        # (T - 1) H W of one SPyNet call stays under video.py's limit: sub-batches that overlap by one frame
        step = max(1, max_clip_pixels() // (H * W))
        if max_pairs is not None:
            step = max(1, min(step, int(max_pairs)))
        for i in range(0, T - 1, step):
            n = min(step, T - 1 - i)
            a = frames_u8[i:i + n + 1].contiguous()
            b = None if truth_u8 is None else truth_u8[i:i + n + 1].contiguous()
            f, g = self.flows(a if b is None else b)
            mask = ops.flow_occlusion(f, g)
            out[:, i:i + n] = ops.warp_error(a, f, mask, a2=b)
        return out.cpu().numpy()


class PairStream:
    """Batches of a video pushed in order -> ``rows``: per frame, None (the first frame, or a frame whose size differs from the
    one before it) or the (sets, 2) float64 array of its pair with the frame BEFORE it.  The last frame of a batch is kept so
    that the pair across two batches is measured too."""

    def __init__(self, model):
        self.model, self.prev, self.rows, self.pixels = model, None, [], []

    def push(self, frames_u8, truth_u8=None):
        a, b = frames_u8, truth_u8
        if self.prev is not None and self.prev[0].shape[1:] == a.shape[1:]:
            a = torch.cat([self.prev[0], a])
            b = None if b is None else torch.cat([self.prev[1], b])
        else:
            self.rows.append(None)
        if a.shape[0] >= 2:
            got = self.model.pairs(a, b)
            self.rows += [got[:, i] for i in range(got.shape[1])]
        self.pixels += [frames_u8.shape[1] * frames_u8.shape[2]] * frames_u8.shape[0]
        self.prev = (frames_u8[-1:], None if truth_u8 is None else truth_u8[-1:])


# ------------------------------------------------------------------------------------------- the host's arithmetic (float64)
def straddling(cuts, factor=1):
    """The later-frame indices of the pairs that straddle a cut.  A cut at k means frame k starts a shot: pair (k - 1, k).  For
    frames written by ``interpolate --factor N`` from a source with those cuts (``factor=N``), every output pair lying between
    source frames k - 1 and k: later frames N (k - 1) + 1 .. N k."""
    return {factor * (k - 1) + j for k in (cuts or ()) for j in range(1, factor + 1)}


def _mean(values):
    have = [v for v in values if v is not None]
    return sum(have) / len(have) if have else None


def scores(rows, pixels, skip=()):
    """``rows`` and ``pixels`` of a PairStream (per frame: None or (sets, 2) of (S, N); H W), ``skip``: later-frame indices
    whose pair is left out (``straddling``) -> (per-frame warp_err, mean dict).  A pair's value S / (255^2 N) belongs to its
    LATER frame; a video's first frame, a left-out pair and a pair with N = 0 have None.  ``warp_err`` is the mean over the
    ``warp_err_pairs`` pairs that have a value, ``warp_err_truth`` (only with two sets) the same of the second set, and
    ``masked`` the mean of 1 - N / (H W) over every pair that was measured (N = 0 included)."""
    def value(row, s):
        return None if row is None or row[s][1] == 0 else float(row[s][0]) / (255.0 ** 2 * float(row[s][1]))
    rows = [None if t in skip else r for t, r in enumerate(rows)]
    values = [value(r, 0) for r in rows]
    mean = dict(warp_err=_mean(values))
    if any(r is not None and len(r) > 1 for r in rows):
        mean["warp_err_truth"] = _mean([value(r, 1) for r in rows])
    mean["warp_err_pairs"] = sum(v is not None for v in values)
    mean["masked"] = _mean([None if r is None else 1.0 - float(r[0][1]) / px for r, px in zip(rows, pixels)])
    return values, mean


def format_value(v, name="warp-err"):
    """``  warp-err 1.2345`` (the value x 10^3) or ``  warp-err n/a``."""
    return f"  {name} n/a" if v is None else f"  {name} {v * PRINT_SCALE:.4f}"


def format_mean(mean):
    """``  warp-err 1.2345 (truth 0.9876)  masked 0.0712``; the bracket only where the result holds a truth value."""
    text = format_value(mean["warp_err"])
    if "warp_err_truth" in mean:
        text += " (truth " + format_value(mean["warp_err_truth"], "").split()[-1] + ")"
    return text + ("  masked n/a" if mean["masked"] is None else f"  masked {mean['masked']:.4f}")


# ------------------------------------------------------------------------------------------- a directory without truth
def warp_error_dir(frames_dir, device, model, skip=(), batch=8):
    """Score the frames of ``frames_dir`` in ``io.list_frames`` order by their own flows: ``dict(frames=[{name, warp_err}],
    mean={warp_err, warp_err_pairs, masked}, count)``.  ``model``: a ``WarpError``; ``skip``: the later frames of the pairs to
    leave out (``straddling`` of the scene cuts).
    ValueError for an empty directory or a frame under 32 pixels a side, checked on the file headers before anything is decoded."""
    from . import io as fio
    from .metrics import _groups
    paths = fio.list_frames(frames_dir)
    if not paths:
        raise ValueError(f"warp-error: no frame files in {frames_dir}")
    sizes = [fio.frame_size(p) for p in paths]
    for p, (h, w) in zip(paths, sizes):
        check_size(h, w, what=f"{p}")
    stream = PairStream(model)
    for _first, (u8,) in fio.iter_frame_batches([paths], _groups(sizes, max(1, int(batch))), device):
        stream.push(u8)
    values, mean = scores(stream.rows, stream.pixels, set(skip))
    return dict(frames=[dict(name=os.path.basename(p), warp_err=v) for p, v in zip(paths, values)], mean=mean, count=len(paths))


def format_report(result):
    """One line per frame and the means."""
    lines = [f["name"] + format_value(f["warp_err"]) for f in result["frames"]]
    lines.append(f"mean of {result['mean']['warp_err_pairs']} pairs of {result['count']} frames" + format_mean(result["mean"]))
    return lines
