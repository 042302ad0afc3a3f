"""ArcFace identity similarity of written frames against ground truth and the identity drift from frame to frame, on the GPU:
``--identity FILE`` of evaluate, restore --ground-truth and interpolate --ground-truth.

The three priors (CodeFormer, RestoreFormer, VQFR) are published with this score ("IDS", "Deg.", "IDD"): a generative face prior
can return a sharp face of somebody else, which PSNR, SSIM, LPIPS and NIQE reward.  The reference ships no scoring tool; the
definition is restated in include/flair_ident.h and computed by the project's own kernels: ``flair_ident_prepare`` (bytes -> the
grey 128 x 128 input of both frame sets, so a batch runs through the network as 2 N frames), ``flair_conv_nhwc`` in f32 with
the BatchNorm after a convolution folded in, ``flair_affine_channels_f32`` for the BatchNorm IN FRONT of a block's first
convolution (that convolution pads its input with zeros after the norm, so a folded shift would be wrong on the border),
``flair_prelu_nhwc`` with the one slope broadcast over the channels and the residual as its second input,
``flair_maxpool2x2s2_nhwc``, and ``flair_ident_embed`` for the final linear layer with both of its BatchNorms folded in.  f32 only.
The cosines and their means are numpy float64 here.

  * ``ids`` of a frame pair = <e_a, e_b> / (|e_a| |e_b|), higher is closer; a zero embedding gives no value (JSON null).
  * ``id_drift`` = the mean over t >= 1 of 1 - cos(e_t, e_{t-1}) on the restored frames, ``id_drift_truth`` the same on the
    truth frames for comparison.  Scene cuts are not consulted: a cut shows up as drift.

Frames are taken as aligned face crops (the package's ``aligned`` mode) and must be square; faces are not detected here
(``flair_amd.facescore`` cuts the faces out of unaligned frames and hands the crops to ``embed``).

The weights are the user's: GFPGAN's / VQFR's ``arcface_resnet18.pth``, ``ResNetArcFace(block='IRBlock', layers=(2, 2, 2, 2),
use_se=False)`` stored with a ``module.`` prefix.  Nothing is downloaded or shipped.  The key names below were restated from
memory of that class; the real file was never loaded here.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .guided_diffusion.packing import PackedModel, dev_f32, packed_conv, run_conv

SIDE = ops.IDENT_SIDE
WIDTH = 512                                     # numbers in an embedding
PLANES = (64, 128, 256, 512)


def check_size(h, w, what="frames"):
    """ValueError where a frame is not square (aligned face crops are)."""
    if h != w:
        raise ValueError(f"identity: {what} is {h}x{w}; the score takes aligned face crops, which are square")


def _conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 3, stride, 1, bias=False)


class IRBlock(nn.Module):
    """bn0 -> conv1 -> bn1 -> prelu -> conv2 (stride) -> bn2, + downsample(x) or x, prelu (the same slope)."""

    def __init__(self, cin, planes, stride):
        super().__init__()
        self.bn0 = nn.BatchNorm2d(cin)
        self.conv1 = _conv3x3(cin, cin)
        self.bn1 = nn.BatchNorm2d(cin)
        self.prelu = nn.PReLU()
        self.conv2 = _conv3x3(cin, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or cin != planes:
            self.downsample = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))

    def pack(self, dtype, device):
        cin, planes = self.conv1.in_channels, self.conv2.out_channels
        sub, mul = (dev_f32(t.float(), device) for t in bn0_terms(self.bn0))
        self._pk = dict(sub=sub, mul=mul, c1=packed_conv(self.conv1, self.bn1, dtype, device),
                        c2=packed_conv(self.conv2, self.bn2, dtype, device),
                        slope=dev_f32(self.prelu.weight.detach().float().expand(max(cin, planes)).contiguous(), device))
        if self.downsample is not None:
            self._pk["ds"] = packed_conv(self.downsample[0], self.downsample[1], dtype, device)

    def forward(self, x):
        pk = self._pk
        t = ops.affine_channels(x, x.shape[3], 1.0, 0.0, float("-inf"), float("inf"), pk["sub"], pk["mul"], torch.empty_like(x))
        t = run_conv(t, pk["c1"], self.conv1)
        ops.prelu(t, pk["slope"], out=t)
        t = run_conv(t, pk["c2"], self.conv2)
        res = run_conv(x, pk["ds"], self.downsample[0]) if self.downsample is not None else x
        return ops.prelu(t, pk["slope"], x1=res, out=t)


def bn0_terms(bn):
    """An eval-mode BatchNorm as y = (x - sub) * mul, the form of flair_affine_channels_f32 -> (sub, mul) in float64.
    ValueError for a channel whose scale is zero (its output is a constant, which the form cannot say)."""
    g = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    if bool((g == 0).any()):
        raise ValueError(f"identity: a BatchNorm in front of a convolution has a zero scale in channel {int((g == 0).nonzero()[0])}")
    return bn.running_mean.detach().double() - bn.bias.detach().double() / g, g


def fold_head(bn4, fc5, bn5, side=8):
    """bn5(fc5(flatten(bn4(x)))) as ONE affine map on the NHWC feature map -> (W (O, side * side * C), b (O,)) in float64.
    Exact: nothing is padded between the three.  Column (h * side + w) * C + c of W is fc5's column (c * side + h) * side + w."""
    g4 = bn4.weight.detach().double() / torch.sqrt(bn4.running_var.detach().double() + bn4.eps)
    t4 = bn4.bias.detach().double() - g4 * bn4.running_mean.detach().double()
    g5 = bn5.weight.detach().double() / torch.sqrt(bn5.running_var.detach().double() + bn5.eps)
    O, C = fc5.out_features, bn4.num_features
    w = fc5.weight.detach().double().view(O, C, side, side)
    b = g5 * ((w * t4.view(1, C, 1, 1)).sum((1, 2, 3)) + fc5.bias.detach().double() - bn5.running_mean.detach().double()) + bn5.bias.detach().double()
    w = w * g4.view(1, C, 1, 1) * g5.view(O, 1, 1, 1)
    return w.permute(0, 2, 3, 1).reshape(O, side * side * C).contiguous(), b


class ArcFace(PackedModel, nn.Module):
    """``ArcFace(device)``: ResNetArcFace(IRBlock, (2, 2, 2, 2), use_se=False) under its state-dict names.
    ``embed(a_u8, b_u8=None)``: one or two (N, H, W, 3) uint8 frame sets on the device -> (N or 2 N, 512) float64 numpy."""

    def __init__(self, device=None):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.prelu = nn.PReLU()
        self.maxpool = nn.MaxPool2d(2, 2)
        cin = 64
        for i, planes in enumerate(PLANES):
            stride = 1 if i == 0 else 2
            setattr(self, f"layer{i + 1}", nn.Sequential(IRBlock(cin, planes, stride), IRBlock(planes, planes, 1)))
            cin = planes
        self.bn4 = nn.BatchNorm2d(512)
        self.dropout = nn.Dropout()
        self.fc5 = nn.Linear(512 * 8 * 8, WIDTH)
        self.bn5 = nn.BatchNorm1d(WIDTH)
        self.requires_grad_(False).eval()
        if device is not None:
            self.to(device)

    def convert_to_bf16(self):
        raise ValueError("ArcFace identity runs in fp32 only")

    def blocks(self):
        return [b for i in range(4) for b in getattr(self, f"layer{i + 1}")]

    def pack(self, dtype, device):
        w, b = fold_head(self.bn4, self.fc5, self.bn5)
        self._pk = dict(stem=packed_conv(self.conv1, self.bn1, dtype, device),
                        slope=dev_f32(self.prelu.weight.detach().float().expand(64).contiguous(), device),
                        w=dev_f32(w.float(), device), b=dev_f32(b.float(), device))

    @torch.no_grad()
    def embed(self, a_u8, b_u8=None):
        if a_u8.dim() != 4 or a_u8.shape[3] != 3 or (b_u8 is not None and tuple(a_u8.shape) != tuple(b_u8.shape)):
            raise ValueError(f"identity: (N, H, W, 3) frame sets of one shape, got {tuple(a_u8.shape)}"
                             + ("" if b_u8 is None else f" and {tuple(b_u8.shape)}"))
        check_size(a_u8.shape[1], a_u8.shape[2], what="a frame")
        self._ensure_packed(a_u8.device)
        pk = self._pk
        x = ops.ident_prepare(a_u8.contiguous(), None if b_u8 is None else b_u8.contiguous())
        x = run_conv(x, pk["stem"], self.conv1)
        ops.prelu(x, pk["slope"], out=x)
        x = ops.maxpool2x2s2(x)
        for block in self.blocks():
            x = block(x)
        e = ops.ident_embed(x.view(x.shape[0], -1), pk["w"], pk["b"])
        return e.cpu().numpy().astype(np.float64)

    forward = embed


# ------------------------------------------------------------------------------------------- the host's arithmetic (float64)
def cosine(ea, eb):
    """<ea, eb> / (|ea| |eb|) of two embeddings in float64; None where one of them is zero.  The norms are taken as ONE root,
    sqrt(<ea, ea> <eb, eb>): sqrt(d * d) is d in binary floating point, so equal embeddings give exactly 1."""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    aa, bb = float(ea @ ea), float(eb @ eb)
    if aa == 0.0 or bb == 0.0:
        return None
    return float(ea @ eb) / math.sqrt(aa * bb)


def _mean(values):
    have = [v for v in values if v is not None]
    return sum(have) / len(have) if have else None


def drift(embeddings):
    """The mean over t >= 1 of 1 - cos(e_t, e_{t-1}); pairs with a zero embedding are left out; None without a pair."""
    cos = [cosine(embeddings[t], embeddings[t - 1]) for t in range(1, len(embeddings))]
    return _mean([None if c is None else 1.0 - c for c in cos])


def scores(restored, truth):
    """Embeddings of the restored and of the truth frames, in order -> (per-frame ids, {ids, id_drift, id_drift_truth})."""
    ids = [cosine(a, b) for a, b in zip(restored, truth)]
    return ids, dict(ids=_mean(ids), id_drift=drift(restored), id_drift_truth=drift(truth))


def format_value(v, name="ids"):
    """``  ids 0.8123`` or ``  ids n/a``."""
    return f"  {name} n/a" if v is None else f"  {name} {v:.4f}"


def format_mean(mean):
    """The three means of a result: ``  ids 0.8123  id-drift 0.0312 (truth 0.0287)``."""
    truth = "n/a" if mean["id_drift_truth"] is None else f"{mean['id_drift_truth']:.4f}"
    return format_value(mean["ids"]) + format_value(mean["id_drift"], "id-drift") + f" (truth {truth})"


# ------------------------------------------------------------------------------------------- the checkpoint
def identity_state_dict(sd, what="checkpoint"):
    """A state dict of the network, plain or with a ``module.`` prefix -> the state dict of ``ArcFace()``.
    ``num_batches_tracked`` is ignored; ValueError names every missing key, every stray key and every shape that differs, and
    says so where the file is a use_se=True network."""
    if not isinstance(sd, dict) or not sd or not all(isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in sd.items()):
        raise ValueError(f"{what}: the file holds no tensor state dict")
    got = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    got = {k: v for k, v in got.items() if not k.endswith("num_batches_tracked")}
    if any(".se." in k for k in got):
        raise ValueError(f"{what}: the file has squeeze-and-excitation weights ({next(k for k in got if '.se.' in k)}); "
                         "use_se=True is not built")
    own = ArcFace().state_dict()
    need = [k for k in own if not k.endswith("num_batches_tracked")]
    stray = [k for k in got if k not in own]
    missing = [k for k in need if k not in got]
    shapes = [f"{k} {tuple(got[k].shape)} for {tuple(own[k].shape)}" for k in need if k in got and got[k].shape != own[k].shape]
    if stray or missing or shapes:
        parts = [f"{name}: {', '.join(keys)}" for name, keys in (("unexpected keys", stray), ("missing keys", missing),
                                                                ("shapes", shapes)) if keys]
        raise ValueError(f"{what} does not fit ResNetArcFace(IRBlock, (2, 2, 2, 2), use_se=False); " + "; ".join(parts))
    return {k: got.get(k, own[k]) for k in own}


def load_identity(path, device):
    """``ArcFace`` on ``device`` with the weights of ``path`` (arcface_resnet18.pth)."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found")
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as exc:            # not a checkpoint at all, or one that needs code to unpickle
        raise ValueError(f"{path}: not a tensor state dict ({type(exc).__name__}: {str(exc).splitlines()[0] if str(exc) else ''})")
    model = ArcFace()
    model.load_state_dict(identity_state_dict(sd, str(path)), strict=True)
    return model.to(device)
