"""The VQGAN building blocks the three face priors share (codeformer.py, restoreformer.py, vqfr.py).

Parameter containers with a ``pack(dtype, device)`` / ``run(x)`` pair on NHWC clip tensors.  The priors subclass them to keep
their reference's constructor signatures and state-dict names; what differs between them is a class attribute here
(``ResBlock.shortcut``, ``AttnBlock.attention``), not a second copy of ``pack`` / ``run``.
"""
import torch
import torch.nn as nn

from .. import ops
from .. import ops as A
from .packing import dev_f32, pack_w, packed_conv, run_conv

GN_EPS = 1e-6


def normalize(channels):
    return nn.GroupNorm(num_groups=32, num_channels=channels, eps=GN_EPS, affine=True)


def gn(x, pk, name, act=A.ACT_NONE, x1=None):
    """GroupNorm(32, eps 1e-6)(+act) per face on pk[name + "_g"], pk[name + "_b"]; x1: a second channel part of the input."""
    return ops.group_norm(x, pk[name + "_g"], pk[name + "_b"], x1=x1, eps=GN_EPS, act=act, frames_per_stat=1)


def _wb(conv, dtype, device, segs=None):
    return pack_w(conv.weight, dtype, device, segs), dev_f32(conv.bias, device)


def _norm(m, device):
    return dev_f32(m.weight, device), dev_f32(m.bias, device)


class Downsample(nn.Module):
    """F.pad(x, (0, 1, 0, 1)) + 3x3 stride-2 convolution without padding."""

    def __init__(self, in_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)

    def pack(self, dtype, device):
        w, b = _wb(self.conv, dtype, device)
        self._pk = dict(w=w, b=b)

    def run(self, x):
        return ops.conv(x, self._pk["w"], self._pk["b"], self.conv.out_channels, (1, 3, 3), stride=2, asym_pad=True)


class Upsample(nn.Module):
    """Nearest x2, then a 3x3 convolution."""

    def __init__(self, in_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)

    def pack(self, dtype, device):
        w, b = _wb(self.conv, dtype, device)
        self._pk = dict(w=w, b=b)

    def run(self, x):
        up = ops.resize(x, (2 * x.shape[1], 2 * x.shape[2]), ops.RESIZE_NEAREST)
        return ops.conv(up, self._pk["w"], self._pk["b"], self.conv.out_channels, (1, 3, 3))


class ResBlock(nn.Module):
    """GroupNorm+SiLU, 3x3, GroupNorm+SiLU, 3x3 with the shortcut (identity, or a 1x1 / 3x3 convolution when the widths
    differ) as the last convolution's ``res0``.  ``run(x, x1)`` takes the input as two channel parts (an implicit
    ``torch.cat``); ``out_scale`` scales the sum."""

    shortcut = "conv_out"       # the attribute (and state-dict) name of the shortcut convolution
    split = None                # widths of the two input parts when they are not one padded segment to the shortcut

    def __init__(self, in_channels, out_channels=None, shortcut_kernel=1, shortcut=None):
        super().__init__()
        if shortcut is not None:
            self.shortcut = shortcut
        self.in_channels = in_channels
        self.out_channels = in_channels if out_channels is None else out_channels
        self.norm1 = normalize(in_channels)
        self.conv1 = nn.Conv2d(in_channels, self.out_channels, kernel_size=3, stride=1, padding=1)
        self.norm2 = normalize(self.out_channels)
        self.conv2 = nn.Conv2d(self.out_channels, self.out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            k = shortcut_kernel
            setattr(self, self.shortcut, nn.Conv2d(in_channels, self.out_channels, kernel_size=k, stride=1, padding=k // 2))

    def pack(self, dtype, device):
        pk = self._pk = {}
        pk["w1"], pk["b1"] = _wb(self.conv1, dtype, device)
        pk["w2"], pk["b2"] = _wb(self.conv2, dtype, device)
        pk["n1_g"], pk["n1_b"] = _norm(self.norm1, device)
        pk["n2_g"], pk["n2_b"] = _norm(self.norm2, device)
        if self.in_channels != self.out_channels:
            segs = [(s, s) for s in self.split] if self.split else None
            pk["ws"], pk["bs"] = _wb(getattr(self, self.shortcut), dtype, device, segs)

    def run(self, x, x1=None, out_scale=1.0):
        pk, co = self._pk, self.out_channels
        h = gn(x, pk, "n1", A.ACT_SILU, x1=x1)
        h = ops.conv(h, pk["w1"], pk["b1"], co, (1, 3, 3))
        h = gn(h, pk, "n2", A.ACT_SILU)
        if "ws" in pk:
            k = getattr(self, self.shortcut).kernel_size[0]
            skip = ops.conv([x] if x1 is None else [x, x1], pk["ws"], pk["bs"], co, (1, k, k))
        else:
            assert x1 is None
            skip = x
        return ops.conv(h, pk["w2"], pk["b2"], co, (1, 3, 3), res0=skip, out_scale=out_scale)


class AttnBlock(nn.Module):
    """GroupNorm, q | k | v as one 1x1 convolution into three channel slices of one buffer, one attention head as wide as
    the channels over the h*w pixels, the 1x1 projection with the residual in its epilogue."""

    @staticmethod
    def attention(qkv, c):
        """The attention entry; a subclass that runs another kernel replaces it."""
        return ops.attention_wide(qkv, 1, c, q_off=0, k_off=c, v_off=2 * c, head_stride=c)

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)

    def pack(self, dtype, device):
        pk = self._pk = {}
        pk["n_g"], pk["n_b"] = _norm(self.norm, device)
        pk["wqkv"] = pack_w(torch.cat([self.q.weight, self.k.weight, self.v.weight], dim=0), dtype, device)
        pk["bqkv"] = dev_f32(torch.cat([self.q.bias, self.k.bias, self.v.bias]), device)
        pk["wp"], pk["bp"] = _wb(self.proj_out, dtype, device)

    def run(self, x):
        pk, c = self._pk, self.in_channels
        qkv = ops.conv(gn(x, pk, "n"), pk["wqkv"], pk["bqkv"], 3 * c, (1, 1, 1))
        return ops.conv(self.attention(qkv, c), pk["wp"], pk["bp"], c, (1, 1, 1), res0=x)


class HeadConv(nn.Conv2d):
    """A bare 3x3 convolution (conv_in / conv_out), its output channels padded to a multiple of 4."""

    def pack(self, dtype, device):
        self._pk = packed_conv(self, None, dtype, device)

    def run(self, x):
        return run_conv(x, self._pk, self)


class NormOut(nn.GroupNorm):
    """The GroupNorm in front of an output convolution, with the activation that follows it (ACT_NONE or ACT_SILU)."""

    def __init__(self, channels, act=A.ACT_NONE):
        super().__init__(32, channels, eps=GN_EPS, affine=True)
        self.act = act

    def pack(self, dtype, device):
        self._pk = dict(zip(("n_g", "n_b"), _norm(self, device)))

    def run(self, x):
        return gn(x, self._pk, "n", self.act)
