"""YOLOv5-face detectors (YOLOv5n, YOLOv5l) on the HIP kernels.

Mirror of ``guided_diffusion/facelib/detection/yolov5face``: ``models/common.py`` (``Conv`` :42-54, ``StemBlock`` :57-71,
``Bottleneck`` :74-84, ``C3`` :106-117, ``ShuffleV2Block`` :120-170, ``SPP`` :173-184, ``Concat`` :197-204), ``models/yolo.py``
(``Detect`` :29-92, ``Model`` :95-132, ``parse_model`` :181-235), ``face_detector.py`` (``YoloDetector``) and the host
functions of ``utils/general.py`` / ``utils/datasets.py``, under the reference's class names, constructor arguments and
state-dict keys: ``yolov5n-face.pth`` / ``yolov5l-face.pth`` load strictly into ``Model``
(``facelib/detection/__init__.py:51-81``).  ``Focus``, ``BottleneckCSP``, ``AutoShape``, ``NMS``, ``Detections``,
``MixConv2d`` and ``CrossConv`` are left out: neither shipped configuration reaches them, and a layer table that names one
is refused at construction.  The two configurations (``models/yolov5n.yaml``, ``models/yolov5l.yaml``) are the Python
constants ``YOLOV5N`` / ``YOLOV5L`` below; nothing is parsed from text and no string is evaluated.

The ``nn.Module`` classes are parameter containers with a ``pack()`` / ``run()`` pair on float32 NHWC clip tensors, like the
RetinaFace modules:
  * every ``Conv`` (Conv2d + eval BatchNorm + SiLU) is ONE ``flair_conv_nhwc`` launch (``FLAIR_ACT_SILU``), the BatchNorm
    folded into the packed weights; a ``Bottleneck``'s shortcut is that launch's ``res0``;
  * every ``Concat`` / ``torch.cat`` is input segments of the consuming convolution or channel-slice outputs of the
    producing ones -- no copy is made;
  * ``nn.Upsample(2, 'nearest')`` is ``flair_resize_nhwc``; the ShuffleNetV2 depthwise 3x3 (BatchNorm folded, no
    activation) is ``flair_dwconv_nhwc`` without its 1x1 stage, the 1x1 + SiLU around it ``flair_conv_nhwc``;
  * StemBlock's ceil-mode pool, SPP's three pools, ``cat`` + ``channel_shuffle(2)``, Detect's decode and the letterbox
    pre-processing are the five entries of ``csrc/detect.hip``.
Candidate selection, NMS and the rescaling to frame pixels run on the host in numpy (``non_max_suppression_face``,
``scale_coords`` ...), as the RetinaFace decoding does.  ``torchvision.ops.nms`` and ``cv2`` are not importable here, so the
greedy NMS is restated (PARITY UNPINNED against torchvision; the fixture's generator uses the same restatement) and the
``target_size`` resize of uint8 images is not built.  float32 only (``detection/__init__.py:73``).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from .. import ops as A
from .packing import PackedModel, fold_bn, packed_conv, run_conv

# ---------------------------------------------------------------------------------------------- configurations
# models/yolov5n.yaml, models/yolov5l.yaml: (from, number, kind, args) per layer; "nc" / "anchors" in Detect's args stand for
# the table's own entries, as in the yaml.
ANCHORS = ((4, 5, 8, 10, 13, 16), (23, 29, 43, 55, 73, 105), (146, 217, 231, 300, 335, 433))      # P3/8, P4/16, P5/32

YOLOV5N = {
    "nc": 1, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": ANCHORS,
    "backbone": ((-1, 1, "StemBlock", (32, 3, 2)),            # 0-P2/4
                 (-1, 1, "ShuffleV2Block", (128, 2)),         # 1-P3/8
                 (-1, 3, "ShuffleV2Block", (128, 1)),         # 2
                 (-1, 1, "ShuffleV2Block", (256, 2)),         # 3-P4/16
                 (-1, 7, "ShuffleV2Block", (256, 1)),         # 4
                 (-1, 1, "ShuffleV2Block", (512, 2)),         # 5-P5/32
                 (-1, 3, "ShuffleV2Block", (512, 1))),        # 6
    "head": ((-1, 1, "Conv", (128, 1, 1)),
             (-1, 1, "nn.Upsample", (None, 2, "nearest")),
             ((-1, 4), 1, "Concat", (1,)),                    # cat backbone P4
             (-1, 1, "C3", (128, False)),                     # 10
             (-1, 1, "Conv", (128, 1, 1)),
             (-1, 1, "nn.Upsample", (None, 2, "nearest")),
             ((-1, 2), 1, "Concat", (1,)),                    # cat backbone P3
             (-1, 1, "C3", (128, False)),                     # 14 (P3/8-small)
             (-1, 1, "Conv", (128, 3, 2)),
             ((-1, 11), 1, "Concat", (1,)),                   # cat head P4
             (-1, 1, "C3", (128, False)),                     # 17 (P4/16-medium)
             (-1, 1, "Conv", (128, 3, 2)),
             ((-1, 7), 1, "Concat", (1,)),                    # cat head P5
             (-1, 1, "C3", (128, False)),                     # 20 (P5/32-large)
             ((14, 17, 20), 1, "Detect", ("nc", "anchors"))),
}

YOLOV5L = {
    "nc": 1, "depth_multiple": 1.0, "width_multiple": 1.0, "anchors": ANCHORS,
    "backbone": ((-1, 1, "StemBlock", (64, 3, 2)),            # 0-P1/2
                 (-1, 3, "C3", (128,)),
                 (-1, 1, "Conv", (256, 3, 2)),                # 2-P3/8
                 (-1, 9, "C3", (256,)),
                 (-1, 1, "Conv", (512, 3, 2)),                # 4-P4/16
                 (-1, 9, "C3", (512,)),
                 (-1, 1, "Conv", (1024, 3, 2)),               # 6-P5/32
                 (-1, 1, "SPP", (1024, (3, 5, 7))),
                 (-1, 3, "C3", (1024, False))),               # 8
    "head": ((-1, 1, "Conv", (512, 1, 1)),
             (-1, 1, "nn.Upsample", (None, 2, "nearest")),
             ((-1, 5), 1, "Concat", (1,)),                    # cat backbone P4
             (-1, 3, "C3", (512, False)),                     # 12
             (-1, 1, "Conv", (256, 1, 1)),
             (-1, 1, "nn.Upsample", (None, 2, "nearest")),
             ((-1, 3), 1, "Concat", (1,)),                    # cat backbone P3
             (-1, 3, "C3", (256, False)),                     # 16 (P3/8-small)
             (-1, 1, "Conv", (256, 3, 2)),
             ((-1, 13), 1, "Concat", (1,)),                   # cat head P4
             (-1, 3, "C3", (512, False)),                     # 19 (P4/16-medium)
             (-1, 1, "Conv", (512, 3, 2)),
             ((-1, 9), 1, "Concat", (1,)),                    # cat head P5
             (-1, 3, "C3", (1024, False)),                    # 22 (P5/32-large)
             ((16, 19, 22), 1, "Detect", ("nc", "anchors"))),
}

CONFIGS = {"yolov5n": YOLOV5N, "yolov5l": YOLOV5L}
UNBUILT_KINDS = ("Focus", "BottleneckCSP", "AutoShape", "NMS", "Detections", "MixConv2d", "CrossConv", "DWConv")


def autopad(k, p=None):
    """common.py:18-22."""
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


def make_divisible(x, divisor):
    """general.py:17-19."""
    return math.ceil(x / divisor) * divisor


def check_img_size(img_size, s=32):
    """general.py:9-14."""
    return make_divisible(img_size, int(s))


# ---------------------------------------------------------------------------------------------- modules
class Conv(nn.Module):
    """common.py:42-54: Conv2d(bias=False) + BatchNorm2d + SiLU -- one flair_conv_nhwc launch."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        if g != 1 or act is not True or autopad(k, p) != k // 2 or s not in (1, 2):
            raise NotImplementedError(f"flair_amd: Conv(k={k}, s={s}, p={p}, g={g}, act={act}) is not built (groups 1, SiLU, "
                                      "'same' padding, stride 1 or 2)")
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU()

    def pack(self, dtype, device):
        self._pk = packed_conv(self.conv, self.bn, dtype, device)

    def run(self, x, out=None, res0=None):
        """x: a clip tensor or a list of them (the segments of a torch.cat); out: optional channel-slice view."""
        return run_conv(x, self._pk, self.conv, A.ACT_SILU, out=out, res0=res0)


class StemBlock(nn.Module):
    """common.py:57-71.  stem_2b and the ceil-mode pool write the two channel halves of the buffer stem_3 reads."""

    def __init__(self, c1, c2, k=3, s=2, p=None, g=1, act=True):
        super().__init__()
        self.stem_1 = Conv(c1, c2, k, s, p, g, act)
        self.stem_2a = Conv(c2, c2 // 2, 1, 1, 0)
        self.stem_2b = Conv(c2 // 2, c2, 3, 2, 1)
        self.stem_2p = nn.MaxPool2d(kernel_size=2, stride=2, ceil_mode=True)
        self.stem_3 = Conv(c2 * 2, c2, 1, 1, 0)
        self.c2 = c2

    def run(self, x):
        c2 = self.c2
        s1 = self.stem_1.run(x)
        T, H, W, _ = s1.shape
        cat = torch.empty((T, (H + 1) // 2, (W + 1) // 2, 2 * c2), dtype=s1.dtype, device=s1.device)
        self.stem_2b.run(self.stem_2a.run(s1), out=cat[..., :c2])
        ops.maxpool2x2s2(s1, out=cat[..., c2:])
        return self.stem_3.run(cat)


class Bottleneck(nn.Module):
    """common.py:74-84; the shortcut is cv2's res0."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def run(self, x, out=None):
        return self.cv2.run(self.cv1.run(x), out=out, res0=x if self.add else None)


class C3(nn.Module):
    """common.py:106-117: cv3(cat(m(cv1(x)), cv2(x))) -- the last Bottleneck and cv2 write the two halves of cv3's input."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)))
        self.c_ = c_

    def run(self, x):
        c_ = self.c_
        x0 = x[0] if isinstance(x, (list, tuple)) else x
        T, H, W, _ = x0.shape
        cat = torch.empty((T, H, W, 2 * c_), dtype=x0.dtype, device=x0.device)
        self.cv2.run(x, out=cat[..., c_:])
        n = len(self.m)
        h = self.cv1.run(x, out=cat[..., :c_] if n == 0 else None)
        for i, blk in enumerate(self.m):
            h = blk.run(h, out=cat[..., :c_] if i == n - 1 else None)
        return self.cv3.run(cat)


def _pack_dw(conv, bn, dtype, device):
    """ShuffleV2Block's depthwise 3x3 + BatchNorm (no activation) for flair_dwconv_nhwc without its 1x1 stage: (w (9, c), b)."""
    assert dtype == torch.float32
    w, b = fold_bn(conv, bn)                                                # (c, 1, 3, 3)
    return w.reshape(conv.out_channels, 9).t().contiguous().to(device), b.contiguous().to(device)


def _run_dw(x, wb, conv):
    return ops.dwconv(x, wb[0], wb[1], stride=conv.stride[0], act=A.ACT_NONE)


class ShuffleV2Block(nn.Module):
    """common.py:120-170.  cat + channel_shuffle(2) is flair_channel_interleave_nhwc; a stride-1 unit's x.chunk(2) halves are
    channel-slice views of its input."""

    def __init__(self, inp, oup, stride):
        super().__init__()
        if not 1 <= stride <= 3:
            raise ValueError("illegal stride value")
        if stride == 3:
            raise NotImplementedError("flair_amd: ShuffleV2Block(stride=3) is not built (flair_dwconv_nhwc: stride 1 or 2)")
        self.stride = stride
        bf = oup // 2
        if stride > 1:
            self.branch1 = nn.Sequential(self.depthwise_conv(inp, inp, kernel_size=3, stride=stride, padding=1), nn.BatchNorm2d(inp),
                                         nn.Conv2d(inp, bf, kernel_size=1, stride=1, padding=0, bias=False), nn.BatchNorm2d(bf),
                                         nn.SiLU())
        else:
            self.branch1 = nn.Sequential()
        self.branch2 = nn.Sequential(nn.Conv2d(inp if stride > 1 else bf, bf, kernel_size=1, stride=1, padding=0, bias=False),
                                     nn.BatchNorm2d(bf), nn.SiLU(),
                                     self.depthwise_conv(bf, bf, kernel_size=3, stride=stride, padding=1), nn.BatchNorm2d(bf),
                                     nn.Conv2d(bf, bf, kernel_size=1, stride=1, padding=0, bias=False), nn.BatchNorm2d(bf), nn.SiLU())
        self.bf = bf

    @staticmethod
    def depthwise_conv(i, o, kernel_size, stride=1, padding=0, bias=False):
        return nn.Conv2d(i, o, kernel_size, stride, padding, bias=bias, groups=i)

    def pack(self, dtype, device):
        b1, b2 = self.branch1, self.branch2
        self._pk = dict(pw2a=packed_conv(b2[0], b2[1], dtype, device), dw2=_pack_dw(b2[3], b2[4], dtype, device),
                        pw2b=packed_conv(b2[5], b2[6], dtype, device))
        if self.stride > 1:
            self._pk.update(dw1=_pack_dw(b1[0], b1[1], dtype, device), pw1=packed_conv(b1[2], b1[3], dtype, device))

    def run(self, x):
        pk, b1, b2, bf = self._pk, self.branch1, self.branch2, self.bf
        if self.stride == 1:
            a, x2 = x[..., :bf], x[..., bf:]                          # x.chunk(2, dim=1)
        else:
            a, x2 = run_conv(_run_dw(x, pk["dw1"], b1[0]), pk["pw1"], b1[2], A.ACT_SILU), x
        h = run_conv(x2, pk["pw2a"], b2[0], A.ACT_SILU)
        h = run_conv(_run_dw(h, pk["dw2"], b2[3]), pk["pw2b"], b2[5], A.ACT_SILU)
        return ops.channel_interleave(a, h)


class SPP(nn.Module):
    """common.py:173-184: cv1 writes channel slice 0 of a 4 c_ wide buffer, flair_spp_maxpool_nhwc fills slices 1..3, cv2 reads
    the buffer as one segment."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        k = tuple(k)
        if len(k) != 3 or any(v % 2 == 0 or not 3 <= v <= 13 for v in k) or not k[0] < k[1] < k[2]:
            raise NotImplementedError(f"flair_amd: SPP(k={k}) is not built (three odd, strictly increasing sizes from 3 to 13)")
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])
        self.k, self.c_ = k, c_

    def run(self, x):
        x0 = x[0] if isinstance(x, (list, tuple)) else x
        T, H, W, _ = x0.shape
        buf = torch.empty((T, H, W, 4 * self.c_), dtype=x0.dtype, device=x0.device)
        self.cv1.run(x, out=buf[..., :self.c_])
        ops.spp_maxpool(buf, self.c_, self.k)
        return self.cv2.run(buf)


class Concat(nn.Module):
    """common.py:197-204: the inputs stay where they are and travel as the segments of the consuming convolution."""

    def __init__(self, dimension=1):
        super().__init__()
        if dimension != 1:
            raise NotImplementedError("flair_amd: Concat along the channels only (dimension=1)")
        self.d = dimension

    def run(self, xs):
        out = []
        for x in xs:
            out.extend(x if isinstance(x, (list, tuple)) else [x])
        return out


class Upsample(nn.Upsample):
    """nn.Upsample(None, 2, 'nearest') on flair_resize_nhwc."""

    def run(self, x):
        if self.mode != "nearest" or self.size is not None or float(self.scale_factor) != 2.0:
            raise NotImplementedError("flair_amd: nn.Upsample(None, 2, 'nearest') only")
        T, H, W, C = x.shape
        return ops.resize(x, (2 * H, 2 * W), ops.RESIZE_NEAREST, out=torch.empty((T, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device))


class Detect(nn.Module):
    """yolo.py:29-92.  run(): the biased 1x1 head convolutions, then flair_yolo_face_decode of each level straight into its
    rows of z (B, N, 16)."""
    stride = None
    export = False

    def __init__(self, nc=80, anchors=(), ch=()):
        super().__init__()
        self.nc = nc
        self.no = nc + 5 + 10
        if self.no != 16:
            raise NotImplementedError(f"flair_amd: Detect(nc={nc}) gives no = {self.no}; flair_yolo_face_decode is built for no = 16 (nc = 1)")
        self.nl = len(anchors)
        self.na = len(anchors[0]) // 2
        a = torch.tensor(anchors).float().view(self.nl, -1, 2)
        self.register_buffer("anchors", a)                                              # (nl, na, 2), divided by the stride by Model
        self.register_buffer("anchor_grid", a.clone().view(self.nl, 1, -1, 1, 1, 2))    # (nl, 1, na, 1, 1, 2), pixels
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)

    def pack(self, dtype, device):
        self._pk = dict(heads=[packed_conv(m, None, dtype, device) for m in self.m],
                        anchor_grid=self.anchor_grid.detach().float().cpu().view(self.nl, self.na, 2).tolist())

    def run(self, xs):
        """-> (z (B, N, 16), [raw head outputs (B, ny, nx, na * 16)])."""
        pk = self._pk
        raw = [run_conv(x, pk["heads"][i], self.m[i]) for i, x in enumerate(xs)]
        B = raw[0].shape[0]
        rows = [self.na * r.shape[1] * r.shape[2] for r in raw]
        z = torch.empty((B, sum(rows), self.no), dtype=torch.float32, device=raw[0].device)
        row0 = 0
        for i, r in enumerate(raw):
            ops.yolo_face_decode(r, self.na, self.strides[i], pk["anchor_grid"][i], z, row0, no=self.no)
            row0 += rows[i]
        return z, raw


_KINDS = {"Conv": Conv, "StemBlock": StemBlock, "Bottleneck": Bottleneck, "C3": C3, "ShuffleV2Block": ShuffleV2Block, "SPP": SPP,
          "Concat": Concat, "nn.Upsample": Upsample, "Detect": Detect}


def _stride_factor(kind, args, n):
    """The factor by which ``n`` layers of ``kind`` with the table's ``args`` divide the resolution: the strides of the
    Detect levels come from the table, not from a dummy forward (yolo.py:113-114)."""
    if kind == "StemBlock":                      # (c2, k, s): stem_1 has stride s, stem_2b / stem_2p stride 2
        return args[2] * 2
    if kind == "Conv":                           # (c2, k, s)
        return args[2] if len(args) > 2 else 1
    if kind == "ShuffleV2Block":                 # (c2, s)
        return args[1] ** n
    if kind == "nn.Upsample":                    # (size, scale_factor, mode)
        return 1.0 / args[1]
    return 1


def parse_model(d, ch):
    """yolo.py:181-235 on a table of this module: -> (nn.Sequential of the layers, sorted save list, the stride of every
    layer's output; for Detect the list of its levels' strides).  ``ch`` keeps the input width at index 0, so layer i's
    width is ch[i + 1], as in the reference."""
    anchors, nc, gd, gw = d["anchors"], d["nc"], d["depth_multiple"], d["width_multiple"]
    na = len(anchors[0]) // 2
    no = na * (nc + 5)
    layers, save, c2 = [], [], ch[-1]
    strides = []
    for i, (f, n, kind, args) in enumerate(tuple(d["backbone"]) + tuple(d["head"])):
        if kind not in _KINDS:
            why = "is left out of this package (no shipped configuration uses it)" if kind in UNBUILT_KINDS else "is unknown"
            raise NotImplementedError(f"flair_amd: layer {i} of the YOLOv5-face table is a {kind}, which {why}")
        m = _KINDS[kind]
        args = [nc if isinstance(a, str) and a == "nc" else (anchors if isinstance(a, str) and a == "anchors" else a) for a in args]
        n = max(round(n * gd), 1) if n > 1 else n
        first = f if isinstance(f, int) else f[0]
        src = (strides[-1] if strides else 1) if first == -1 else strides[first]
        strides.append([strides[x] for x in f] if m is Detect else src * _stride_factor(kind, args, n))
        if m in (Conv, Bottleneck, SPP, C3, ShuffleV2Block, StemBlock):
            c1, c2 = ch[f], args[0]
            c2 = make_divisible(c2 * gw, 8) if c2 != no else c2
            args = [c1, c2, *args[1:]]
            if m is C3:
                args.insert(2, n)
                n = 1
        elif m is Concat:
            c2 = sum(ch[-1 if x == -1 else x + 1] for x in f)
        elif m is Detect:
            args.append([ch[x + 1] for x in f])
        else:
            c2 = ch[f]
        m_ = nn.Sequential(*(m(*args) for _ in range(n))) if n > 1 else m(*args)
        m_.i, m_.f, m_.type = i, f, kind
        m_.np = sum(x.numel() for x in m_.parameters())
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save), strides


def _table(cfg):
    if isinstance(cfg, dict):
        return cfg, "custom"
    name = os.path.basename(str(cfg))
    for key in CONFIGS:
        if name in (key, key + ".yaml"):
            return CONFIGS[key], key + ".yaml"
    raise ValueError(f"flair_amd: cfg={cfg!r}: 'yolov5n', 'yolov5l', or a path whose file name is yolov5n.yaml / yolov5l.yaml")


class Model(PackedModel, nn.Module):
    """yolo.py:95-132.  ``cfg``: "yolov5n" / "yolov5l", a path whose file name is ``yolov5n.yaml`` / ``yolov5l.yaml`` (what
    the reference passes; the file is not read), or a table of this module's form."""

    def __init__(self, cfg="yolov5n", ch=3, nc=None):
        super().__init__()
        table, self.yaml_file = _table(cfg)
        self.yaml = dict(table)
        ch = self.yaml["ch"] = self.yaml.get("ch", ch)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save, strides = parse_model(self.yaml, ch=[ch])
        self.names = [str(i) for i in range(self.yaml["nc"])]
        m = self.model[-1]
        if isinstance(m, Detect):
            m.strides = [float(s) for s in strides[-1]]                          # what run hands to the decode kernel
            m.stride = torch.tensor(m.strides)
            m.anchors /= m.stride.view(-1, 1, 1)                                 # yolo.py:114-115
            a = m.anchor_grid.prod(-1).view(-1)                                  # check_anchor_order: the shipped tables ascend
            assert (a[-1] - a[0]).sign() == (m.stride[-1] - m.stride[0]).sign(), "anchors must ascend with the strides"
            self.stride = m.stride
            self._initialize_biases()
        self._loaded = False
        self.eval()

    def _initialize_biases(self, cf=None):
        """yolo.py:134-141."""
        m = self.model[-1]
        for mi, s in zip(m.m, m.stride):
            b = mi.bias.detach().view(m.na, -1).clone()
            b[:, 4] += math.log(8 / (640 / float(s)) ** 2)
            b[:, 5:] += math.log(0.6 / (m.nc - 0.99))
            mi.bias = torch.nn.Parameter(b.view(-1), requires_grad=True)

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = super().load_state_dict(state_dict, *args, **kwargs)
        if not out.missing_keys:                        # a non-strict load that leaves tensors unset does not count as loaded
            self._loaded = True
        return out

    def run_clip(self, x, taps=None):
        """x: (B, H, W, 16) float32 clip tensor (channels 0-2 the image in [0, 1], the rest zero) -> (z (B, N, 16), raw head
        outputs).  ``taps``: optional dict whose keys are layer indices; filled with those layers' outputs (tests)."""
        self._ensure_packed(x.device)
        y = []
        for m in self.model:
            if m.f != -1:
                x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
            for blk in (m if type(m) is nn.Sequential else [m]):
                x = blk.run(x)
            if taps is not None and m.i in taps:
                taps[m.i] = x
            y.append(x if m.i in self.save else None)
        return x

    def to_clip(self, inputs):
        if not inputs.is_cuda:
            raise _lib.FlairHipError("flair_amd YOLOv5-face needs its input in HBM (device='cuda'); no CPU path exists")
        B, _, H, W = inputs.shape
        x = torch.zeros((B, H, W, ops.pad_channels(3, self.dtype)), dtype=self.dtype, device=inputs.device)
        return ops.nchw_to_clip(inputs.float().contiguous(), x, 0)

    @torch.no_grad()
    def forward(self, x):
        """(B, 3, H, W) float images in [0, 1], H and W multiples of 32 -> (z (B, N, 16), [x_i (B, na, ny, nx, 16)]), the
        reference's inference output."""
        z, raw = self.run_clip(self.to_clip(x))
        na, no = self.model[-1].na, self.model[-1].no
        return z, [r[..., :na * no].reshape(r.shape[0], r.shape[1], r.shape[2], na, no).permute(0, 3, 1, 2, 4) for r in raw]


# ---------------------------------------------------------------------------------------------- host side (numpy)
def xywh2xyxy(x):
    """general.py:32-39."""
    y = np.copy(x)
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def nms(boxes, scores, iou_thres):
    """``torchvision.ops.nms``, restated: greedy suppression in decreasing score order, areas (x2 - x1) * (y2 - y1) without a
    ``+ 1``, a box is suppressed when its IoU with a kept one is > iou_thres; float32 arithmetic.  Returns the kept indices in
    decreasing score order.  (``retinaface_utils.py_cpu_nms`` has the ``+ 1``.)  PARITY UNPINNED: torchvision is not importable
    here."""
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    areas = (x2 - x1) * (y2 - y1)
    order = np.argsort(-scores, kind="stable")
    suppressed = np.zeros(len(scores), dtype=bool)
    keep = []
    for _i, i in enumerate(order):
        if suppressed[i]:
            continue
        keep.append(int(i))
        rest = order[_i + 1:]
        w = np.maximum(np.float32(0), np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
        h = np.maximum(np.float32(0), np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]))
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[rest] - inter)
        suppressed[rest[ovr > np.float32(iou_thres)]] = True
    return np.asarray(keep, dtype=np.int64)


def non_max_suppression_face(prediction, conf_thres=0.25, iou_thres=0.45):
    """general.py:89-165 for nc = 1: prediction (B, N, 16) -> per image an (n, 16) float32 array (x1, y1, x2, y2, conf, ten
    landmark coordinates, class), best first.  The candidate test is on objectness, then on objectness * class score."""
    prediction = np.asarray(prediction, dtype=np.float32)
    if prediction.shape[2] != 16:
        raise NotImplementedError(f"flair_amd: non_max_suppression_face is built for nc = 1 (16 columns), got {prediction.shape[2]}")
    max_wh = 4096
    output = [np.zeros((0, 16), dtype=np.float32) for _ in range(prediction.shape[0])]
    for xi, x in enumerate(prediction):
        x = x[x[:, 4] > conf_thres].copy()
        if not x.shape[0]:
            continue
        x[:, 15:] *= x[:, 4:5]                                   # conf = obj_conf * cls_conf
        box = xywh2xyxy(x[:, :4])
        conf = x[:, 15:16]                                       # best (only) class
        x = np.concatenate((box, conf, x[:, 5:15], np.zeros_like(conf)), axis=1)[conf[:, 0] > conf_thres]
        if not x.shape[0]:
            continue
        c = x[:, 15:16] * max_wh
        keep = nms(x[:, :4] + c, x[:, 4], iou_thres)
        output[xi] = x[keep]
    return output


def clip_coords(boxes, img_shape):
    """general.py:58-63 (in place)."""
    boxes[:, 0] = boxes[:, 0].clip(0, img_shape[1])
    boxes[:, 1] = boxes[:, 1].clip(0, img_shape[0])
    boxes[:, 2] = boxes[:, 2].clip(0, img_shape[1])
    boxes[:, 3] = boxes[:, 3].clip(0, img_shape[0])


def _gain_pad(img1_shape, img0_shape):
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    return gain, ((img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2)


def scale_coords(img1_shape, coords, img0_shape):
    """general.py:42-55: xyxy boxes from the letterboxed img1_shape to img0_shape, in place (float32, like the tensors of the
    reference)."""
    gain, pad = _gain_pad(img1_shape, img0_shape)
    coords[:, [0, 2]] -= np.float32(pad[0])
    coords[:, [1, 3]] -= np.float32(pad[1])
    coords[:, :4] /= np.float32(gain)
    clip_coords(coords, img0_shape)
    return coords


def scale_coords_landmarks(img1_shape, coords, img0_shape):
    """general.py:249-271, in place."""
    gain, pad = _gain_pad(img1_shape, img0_shape)
    coords[:, [0, 2, 4, 6, 8]] -= np.float32(pad[0])
    coords[:, [1, 3, 5, 7, 9]] -= np.float32(pad[1])
    coords[:, :10] /= np.float32(gain)
    for j in range(10):
        coords[:, j] = coords[:, j].clip(0, img0_shape[1] if j % 2 == 0 else img0_shape[0])
    return coords


def letterbox_geometry(h0, w0, stride_max=32):
    """What YoloDetector._preprocess and letterbox (face_detector.py:66-69, datasets.py:5-35: new_shape = imgsz, auto=True,
    scaleup=True) do to an h0 x w0 image: -> (new_unpad (w, h), (top, bottom, left, right))."""
    imgsz = check_img_size(max(h0, w0), s=stride_max)
    r = min(imgsz / h0, imgsz / w0)
    new_unpad = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = imgsz - new_unpad[0], imgsz - new_unpad[1]
    dw, dh = np.mod(dw, 64), np.mod(dh, 64)
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_unpad, (top, bottom, left, right)


def postprocess(pred, net_hw, orig_shapes, conf_thres, iou_thres, min_face=10):
    """YoloDetector._postprocess (face_detector.py:81-133) on a host copy of z: -> per image (float (n, 15) array: box, score,
    landmarks in frame pixels, best first; int boxes (n, 4); int landmarks (n, 10)), the ``min_face`` filter applied to the
    truncated boxes like the reference.  The reference's ``.round()`` calls discard their result; so nothing is rounded."""
    out = []
    dets = non_max_suppression_face(pred, conf_thres, iou_thres)
    for det, shape in zip(dets, orig_shapes):
        h, w = int(shape[0]), int(shape[1])
        det = det.copy()
        box = scale_coords(net_hw, det[:, :4], (h, w))
        lms = scale_coords_landmarks(net_hw, det[:, 5:15], (h, w))
        gn = np.array([w, h, w, h], dtype=np.float32)
        gl = np.array([w, h] * 5, dtype=np.float32)
        ibox = ((box / gn).astype(np.float64) * np.array([w, h, w, h], dtype=np.float64)).astype(np.int64)    # int() truncates
        ilms = ((lms / gl).astype(np.float64) * np.array([w, h] * 5, dtype=np.float64)).astype(np.int64)
        ok = ibox[:, 3] - ibox[:, 1] >= min_face
        out.append((np.concatenate((box, det[:, 4:5], lms), axis=1)[ok], ibox[ok], ilms[ok]))
    return out


class YoloDetector:
    """face_detector.py:35-198, plus ``batched_detect_faces`` with the RetinaFace method's contract (the reference's helper
    calls it, face_restoration_helper.py:149, and its YoloDetector has none).  The network must have been loaded
    (``load_state_dict`` here or on ``.detector``) before it detects; ``allow_random_init=True`` is the opt-out for tests."""

    def __init__(self, config_name, min_face=10, target_size=None, device="cuda", allow_random_init=False):
        if target_size is not None:
            raise NotImplementedError("flair_amd: YoloDetector(target_size=...) is not built (a cv2.resize of the uint8 input)")
        self.target_size = target_size
        self.min_face = min_face
        self.detector = Model(cfg=config_name)
        self.device = torch.device(device)
        self.allow_random_init = allow_random_init
        self.model_name = {"yolov5n.yaml": "YOLOv5n", "yolov5l.yaml": "YOLOv5l"}.get(self.detector.yaml_file, "YOLOv5")
        self.detector.to(self.device)

    def load_state_dict(self, state_dict, strict=True):
        return self.detector.load_state_dict(state_dict, strict=strict)

    def _check_loaded(self):
        if not (self.detector._loaded or self.allow_random_init):
            raise RuntimeError("flair_amd: this YoloDetector holds random weights: load yolov5n-face.pth / yolov5l-face.pth with "
                               "load_state_dict first (allow_random_init=True is the opt-out for tests)")

    @torch.no_grad()
    def _detect_raw(self, frames, pre, scale):
        """frames: (B, 3, H, W) float tensor -> (z on the host (B, N, 16), letterboxed (Ho, Wo))."""
        self._check_loaded()
        frames = frames.to(self.device)
        if not frames.is_cuda:
            raise _lib.FlairHipError("flair_amd YoloDetector needs its input in HBM (device='cuda'); no CPU path exists")
        B, _, H, W = frames.shape
        (nw, nh), (top, bottom, left, right) = letterbox_geometry(H, W, int(self.detector.stride.max()))
        Ho, Wo = nh + top + bottom, nw + left + right
        x = ops.letterbox(frames.float().contiguous(), (nh, nw), (top, left), (Ho, Wo),
                          pre=pre if pre is not None else (1.0, 0.0, float("-inf"), float("inf")), scale=scale)
        z, _ = self.detector.run_clip(x)
        return z.cpu().numpy(), (Ho, Wo)

    def detect_faces(self, imgs, conf_thres=0.7, iou_thres=0.5):
        """imgs: a BGR (H, W, 3) array or a list of them (all of one size) -> (n, 15) int array over all images: box, x1
        again (face_detector.py:165-169), five landmarks; None when nothing is found."""
        images = imgs if isinstance(imgs, list) else [imgs]
        self._check_loaded()
        arr = np.stack([np.asarray(im)[:, :, ::-1] for im in images]).astype(np.float32)            # BGR -> RGB
        frames = torch.from_numpy(np.ascontiguousarray(arr.transpose(0, 3, 1, 2)))
        z, net_hw = self._detect_raw(frames, None, 1.0 / 255.0)
        res = postprocess(z, net_hw, [im.shape for im in images], conf_thres, iou_thres, self.min_face)
        return self._assemble([r[1] for r in res], [r[2] for r in res])

    @staticmethod
    def _assemble(bboxes, points):
        """The return statement of detect_faces (face_detector.py:163-171)."""
        if sum(len(p) for p in points) == 0:
            return None
        bboxes = np.concatenate(bboxes).reshape(-1, 4)
        points = np.concatenate(points).reshape(-1, 10)
        return np.concatenate((bboxes, bboxes[:, 0].reshape(-1, 1), points), axis=1)

    @torch.no_grad()
    def batched_detect_faces(self, frames, conf_threshold=0.7, nms_threshold=0.5, pre=None, keep_empty=False):
        """frames: (B, 3, H, W) float tensor in [0, 255] after ``pre`` = (a, b, lo, hi) (clamp(a x + b, lo, hi); None: as they
        are), in the channel order they have.  Returns one (n_i, 15) float32 array per frame that has detections: box, score,
        five landmarks in frame pixels (not truncated), best first, ``min_face`` applied; ``keep_empty``: one entry per frame,
        a (0, 15) array for a frame without a detection (RetinaFace.batched_detect_faces' contract)."""
        B, _, H, W = frames.shape
        z, net_hw = self._detect_raw(frames, pre, 1.0 / 255.0)
        res = postprocess(z, net_hw, [(H, W)] * B, conf_threshold, nms_threshold, self.min_face)
        return [r[0] for r in res if keep_empty or len(r[0])]
