"""BiSeNet face parsing on the HIP kernels: the second parser of ``facelib/parsing/__init__.py:8-25`` (its default).

Mirror of the reference's ``guided_diffusion/facelib/parsing/bisenet.py`` and ``resnet.py``: ``BiSeNet(num_class)``,
``forward(x, return_feat=False) -> (out, out16, out32[, feat, feat16, feat32])`` as NCHW tensors at the input size, the
reference's module tree and state-dict names (191 entries, 13 300 416 parameters: ``parsing_bisenet.pth`` loads unchanged
through ``checkpoint.load_reference_checkpoint``).

The modules are parameter containers.  Every Conv2d + eval BatchNorm (+ ReLU) is ONE ``flair_conv_nhwc`` launch with the
BatchNorm folded into the packed weights: the 7x7 stride-2 stem, the BasicBlocks' 3x3 convolutions and their 1x1
stride-2 ``downsample``, the heads.  ``relu(shortcut + residual)`` is ``flair_add_act_nhwc``, the stem pool
``flair_maxpool3x3s2_nhwc``, the nearest enlargements ``flair_resize_nhwc``; ``torch.cat([fsp, fcp])`` is the two input
segments of the fusion module's 1x1 convolution.  The attention modules run on the three entries of ``parse.hip``:
``flair_global_avgpool_nhwc`` for ``F.avg_pool2d(feat, feat.size()[2:])``, ``ops.linear`` for the one-pixel 1x1
convolutions behind it (``conv_atten`` with ``bn_atten`` folded, ``conv_avg``, ``conv1`` / ReLU / ``conv2``), and one
``flair_channel_gate_nhwc`` launch each for ``arm32(feat32) + avg_up``, ``arm16(feat16) + feat32_up`` and
``feat * atten + feat`` (the sigmoid is evaluated by the gate kernel).

``forward`` enlarges the class logits with ``flair_resize_nhwc`` (bilinear, align_corners=True) like the reference.  The
two consumers of the parsing MAP do not: ``parse_indices`` and ``face_weight`` hand the 1/8-resolution logits of the main
head to ``flair_upsample_argmax_nhwc``, which writes the arg-max of the enlarged logits (and the weight looked up from
it) without the enlarged tensor -- 10 x 512 x 512 x 19 floats per sampler step otherwise -- and skip the two auxiliary heads,
whose outputs the reference computes and drops there.

float32 by default, like ParseNet; ``convert_to_bf16()`` switches the activations and packed weights to bfloat16.
"""
import torch
import torch.nn as nn

from .. import _lib, ops
from .. import ops as A
from .retinaface import _conv, _fold, _fold_bn


class ConvBNReLU(nn.Module):
    """bisenet.py:8-19."""

    def __init__(self, in_chan, out_chan, ks=3, stride=1, padding=1):
        super().__init__()
        if ks % 2 != 1 or padding != ks // 2:
            raise NotImplementedError(f"flair_amd: BiSeNet ConvBNReLU with ks={ks}, padding={padding} (odd kernels padded by ks // 2 only)")
        self.conv = nn.Conv2d(in_chan, out_chan, kernel_size=ks, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_chan)

    def pack(self, dtype, device):
        self._p = _fold(self.conv, self.bn, dtype, device)
        w, b = _fold_bn(self.conv, self.bn)                     # the same layer on a 1x1 map (conv_avg): a matrix
        self._lin = (w.reshape(w.shape[0], -1).to(device).contiguous(), b.to(device).contiguous()) if w.shape[2] == 1 else None

    def run(self, x):
        return _conv(x, self._p, self.conv, A.ACT_RELU)


class BiSeNetOutput(nn.Module):
    """bisenet.py:22-33."""

    def __init__(self, in_chan, mid_chan, num_class):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, mid_chan, ks=3, stride=1, padding=1)
        self.conv_out = nn.Conv2d(mid_chan, num_class, kernel_size=1, bias=False)

    def pack(self, dtype, device):
        self.conv.pack(dtype, device)
        g = 16 // torch.empty((), dtype=dtype).element_size()    # class vectors padded to whole 16-byte chunks
        n = self.conv_out.out_channels
        self._p = _fold(self.conv_out, None, dtype, device, cout_pad=(n + g - 1) // g * g)

    def run(self, x):
        feat = self.conv.run(x)
        return _conv(feat, self._p, self.conv_out, A.ACT_NONE), feat


def _linear(x, w, b, act=A.ACT_NONE):
    """ops.linear on (F, K) rows, 32 rows per launch."""
    if x.shape[0] <= 32:
        return ops.linear(x, w, b, act_out=act)
    return torch.cat([ops.linear(x[i:i + 32].contiguous(), w, b, act_out=act) for i in range(0, x.shape[0], 32)])


class AttentionRefinementModule(nn.Module):
    """bisenet.py:36-52."""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, out_chan, ks=3, stride=1, padding=1)
        self.conv_atten = nn.Conv2d(out_chan, out_chan, kernel_size=1, bias=False)
        self.bn_atten = nn.BatchNorm2d(out_chan)
        self.sigmoid_atten = nn.Sigmoid()

    def pack(self, dtype, device):
        self.conv.pack(dtype, device)
        w, b = _fold_bn(self.conv_atten, self.bn_atten)
        self._w, self._b = w.reshape(w.shape[0], -1).to(device).contiguous(), b.to(device).contiguous()

    def run(self, x, bias=None, add=None):
        """torch.mul(feat, atten) plus what the caller adds to it next: a per-(frame, channel) term or a full tensor."""
        feat = self.conv.run(x)
        logit = _linear(ops.global_avgpool(feat), self._w, self._b)
        return ops.channel_gate(feat, logit, logit=True, bias=bias, add=add, out=feat)


class BasicBlock(nn.Module):
    """resnet.py:10-40."""

    def __init__(self, in_chan, out_chan, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chan, out_chan, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_chan)
        self.conv2 = nn.Conv2d(out_chan, out_chan, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chan)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if in_chan != out_chan or stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(in_chan, out_chan, kernel_size=1, stride=stride, bias=False),
                                            nn.BatchNorm2d(out_chan))

    def pack(self, dtype, device):
        self._p = [_fold(self.conv1, self.bn1, dtype, device), _fold(self.conv2, self.bn2, dtype, device)]
        self._pd = _fold(self.downsample[0], self.downsample[1], dtype, device) if self.downsample is not None else None

    def run(self, x):
        shortcut = _conv(x, self._pd, self.downsample[0], A.ACT_NONE) if self._pd is not None else x
        h = _conv(x, self._p[0], self.conv1, A.ACT_RELU)
        h = _conv(h, self._p[1], self.conv2, A.ACT_NONE)
        return ops.add_act(shortcut, h, A.ACT_RELU, out=h)           # relu(shortcut + residual)


def create_layer_basic(in_chan, out_chan, bnum, stride=1):
    """resnet.py:43-47."""
    return nn.Sequential(BasicBlock(in_chan, out_chan, stride=stride), *[BasicBlock(out_chan, out_chan) for _ in range(bnum - 1)])


class ResNet18(nn.Module):
    """resnet.py:50-72."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = create_layer_basic(64, 64, bnum=2, stride=1)
        self.layer2 = create_layer_basic(64, 128, bnum=2, stride=2)
        self.layer3 = create_layer_basic(128, 256, bnum=2, stride=2)
        self.layer4 = create_layer_basic(256, 512, bnum=2, stride=2)

    def pack(self, dtype, device):
        self._p = _fold(self.conv1, self.bn1, dtype, device)
        for m in self.modules():
            if isinstance(m, BasicBlock):
                m.pack(dtype, device)

    def run(self, x):
        h = ops.maxpool3x3s2(_conv(x, self._p, self.conv1, A.ACT_RELU))
        feats = []
        for i in range(1, 5):
            for blk in getattr(self, f"layer{i}"):
                h = blk.run(h)
            feats.append(h)
        return feats[1], feats[2], feats[3]                     # 1/8, 1/16, 1/32


class ContextPath(nn.Module):
    """bisenet.py:55-85."""

    def __init__(self):
        super().__init__()
        self.resnet = ResNet18()
        self.arm16 = AttentionRefinementModule(256, 128)
        self.arm32 = AttentionRefinementModule(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_head16 = ConvBNReLU(128, 128, ks=3, stride=1, padding=1)
        self.conv_avg = ConvBNReLU(512, 128, ks=1, stride=1, padding=0)

    def pack(self, dtype, device):
        self.resnet.pack(dtype, device)
        for m in (self.arm16, self.arm32, self.conv_head32, self.conv_head16, self.conv_avg):
            m.pack(dtype, device)

    def run(self, x):
        feat8, feat16, feat32 = self.resnet.run(x)
        # avg_up: conv_avg on the 1x1 pooled map, enlarged by nearest = one value per (frame, channel)
        avg = _linear(ops.global_avgpool(feat32), *self.conv_avg._lin, act=A.ACT_RELU)
        feat32_sum = self.arm32.run(feat32, bias=avg)
        feat32_up = self.conv_head32.run(ops.resize(feat32_sum, tuple(feat16.shape[1:3]), 4))
        feat16_sum = self.arm16.run(feat16, add=feat32_up)
        feat16_up = self.conv_head16.run(ops.resize(feat16_sum, tuple(feat8.shape[1:3]), 4))
        return feat8, feat16_up, feat32_up


class FeatureFusionModule(nn.Module):
    """bisenet.py:88-108."""

    def __init__(self, in_chan, out_chan):
        super().__init__()
        self.convblk = ConvBNReLU(in_chan, out_chan, ks=1, stride=1, padding=0)
        self.conv1 = nn.Conv2d(out_chan, out_chan // 4, kernel_size=1, stride=1, padding=0, bias=False)
        self.conv2 = nn.Conv2d(out_chan // 4, out_chan, kernel_size=1, stride=1, padding=0, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.sigmoid = nn.Sigmoid()

    def pack(self, dtype, device):
        self.convblk.pack(dtype, device)
        self._w1 = self.conv1.weight.detach().float().reshape(self.conv1.out_channels, -1).to(device).contiguous()
        self._w2 = self.conv2.weight.detach().float().reshape(self.conv2.out_channels, -1).to(device).contiguous()

    def run(self, fsp, fcp):
        wp, b, cout = self.convblk._p
        feat = ops.conv([fsp, fcp], wp, b, cout, (1, 1, 1), act=A.ACT_RELU)          # convblk(torch.cat([fsp, fcp], dim=1))
        logit = _linear(_linear(ops.global_avgpool(feat), self._w1, None, act=A.ACT_RELU), self._w2, None)
        return ops.channel_gate(feat, logit, logit=True, add_x=True, out=feat)       # feat * atten + feat


class BiSeNet(nn.Module):
    """bisenet.py:111-140."""

    def __init__(self, num_class):
        super().__init__()
        if not 1 <= num_class <= 32:
            raise NotImplementedError(f"flair_amd: BiSeNet with num_class={num_class} (the fused arg-max kernel holds 1 .. 32 classes)")
        self.num_class = num_class
        self.cp = ContextPath()
        self.ffm = FeatureFusionModule(256, 256)
        self.conv_out = BiSeNetOutput(256, 256, num_class)
        self.conv_out16 = BiSeNetOutput(128, 64, num_class)
        self.conv_out32 = BiSeNetOutput(128, 64, num_class)
        self.dtype = torch.float32
        self._packed_key = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._packed_key = None                 # folded / packed weights are rebuilt on the next forward
        return out

    def convert_to_bf16(self):
        self.dtype, self._packed_key = torch.bfloat16, None
        return self

    def convert_to_fp32(self):
        self.dtype, self._packed_key = torch.float32, None
        return self

    def _ensure_packed(self, device):
        key = (self.dtype, device)
        if self._packed_key != key:
            for m in (self.cp, self.ffm, self.conv_out, self.conv_out16, self.conv_out32):
                m.pack(self.dtype, device)
            self._packed_key = key

    def _to_clip(self, x):
        if not x.is_cuda:
            raise _lib.FlairHipError("flair_amd BiSeNet needs its input in HBM (device='cuda'); no CPU path exists")
        self._ensure_packed(x.device)
        B, C, H, W = x.shape
        if C != 3:
            raise ValueError(f"BiSeNet takes (B, 3, H, W) frames, got {tuple(x.shape)}")
        h = torch.zeros((B, H, W, ops.pad_channels(3, self.dtype)), dtype=self.dtype, device=x.device)
        return ops.nchw_to_clip(x.float().contiguous(), h, 0)

    def _main_logits(self, x):
        """(B, 3, H, W) -> the main head's class logits at 1/8 resolution, a (B, ceil(H/8), ceil(W/8), >= num_class) clip
        tensor (what forward() enlarges into ``out``)."""
        feat_res8, feat_cp8, _ = self.cp.run(self._to_clip(x))
        return self.conv_out.run(self.ffm.run(feat_res8, feat_cp8))[0]

    @torch.no_grad()
    def forward(self, x, return_feat=False):
        H, W = x.shape[2:]
        feat_res8, feat_cp8, feat_cp16 = self.cp.run(self._to_clip(x))
        feat_fuse = self.ffm.run(feat_res8, feat_cp8)
        heads = [self.conv_out.run(feat_fuse), self.conv_out16.run(feat_cp8), self.conv_out32.run(feat_cp16)]

        def up(t, c):           # F.interpolate(t, (H, W), mode='bilinear', align_corners=True), back in NCHW
            return ops.clip_to_nchw(ops.resize(t, (H, W), 1, channels=c), c)
        outs = tuple(up(o, self.num_class) for o, _ in heads)
        if return_feat:
            outs += tuple(up(f, f.shape[3]) for _, f in heads)
        return outs

    # -- the parser protocol of FaceRestoreHelper / workload.parsenet_weights_fn (shared with ParseNet)
    @torch.no_grad()
    def parse_indices(self, x):
        """``face_parse(x)[0].argmax(dim=1)`` (face_restoration_helper.py:279-281): (B, H, W) int32, from the 1/8-resolution
        logits in one fused launch."""
        H, W = x.shape[2:]
        return ops.upsample_argmax(self._main_logits(x), self.num_class, (H, W))[0]

    @torch.no_grad()
    def face_weight(self, frames, w_face):
        """``mask * w_face + (1 - mask)`` with ``mask = (face_parse(frames)[0].argmax(1, keepdim=True) == 0)``
        (scripts/video_sample.py:427-444): (T, 1, H, W) float32; the fused arg-max kernel looks the weight up in a
        ``num_class``-entry table.  Class 0 is taken to be the background in ``parsing_bisenet.pth``'s label order as it is
        in ParseNet's (CelebAMask-HQ convention); the file cannot be inspected offline: **parity unpinned**."""
        H, W = frames.shape[2:]
        table = torch.ones((self.num_class, 1), dtype=torch.float32, device=frames.device)
        table[0, 0] = float(w_face)
        w = ops.upsample_argmax(self._main_logits(frames), self.num_class, (H, W), table)[1]
        return w.permute(0, 3, 1, 2).contiguous()
