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
from .packing import PackedModel, dev_f32, fold_bn, pad_cout, packed_conv, run_conv


def _matrix(conv, bn, device):
    """A 1x1 convolution (+ eval BatchNorm) on a one-pixel map as ops.linear's (weight, bias), f32."""
    w, b = fold_bn(conv, bn)
    return w.reshape(w.shape[0], -1).to(device).contiguous(), b.to(device).contiguous()


class ConvBNReLU(nn.Module):
    """bisenet.py:8-19."""

    def __init__(self, in_chan, out_chan, ks=3, stride=1, padding=1):
        super().__init__()
        if ks % 2 != 1 or padding != ks // 2:
            raise NotImplementedError(f"flair_amd: BiSeNet ConvBNReLU with ks={ks}, padding={padding} (odd kernels padded by ks // 2 only)")
        self.conv = nn.Conv2d(in_chan, out_chan, kernel_size=ks, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_chan)

    def pack(self, dtype, device):
        self._pk = packed_conv(self.conv, self.bn, dtype, device)
        if self.conv.kernel_size[0] == 1:                       # the same layer on a 1x1 map (conv_avg): a matrix
            self._pk["lin"] = _matrix(self.conv, self.bn, device)

    def run(self, x):
        return run_conv(x, self._pk, self.conv, A.ACT_RELU)


class BiSeNetOutput(nn.Module):
    """bisenet.py:22-33."""

    def __init__(self, in_chan, mid_chan, num_class):
        super().__init__()
        self.conv = ConvBNReLU(in_chan, mid_chan, ks=3, stride=1, padding=1)
        self.conv_out = nn.Conv2d(mid_chan, num_class, kernel_size=1, bias=False)

    def pack(self, dtype, device):
        g = 16 // torch.empty((), dtype=dtype).element_size()    # class vectors padded to whole 16-byte chunks
        self._pk = packed_conv(self.conv_out, None, dtype, device, cout_pad=pad_cout(self.conv_out.out_channels, g))

    def run(self, x):
        feat = self.conv.run(x)
        return run_conv(feat, self._pk, self.conv_out), feat


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
        w, b = _matrix(self.conv_atten, self.bn_atten, device)
        self._pk = dict(w=w, b=b)

    def run(self, x, bias=None, add=None):
        """torch.mul(feat, atten) plus what the caller adds to it next: a per-(frame, channel) term or a full tensor."""
        feat = self.conv.run(x)
        logit = _linear(ops.global_avgpool(feat), self._pk["w"], self._pk["b"])
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
        self._pk = dict(c1=packed_conv(self.conv1, self.bn1, dtype, device), c2=packed_conv(self.conv2, self.bn2, dtype, device))
        if self.downsample is not None:
            self._pk["down"] = packed_conv(self.downsample[0], self.downsample[1], dtype, device)

    def run(self, x):
        pk = self._pk
        shortcut = run_conv(x, pk["down"], self.downsample[0]) if "down" in pk else x
        h = run_conv(x, pk["c1"], self.conv1, A.ACT_RELU)
        h = run_conv(h, pk["c2"], self.conv2)
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
        self._pk = packed_conv(self.conv1, self.bn1, dtype, device)

    def run(self, x):
        h = ops.maxpool3x3s2(run_conv(x, self._pk, self.conv1, A.ACT_RELU))
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

    def run(self, x):
        feat8, feat16, feat32 = self.resnet.run(x)
        # avg_up: conv_avg on the 1x1 pooled map, enlarged by nearest = one value per (frame, channel)
        avg = _linear(ops.global_avgpool(feat32), *self.conv_avg._pk["lin"], act=A.ACT_RELU)
        feat32_sum = self.arm32.run(feat32, bias=avg)
        feat32_up = self.conv_head32.run(ops.resize(feat32_sum, tuple(feat16.shape[1:3]), ops.RESIZE_NEAREST))
        feat16_sum = self.arm16.run(feat16, add=feat32_up)
        feat16_up = self.conv_head16.run(ops.resize(feat16_sum, tuple(feat8.shape[1:3]), ops.RESIZE_NEAREST))
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
        self._pk = dict(w1=dev_f32(self.conv1.weight.detach().reshape(self.conv1.out_channels, -1), device),
                        w2=dev_f32(self.conv2.weight.detach().reshape(self.conv2.out_channels, -1), device))

    def run(self, fsp, fcp):
        feat = self.convblk.run([fsp, fcp])                                          # convblk(torch.cat([fsp, fcp], dim=1))
        logit = _linear(_linear(ops.global_avgpool(feat), self._pk["w1"], None, act=A.ACT_RELU), self._pk["w2"], None)
        return ops.channel_gate(feat, logit, logit=True, add_x=True, out=feat)       # feat * atten + feat


class BiSeNet(PackedModel, nn.Module):
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
