"""SuperSloMo frame interpolation on the HIP kernels.

Mirror of the reference's ``guided_diffusion/superslomo.py``: ``down``, ``up``, ``UNet`` and ``SuperSloMo`` with the
reference's constructor arguments and state-dict names (``flow_estimator.conv1.weight`` ... ``interp.conv3.bias``, 92
entries, 39 610 473 parameters: the flat state dict the reference module loads goes through ``load_state_dict`` unchanged).

The modules are parameter containers.  Every Conv2d + LeakyReLU(0.1) is ONE ``flair_conv_nhwc`` launch (7x7, 5x5 and 3x3,
stride 1, no normalisation layer anywhere), ``F.avg_pool2d(x, 2)`` and the bilinear x2 enlargement are
``flair_resize_nhwc`` (modes 3 and 0), and ``torch.cat((x, skpCn), 1)`` is the two input segments of ``up.conv2``.  The 6-
and 20-channel network inputs are padded to the convolution's K step with zero weight columns.

Launch sequence of ``forward`` (slomo.hip has the two fused entries):

  per pair      2 x ``flair_nchw_f32_to_nhwc`` + ``flair_affine_channels_f32`` (``normalize((frame + 1) / 2, mean)``, :250-252),
                the flow UNet (:254): 23 convolutions, 5 pools, 5 enlargements;
  per timestep  ``flair_slomo_warp_pack`` (stage A, :260-270: both flow combinations, two back-warps, the 20-channel concat),
                the interpolation UNet (:271), ``flair_slomo_blend`` (stage B, :273-287: refined flows, sigmoid visibility,
                two back-warps, the normalised blend, the de-normalisation) straight into slot ``[:, k]`` of the result.

float32 by default (the mode the tests gate); ``convert_to_bf16()`` switches the activations and packed weights to bfloat16.
"""
import torch
import torch.nn as nn

from .. import ops
from .. import ops as A
from .packing import PackedModel, pack_w, pad_bias, pad_cout, packed_conv, run_conv


def _vec(dtype):
    """Elements per 16 bytes: the granularity of a view the fused entries read."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, k, stride=1, padding=int((k - 1) / 2))


class down(nn.Module):
    """superslomo.py:8-79: average pooling, then two convolutions + LeakyReLU(0.1)."""

    def __init__(self, inChannels, outChannels, filterSize):
        super().__init__()
        self.conv1 = _conv(inChannels, outChannels, filterSize)
        self.conv2 = _conv(outChannels, outChannels, filterSize)

    def pack(self, dtype, device):
        self._pk = dict(c1=packed_conv(self.conv1, None, dtype, device), c2=packed_conv(self.conv2, None, dtype, device))

    def run(self, x):
        _, H, W, _ = x.shape
        x = ops.resize(x, (H // 2, W // 2), ops.RESIZE_AVGPOOL2)
        x = run_conv(x, self._pk["c1"], self.conv1, A.ACT_LRELU01)
        return run_conv(x, self._pk["c2"], self.conv2, A.ACT_LRELU01)


class up(nn.Module):
    """superslomo.py:82-143: bilinear x2, a convolution, then one on torch.cat((x, skpCn), 1); LeakyReLU(0.1) after each."""

    def __init__(self, inChannels, outChannels):
        super().__init__()
        self.conv1 = _conv(inChannels, outChannels, 3)
        self.conv2 = _conv(2 * outChannels, outChannels, 3)

    def pack(self, dtype, device):
        c = self.conv1.out_channels
        cpad = pad_cout(c)
        w2 = pack_w(self.conv2.weight.detach().float(), dtype, device, segs=[(c, c), (c, c)], cout_pad=cpad)
        self._pk = dict(c1=packed_conv(self.conv1, None, dtype, device),
                        c2=dict(w=w2, b=pad_bias(self.conv2.bias.detach().float().to(device), cpad), cout=cpad))

    def run(self, x, skpCn):
        _, H, W, _ = x.shape
        x = ops.resize(x, (2 * H, 2 * W), ops.RESIZE_BILINEAR)
        x = run_conv(x, self._pk["c1"], self.conv1, A.ACT_LRELU01)
        return run_conv([x, skpCn], self._pk["c2"], self.conv2, A.ACT_LRELU01)


class UNet(nn.Module):
    """superslomo.py:146-214."""

    def __init__(self, inChannels, outChannels):
        super().__init__()
        self.conv1 = _conv(inChannels, 32, 7)
        self.conv2 = _conv(32, 32, 7)
        self.down1 = down(32, 64, 5)
        self.down2 = down(64, 128, 3)
        self.down3 = down(128, 256, 3)
        self.down4 = down(256, 512, 3)
        self.down5 = down(512, 512, 3)
        self.up1 = up(512, 512)
        self.up2 = up(512, 256)
        self.up3 = up(256, 128)
        self.up4 = up(128, 64)
        self.up5 = up(64, 32)
        self.conv3 = _conv(32, outChannels, 3)

    def pack(self, dtype, device):
        # conv1's input is padded to the K step with zero weight columns (packed_conv); conv3's 4 / 5 outputs are padded to
        # whole 16-byte chunks, the granularity of the views slomo.hip reads
        self._pk = dict(c1=packed_conv(self.conv1, None, dtype, device), c2=packed_conv(self.conv2, None, dtype, device),
                        c3=packed_conv(self.conv3, None, dtype, device,
                                       cout_pad=pad_cout(self.conv3.out_channels, _vec(dtype))))

    def run(self, x):
        """x: (B, H, W, pad_channels(inChannels)) clip tensor, H and W multiples of 32 -> (B, H, W, >= outChannels)."""
        x = run_conv(x, self._pk["c1"], self.conv1, A.ACT_LRELU01)
        s1 = run_conv(x, self._pk["c2"], self.conv2, A.ACT_LRELU01)
        s2 = self.down1.run(s1)
        s3 = self.down2.run(s2)
        s4 = self.down3.run(s3)
        s5 = self.down4.run(s4)
        x = self.down5.run(s5)
        x = self.up1.run(x, s5)
        x = self.up2.run(x, s4)
        x = self.up3.run(x, s3)
        x = self.up4.run(x, s2)
        x = self.up5.run(x, s1)
        return run_conv(x, self._pk["c3"], self.conv3, A.ACT_LRELU01)


class SuperSloMo(PackedModel, nn.Module):
    """superslomo.py:217-291."""

    MULTIPLE = 32           # five 2x2 poolings

    def __init__(self, pretrained=None):
        super().__init__()
        self.flow_estimator = UNet(6, 4)
        self.interp = UNet(20, 5)
        if pretrained is not None:
            self.load_state_dict(torch.load(pretrained, map_location="cpu"))

    def _check(self, frame0, frame1, factor):
        if not (isinstance(frame0, torch.Tensor) and isinstance(frame1, torch.Tensor)) or frame0.dim() != 4 or frame0.shape[1] != 3:
            raise ValueError("SuperSloMo takes two (B, 3, H, W) frame tensors")
        if tuple(frame0.shape) != tuple(frame1.shape):
            raise ValueError(f"SuperSloMo: frame0 is {tuple(frame0.shape)} and frame1 is {tuple(frame1.shape)}")
        if frame0.shape[0] < 1:
            raise ValueError("SuperSloMo: an empty batch")
        H, W = frame0.shape[2:]
        if H % self.MULTIPLE or W % self.MULTIPLE or not H or not W:
            raise ValueError(f"SuperSloMo: frames of {H}x{W}; height and width must be multiples of {self.MULTIPLE} "
                             "(interpolate.interpolate_frames pads other sizes)")
        if isinstance(factor, bool) or int(factor) != factor or factor < 2:
            raise ValueError(f"SuperSloMo: factor={factor!r}; an integer >= 2 (factor - 1 frames are made per pair)")
        if not (frame0.is_cuda and frame1.is_cuda) or frame0.device != frame1.device:
            raise ValueError("flair_amd SuperSloMo needs both frames in HBM on one device (device='cuda'); no CPU path exists")

    def _pair(self, frame0, frame1):
        """normalize((frame + 1) / 2, mean, [1, 1, 1]) of both frames (:250-252) as one clip tensor: i0 | i1 | zeros."""
        B, _, H, W = frame0.shape
        dev = frame0.device
        x = torch.zeros((B, H, W, ops.pad_channels(6, torch.float32)), dtype=torch.float32, device=dev)
        ops.nchw_to_clip(frame0.float().contiguous(), x, 0)
        ops.nchw_to_clip(frame1.float().contiguous(), x, 3)
        mean = torch.tensor(ops.SLOMO_MEAN * 2, dtype=torch.float32, device=dev)
        ops.affine_channels(x, 6, 0.5, 0.5, float("-inf"), float("inf"), mean, None, x)
        if self.dtype == torch.float32:
            return x
        pair = torch.zeros((B, H, W, ops.pad_channels(6, self.dtype)), dtype=self.dtype, device=dev)
        return ops.cast_channels(x[..., :6], pair, 0)

    @torch.no_grad()
    def forward(self, frame0, frame1, factor, return_flow=False):
        """frame0, frame1: (B, 3, H, W) f32 in [-1, 1] -> the factor - 1 frames between them, (B, factor - 1, 3, H, W) f32;
        with return_flow also f01 and f10, (B, 2, H, W) f32 each."""
        self._check(frame0, frame1, factor)
        factor = int(factor)
        self._ensure_packed(frame0.device)
        B, _, H, W = frame0.shape
        pair = self._pair(frame0, frame1)
        flow = self.flow_estimator.run(pair)                    # f01 | f10 (| pad)
        out = torch.empty((B, factor - 1, 3, H, W), dtype=torch.float32, device=frame0.device)
        iy = torch.empty((B, H, W, ops.pad_channels(20, self.dtype)), dtype=self.dtype, device=frame0.device)
        for k in range(1, factor):
            t, coef = ops.slomo_coefficients(k, factor)
            ops.slomo_warp_pack(pair, flow, coef, out=iy)
            io = self.interp.run(iy)
            ops.slomo_blend(pair, flow, io, coef, t, out[:, k - 1])
        if return_flow:
            return out, ops.clip_to_nchw(flow, 2, 0), ops.clip_to_nchw(flow, 2, 2)
        return out
