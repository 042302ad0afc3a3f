"""VQFR v2 auxiliary prior on the HIP kernels: the reference's ``guided_diffusion/vqfr.py``.

Mirror of ``VQFRv2`` (vqfr.py:490-586) and the classes it is built from (``L2VectorQuantizer`` :11-80, ``Downsample`` /
``Upsample`` :83-107, ``ResnetBlock`` :110-144, ``AttnBlock`` :147-194, ``VQGANEncoder`` :197-266, ``VQGANDecoder``
:269-338, ``DCNv2Pack`` :341-380, ``TextureWarpingModule`` :383-427, ``MainDecoder`` :430-487) with the reference's
constructor arguments, so a checkpoint's state dict loads under its own names.  The sampler calls it as
``aux_model(pred_xstart, t, x)`` = ``net(x0, fidelity_ratio)["main_dec"]`` (workload.vqfr_aux).  The modules are
parameter containers; the arithmetic runs on libflair_hip.so through ``flair_amd.ops`` on NHWC tensors:

  * 3x3 / 1x1 convolutions, with two-part inputs as segments instead of ``torch.cat``, and the asymmetric stride-2
    ``Downsample``: ``flair_conv_nhwc``;  GroupNorm(32, eps 1e-6)(+SiLU) per face, also over the two-part input of
    ``ResnetBlock(2c -> c)``: ``flair_groupnorm_nhwc``;  nearest x2 and bilinear (align_corners=False) resizes:
    ``flair_resize_nhwc``;  the single-head ``AttnBlock``: ``flair_qkv_attention``;
  * the 7x7 depthwise convolution of ``offset_conv1``: ``flair_dwconv7_nhwc``;
  * ``DCNv2Pack``: ``flair_dcn_align`` with ``raw_activated = 2`` (offsets as they are, sigmoid masks, x_main's two
    channel halves as its two inputs); ``conv_offset``'s output channels are permuted to the tap-major order once, at
    pack time, and padded to a multiple of 8;
  * code selection: "Predict" = LayerNorm(256) + Linear(256, 1024) as a 1x1 convolution + ``flair_argmax_codebook``;
    "Nearest" = ``flair_vq_nearest_nhwc``.

The ``* 2`` of the upsampled offsets (vqfr.py:470-476) is folded into the ``offset_conv2`` weights of those input
channels (exact), and at level 1 the bilinear resize of ``inpfeat`` to its own size is the identity, so it is skipped.
The default dtype is float32; ``convert_to_bf16()`` switches activations and conv weights to bf16 (GroupNorm / LayerNorm
statistics, the depthwise and deformable accumulations, the codebook and the distances of the "Nearest" search stay f32;
the "Predict" logits are formed in the activation dtype, as CodeFormer's).  Faces are a batch: nothing mixes them.
The prior path only needs ``main_dec``: ``texture_dec`` (the decoder's own ``conv_out``) is computed on request only.
The codebook loss and the ``usage`` counter are training state and are not ported.
"""
from collections.abc import Mapping

import torch
import torch.nn as nn

from .. import ops
from .. import ops as A
from . import vqgan_blocks as vb
from .packing import PackedModel, dev_f32, pack_w
from .unet_new import qkv_head_width
from .vqgan_blocks import Downsample, HeadConv, NormOut, Upsample, gn  # noqa: F401  (Downsample :83-94, Upsample :97-107)

DCN_GROUPS = (4, 8, 16)          # flair_dcn_align's deformable groups (4 with raw offsets only)
CODE_DIM = 256                   # fixed by L2VectorQuantizer(code_dim=256) and LayerNorm(256) (vqfr.py:536-547)
RESOLUTION = 512                 # the 16 x 16 code grid (spatial_size) after len(channel_multipliers) - 1 = 5 halvings


class L2VectorQuantizer(nn.Module):
    """vqfr.py:11-80: nearest codebook row under the L2 distance.  Only the search and the lookup run (``run``)."""

    def __init__(self, num_code, code_dim, spatial_size):
        super().__init__()
        self.num_code = num_code
        self.code_dim = code_dim
        self.spatial_size = spatial_size
        self.beta = 0.25
        self.embedding = nn.Embedding(self.num_code, self.code_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.num_code, 1.0 / self.num_code)

    def pack(self, dtype, device):
        self._pk = dict(codebook=dev_f32(self.embedding.weight, device))

    def run(self, z, forced_idx=None):
        return ops.vq_nearest(z, self._pk["codebook"], forced_idx=forced_idx)


class ResnetBlock(vb.ResBlock):
    """vqfr.py:110-144.  ``run(x, x1)`` takes the input as two channel parts (cat([x, x1]) of MainDecoder, :486), which
    reach the 1x1 shortcut ``residual_func`` as two equal unpadded segments."""

    shortcut = "residual_func"

    def __init__(self, channels_in, channels_out):
        super().__init__(channels_in, channels_out)
        self.act = nn.SiLU(inplace=True)
        if channels_in == channels_out:
            self.residual_func = nn.Identity()
        self.channels_in, self.channels_out = channels_in, channels_out


class AttnBlock(vb.AttnBlock):
    """vqfr.py:147-194: the single head runs on flair_qkv_attention (scale c**-0.5)."""

    @staticmethod
    def attention(qkv, c):
        return ops.qkv_attention(qkv, 1, new_order=True)

    def __init__(self, in_channels):
        qkv_head_width(in_channels, 1)          # widths the attention kernels cannot run are refused here
        super().__init__(in_channels)


def _run_seq(seq, x):
    for m in seq:
        x = m.run(x)
    return x


def _conv_out(channels, cout):
    """conv_out = Sequential(GroupNorm, SiLU, Conv2d 3x3) with the reference's entry names; entry 1 is applied by entry 0."""
    return nn.Sequential(NormOut(channels, A.ACT_SILU), nn.SiLU(inplace=True),
                         HeadConv(channels, cout, kernel_size=3, padding=1))


def _run_conv_out(seq, x):
    return seq[2].run(seq[0].run(x))


class VQGANEncoder(nn.Module):
    """vqfr.py:197-266."""

    def __init__(self, base_channels, channel_multipliers, num_blocks, use_enc_attention, code_dim):
        super(VQGANEncoder, self).__init__()
        self.num_levels = len(channel_multipliers)
        self.num_blocks = num_blocks
        self.conv_in = HeadConv(3, base_channels * channel_multipliers[0], kernel_size=(3, 3), stride=(1, 1), padding=1)
        self.blocks = nn.ModuleList()
        for i in range(self.num_levels):
            blocks = []
            if i == 0:
                channels_prev = base_channels * channel_multipliers[i]
            else:
                channels_prev = base_channels * channel_multipliers[i - 1]
            if i != 0:
                blocks.append(Downsample(channels_prev))
            channels = base_channels * channel_multipliers[i]
            blocks.append(ResnetBlock(channels_prev, channels))
            if i == self.num_levels - 1 and use_enc_attention:
                blocks.append(AttnBlock(channels))
            for j in range(self.num_blocks - 1):
                blocks.append(ResnetBlock(channels, channels))
                if i == self.num_levels - 1 and use_enc_attention:
                    blocks.append(AttnBlock(channels))
            self.blocks.append(nn.Sequential(*blocks))
        channels = base_channels * channel_multipliers[-1]
        if use_enc_attention:
            self.mid_blocks = nn.Sequential(ResnetBlock(channels, channels), AttnBlock(channels),
                                            ResnetBlock(channels, channels))
        else:
            self.mid_blocks = nn.Sequential(ResnetBlock(channels, channels), ResnetBlock(channels, channels))
        self.conv_out = _conv_out(channels, code_dim)

    def run(self, x):
        x = self.conv_in.run(x)
        for i in range(self.num_levels):
            x = _run_seq(self.blocks[i], x)
        x = _run_seq(self.mid_blocks, x)
        return _run_conv_out(self.conv_out, x)


class VQGANDecoder(nn.Module):
    """vqfr.py:269-338.  ``run`` returns the level features (``dec_res``, NHWC); ``conv_out`` is applied by the caller."""

    def __init__(self, base_channels, channel_multipliers, num_blocks, use_dec_attention, code_dim):
        super(VQGANDecoder, self).__init__()
        self.num_levels = len(channel_multipliers)
        self.num_blocks = num_blocks
        self.conv_in = HeadConv(code_dim, base_channels * channel_multipliers[-1], kernel_size=(3, 3), stride=(1, 1),
                                padding=1)
        self.blocks = nn.ModuleList()
        channels = base_channels * channel_multipliers[-1]
        if use_dec_attention:
            self.mid_blocks = nn.Sequential(ResnetBlock(channels, channels), AttnBlock(channels),
                                            ResnetBlock(channels, channels))
        else:
            self.mid_blocks = nn.Sequential(ResnetBlock(channels, channels), ResnetBlock(channels, channels))
        for i in reversed(range(self.num_levels)):
            blocks = []
            if i == self.num_levels - 1:
                channels_prev = base_channels * channel_multipliers[i]
            else:
                channels_prev = base_channels * channel_multipliers[i + 1]
            if i != self.num_levels - 1:
                blocks.append(Upsample(channels_prev))
            channels = base_channels * channel_multipliers[i]
            blocks.append(ResnetBlock(channels_prev, channels))
            if i == self.num_levels - 1 and use_dec_attention:
                blocks.append(AttnBlock(channels))
            for j in range(self.num_blocks - 1):
                blocks.append(ResnetBlock(channels, channels))
                if i == self.num_levels - 1 and use_dec_attention:
                    blocks.append(AttnBlock(channels))
            self.blocks.append(nn.Sequential(*blocks))
        channels = base_channels * channel_multipliers[0]
        self.conv_out = _conv_out(channels, 3)

    def run(self, x):
        dec_res = {}
        x = self.conv_in.run(x)
        x = _run_seq(self.mid_blocks, x)
        for i, level in enumerate(reversed(range(self.num_levels))):
            x = _run_seq(self.blocks[i], x)
            dec_res["Level_%d" % 2 ** level] = x
        return dec_res


class DCNv2Pack(nn.Module):
    """vqfr.py:341-380 (a ``ModulatedDeformConvPack``: ``weight``, ``bias`` and ``conv_offset``, dcn/deform_conv.py:289-379)
    with its offsets and masks computed from a second feature: ``run(x, feat)``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=True):
        super().__init__()
        if (kernel_size, stride, padding, dilation, groups) != (3, 1, 1, 1, 1) or not bias:
            raise NotImplementedError("flair_amd: DCNv2Pack runs as a 3x3 stride-1 padding-1 convolution with bias")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = (3, 3)
        self.stride, self.padding, self.dilation, self.groups = stride, padding, dilation, groups
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, 3, 3).uniform_(
            -1.0 / (in_channels * 9) ** 0.5, 1.0 / (in_channels * 9) ** 0.5))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.conv_offset = nn.Conv2d(in_channels, deformable_groups * 3 * 9, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def pack(self, dtype, device):
        G = self.deformable_groups
        perm = ops.dcn_raw_permutation(G)       # tap-major offsets / masks for flair_dcn_align
        cpad = (27 * G + 7) // 8 * 8            # raw rows 16-byte granular in bf16 (27 * 4 = 108 channels is not)
        b = self.conv_offset.bias.detach()[perm]
        self._pk = dict(wo=pack_w(self.conv_offset.weight.detach()[perm], dtype, device, cout_pad=cpad),
                        bo=dev_f32(torch.cat([b, b.new_zeros(cpad - 27 * G)]), device), cpad=cpad,
                        w=pack_w(self.weight, dtype, device, [(self.in_channels, self.in_channels)]),
                        b=dev_f32(self.bias, device))

    def run(self, x, feat):
        pk = self._pk
        raw = ops.conv(feat, pk["wo"], pk["bo"], pk["cpad"], (1, 3, 3))
        return ops.dcn_pack(x, raw, pk["w"], pk["b"], self.out_channels, groups=self.deformable_groups)


class TextureWarpingModule(nn.Module):
    """vqfr.py:383-427.  ``run`` returns (warp_feat, offset); ``previous_offset`` is the offset of the level below at
    ITS resolution: the bilinear x2 happens here, its ``* 2`` is folded into ``offset_conv2``'s weights."""

    def __init__(self, channel, cond_channels, cond_downscale_rate, deformable_groups, previous_offset_channel=0):
        super(TextureWarpingModule, self).__init__()
        self.cond_downscale_rate = cond_downscale_rate
        self.offset_conv1 = nn.Sequential(
            nn.Conv2d(channel + cond_channels, channel, kernel_size=1),
            nn.GroupNorm(num_groups=32, num_channels=channel, eps=1e-6, affine=True),
            nn.SiLU(inplace=True),
            nn.Conv2d(channel, channel, groups=channel, kernel_size=7, padding=3),
            nn.GroupNorm(num_groups=32, num_channels=channel, eps=1e-6, affine=True),
            nn.SiLU(inplace=True),
            nn.Conv2d(channel, channel, kernel_size=1),
        )
        self.offset_conv2 = nn.Sequential(
            nn.Conv2d(channel + previous_offset_channel, channel, 3, 1, 1),
            nn.GroupNorm(num_groups=32, num_channels=channel, eps=1e-6, affine=True),
            nn.SiLU(inplace=True),
        )
        self.dcn = DCNv2Pack(channel, channel, 3, padding=1, deformable_groups=deformable_groups)
        self.channel, self.cond_channels, self.previous_offset_channel = channel, cond_channels, previous_offset_channel

    def pack(self, dtype, device):
        c, cc, pc = self.channel, self.cond_channels, self.previous_offset_channel
        o1, o2 = self.offset_conv1, self.offset_conv2
        w2 = o2[0].weight.detach().clone()
        w2[:, c:] *= 2                          # upsample_offset = interpolate(offset) * 2 (vqfr.py:470-476): exact
        self._pk = dict(w_a=pack_w(o1[0].weight, dtype, device, [(cc, cc), (c, c)]), b_a=dev_f32(o1[0].bias, device),
                        na_g=dev_f32(o1[1].weight, device), na_b=dev_f32(o1[1].bias, device),
                        w_dw=dev_f32(o1[3].weight.detach().reshape(c, 49).t(), device), b_dw=dev_f32(o1[3].bias, device),
                        nb_g=dev_f32(o1[4].weight, device), nb_b=dev_f32(o1[4].bias, device),
                        w_b=pack_w(o1[6].weight, dtype, device), b_b=dev_f32(o1[6].bias, device),
                        w_2=pack_w(w2, dtype, device, [(c, c)] + ([(pc, pc)] if pc else [])),
                        b_2=dev_f32(o2[0].bias, device), n2_g=dev_f32(o2[1].weight, device), n2_b=dev_f32(o2[1].bias, device))

    def run(self, x_main, inpfeat, previous_offset=None):
        pk, c = self._pk, self.channel
        F_, H, W, _ = x_main.shape
        r = self.cond_downscale_rate
        if r != 1:      # at r = 1 the bilinear resize of inpfeat to its own size is the identity
            h, w = inpfeat.shape[1], inpfeat.shape[2]
            inpfeat = ops.resize(inpfeat, (h // r, w // r), ops.RESIZE_BILINEAR,
                                 out=torch.empty((F_, h // r, w // r, inpfeat.shape[3]), dtype=inpfeat.dtype,
                                                 device=inpfeat.device))
        o = ops.conv([inpfeat, x_main], pk["w_a"], pk["b_a"], c, (1, 1, 1))
        o = gn(o, pk, "na", A.ACT_SILU)
        o = ops.dwconv7(o, pk["w_dw"], pk["b_dw"])
        o = gn(o, pk, "nb", A.ACT_SILU)
        o = ops.conv(o, pk["w_b"], pk["b_b"], c, (1, 1, 1))
        xs = [o]
        if previous_offset is not None:
            up = torch.empty((F_, H, W, previous_offset.shape[3]), dtype=o.dtype, device=o.device)
            xs.append(ops.resize(previous_offset, (H, W), ops.RESIZE_BILINEAR, out=up))
        offset = gn(ops.conv(xs, pk["w_2"], pk["b_2"], c, (1, 3, 3)), pk, "n2", A.ACT_SILU)
        return self.dcn.run(x_main, offset), offset


class MainDecoder(nn.Module):
    """vqfr.py:430-487."""

    def __init__(self, base_channels, channel_multipliers, align_opt):
        super(MainDecoder, self).__init__()
        self.num_levels = len(channel_multipliers)
        self.decoder_dict = nn.ModuleDict()
        self.pre_upsample_dict = nn.ModuleDict()
        self.align_func_dict = nn.ModuleDict()
        for i in reversed(range(self.num_levels)):
            if i == self.num_levels - 1:
                channels_prev = base_channels * channel_multipliers[i]
            else:
                channels_prev = base_channels * channel_multipliers[i + 1]
            channels = base_channels * channel_multipliers[i]
            if i != self.num_levels - 1:
                self.pre_upsample_dict["Level_%d" % 2 ** i] = nn.Sequential(
                    nn.UpsamplingNearest2d(scale_factor=2),
                    HeadConv(channels_prev, channels, kernel_size=3, padding=1),
                )
            previous_offset_channel = 0 if i == self.num_levels - 1 else channels_prev
            self.align_func_dict["Level_%d" % (2 ** i)] = TextureWarpingModule(
                channel=channels,
                cond_channels=align_opt["cond_channels"],
                cond_downscale_rate=2 ** i,
                deformable_groups=align_opt["deformable_groups"],
                previous_offset_channel=previous_offset_channel,
            )
            if i != self.num_levels - 1:
                self.decoder_dict["Level_%d" % 2 ** i] = ResnetBlock(2 * channels, channels)

    def run(self, dec_res, inpfeat, fidelity_ratio=1.0, trace=None):
        top = "Level_%d" % 2 ** (self.num_levels - 1)
        x, offset = self.align_func_dict[top].run(dec_res[top], inpfeat)
        if trace is not None:
            trace["twm." + top] = (x, offset)
        for scale in reversed(range(self.num_levels - 1)):
            key = "Level_%d" % 2 ** scale
            up = ops.resize(x, (2 * x.shape[1], 2 * x.shape[2]), ops.RESIZE_NEAREST)
            x = self.pre_upsample_dict[key][1].run(up)
            warp_feat, offset = self.align_func_dict[key].run(dec_res[key], inpfeat, previous_offset=offset)
            if trace is not None:
                trace["twm." + key] = (warp_feat, offset)
            # dec_res["Level_1"] + fidelity_ratio * x (:487): the ratio scales the last block's output in its epilogue
            x = self.decoder_dict[key].run(x, warp_feat, out_scale=fidelity_ratio if scale == 0 else 1.0)
        return ops.add_act(dec_res["Level_1"], x)


def _check_config(base_channels, channel_multipliers, code_dim, inpfeat_dim, code_selection_mode, align_opt):
    if code_dim != CODE_DIM:
        raise ValueError(f"VQFRv2: code_dim={code_dim}: the quantizer and LayerNorm(256) fix it to {CODE_DIM}")
    if len(channel_multipliers) != 6:
        raise ValueError(f"VQFRv2: {len(channel_multipliers)} levels give a {RESOLUTION >> (len(channel_multipliers) - 1)}"
                         f"^2 code grid at {RESOLUTION}^2; the quantizer's spatial_size is 16 x 16 (six levels)")
    chans = sorted({base_channels * m for m in channel_multipliers})
    if any(c % 32 or c < 64 for c in chans):
        raise ValueError(f"VQFRv2: level widths {chans} must be multiples of 32 (GroupNorm(32) and the kernels' channel "
                         "granularity) and at least 64 (the deformable kernel's K step)")
    if code_selection_mode not in ("Predict", "Nearest"):
        raise ValueError(f"VQFRv2: code_selection_mode={code_selection_mode!r}: 'Predict' or 'Nearest'")
    cc = align_opt["cond_channels"]
    if cc != inpfeat_dim or inpfeat_dim % 32:
        raise ValueError(f"VQFRv2: align_opt cond_channels={cc} must equal inpfeat_dim={inpfeat_dim} (the conditioning "
                         "input of every TextureWarpingModule), a multiple of 32")
    G = align_opt["deformable_groups"]
    for c in chans:
        cpg = c // G if G > 0 and c % G == 0 else 0
        if G not in DCN_GROUPS or cpg < 8 or cpg & (cpg - 1) or c > 1024:
            raise NotImplementedError(f"flair_amd: deformable_groups={G} at {c} channels: flair_dcn_align takes G in "
                                      f"{DCN_GROUPS} with a power-of-two group width >= 8 and <= 1024 channels")


class VQFRv2(PackedModel, nn.Module):
    """vqfr.py:490-586 (VQFR v2)."""

    def __init__(self, base_channels, channel_multipliers, num_enc_blocks, use_enc_attention, num_dec_blocks,
                 use_dec_attention, code_dim, inpfeat_dim, code_selection_mode, align_opt):
        super().__init__()
        _check_config(base_channels, channel_multipliers, code_dim, inpfeat_dim, code_selection_mode, align_opt)
        self.encoder = VQGANEncoder(base_channels=base_channels, channel_multipliers=channel_multipliers,
                                    num_blocks=num_enc_blocks, use_enc_attention=use_enc_attention, code_dim=code_dim)
        if code_selection_mode == "Nearest":
            self.feat2index = None
        elif code_selection_mode == "Predict":
            self.feat2index = nn.Sequential(nn.LayerNorm(256), nn.Linear(256, 1024))
        self.decoder = VQGANDecoder(base_channels=base_channels, channel_multipliers=channel_multipliers,
                                    num_blocks=num_dec_blocks, use_dec_attention=use_dec_attention, code_dim=code_dim)
        self.main_branch = MainDecoder(base_channels=base_channels, channel_multipliers=channel_multipliers,
                                       align_opt=align_opt)
        self.inpfeat_extraction = HeadConv(3, inpfeat_dim, 3, padding=1)
        self.quantizer = L2VectorQuantizer(num_code=1024, code_dim=256, spatial_size=(16, 16))
        self.apply(self._init_weights)
        self.code_selection_mode, self.inpfeat_dim, self.code_dim = code_selection_mode, inpfeat_dim, code_dim

    @torch.no_grad()
    def _init_weights(self, m):
        """vqfr.py:551-563 (trunc_normal_(std=0.02) on Linear and Conv2d weights, zero biases, unit norms)."""
        if isinstance(m, (nn.Linear, nn.Conv2d)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, nn.GroupNorm)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """A bare state dict, or a BasicSR checkpoint holding it under ``params_ema`` (preferred) or ``params``."""
        for key in ("params_ema", "params"):
            if key in state_dict and isinstance(state_dict[key], Mapping):
                state_dict = state_dict[key]
                break
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    def pack(self, dtype, device):
        self._pk = {}
        if self.feat2index is not None:
            ln, lin = self.feat2index
            self._pk = dict(ln_g=dev_f32(ln.weight, device), ln_b=dev_f32(ln.bias, device),
                            w_lin=pack_w(lin.weight, dtype, device), b_lin=dev_f32(lin.bias, device))

    @torch.no_grad()
    def forward(self, x_lq, fidelity_ratio=1.0, *, code_idx=None, texture=False, trace=None):
        """x_lq: (B, 3, 512, 512) f32 in [-1, 1] on the GPU -> the reference's dict (vqfr.py:565-586): ``main_dec``
        (B, 3, 512, 512) f32, ``enc_feat`` (B, 256, 16, 16) f32, ``quant_logit`` (B, 256, 1024) f32 in "Predict" mode,
        and ``texture_dec`` when ``texture=True`` (else absent); plus ``quant_index`` (B, 256) int64, the selected codes.
        ``code_idx`` ((B, 256) integers) replaces the code selection (tests).  ``trace``: a dict that receives each
        TextureWarpingModule's (warp_feat, offset) as NHWC tensors under ``"twm.Level_<s>"`` (tests)."""
        r = RESOLUTION
        if x_lq.dim() != 4 or tuple(x_lq.shape[1:]) != (3, r, r):
            raise ValueError(f"VQFRv2 works on aligned {r}x{r} faces, got {tuple(x_lq.shape)}")
        dev, dt = x_lq.device, self.dtype
        self._ensure_packed(dev)
        B = x_lq.shape[0]
        x = torch.zeros((B, r, r, ops.pad_channels(3, dt)), dtype=dt, device=dev)
        ops.nchw_to_clip(x_lq.float().contiguous(), x, 0)
        pk = self._pk
        inp_feat = self.inpfeat_extraction.run(x)
        enc = self.encoder.run(x)                                           # (B, 16, 16, 256)
        res = {"enc_feat": ops.clip_to_nchw(enc, self.code_dim)}
        forced = None if code_idx is None else code_idx.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if self.feat2index is not None:
            t = ops.layer_norm(enc, pk["ln_g"], pk["ln_b"], eps=self.feat2index[0].eps)
            logits = ops.conv(t, pk["w_lin"], pk["b_lin"], 1024, (1, 1, 1))
            res["quant_logit"] = logits.float().reshape(B, 256, 1024)
            quant, idx = ops.argmax_codebook(logits, 1024, self.quantizer._pk["codebook"], forced_idx=forced)
        else:
            quant, idx = self.quantizer.run(enc, forced_idx=forced)
        res["quant_index"] = idx.long().reshape(B, -1)
        dec_res = self.decoder.run(quant)
        if texture:
            res["texture_dec"] = ops.clip_to_nchw(_run_conv_out(self.decoder.conv_out, dec_res["Level_1"]), 3)
        main = self.main_branch.run(dec_res, inp_feat, fidelity_ratio=fidelity_ratio, trace=trace)
        res["main_dec"] = ops.clip_to_nchw(_run_conv_out(self.decoder.conv_out, main), 3)
        return res
