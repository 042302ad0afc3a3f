"""RestoreFormer auxiliary prior on the HIP kernels: the reference's ``guided_diffusion/restoreformer.py``.

Mirror of ``VQVAEGANMultiHeadTransformer`` (restoreformer.py:764-861) and the classes it is built from
(``VectorQuantizer`` :7-108, ``Upsample`` / ``Downsample`` :122-155, ``ResnetBlock`` :158-215,
``MultiHeadAttnBlock`` :218-285, ``MultiHeadEncoder`` :288-412, ``MultiHeadDecoderTransformer`` :543-675) with the
reference's constructor arguments and defaults, so the 441 state-dict tensors keep their names and shapes.  The
sampler calls it as ``aux_model(pred_xstart, t, x)`` = ``net(x0)[0]`` (workload.restoreformer_aux,
gaussian_diffusion.py:471-496).  The modules are parameter containers; the arithmetic runs on libflair_hip.so
through ``flair_amd.ops`` on NHWC tensors, as for the CodeFormer prior:

  * 3x3 / 1x1 convolutions and the asymmetric stride-2 ``Downsample``: ``flair_conv_nhwc`` (MFMA);
    GroupNorm(32, eps 1e-6)(+swish) per face: ``flair_groupnorm_nhwc``;  nearest x2: ``flair_resize_nhwc``;
  * ``MultiHeadAttnBlock``: q | k | v as three channel slices of one buffer (the reference's
    ``reshape(b, head, att, hw)`` is the new-order layout) on ``flair_qkv_attention``, the projection with the
    residual in its epilogue.  Self-attention in the encoder; in the decoder q comes from ``norm2`` of the encoder
    feature ``hs[...]`` and k, v from ``norm1(x)``;
  * the codebook search (f32 distances whatever the activation dtype): ``flair_vq_nearest_nhwc``.

The reference runs the prior in fp32: ``dtype`` is float32 by default; ``convert_to_bf16()`` switches activations and
conv weights to bf16 (statistics and the codebook search stay f32).  Faces are a batch: nothing mixes them.
The non-transformer ``VQVAEGAN`` / ``MultiHeadDecoder`` are not ported: no path reaches them.
"""
from collections.abc import Mapping

import torch
import torch.nn as nn

from .. import ops
from .. import ops as A
from . import vqgan_blocks as vb
from .packing import PackedModel, dev_f32, pack_w
from .unet_new import qkv_head_width
from .vqgan_blocks import HeadConv, NormOut, gn
from .vqgan_blocks import normalize as Normalize          # restoreformer.py:116-119


class VectorQuantizer(nn.Module):
    """restoreformer.py:7-108: nearest-codebook-row quantiser.  Only the search and the lookup run at inference
    (``run``); the commitment loss, perplexity and one-hot encodings belong to training."""

    def __init__(self, n_e, e_dim, beta):
        super().__init__()
        self.n_e, self.e_dim, self.beta = n_e, e_dim, beta
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)

    def pack(self, dtype, device):
        self._pk = dict(codebook=dev_f32(self.embedding.weight, device))

    def run(self, z, forced_idx=None):
        return ops.vq_nearest(z, self._pk["codebook"], forced_idx=forced_idx)


def _with_conv(with_conv):
    if not with_conv:
        raise NotImplementedError("flair_amd: RestoreFormer resamples with convolutions (resamp_with_conv=True)")
    return with_conv


class Upsample(vb.Upsample):
    """restoreformer.py:122-135."""

    def __init__(self, in_channels, with_conv):
        super().__init__(in_channels)
        self.with_conv = _with_conv(with_conv)


class Downsample(vb.Downsample):
    """restoreformer.py:138-155."""

    def __init__(self, in_channels, with_conv):
        super().__init__(in_channels)
        self.with_conv = _with_conv(with_conv)


class ResnetBlock(vb.ResBlock):
    """restoreformer.py:158-215; the shortcut is ``nin_shortcut`` (1x1) or ``conv_shortcut`` (3x3).  The network never
    passes a timestep embedding (temb is None throughout), so a ``temb_proj`` built for ``temb_channels > 0`` is a
    parameter container only; dropout is inference-time identity."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512):
        super().__init__(in_channels, out_channels, shortcut_kernel=3 if conv_shortcut else 1,
                         shortcut="conv_shortcut" if conv_shortcut else "nin_shortcut")
        self.use_conv_shortcut = conv_shortcut
        if temb_channels > 0:
            self.temb_proj = nn.Linear(temb_channels, self.out_channels)
        self.dropout = nn.Dropout(dropout)


class MultiHeadAttnBlock(nn.Module):
    """restoreformer.py:218-285: ``head_size`` heads of width ``in_channels // head_size`` over the h*w pixels, scale
    att_size**-0.5.  ``run(x)`` is self-attention (q, k, v from norm1(x)); ``run(x, y)`` takes q from norm2(y)."""

    def __init__(self, in_channels, head_size=1):
        super().__init__()
        self.in_channels = in_channels
        self.head_size = head_size
        self.att_size = in_channels // head_size
        assert in_channels % head_size == 0, "The size of head should be divided by the number of channels."
        qkv_head_width(in_channels, head_size)          # widths flair_qkv_attention cannot run are refused here
        self.norm1 = Normalize(in_channels)
        self.norm2 = Normalize(in_channels)
        self.q = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.num = 0

    def pack(self, dtype, device):
        self._pk = dict(n1_g=dev_f32(self.norm1.weight, device), n1_b=dev_f32(self.norm1.bias, device),
                        n2_g=dev_f32(self.norm2.weight, device), n2_b=dev_f32(self.norm2.bias, device),
                        wq=pack_w(self.q.weight, dtype, device), bq=dev_f32(self.q.bias, device),
                        wkv=pack_w(torch.cat([self.k.weight, self.v.weight], dim=0), dtype, device),
                        bkv=dev_f32(torch.cat([self.k.bias, self.v.bias]), device),
                        wqkv=pack_w(torch.cat([self.q.weight, self.k.weight, self.v.weight], dim=0), dtype, device),
                        bqkv=dev_f32(torch.cat([self.q.bias, self.k.bias, self.v.bias]), device),
                        wp=pack_w(self.proj_out.weight, dtype, device), bp=dev_f32(self.proj_out.bias, device))

    def run(self, x, y=None):
        pk, c = self._pk, self.in_channels
        h_ = gn(x, pk, "n1")
        if y is None:
            qkv = ops.conv(h_, pk["wqkv"], pk["bqkv"], 3 * c, (1, 1, 1))
        else:
            assert y.shape == x.shape, (tuple(y.shape), tuple(x.shape))
            qkv = torch.empty(x.shape[:3] + (3 * c,), dtype=x.dtype, device=x.device)
            ops.conv(gn(y, pk, "n2"), pk["wq"], pk["bq"], c, (1, 1, 1), out=qkv[..., :c])
            ops.conv(h_, pk["wkv"], pk["bkv"], 2 * c, (1, 1, 1), out=qkv[..., c:])
        a = ops.qkv_attention(qkv, self.head_size, new_order=True)
        return ops.conv(a, pk["wp"], pk["bp"], c, (1, 1, 1), res0=x)


class MultiHeadEncoder(nn.Module):
    """restoreformer.py:288-412.  ``run`` returns the NHWC features under the reference's ``hs`` keys."""

    def __init__(self, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks=2, attn_resolutions=[16], dropout=0.0,
                 resamp_with_conv=True, in_channels=3, resolution=512, z_channels=256, double_z=True, enable_mid=True,
                 head_size=1, **ignore_kwargs):
        super().__init__()
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.enable_mid = enable_mid
        self.conv_in = HeadConv(in_channels, self.ch, kernel_size=3, stride=1, padding=1)
        curr_res = resolution
        in_ch_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        for i_level in range(self.num_resolutions):
            block, attn = nn.ModuleList(), nn.ModuleList()
            block_in = ch * in_ch_mult[i_level]
            block_out = ch * ch_mult[i_level]
            for _ in range(self.num_res_blocks):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch,
                                         dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(MultiHeadAttnBlock(block_in, head_size))
            down = nn.Module()
            down.block = block
            down.attn = attn
            if i_level != self.num_resolutions - 1:
                down.downsample = Downsample(block_in, resamp_with_conv)
                curr_res = curr_res // 2
            self.down.append(down)
        if self.enable_mid:
            self.mid = nn.Module()
            self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch,
                                           dropout=dropout)
            self.mid.attn_1 = MultiHeadAttnBlock(block_in, head_size)
            self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch,
                                           dropout=dropout)
        self.norm_out = NormOut(block_in, A.ACT_SILU)
        self.conv_out = HeadConv(block_in, 2 * z_channels if double_z else z_channels, kernel_size=3, stride=1, padding=1)

    def run(self, x):
        """restoreformer.py:375-412 on a clip tensor -> {hs key: clip tensor}."""
        hs = {}
        h = self.conv_in.run(x)
        hs["in"] = h
        for i_level in range(self.num_resolutions):
            for i_block in range(self.num_res_blocks):
                h = self.down[i_level].block[i_block].run(h)
                if len(self.down[i_level].attn) > 0:
                    h = self.down[i_level].attn[i_block].run(h)
            if i_level != self.num_resolutions - 1:
                hs["block_" + str(i_level)] = h
                h = self.down[i_level].downsample.run(h)
        if self.enable_mid:
            h = self.mid.block_1.run(h)
            hs["block_" + str(i_level) + "_atten"] = h
            h = self.mid.attn_1.run(h)
            h = self.mid.block_2.run(h)
            hs["mid_atten"] = h
        hs["out"] = self.conv_out.run(self.norm_out.run(h))
        return hs


class MultiHeadDecoderTransformer(nn.Module):
    """restoreformer.py:543-675: the decoder whose attention blocks take their queries from the encoder's features."""

    def __init__(self, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks=2, attn_resolutions=16, dropout=0.0,
                 resamp_with_conv=True, in_channels=3, resolution=512, z_channels=256, give_pre_end=False,
                 enable_mid=True, head_size=1, **ignorekwargs):
        super().__init__()
        self.ch = ch
        self.temb_ch = 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution = resolution
        self.in_channels = in_channels
        self.give_pre_end = give_pre_end
        self.enable_mid = enable_mid
        self.out_ch = out_ch
        block_in = ch * ch_mult[self.num_resolutions - 1]
        curr_res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, curr_res, curr_res)
        self.conv_in = HeadConv(z_channels, block_in, kernel_size=3, stride=1, padding=1)
        if self.enable_mid:
            self.mid = nn.Module()
            self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch,
                                           dropout=dropout)
            self.mid.attn_1 = MultiHeadAttnBlock(block_in, head_size)
            self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch,
                                           dropout=dropout)
        self.up = nn.ModuleList()
        for i_level in reversed(range(self.num_resolutions)):
            block, attn = nn.ModuleList(), nn.ModuleList()
            block_out = ch * ch_mult[i_level]
            for _ in range(self.num_res_blocks + 1):
                block.append(ResnetBlock(in_channels=block_in, out_channels=block_out, temb_channels=self.temb_ch,
                                         dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    attn.append(MultiHeadAttnBlock(block_in, head_size))
            up = nn.Module()
            up.block = block
            up.attn = attn
            if i_level != 0:
                up.upsample = Upsample(block_in, resamp_with_conv)
                curr_res = curr_res * 2
            self.up.insert(0, up)
        self.norm_out = NormOut(block_in, A.ACT_SILU)
        self.conv_out = HeadConv(block_in, out_ch, kernel_size=3, stride=1, padding=1)

    def run(self, z, hs):
        """restoreformer.py:636-675 on clip tensors (``hs``: the encoder's NHWC features)."""
        h = self.conv_in.run(z)
        if self.enable_mid:
            h = self.mid.block_1.run(h)
            h = self.mid.attn_1.run(h, hs["mid_atten"])
            h = self.mid.block_2.run(h)
        for i_level in reversed(range(self.num_resolutions)):
            for i_block in range(self.num_res_blocks + 1):
                h = self.up[i_level].block[i_block].run(h)
                if len(self.up[i_level].attn) > 0:
                    key = "block_" + str(i_level) + "_atten"
                    if key not in hs:
                        key = "block_" + str(i_level)
                    h = self.up[i_level].attn[i_block].run(h, hs[key])
            if i_level != 0:
                h = self.up[i_level].upsample.run(h)
        if self.give_pre_end:
            return h
        return self.conv_out.run(self.norm_out.run(h))


class Features(Mapping):
    """The encoder's ``hs`` as the reference returns it -- (B, C, H, W) float32 tensors under its keys -- converted
    from the NHWC features on first access (the sampler's closure never reads them)."""

    def __init__(self, clips):
        self._clips, self._nchw = clips, {}

    def __getitem__(self, key):
        if key not in self._nchw:
            h = self._clips[key]
            self._nchw[key] = ops.clip_to_nchw(h, h.shape[3])
        return self._nchw[key]

    def __iter__(self):
        return iter(self._clips)

    def __len__(self):
        return len(self._clips)


STRIP_PREFIX = "vqvae."


class VQVAEGANMultiHeadTransformer(PackedModel, nn.Module):
    """restoreformer.py:764-861 (RestoreFormer).  The ``fix_*`` switches only set ``requires_grad`` (training)."""

    def __init__(self, n_embed=1024, embed_dim=256, ch=64, out_ch=3, ch_mult=(1, 2, 2, 4, 4, 8), num_res_blocks=2,
                 attn_resolutions=(16,), dropout=0.0, in_channels=3, resolution=512, z_channels=256, double_z=False,
                 enable_mid=True, fix_decoder=False, fix_codebook=True, fix_encoder=False, head_size=4,
                 ex_multi_scale_num=1):
        super().__init__()
        self.encoder = MultiHeadEncoder(ch=ch, out_ch=out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                                        attn_resolutions=attn_resolutions, dropout=dropout, in_channels=in_channels,
                                        resolution=resolution, z_channels=z_channels, double_z=double_z,
                                        enable_mid=enable_mid, head_size=head_size)
        for _ in range(ex_multi_scale_num):
            attn_resolutions = [attn_resolutions[0], attn_resolutions[-1] * 2]
        self.decoder = MultiHeadDecoderTransformer(ch=ch, out_ch=out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                                                   attn_resolutions=attn_resolutions, dropout=dropout,
                                                   in_channels=in_channels, resolution=resolution,
                                                   z_channels=z_channels, enable_mid=enable_mid, head_size=head_size)
        self.quantize = VectorQuantizer(n_embed, embed_dim, beta=0.25)
        self.quant_conv = nn.Conv2d(z_channels, embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, z_channels, 1)
        if fix_decoder:
            for m in (self.decoder, self.post_quant_conv, self.quantize):
                for p in m.parameters():
                    p.requires_grad = False
        elif fix_codebook:
            for p in self.quantize.parameters():
                p.requires_grad = False
        if fix_encoder:
            for m in (self.encoder, self.quant_conv):
                for p in m.parameters():
                    p.requires_grad = False
        self.in_channels, self.resolution, self.embed_dim, self.z_channels = in_channels, resolution, embed_dim, z_channels

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """The reference's names; also a RestoreFormer training checkpoint's ``state_dict`` (the network under
        ``vqvae.``, next to loss / discriminator entries): with that prefix present, it is stripped and every other
        key dropped before the strict load.  (That layout is the RestoreFormer project's Lightning format, unverified
        against a released file.)"""
        if "state_dict" in state_dict and isinstance(state_dict["state_dict"], Mapping):
            state_dict = state_dict["state_dict"]
        if any(k.startswith(STRIP_PREFIX) for k in state_dict):
            state_dict = {k[len(STRIP_PREFIX):]: v for k, v in state_dict.items() if k.startswith(STRIP_PREFIX)}
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    def pack(self, dtype, device):
        self._pk = dict(wq=pack_w(self.quant_conv.weight, dtype, device), bq=dev_f32(self.quant_conv.bias, device),
                        wpq=pack_w(self.post_quant_conv.weight, dtype, device),
                        bpq=dev_f32(self.post_quant_conv.bias, device))

    def _encode(self, input):
        """input (B, 3, r, r) f32 NCHW -> (z, hs): quant_conv's output and the encoder's features, clip tensors."""
        r = self.resolution
        if input.dim() != 4 or tuple(input.shape[1:]) != (self.in_channels, r, r):
            raise ValueError(f"RestoreFormer works on aligned {r}x{r} faces, got {tuple(input.shape)}")
        dev, dt = input.device, self.dtype
        self._ensure_packed(dev)
        h = torch.zeros((input.shape[0], r, r, ops.pad_channels(self.in_channels, dt)), dtype=dt, device=dev)
        ops.nchw_to_clip(input.float().contiguous(), h, 0)
        hs = self.encoder.run(h)
        return ops.conv(hs["out"], self._pk["wq"], self._pk["bq"], self.embed_dim, (1, 1, 1)), hs

    @torch.no_grad()
    def quant_input(self, input):
        """The tokens the codebook search ranks: quant_conv(encoder(input)["out"]) as (B, embed_dim, h, w) f32."""
        return ops.clip_to_nchw(self._encode(input)[0], self.embed_dim)

    @torch.no_grad()
    def forward(self, input, code_idx=None):
        """input: (B, 3, 512, 512) f32 in [-1, 1] on the GPU -> ``(dec, emb_loss, info, hs)`` like the reference:
        dec (B, 3, 512, 512) f32; info = (perplexity, min_encodings, min_encoding_indices (B*256, 1) int64, d);
        hs the encoder's features (a read-only mapping of (B, C, H, W) f32 tensors under the reference's keys).
        The training-only fields -- emb_loss, perplexity, the one-hot encodings and the distance matrix -- are None.
        ``code_idx`` ((B, 256) integer tensor) replaces the codebook search (tests)."""
        z, hs = self._encode(input)
        forced = None if code_idx is None else code_idx.to(device=z.device, dtype=torch.int32).reshape(-1).contiguous()
        quant, idx = self.quantize.run(z, forced_idx=forced)
        quant = ops.conv(quant, self._pk["wpq"], self._pk["bpq"], self.z_channels, (1, 1, 1))
        dec = self.decoder.run(quant, hs)
        dec = ops.clip_to_nchw(dec, dec.shape[3] if self.decoder.give_pre_end else self.decoder.out_ch)
        return dec, None, (None, None, idx.long().unsqueeze(1), None), Features(hs)
