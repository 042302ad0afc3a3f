"""CodeFormer auxiliary prior on the HIP kernels.

Mirror of the reference's ``guided_diffusion/codeformer.py``: ``CodeFormer(dim_embd, n_head, n_layers,
codebook_size, latent_size, connect_list)`` (:600-681) with ``forward(x, w=0, detach_16=True,
code_only=False, adain=False) -> (out, logits, lq_feat)`` (:692-753), called by the sampler as
``aux_model(pred_xstart, t, x)`` = ``gan(x0, w=1.0, adain=True)[0]`` (scripts/video_sample.py:450-452,
gaussian_diffusion.py:471-496).  The modules below are parameter containers that reproduce the
reference's state-dict names (``encoder.blocks.N.conv1.weight`` ...), so ``codeformer.pth``
(``params_ema``) loads unchanged through ``checkpoint.load_reference_checkpoint``; the arithmetic runs
on libflair_hip.so through ``flair_amd.ops`` on NHWC tensors:

  * 3x3 / 1x1 convolutions, the asymmetric stride-2 ``Downsample`` and all Linear layers (1x1 on the
    16x16 token grid): ``flair_conv_nhwc`` (MFMA);  GroupNorm(32, eps 1e-6)(+swish): ``flair_groupnorm_nhwc``;
  * transformer: ``flair_layernorm_nhwc`` (+ positional add), 8 x 64 heads on ``flair_qkv_attention``,
    GELU in the conv epilogue;  AttnBlock (one head of 512): ``flair_attention_wide``;
  * code arg-max + codebook lookup, AdaIN, SFT fusion: ``flair_argmax_codebook`` / ``flair_adain_nhwc`` /
    ``flair_sft_fuse``.

The reference runs the prior in fp32 (only the UNet is converted to fp16): ``dtype`` is float32 by default;
``convert_to_bf16()`` switches the activations / conv weights to bf16 (statistics stay f32).
Frames are a batch: no cross-frame arithmetic exists in the prior.
"""
import torch
import torch.nn as nn

from .. import ops
from .. import ops as A
from .packing import PackedModel, dev_f32, pack_w
from .vqgan_blocks import GN_EPS, AttnBlock, Downsample, HeadConv, NormOut, ResBlock, Upsample, normalize  # noqa: F401

CH_MULT = (1, 2, 2, 4, 4, 8)


class VectorQuantizer(nn.Module):
    """codeformer.py:21-94 -- only the codebook is used at inference (get_codebook_feat, via the transformer's
    indices); the nearest-neighbour ``forward`` belongs to VQGAN training."""

    def __init__(self, codebook_size, emb_dim, beta):
        super().__init__()
        self.codebook_size, self.emb_dim, self.beta = codebook_size, emb_dim, beta
        self.embedding = nn.Embedding(codebook_size, emb_dim)
        self.embedding.weight.data.uniform_(-1.0 / codebook_size, 1.0 / codebook_size)


# Downsample (codeformer.py:138-149), Upsample (:152-163), ResBlock (:166-195, shortcut ``conv_out``) and AttnBlock
# (:198-241, one head of width C on flair_attention_wide) are the shared blocks as they stand.  encoder.blocks /
# generator.blocks begin and end with a bare 3x3 convolution (HeadConv); no activation follows the final ``normalize``
# (NormOut: codeformer.py:288-292, :341-347).


class Encoder(nn.Module):
    """codeformer.py:244-299."""

    def __init__(self, in_channels, nf, emb_dim, ch_mult, num_res_blocks, resolution, attn_resolutions):
        super().__init__()
        curr_res = resolution
        in_ch_mult = (1,) + tuple(ch_mult)
        blocks = [HeadConv(in_channels, nf, kernel_size=3, stride=1, padding=1)]
        block_in_ch = nf
        for i in range(len(ch_mult)):
            block_in_ch = nf * in_ch_mult[i]
            block_out_ch = nf * ch_mult[i]
            for _ in range(num_res_blocks):
                blocks.append(ResBlock(block_in_ch, block_out_ch))
                block_in_ch = block_out_ch
                if curr_res in attn_resolutions:
                    blocks.append(AttnBlock(block_in_ch))
            if i != len(ch_mult) - 1:
                blocks.append(Downsample(block_in_ch))
                curr_res //= 2
        blocks += [ResBlock(block_in_ch, block_in_ch), AttnBlock(block_in_ch), ResBlock(block_in_ch, block_in_ch)]
        n = NormOut(block_in_ch)
        blocks += [n, HeadConv(block_in_ch, emb_dim, kernel_size=3, stride=1, padding=1)]
        self.blocks = nn.ModuleList(blocks)


class Generator(nn.Module):
    """codeformer.py:302-354."""

    def __init__(self, nf, emb_dim, ch_mult, res_blocks, img_size, attn_resolutions):
        super().__init__()
        block_in_ch = nf * ch_mult[-1]
        curr_res = img_size // 2 ** (len(ch_mult) - 1)
        blocks = [HeadConv(emb_dim, block_in_ch, kernel_size=3, stride=1, padding=1),
                  ResBlock(block_in_ch, block_in_ch), AttnBlock(block_in_ch), ResBlock(block_in_ch, block_in_ch)]
        for i in reversed(range(len(ch_mult))):
            block_out_ch = nf * ch_mult[i]
            for _ in range(res_blocks):
                blocks.append(ResBlock(block_in_ch, block_out_ch))
                block_in_ch = block_out_ch
                if curr_res in attn_resolutions:
                    blocks.append(AttnBlock(block_in_ch))
            if i != 0:
                blocks.append(Upsample(block_in_ch))
                curr_res *= 2
        blocks += [NormOut(block_in_ch),
                   HeadConv(block_in_ch, 3, kernel_size=3, stride=1, padding=1)]
        self.blocks = nn.ModuleList(blocks)


class TransformerSALayer(nn.Module):
    """codeformer.py:531-571: pre-norm self-attention (q = k = norm(x) + pos, v = norm(x)) and GELU MLP."""

    def __init__(self, embed_dim, nhead=8, dim_mlp=2048, dropout=0.0, activation="gelu"):
        super().__init__()
        if activation != "gelu" or dropout != 0.0:
            raise NotImplementedError("flair_amd: CodeFormer's transformer uses GELU and dropout 0")
        self.embed_dim, self.nhead, self.dim_mlp = embed_dim, nhead, dim_mlp
        self.self_attn = nn.MultiheadAttention(embed_dim, nhead, dropout=dropout)
        self.linear1 = nn.Linear(embed_dim, dim_mlp)
        self.linear2 = nn.Linear(dim_mlp, embed_dim)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)

    def pack(self, dtype, device):
        e, at = self.embed_dim, self.self_attn
        self._pk = dict(
            wqk=pack_w(at.in_proj_weight[:2 * e], dtype, device), bqk=dev_f32(at.in_proj_bias[:2 * e], device),
            wv=pack_w(at.in_proj_weight[2 * e:], dtype, device), bv=dev_f32(at.in_proj_bias[2 * e:], device),
            wo=pack_w(at.out_proj.weight, dtype, device), bo=dev_f32(at.out_proj.bias, device),
            w1=pack_w(self.linear1.weight, dtype, device), b1=dev_f32(self.linear1.bias, device),
            w2=pack_w(self.linear2.weight, dtype, device), b2=dev_f32(self.linear2.bias, device),
            n1_g=dev_f32(self.norm1.weight, device), n1_b=dev_f32(self.norm1.bias, device),
            n2_g=dev_f32(self.norm2.weight, device), n2_b=dev_f32(self.norm2.bias, device))

    def run(self, tgt, pos):
        pk, e = self._pk, self.embed_dim
        t2, t2pos = ops.layer_norm(tgt, pk["n1_g"], pk["n1_b"], eps=self.norm1.eps, pos=pos)
        qkv = torch.empty(tgt.shape[:3] + (3 * e,), dtype=tgt.dtype, device=tgt.device)
        ops.conv(t2pos, pk["wqk"], pk["bqk"], 2 * e, (1, 1, 1), out=qkv[..., :2 * e])
        ops.conv(t2, pk["wv"], pk["bv"], e, (1, 1, 1), out=qkv[..., 2 * e:])
        a = ops.qkv_attention(qkv, self.nhead, new_order=True)
        tgt = ops.conv(a, pk["wo"], pk["bo"], e, (1, 1, 1), res0=tgt)
        t2 = ops.layer_norm(tgt, pk["n2_g"], pk["n2_b"], eps=self.norm2.eps)
        h = ops.conv(t2, pk["w1"], pk["b1"], self.dim_mlp, (1, 1, 1), act=A.ACT_GELU)
        return ops.conv(h, pk["w2"], pk["b2"], e, (1, 1, 1), res0=tgt)


class Fuse_sft_block(nn.Module):
    """codeformer.py:574-597: out = dec + w * (dec * scale(enc) + shift(enc)), enc = ResBlock(cat[enc, dec])."""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.in_ch, self.out_ch = in_ch, out_ch
        self.encode_enc = ResBlock(2 * in_ch, out_ch)
        self.encode_enc.split = (in_ch, in_ch)      # cat[enc, dec] arrives as two segments
        self.scale = nn.Sequential(nn.Conv2d(in_ch, out_ch, kernel_size=3, padding=1), nn.LeakyReLU(0.2, True),
                                   nn.Conv2d(out_ch, out_ch, kernel_size=3, padding=1))
        self.shift = nn.Sequential(nn.Conv2d(in_ch, out_ch, kernel_size=3, padding=1), nn.LeakyReLU(0.2, True),
                                   nn.Conv2d(out_ch, out_ch, kernel_size=3, padding=1))

    def pack(self, dtype, device):
        # the first convolutions of both branches read the same tensor: one launch, 2 * out_ch outputs
        self._pk = dict(
            w0=pack_w(torch.cat([self.scale[0].weight, self.shift[0].weight], dim=0), dtype, device),
            b0=dev_f32(torch.cat([self.scale[0].bias, self.shift[0].bias]), device),
            ws=pack_w(self.scale[2].weight, dtype, device), bs=dev_f32(self.scale[2].bias, device),
            wh=pack_w(self.shift[2].weight, dtype, device), bh=dev_f32(self.shift[2].bias, device))

    def run(self, enc_feat, dec_feat, w=1.0):
        pk, co = self._pk, self.out_ch
        enc = self.encode_enc.run(enc_feat, x1=dec_feat)
        mid = ops.conv(enc, pk["w0"], pk["b0"], 2 * co, (1, 3, 3), act=A.ACT_LRELU02)
        scale = ops.conv(mid[..., :co], pk["ws"], pk["bs"], co, (1, 3, 3))
        shift = ops.conv(mid[..., co:], pk["wh"], pk["bh"], co, (1, 3, 3))
        return ops.sft_fuse(dec_feat, scale, shift, float(w))


class VQAutoEncoder(nn.Module):
    """codeformer.py:357-434 ('nearest' quantiser; the Gumbel variant and ``model_path`` loading are training-side)."""

    def __init__(self, img_size, nf, ch_mult, quantizer="nearest", res_blocks=2, attn_resolutions=(16,),
                 codebook_size=1024, emb_dim=256, beta=0.25, gumbel_straight_through=False, gumbel_kl_weight=1e-8,
                 model_path=None):
        super().__init__()
        if quantizer != "nearest":
            raise NotImplementedError("flair_amd: CodeFormer uses the 'nearest' quantiser")
        self.in_channels, self.nf, self.n_blocks = 3, nf, res_blocks
        self.codebook_size, self.embed_dim, self.ch_mult = codebook_size, emb_dim, ch_mult
        self.resolution, self.attn_resolutions = img_size, list(attn_resolutions)
        self.encoder = Encoder(3, nf, emb_dim, ch_mult, res_blocks, img_size, self.attn_resolutions)
        self.quantize = VectorQuantizer(codebook_size, emb_dim, beta)
        self.generator = Generator(nf, emb_dim, ch_mult, res_blocks, img_size, self.attn_resolutions)
        if model_path is not None:                             # {'params_ema' | 'params': state_dict}, :415-428
            from ..checkpoint import load_reference_checkpoint
            load_reference_checkpoint(self, model_path)


class CodeFormer(PackedModel, VQAutoEncoder):
    """codeformer.py:600-753."""

    def __init__(self, dim_embd=512, n_head=8, n_layers=9, codebook_size=1024, latent_size=256,
                 connect_list=("32", "64", "128", "256"), fix_modules=("quantize", "generator"), vqgan_path=None):
        super().__init__(512, 64, list(CH_MULT), "nearest", 2, [16], codebook_size)
        if vqgan_path is not None:
            from ..checkpoint import load_reference_checkpoint
            load_reference_checkpoint(self, vqgan_path, strict=False)
        for module in fix_modules or ():
            for p in getattr(self, module).parameters():
                p.requires_grad = False
        self.connect_list = list(connect_list)
        self.n_layers, self.dim_embd, self.dim_mlp = n_layers, dim_embd, dim_embd * 2
        self.position_emb = nn.Parameter(torch.zeros(latent_size, dim_embd))
        self.feat_emb = nn.Linear(256, dim_embd)
        self.ft_layers = nn.Sequential(*[TransformerSALayer(embed_dim=dim_embd, nhead=n_head, dim_mlp=self.dim_mlp,
                                                            dropout=0.0) for _ in range(n_layers)])
        self.idx_pred_layer = nn.Sequential(nn.LayerNorm(dim_embd), nn.Linear(dim_embd, codebook_size, bias=False))
        self.channels = {"16": 512, "32": 256, "64": 256, "128": 128, "256": 128, "512": 64}
        self.fuse_encoder_block = {"512": 2, "256": 5, "128": 8, "64": 11, "32": 14, "16": 18}
        self.fuse_generator_block = {"16": 6, "32": 9, "64": 12, "128": 15, "256": 18, "512": 21}
        self.fuse_convs_dict = nn.ModuleDict()
        for f_size in self.connect_list:
            in_ch = self.channels[f_size]
            self.fuse_convs_dict[f_size] = Fuse_sft_block(in_ch, in_ch)

    def pack(self, dtype, device):
        self._pk = dict(
            pos=dev_f32(self.position_emb, device),
            wf=pack_w(self.feat_emb.weight, dtype, device), bf=dev_f32(self.feat_emb.bias, device),
            hn_g=dev_f32(self.idx_pred_layer[0].weight, device), hn_b=dev_f32(self.idx_pred_layer[0].bias, device),
            wi=pack_w(self.idx_pred_layer[1].weight, dtype, device),
            codebook=dev_f32(self.quantize.embedding.weight, device))

    @torch.no_grad()
    def forward(self, x, w=0, detach_16=True, code_only=False, adain=False, code_idx=None):
        """x: (B, 3, 512, 512) in [-1, 1] on the GPU -> (out (B, 3, 512, 512), logits (B, 256, codebook),
        lq_feat (B, 256, 16, 16)), all float32 NCHW like the reference.  ``code_idx`` ((B, 256) integer tensor)
        replaces the arg-max of the logits (tests)."""
        if x.shape[1:] != (3, 512, 512):
            raise ValueError(f"CodeFormer works on aligned 512x512 faces (codeformer.py:730), got {tuple(x.shape)}")
        dev, dt = x.device, self.dtype
        self._ensure_packed(dev)
        pk = self._pk
        B = x.shape[0]
        h = torch.zeros((B, 512, 512, ops.pad_channels(3, dt)), dtype=dt, device=dev)
        ops.nchw_to_clip(x.float().contiguous(), h, 0)
        # ---- encoder (:694-701)
        enc_feat = {}
        taps = {self.fuse_encoder_block[s] for s in self.connect_list}
        for i, blk in enumerate(self.encoder.blocks):
            h = blk.run(h)
            if i in taps:
                enc_feat[str(h.shape[2])] = h
        lq = h                                                     # (B, 16, 16, 256)
        # ---- transformer over the 256 tokens (:703-714); Linear layers are 1x1 convolutions on the token grid
        q = ops.conv(lq, pk["wf"], pk["bf"], self.dim_embd, (1, 1, 1))
        for layer in self.ft_layers:
            q = layer.run(q, pk["pos"])
        t = ops.layer_norm(q, pk["hn_g"], pk["hn_b"], eps=self.idx_pred_layer[0].eps)
        logits = ops.conv(t, pk["wi"], None, self.codebook_size, (1, 1, 1))
        logits_out = logits.float().reshape(B, 256, self.codebook_size)
        lq_out = ops.clip_to_nchw(lq, 256)
        if code_only:
            return logits_out, lq_out
        # ---- code lookup + AdaIN (:727-741)
        forced = None if code_idx is None else code_idx.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        quant, _ = ops.argmax_codebook(logits, self.codebook_size, pk["codebook"], forced_idx=forced)
        if adain:
            quant = ops.adain(quant, lq)
        # ---- generator with SFT fusion (:743-751)
        h = quant
        fuse = {self.fuse_generator_block[s] for s in self.connect_list}
        for i, blk in enumerate(self.generator.blocks):
            h = blk.run(h)
            if i in fuse and w > 0:
                s = str(h.shape[2])
                h = self.fuse_convs_dict[s].run(enc_feat[s], h, w)
        return ops.clip_to_nchw(h, 3), logits_out, lq_out
