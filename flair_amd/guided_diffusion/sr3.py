"""SR3-style video UNet of the bicubic x8 / x16 tasks, executed by the gfx950 kernels.

Python surface of the reference's ``guided_diffusion/sr3.py`` (``UNet`` with the same
constructor / ``forward`` arguments and state-dict names, sr3.py:317-525) including the blocks
it borrows from ``guided_diffusion/unet.py`` (ResBlock with a (3,1,1) kernel, 7-frame
TemporalAttention, BasicVSRPP that computes its own flows).  Same execution model as
``unet_new.UNetModel``: NHWC clip tensors, every layer a few calls into libflair_hip.so.

MI355X-specific restructuring:
  * every noise-embedding linear of the network (FeatureWiseAffine, the gates of
    TemporalWrapper2, ResBlock.emb_layers) is evaluated in two launches per step and the
    per-frame terms are folded into the convolution epilogue (``frame_bias``);
  * each BasicVSRPP instance of the reference resizes the low-quality clip and runs SPyNet
    itself on every step (unet.py:546-564): flows are a function of (clip, resolution) only
    and are computed once per clip and shared by all instances of that resolution;
  * Downsample = 3x3 stride-2 convolution on the im2col MFMA path.
Shipped configuration only: spatial_attn=False, with_noise_level_emb=True.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .clip_model import ClipModel
from .nn_new import linear, zero_module
from .packing import LinearStack, dev_f32, pack_w, packed_conv, pk_int, run_conv
from .unet_new import A, BasicVSRPP, Ctx, PlaceHolder, SPyNet, TemporalAttention, normalization

LazyReshaper2D = LazyReshaper3D = PlaceHolder


# ------------------------------------------------------------------------ antialiased resize
def aa_bilinear_table(n_in, n_out):
    """Index/weight table of F.interpolate(mode='bilinear', antialias=True, align_corners=False)
    along one axis (triangle filter stretched by the scale when down-sampling), as
    (taps, n_out) arrays for ``flair_gather_mac_f32``."""
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows_i, rows_w = [], []
    for i in range(n_out):
        center = scale * (i + 0.5)
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        js = np.arange(lo, hi)
        w = np.clip(1.0 - np.abs((js - center + 0.5) * inv), 0.0, None).astype(np.float32)
        w = w / w.sum()
        rows_i.append(js)
        rows_w.append(w)
    taps = max(len(r) for r in rows_i)
    idx = np.zeros((taps, n_out), dtype=np.int32)
    wt = np.zeros((taps, n_out), dtype=np.float32)
    for i, (js, w) in enumerate(zip(rows_i, rows_w)):
        idx[:len(js), i] = js
        wt[:len(js), i] = w
        idx[len(js):, i] = js[-1]
    return idx, wt


def aa_resize(x, size):
    """(N,C,H,W) f32 device tensor -> (N,C,*size) with antialiased bilinear filtering; size: a side or (h, w)."""
    N, C, H, W = x.shape
    dev = x.device
    out = x.float().contiguous()
    sizes = (size, size) if isinstance(size, int) else tuple(size)
    for dim, n_in, size in ((2, H, sizes[0]), (3, W, sizes[1])):
        idx, wt = aa_bilinear_table(n_in, size)
        shape = list(out.shape)
        outer = int(np.prod(shape[:dim]))
        inner = int(np.prod(shape[dim + 1:])) if dim + 1 < 4 else 1
        out = ops.gather_mac(out, outer, n_in, inner, torch.from_numpy(idx).to(dev), torch.from_numpy(wt).to(dev))
        shape[dim] = size
        out = out.reshape(shape)
    return out


# ------------------------------------------------------------------------------- containers
class PositionalEncoding(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim


class Swish(nn.Module):
    pass


class FeatureWiseAffine(nn.Module):
    def __init__(self, in_channels, out_channels, use_affine_level=False):
        super().__init__()
        if use_affine_level:
            raise NotImplementedError("flair_amd: use_affine_level is not used by FLAIR")
        self.noise_func = nn.Sequential(nn.Linear(in_channels, out_channels))


class Block(nn.Module):
    """sr3.py:113-126."""

    def __init__(self, dim, dim_out, groups=32, dropout=0):
        super().__init__()
        self.block = nn.Sequential(LazyReshaper3D(nn.GroupNorm(groups, dim)), Swish(), nn.Identity(),
                                   LazyReshaper2D(nn.Conv2d(dim, dim_out, 3, padding=1)))
        self.groups = groups


class ResnetBlock(nn.Module):
    """sr3.py:129-161."""

    def __init__(self, dim, dim_out, noise_level_emb_dim=None, dropout=0, use_affine_level=False,
                 norm_groups=32, use_checkpoint=False):
        super().__init__()
        self.dim, self.dim_out = dim, dim_out
        self.noise_func = FeatureWiseAffine(noise_level_emb_dim, dim_out, use_affine_level)
        self.block1 = Block(dim, dim_out, groups=norm_groups)
        self.block2 = Block(dim_out, dim_out, groups=norm_groups, dropout=dropout)
        self.res_conv = LazyReshaper2D(nn.Conv2d(dim, dim_out, 1)) if dim != dim_out else nn.Identity()

    plain_off = pk_int("plain_off")

    def pack(self, dtype, device, split=None, plain_off=0):
        """plain_off / silu_off (below): where a module's noise-embedding linear starts in the network's two batched
        matrices (Ctx.plain_all, Ctx.silu_all)."""
        c, co = self.dim, self.dim_out
        b1, b2 = self.block1.block, self.block2.block
        self._pk = dict(
            plain_off=plain_off,
            g1=dev_f32(b1[0].wrapped_module.weight, device), be1=dev_f32(b1[0].wrapped_module.bias, device),
            w1=pack_w(b1[3].wrapped_module.weight, dtype, device, [(c, c)]), b1=dev_f32(b1[3].wrapped_module.bias, device),
            g2=dev_f32(b2[0].wrapped_module.weight, device), be2=dev_f32(b2[0].wrapped_module.bias, device),
            w2=pack_w(b2[3].wrapped_module.weight, dtype, device, [(co, co)]), b2=dev_f32(b2[3].wrapped_module.bias, device))
        if not isinstance(self.res_conv, nn.Identity):
            segs = [(s, s) for s in (split or [c])]
            self._pk["ws"] = pack_w(self.res_conv.wrapped_module.weight, dtype, device, segs)
            self._pk["bs"] = dev_f32(self.res_conv.wrapped_module.bias, device)

    def run(self, ctx, x, x1=None):
        pk, co = self._pk, self.dim_out
        g = self.block1.groups
        eps = self.block1.block[0].wrapped_module.eps
        h = ops.group_norm(x, pk["g1"], pk["be1"], x1=x1, groups=g, eps=eps, act=A.ACT_SILU)
        h = ops.conv(h, pk["w1"], pk["b1"], co, (1, 3, 3),
                     frame_bias=ctx.plain_all[:, pk["plain_off"]:pk["plain_off"] + co])
        h = ops.group_norm(h, pk["g2"], pk["be2"], groups=g, eps=eps, act=A.ACT_SILU)
        if "ws" in pk:
            skip = ops.conv([x] if x1 is None else [x, x1], pk["ws"], pk["bs"], co, (1, 1, 1))
        else:
            assert x1 is None
            skip = x
        return ops.conv(h, pk["w2"], pk["b2"], co, (1, 3, 3), res0=skip)


class ResBlock(nn.Module):
    """guided_diffusion/unet.py:113-254 as sr3 uses it: dims=3, kernel (3,1,1), no FiLM
    (``h + emb_out`` before the second norm), identity skip."""

    def __init__(self, channels, emb_channels, dropout, kernel_size=3, padding=1, out_channels=None,
                 use_scale_shift_norm=False, dims=2, use_checkpoint=False, **kw):
        super().__init__()
        if use_scale_shift_norm or (out_channels or channels) != channels:
            raise NotImplementedError("flair_amd: sr3 uses plain ResBlocks with identity skip")
        self.channels, self.dims = channels, dims
        self.kernel = (kernel_size,) * dims if isinstance(kernel_size, int) else tuple(kernel_size)
        conv = nn.Conv2d if dims == 2 else nn.Conv3d
        self.in_layers = nn.Sequential(LazyReshaper3D(normalization(channels)), nn.SiLU(),
                                       PlaceHolder(conv(channels, channels, kernel_size, padding=padding)))
        self.emb_layers = nn.Sequential(nn.SiLU(), linear(emb_channels, channels))
        self.out_layers = nn.Sequential(
            LazyReshaper3D(normalization(channels)), nn.SiLU(), nn.Dropout(p=dropout),
            zero_module(PlaceHolder(conv(channels, channels, kernel_size, padding=padding))))
        self.skip_connection = nn.Identity()

    silu_off = pk_int("silu_off")

    def pack(self, dtype, device, silu_off=0):
        c = self.channels
        self._pk = dict(
            silu_off=silu_off,
            g1=dev_f32(self.in_layers[0].wrapped_module.weight, device), be1=dev_f32(self.in_layers[0].wrapped_module.bias, device),
            w1=pack_w(self.in_layers[2].wrapped_module.weight, dtype, device, [(c, c)]),
            b1=dev_f32(self.in_layers[2].wrapped_module.bias, device),
            g2=dev_f32(self.out_layers[0].wrapped_module.weight, device), be2=dev_f32(self.out_layers[0].wrapped_module.bias, device),
            w2=pack_w(self.out_layers[3].wrapped_module.weight, dtype, device, [(c, c)]),
            b2=dev_f32(self.out_layers[3].wrapped_module.bias, device))

    def run(self, ctx, x):
        pk, c = self._pk, self.channels
        k = self.kernel if self.dims == 3 else (1,) + self.kernel
        eps = self.in_layers[0].wrapped_module.eps
        h = ops.group_norm(x, pk["g1"], pk["be1"], eps=eps, act=A.ACT_SILU)
        h = ops.conv(h, pk["w1"], pk["b1"], c, k, frame_bias=ctx.silu_all[:, pk["silu_off"]:pk["silu_off"] + c])
        h = ops.group_norm(h, pk["g2"], pk["be2"], eps=eps, act=A.ACT_SILU)
        return ops.conv(h, pk["w2"], pk["b2"], c, k, res0=x)


class TemporalWrapper(PlaceHolder):
    """unet.py:64-77 (learnable scalar gate) -- not used by the shipped sr3 configuration."""

    def __init__(self, module):
        super().__init__(module)
        self.weight = nn.Parameter(torch.zeros(1))


class TemporalWrapper2(nn.Module):
    """sr3.py:203-226: (1 - s) x + s module(x), s = sigmoid(Linear(SiLU(emb)))."""

    def __init__(self, module, dim, time_emb_dim=512):
        super().__init__()
        self.wrapped_module = module
        self.dim = dim
        self.emb_layers = nn.Sequential(nn.SiLU(), zero_module(linear(time_emb_dim, dim)))

    silu_off = pk_int("silu_off")

    def pack(self, dtype, device, silu_off=0):
        self._pk = dict(silu_off=silu_off)

    def blend(self, ctx, x, m):
        off = self._pk["silu_off"]
        return ops.gated_blend(x, m, ctx.silu_all[:, off:off + self.dim])


class FlowVSRPP(BasicVSRPP):
    """unet.py:313-595: BasicVSRPP holding the shared SPyNet (state-dict compatibility); flows
    are supplied by the UNet (computed once per clip and resolution)."""

    def __init__(self, mid_channels=64, max_residue_magnitude=10, use_checkpoint=False, shared_spynet=None):
        super().__init__(mid_channels, max_residue_magnitude, use_checkpoint)
        self.spynet = shared_spynet


class ResnetBlocWithAttn(nn.Module):
    """sr3.py:229-314."""

    def __init__(self, dim, dim_out, *, noise_level_emb_dim=None, norm_groups=32, dropout=0, conv_3d=False,
                 spatial_attn=False, temporal_attn=False, conv_3d_kernel_size=(3, 1, 1), num_frames=5,
                 head_dim=32, vsrpp=False, shared_spynet=None, use_checkpoint=False):
        super().__init__()
        if spatial_attn:
            raise NotImplementedError("flair_amd: sr3 SelfAttention is disabled in FLAIR's configuration")
        self.spatial_attn = False
        e = noise_level_emb_dim
        self.res_block = ResnetBlock(dim, dim_out, e, norm_groups=norm_groups, dropout=dropout)
        if conv_3d:
            k = conv_3d_kernel_size
            self.conv_3d = TemporalWrapper2(
                ResBlock(dim_out, e, 0.0, dims=3, kernel_size=k, padding=(k[0] // 2, k[1] // 2, k[2] // 2)),
                dim_out, time_emb_dim=e)
        if temporal_attn:
            self.temp_attn = TemporalWrapper2(
                TemporalAttention(dim_out, num_frames=num_frames, num_heads=8, num_head_channels=head_dim),
                dim_out, time_emb_dim=e)
        if vsrpp:
            self.vsrpp = TemporalWrapper2(FlowVSRPP(dim_out, max_residue_magnitude=5, shared_spynet=shared_spynet),
                                          dim_out, time_emb_dim=e)

    def run(self, ctx, x, x1=None):
        x = self.res_block.run(ctx, x, x1)
        if not ctx.enable_cross_frames:
            return x
        if hasattr(self, "conv_3d"):
            x = self.conv_3d.blend(ctx, x, self.conv_3d.wrapped_module.run(ctx, x))
        if hasattr(self, "temp_attn"):
            x = self.temp_attn.blend(ctx, x, self.temp_attn.wrapped_module.run(ctx, x))
        if hasattr(self, "vsrpp"):
            x = self.vsrpp.blend(ctx, x, self.vsrpp.wrapped_module.run(ctx, x))
        return x


class Downsample(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv2d(dim, dim, 3, 2, 1)

    def pack(self, dtype, device):
        self._pk = packed_conv(self.conv, None, dtype, device)

    def run(self, x):
        return run_conv(x, self._pk, self.conv)


class Upsample(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="nearest")
        self.conv = nn.Conv2d(dim, dim, 3, padding=1)

    def pack(self, dtype, device):
        self._pk = packed_conv(self.conv, None, dtype, device)

    def run(self, x):
        up = ops.resize(x, (2 * x.shape[1], 2 * x.shape[2]), ops.RESIZE_NEAREST)
        return run_conv(up, self._pk, self.conv)


class UNet(ClipModel, nn.Module):
    """sr3.py:317-525.  ``timesteps`` is the continuous noise level sqrt(acp_prev)[t+1] that
    respace._WrappedModel supplies (attribute ``takes_noise_level``)."""

    takes_noise_level = True
    _name = "flair_amd.sr3.UNet"

    def __init__(self, in_channel=6, out_channel=3, inner_channel=32, norm_groups=32,
                 channel_mults=(1, 2, 4, 8, 8), attn_res=(8,), vsrpp_res=(64,), spatial_attn=False,
                 temporal_attn=False, res_blocks=3, dropout=0, with_noise_level_emb=True, image_size=128,
                 dtype=torch.float32, cross_frame_module=False, use_checkpoint=False, num_frames=5, head_dim=32):
        super().__init__()
        if spatial_attn or not with_noise_level_emb:
            raise NotImplementedError("flair_amd: sr3.UNet covers FLAIR's configuration "
                                      "(spatial_attn=False, with_noise_level_emb=True)")
        self.in_channel, self.out_channel, self.inner_channel = in_channel, out_channel, inner_channel
        self.image_size = image_size
        self.dtype = torch.bfloat16 if dtype in (torch.float16, torch.bfloat16) else torch.float32
        shared = SPyNet(pretrained=None) if len(vsrpp_res) > 0 else None
        self._shared_spynet = [shared]          # not a registered child here (as in the reference)
        e = inner_channel
        self.noise_level_mlp = nn.Sequential(PositionalEncoding(inner_channel), nn.Linear(inner_channel, inner_channel * 4),
                                             Swish(), nn.Linear(inner_channel * 4, inner_channel))

        def blk(cin, cout, res):
            return ResnetBlocWithAttn(
                cin, cout, noise_level_emb_dim=e, norm_groups=norm_groups, dropout=dropout, conv_3d=cross_frame_module,
                temporal_attn=(res in attn_res and temporal_attn and cross_frame_module), num_frames=num_frames,
                head_dim=head_dim, vsrpp=(res in vsrpp_res and cross_frame_module),
                shared_spynet=shared if (res in vsrpp_res and cross_frame_module) else None)

        pre, res = inner_channel, image_size
        feats = [pre]
        downs = [LazyReshaper2D(nn.Conv2d(in_channel, inner_channel, kernel_size=3, padding=1))]
        n = len(channel_mults)
        for i in range(n):
            ch = inner_channel * channel_mults[i]
            for _ in range(res_blocks):
                downs.append(blk(pre, ch, res))
                feats.append(ch)
                pre = ch
            if i != n - 1:
                downs.append(LazyReshaper2D(Downsample(pre)))
                feats.append(pre)
                res //= 2
        self.downs = nn.ModuleList(downs)
        mk = dict(noise_level_emb_dim=e, norm_groups=norm_groups, dropout=dropout, conv_3d=cross_frame_module,
                  temporal_attn=temporal_attn and cross_frame_module, num_frames=num_frames, head_dim=head_dim)
        self.mid = nn.ModuleList([ResnetBlocWithAttn(pre, pre, **mk), ResnetBlocWithAttn(pre, pre, **mk)])
        ups, self._skip_split = [], {}
        for i in reversed(range(n)):
            ch = inner_channel * channel_mults[i]
            for _ in range(res_blocks + 1):
                skip = feats.pop()
                b = blk(pre + skip, ch, res)
                self._skip_split[id(b.res_block)] = [pre, skip]
                ups.append(b)
                pre = ch
            if i >= 1:
                ups.append(LazyReshaper2D(Upsample(pre)))
                res *= 2
        self.ups = nn.ModuleList(ups)
        self.final_conv = Block(pre, out_channel if out_channel is not None else in_channel, groups=norm_groups)

    # ---- packing -----------------------------------------------------------------------
    def _pack_all(self, dt, device):
        stem = self.downs[0].wrapped_module
        stem._pk = packed_conv(stem, None, dt, device)
        plain, silu = LinearStack(), LinearStack()
        for m in self.modules():
            if isinstance(m, ResnetBlock):
                m.pack(dt, device, self._skip_split.get(id(m)), plain_off=plain.add(m.noise_func.noise_func[0]))
            elif isinstance(m, (ResBlock, TemporalWrapper2)):
                m.pack(dt, device, silu_off=silu.add(m.emb_layers[1]))
            elif isinstance(m, (TemporalAttention, BasicVSRPP, Downsample, Upsample)):
                m.pack(dt, device)
        if self._shared_spynet[0] is not None:
            self._shared_spynet[0].to(device)
            self._shared_spynet[0].pack(dt, device)
        mlp, fc = self.noise_level_mlp, self.final_conv.block
        self._pk = dict(
            plain=plain.cat(device), silu=silu.cat(device),
            mlp=[dev_f32(p, device) for p in (mlp[1].weight, mlp[1].bias, mlp[3].weight, mlp[3].bias)],
            fin_g=dev_f32(fc[0].wrapped_module.weight, device), fin_b=dev_f32(fc[0].wrapped_module.bias, device),
            fin=packed_conv(fc[3].wrapped_module, None, dt, device))
        self._flow_cache = {}

    # ---- flows: once per (clip, resolution) ----------------------------------------------
    def _flow_spec(self, H, W, enable_cross_frames):
        return tuple(self._flow_resolutions(H, W)) if enable_cross_frames else ()

    def _compute_flows(self, rnn_clip, resolutions):
        flows = {}
        for rh, r in resolutions:                         # (height, width) of a level, stored under its width
            src = rnn_clip if tuple(rnn_clip.shape[-2:]) == (rh, r) else aa_resize(rnn_clip, (rh, r))
            raw = torch.zeros((src.shape[0], rh, r, 4), dtype=torch.float32, device=src.device)
            ops.nchw_to_clip(src.contiguous(), raw, 0)
            flows[r] = self._shared_spynet[0].pair_flows(raw)
        return flows

    # ---- forward (clip_model.ClipModel: per-clip slicing, graph capture / replay, the flow cache) ------------------
    def forward(self, x, timesteps, low_res_input=None, rnn_input=None, num_frames=None,
                enable_cross_frames=True, vsrpp_weights=None, **kwargs):
        return self._run_clips(x, timesteps, low_res_input, rnn_input, num_frames, enable_cross_frames, vsrpp_weights)

    def _forward_clip(self, x, level, low_res, flows, enable_cross_frames, vsrpp_weights):
        T, _, H, W = x.shape
        dev, dt = x.device, self.dtype
        ctx = Ctx(dt, dev, T)
        ctx.enable_cross_frames = enable_cross_frames
        ctx.vsrpp_weights = vsrpp_weights
        ctx.flows = flows
        pe = ops.timestep_embedding(level, self.inner_channel, sin_first=True)
        pk = self._pk
        e = ops.linear(pe, pk["mlp"][0], pk["mlp"][1], act_out=A.ACT_SILU)
        emb = ops.linear(e, pk["mlp"][2], pk["mlp"][3])
        ctx.plain_all = ops.linear(emb, pk["plain"][0], pk["plain"][1])
        ctx.silu_all = ops.linear(emb, pk["silu"][0], pk["silu"][1], act_in=A.ACT_SILU)
        cin = ops.pad_channels(self.in_channel, dt)
        h = torch.zeros((T, H, W, cin), dtype=dt, device=dev)
        ops.nchw_to_clip(low_res, h, 0)
        ops.nchw_to_clip(x, h, low_res.shape[1])
        feats = []
        for layer in self.downs:
            h = self._run_layer(ctx, layer, h)
            feats.append(h)
        for layer in self.mid:
            h = layer.run(ctx, h)
        for layer in self.ups:
            if isinstance(layer, ResnetBlocWithAttn):
                h = layer.run(ctx, h, feats.pop())
            else:
                h = self._run_layer(ctx, layer, h)
        fc = self.final_conv
        h = ops.group_norm(h, pk["fin_g"], pk["fin_b"], groups=fc.groups, eps=fc.block[0].wrapped_module.eps, act=A.ACT_SILU)
        y = run_conv(h, pk["fin"], fc.block[3].wrapped_module)
        return ops.clip_to_nchw(y, fc.block[3].wrapped_module.out_channels)

    def _flow_resolutions(self, H, W):
        """(h, w) of every level that carries a BasicVSRPP for an H x W clip, by ascending width: the flow input is
        resized to the level's own shape (the reference resizes to ``hidden.shape[-2:]``)."""
        hs, ws = ([r for r, _ in self._vsrpp_levels(n)] for n in (H, W))
        return sorted(set(zip(hs, ws)), key=lambda p: p[1])

    def _vsrpp_levels(self, size):
        """(resolution, module) of every BasicVSRPP in the network for an input of side `size`."""
        out, res = [], size
        for layer in self.downs:
            if isinstance(layer, ResnetBlocWithAttn):
                if hasattr(layer, "vsrpp"):
                    out.append((res, layer.vsrpp.wrapped_module))
            elif isinstance(layer.wrapped_module, Downsample):
                res //= 2
        for layer in self.ups:
            if isinstance(layer, ResnetBlocWithAttn):
                if hasattr(layer, "vsrpp"):
                    out.append((res, layer.vsrpp.wrapped_module))
            elif isinstance(layer.wrapped_module, Upsample):
                res *= 2
        return out

    def _run_layer(self, ctx, layer, h):
        if isinstance(layer, ResnetBlocWithAttn):
            return layer.run(ctx, h)
        inner = layer.wrapped_module
        if isinstance(inner, nn.Conv2d):                # the stem
            return run_conv(h, inner._pk, inner)
        if isinstance(inner, (Downsample, Upsample)):
            return inner.run(h)
        raise TypeError(f"flair_amd: no executor for {type(inner).__name__}")
