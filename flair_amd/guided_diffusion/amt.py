"""AMT-G frame interpolation on the HIP kernels.

Mirror of the reference's ``guided_diffusion/amt.py`` and ``amt_blocks/``: ``AMT``, ``LargeEncoder`` / ``ResidualBlock``,
``Encoder``, ``ResBlock``, ``InitDecoder``, ``IntermediateDecoder``, ``MultiFlowDecoder``, ``BasicUpdateBlock`` and
``comb_block`` with the reference's constructor arguments and state-dict names (259 entries, 30 638 919 parameters: the
``state_dict`` the reference loads from ``amt-g.pth`` goes through ``load_state_dict`` unchanged).

The modules are parameter containers; float32 only.  Every convolution is one ``flair_conv_nhwc`` launch (LeakyReLU(0.1)
in its epilogue, per-channel PReLU as a separate ``flair_prelu_nhwc`` launch in place), ``torch.cat`` inputs are
convolution segments, InstanceNorm2d + ReLU is the two-pass ``flair_instnorm_nhwc``, ``ConvTranspose2d(4, 2,
1)`` is a 3x3 convolution on repacked weights plus ``flair_depth_to_space2_nhwc``, the warps are ``flair_flow_warp`` with
border padding, and the correlation pyramid and its lookup are amt.hip's.  Activations whose width is no multiple of the
16-channel K step (84, 188, 252 ...) live in wider zero-filled buffers and are read with zero weight columns; ``ResBlock``
convolves the last 84 channels of such a buffer as a view (``ifrnet.py:42-50``), no copy.

Launch schedule of ``forward``:

Pairs of a batch run one after the other (the same bits for a pair in any batch; one pair's volumes in memory at a time).

  per pair      (frame + 1) / 2, the mean and its subtraction, the x2 enlargement for frames up to 64 wide, ``feat_encoder``
                on both frames as one batch, the two volume products with their division, three poolings per direction,
                ``encoder`` on both frames as one batch (``amt.py:114-135``; the reference repeats all of it per timestep);
  per timestep  the four decoders, three lookups, five update blocks and the combine (``amt.py:137-216``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import ops as A
from .packing import PackedModel, pack_w, pad_bias, pad_cout

FP = torch.float32
K = 16                                      # f32 K step of a convolution segment


def padc(c):
    return (c + K - 1) // K * K


def supported_size(h, w):
    """(ok, padded (H, W), scale): whether AMT runs frames of h x w.  The frame is padded to multiples of 16 and, when the
    padded width is at most 64, doubled; the lookup grid g is 1/8 of that and its coarsest pyramid level g // 8 must be at
    least 2 on both sides, or exactly 1 x 1 (the reference raises on anything else, raft.py:186-191)."""
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    s = 2 if W <= 64 else 1
    gh, gw = s * H // 8 // 8, s * W // 8 // 8
    return (gh >= 2 and gw >= 2) or (gh == 1 and gw == 1), (H, W), s


def size_error(h, w):
    _, (H, W), s = supported_size(h, w)
    return (f"AMT: frames of {h}x{w} (padded to {H}x{W}, processed at x{s}) give a {s * H // 8}x{s * W // 8} lookup grid "
            f"whose coarsest pyramid level is {s * H // 64}x{s * W // 64}; that level must be at least 2x2, or exactly 1x1 "
            "(the reference raises on anything else): 32x32, 64x64 and 128x144 run; 72x144, 40x56 and 100x136 do not")


def _zeros(B, H, W, C, dev):
    return torch.zeros((B, H, W, C), dtype=FP, device=dev)


def _pack(conv, segs, dev, cout_pad=None, weight=None, bias=None):
    """A Conv2d (or explicit weight / bias) as the kernels' record: segs = (real, padded) widths of the input segments."""
    w = conv.weight.detach().float() if weight is None else weight
    b = conv.bias.detach().float() if bias is None else bias
    cpad = cout_pad or pad_cout(w.shape[0])
    return dict(w=pack_w(w, FP, dev, segs=list(segs), cout_pad=cpad), b=pad_bias(b.to(dev), cpad), cout=cpad,
                k=w.shape[2], stride=1 if conv is None else conv.stride[0])


def _run(pk, xs, act=A.ACT_NONE, out=None, res0=None):
    return ops.conv(xs, pk["w"], pk["b"], pk["cout"], (1, pk["k"], pk["k"]), stride=pk["stride"], act=act, out=out, res0=res0)


def _slope(prelu, dev):
    w = prelu.weight.detach().float().to(dev)
    return pad_bias(w, pad_cout(w.shape[0]))


def _seg(c):
    return (c, padc(c))


def convrelu(in_channels, out_channels, kernel_size=3, stride=1, padding=1):
    """ifrnet.py:10-14."""
    return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding), nn.PReLU(out_channels))


def _pack_convrelu(seq, segs, dev):
    return dict(conv=_pack(seq[0], segs, dev), slope=_slope(seq[1], dev))


def _run_convrelu(pk, xs, width=None):
    """conv + PReLU into a zero-filled buffer ``width`` channels wide (default: the output padded to the K step)."""
    x0 = xs[0] if isinstance(xs, (list, tuple)) else xs
    B, H, W, _ = x0.shape
    s = pk["conv"]["stride"]
    c = pk["conv"]["cout"]
    buf = _zeros(B, (H + s - 1) // s, (W + s - 1) // s, width or padc(c), x0.device)
    _run(pk["conv"], xs, out=buf)
    ops.prelu(buf[..., :c], pk["slope"], out=buf[..., :c])
    return buf


class ResBlock(nn.Module):
    """ifrnet.py:16-53: five 3x3 convolutions, two of them on the last ``side_channels`` channels only."""

    def __init__(self, in_channels, side_channels, bias=True):
        super().__init__()
        self.side_channels = side_channels
        self.conv1 = convrelu(in_channels, in_channels)
        self.conv2 = convrelu(side_channels, side_channels)
        self.conv3 = convrelu(in_channels, in_channels)
        self.conv4 = convrelu(side_channels, side_channels)
        self.conv5 = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self.prelu = nn.PReLU(in_channels)

    def pack(self, dtype, device):
        C, S = self.conv5.in_channels, self.side_channels
        two = [_seg(C - S), _seg(S)]                    # cat([res_feat, side_feat], 1)
        self._pk = dict(c1=_pack_convrelu(self.conv1, [_seg(C)], device), c2=_pack_convrelu(self.conv2, [_seg(S)], device),
                        c3=_pack_convrelu(self.conv3, two, device), c4=_pack_convrelu(self.conv4, [_seg(S)], device),
                        c5=_pack(self.conv5, two, device), slope=_slope(self.prelu, device))

    def run(self, x):
        """x: (B, H, W, >= padc(C)), zeros past channel C -> (B, H, W, padc(C)) likewise."""
        C, S = self.conv5.in_channels, self.side_channels
        R = C - S
        wide = padc(R + padc(S))                        # the side view R .. R + padc(S) must stay inside its pixel
        pk = self._pk
        a = _run_convrelu(pk["c1"], x[..., :padc(C)], wide)
        s = _run_convrelu(pk["c2"], a[..., R:R + padc(S)])
        b = _run_convrelu(pk["c3"], [a[..., :padc(R)], s], wide)
        s = _run_convrelu(pk["c4"], b[..., R:R + padc(S)])
        o = _run(pk["c5"], [b[..., :padc(R)], s])
        out = _zeros(*x.shape[:3], padc(C), x.device)
        ops.prelu(x[..., :C], pk["slope"], o[..., :C], out=out[..., :C])
        return out


def _pack_deconv(deconv, device):
    cin, cout = deconv.in_channels, deconv.out_channels
    w3, b3 = ops.deconv_as_conv3x3(deconv.weight.detach().float(), deconv.bias.detach().float())
    return dict(conv=_pack(None, [_seg(cin)], device, cout_pad=w3.shape[0], weight=w3, bias=b3), cout=w3.shape[0] // 4)


def _run_convblock(seq, pk, xs, out_width):
    """convrelu, ResBlock, ConvTranspose2d(4, 2, 1) -> (B, 2H, 2W, out_width), zeros past the deconvolution's channels."""
    C = seq[1].conv5.in_channels
    x = _run_convrelu(pk["c0"], xs, padc(C))
    x = seq[1].run(x)
    y4 = _run(pk["up"]["conv"], x)
    B, H, W, _ = y4.shape
    out = _zeros(B, 2 * H, 2 * W, out_width, y4.device)
    ops.depth_to_space2(y4, pk["up"]["cout"], out=out)
    return out


class Encoder(nn.Module):
    """ifrnet.py:55-76."""

    def __init__(self, channels, large=False):
        super().__init__()
        self.channels = channels
        prev_ch = 3
        for idx, ch in enumerate(channels, 1):
            k = 7 if large and idx == 1 else 3
            p = 3 if k == 7 else 1
            self.register_module(f"pyramid{idx}", nn.Sequential(convrelu(prev_ch, ch, k, 2, p), convrelu(ch, ch, 3, 1, 1)))
            prev_ch = ch

    def pack(self, dtype, device):
        self._pk, prev = [], 3
        for idx, ch in enumerate(self.channels, 1):
            pyr = getattr(self, f"pyramid{idx}")
            self._pk.append((_pack_convrelu(pyr[0], [_seg(prev)], device), _pack_convrelu(pyr[1], [_seg(ch)], device)))
            prev = ch

    def run(self, x):
        fs = []
        for a, b in self._pk:
            x = _run_convrelu(b, _run_convrelu(a, x))
            fs.append(x)
        return fs


class InitDecoder(nn.Module):
    """ifrnet.py:78-92."""

    def __init__(self, in_ch, out_ch, skip_ch):
        super().__init__()
        self.convblock = nn.Sequential(convrelu(in_ch * 2 + 1, in_ch * 2), ResBlock(in_ch * 2, skip_ch),
                                       nn.ConvTranspose2d(in_ch * 2, out_ch + 4, 4, 2, 1, bias=True))
        self.in_ch, self.out_ch = in_ch, out_ch

    def pack(self, dtype, device):
        c = self.in_ch
        self._pk = dict(c0=_pack_convrelu(self.convblock[0], [_seg(c), _seg(c), _seg(1)], device),
                        up=_pack_deconv(self.convblock[2], device))

    def run(self, f0, f1, embt):
        return _run_convblock(self.convblock, self._pk, [f0, f1, embt], 4 + padc(self.out_ch))


class IntermediateDecoder(nn.Module):
    """ifrnet.py:94-111."""

    def __init__(self, in_ch, out_ch, skip_ch):
        super().__init__()
        self.convblock = nn.Sequential(convrelu(in_ch * 3 + 4, in_ch * 3), ResBlock(in_ch * 3, skip_ch),
                                       nn.ConvTranspose2d(in_ch * 3, out_ch + 4, 4, 2, 1, bias=True))
        self.in_ch, self.out_width = in_ch, 4 + padc(out_ch)

    def pack(self, dtype, device):
        c = self.in_ch
        self._pk = dict(c0=_pack_convrelu(self.convblock[0], [_seg(c), _seg(c), _seg(c), _seg(4)], device),
                        up=_pack_deconv(self.convblock[2], device))

    def run(self, ft, f0, f1, flow):
        """ft: (B, H, W, padc(in_ch)) view; f0, f1: encoder features; flow: (B, H, W, 16) flow0 | flow1 | zeros."""
        c = self.in_ch
        B, H, W, _ = flow.shape
        w0, w1 = _zeros(B, H, W, padc(c), flow.device), _zeros(B, H, W, padc(c), flow.device)
        ops.flow_warp(f0[..., :c], flow[..., 0:2], border=True, out=w0[..., :c])
        ops.flow_warp(f1[..., :c], flow[..., 2:4], border=True, out=w1[..., :c])
        return _run_convblock(self.convblock, self._pk, [ft, w0, w1, flow], self.out_width)


class MultiFlowDecoder(IntermediateDecoder):
    """multi_flow.py:58-85 (its arithmetic behind the convblock is flair_amt_multiflow_prepare)."""

    def __init__(self, in_ch, skip_ch, num_flows=3):
        nn.Module.__init__(self)
        self.num_flows = num_flows
        self.convblock = nn.Sequential(convrelu(in_ch * 3 + 4, in_ch * 3), ResBlock(in_ch * 3, skip_ch),
                                       nn.ConvTranspose2d(in_ch * 3, 8 * num_flows, 4, 2, 1, bias=True))
        self.in_ch, self.out_width = in_ch, 8 * num_flows


class BasicUpdateBlock(nn.Module):
    """raft.py:88-139."""

    def __init__(self, cdim, hidden_dim, flow_dim, corr_dim, corr_dim2, fc_dim, corr_levels=4, radius=3, scale_factor=None,
                 out_num=1):
        super().__init__()
        cor_planes = corr_levels * (2 * radius + 1) ** 2
        self.scale_factor = scale_factor
        self.cdim, self.cor_planes = cdim, cor_planes
        self.convc1 = nn.Conv2d(2 * cor_planes, corr_dim, 1, padding=0)
        self.convc2 = nn.Conv2d(corr_dim, corr_dim2, 3, padding=1)
        self.convf1 = nn.Conv2d(4, flow_dim * 2, 7, padding=3)
        self.convf2 = nn.Conv2d(flow_dim * 2, flow_dim, 3, padding=1)
        self.conv = nn.Conv2d(flow_dim + corr_dim2, fc_dim, 3, padding=1)
        self.gru = nn.Sequential(nn.Conv2d(fc_dim + 4 + cdim, hidden_dim, 3, padding=1), nn.LeakyReLU(negative_slope=0.1, inplace=True),
                                 nn.Conv2d(hidden_dim, hidden_dim, 3, padding=1))
        self.feat_head = nn.Sequential(nn.Conv2d(hidden_dim, hidden_dim, 3, padding=1), nn.LeakyReLU(negative_slope=0.1, inplace=True),
                                       nn.Conv2d(hidden_dim, cdim, 3, padding=1))
        self.flow_head = nn.Sequential(nn.Conv2d(hidden_dim, hidden_dim, 3, padding=1), nn.LeakyReLU(negative_slope=0.1, inplace=True),
                                       nn.Conv2d(hidden_dim, 4 * out_num, 3, padding=1))
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)

    def pack(self, dtype, device):
        one = lambda conv: _pack(conv, [_seg(conv.in_channels)], device)     # noqa: E731
        self._pk = dict(c1=one(self.convc1), c2=one(self.convc2), f1=one(self.convf1), f2=one(self.convf2),
                        c=_pack(self.conv, [_seg(self.convc2.out_channels), _seg(self.convf2.out_channels)], device),
                        g0=_pack(self.gru[0], [_seg(self.conv.out_channels), _seg(4), _seg(self.cdim)], device),
                        g2=one(self.gru[2]), h0=one(self.feat_head[0]), h2=one(self.feat_head[2]),
                        w0=one(self.flow_head[0]), w2=one(self.flow_head[2]))

    def deltas(self, net_in, flow, corr, res_net=None, res_flow=None):
        """net_in (B, h, w, padc(cdim)), flow (B, h, w, 16), corr (B, h, w, padc(392)) at the block's own size -> delta_net
        (+ res_net) as (B, h, w, padc(cdim)) and delta_flow (+ res_flow) as (B, h, w, 16), zeros in the pad channels."""
        pk, L = self._pk, A.ACT_LRELU01
        B, h, w, _ = flow.shape
        dev = flow.device
        cor = _run(pk["c2"], _run(pk["c1"], corr, L), L)
        flo = _run(pk["f2"], _run(pk["f1"], flow, L), L)
        inp = _zeros(B, h, w, padc(pk["c"]["cout"]), dev)
        _run(pk["c"], [cor, flo], L, out=inp)
        out = _run(pk["g2"], _run(pk["g0"], [inp, flow, net_in], L))
        d_net = _zeros(B, h, w, padc(self.cdim), dev)
        _run(pk["h2"], _run(pk["h0"], out, L), out=d_net, res0=res_net)
        d_flow = _zeros(B, h, w, K, dev)
        _run(pk["w2"], _run(pk["w0"], out, L), out=d_flow, res0=res_flow)
        return d_net, d_flow


class ResidualBlock(nn.Module):
    """feat_enc.py:64-114 with norm_fn='instance'."""

    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        if norm_fn != "instance":
            raise ValueError("flair_amd's AMT feature encoder runs norm_fn='instance' (what AMT-G builds)")
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = nn.InstanceNorm2d(planes)
        self.norm2 = nn.InstanceNorm2d(planes)
        if not stride == 1:
            self.norm3 = nn.InstanceNorm2d(planes)
        self.downsample = None if stride == 1 else nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def pack(self, dtype, device):
        one = lambda conv: _pack(conv, [_seg(conv.in_channels)], device)     # noqa: E731
        self._pk = dict(c1=one(self.conv1), c2=one(self.conv2), d=one(self.downsample[0]) if self.downsample is not None else None)

    def run(self, x, inorm):
        y = inorm(_run(self._pk["c1"], x), A.ACT_RELU)
        y = inorm(_run(self._pk["c2"], y), A.ACT_RELU)
        if self.downsample is not None:
            x = inorm(_run(self._pk["d"], x), A.ACT_NONE)
        return ops.add_act(x, y, A.ACT_RELU)


class LargeEncoder(nn.Module):
    """feat_enc.py:267-343."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__()
        if norm_fn != "instance":
            raise ValueError("flair_amd's AMT feature encoder runs norm_fn='instance' (what AMT-G builds)")
        self.norm_fn = norm_fn
        self.norm1 = nn.InstanceNorm2d(64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 64
        self.layer1 = self._make_layer(64, stride=1)
        self.layer2 = self._make_layer(112, stride=2)
        self.layer3 = self._make_layer(160, stride=2)
        self.layer3_2 = self._make_layer(160, stride=1)
        self.conv2 = nn.Conv2d(self.in_planes, output_dim, kernel_size=1)
        self.dropout = None

    def _make_layer(self, dim, stride=1):
        layers = (ResidualBlock(self.in_planes, dim, self.norm_fn, stride=stride), ResidualBlock(dim, dim, self.norm_fn, stride=1))
        self.in_planes = dim
        return nn.Sequential(*layers)

    def pack(self, dtype, device):
        self._pk = dict(c1=_pack(self.conv1, [_seg(3)], device), c2=_pack(self.conv2, [_seg(self.conv2.in_channels)], device))

    @staticmethod
    def _inorm(x, act):
        """InstanceNorm2d (no affine, eps 1e-5) + activation."""
        return ops.instance_norm(x, act, 1e-5)

    def run(self, x):
        """(N, H, W, 16) images (3 channels + zeros) -> (N, H / 8, W / 8, 128)."""
        x = self._inorm(_run(self._pk["c1"], x), A.ACT_RELU)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer3_2):
            for block in layer:
                x = block.run(x, self._inorm)
        return _run(self._pk["c2"], x)


class AMT(PackedModel, nn.Module):
    """amt.py:44-236 (AMT-G: the defaults)."""

    MULTIPLE = 1            # pads to multiples of 16 itself, centred, like the reference's InputPadder

    def __init__(self, corr_radius=3, corr_lvls=4, num_flows=5, channels=[84, 96, 112, 128], skip_channels=84, pretrained=None):
        super().__init__()
        if corr_radius != 3 or not 1 <= corr_lvls <= 4 or num_flows != 5:
            raise ValueError("flair_amd's AMT kernels are built for corr_radius=3, corr_lvls <= 4 and num_flows=5 (AMT-G)")
        self.radius = corr_radius
        self.corr_levels = corr_lvls
        self.num_flows = num_flows
        self.channels = list(channels)
        self.feat_encoder = LargeEncoder(output_dim=128, norm_fn="instance", dropout=0.0)
        self.encoder = Encoder(channels, large=True)
        self.decoder4 = InitDecoder(channels[3], channels[2], skip_channels)
        self.decoder3 = IntermediateDecoder(channels[2], channels[1], skip_channels)
        self.decoder2 = IntermediateDecoder(channels[1], channels[0], skip_channels)
        self.decoder1 = MultiFlowDecoder(channels[0], skip_channels, num_flows)
        self.update4 = self._get_updateblock(channels[2], None)
        self.update3_low = self._get_updateblock(channels[1], 2.0)
        self.update2_low = self._get_updateblock(channels[0], 4.0)
        self.update3_high = self._get_updateblock(channels[1], None)
        self.update2_high = self._get_updateblock(channels[0], None)
        self.comb_block = nn.Sequential(nn.Conv2d(3 * self.num_flows, 6 * self.num_flows, 7, 1, 3), nn.PReLU(6 * self.num_flows),
                                        nn.Conv2d(6 * self.num_flows, 3, 7, 1, 3))
        self._reference_schedule = False        # True: the per-pair work is repeated per timestep, as amt.py:113-135 does
        if pretrained is not None:
            self.load_state_dict(torch.load(pretrained, map_location="cpu")["state_dict"])

    def _get_updateblock(self, cdim, scale_factor=None):
        return BasicUpdateBlock(cdim=cdim, hidden_dim=192, flow_dim=64, corr_dim=256, corr_dim2=192, fc_dim=188,
                                scale_factor=scale_factor, corr_levels=self.corr_levels, radius=self.radius)

    def convert_to_bf16(self):
        raise ValueError("AMT runs in float32 only: its 84 / 252 / 257 / 292 / 340-channel inputs against the 32-channel bf16 K "
                         "step and a bf16 correlation volume are not built")

    def pack(self, dtype, device):
        if dtype != FP:
            raise ValueError("AMT runs in float32 only")
        n = self.num_flows
        wm = torch.zeros(8, 8, dtype=FP)
        wm[:6, :6] = -1.0 / 6.0                  # (per-channel means of i0 | i1) -> minus the pair's mean in columns 0 .. 5
        self._pk = dict(comb0=_pack(self.comb_block[0], [_seg(3 * n)], device), slope=_slope(self.comb_block[1], device),
                        comb2=_pack(self.comb_block[2], [_seg(6 * n)], device), wm=wm.to(device),
                        half=torch.full((4,), 0.5, dtype=FP, device=device), two=torch.full((4,), 2.0, dtype=FP, device=device))

    # ------------------------------------------------------------------------------------------------ checks
    def _check(self, frame0, frame1, factor):
        if not (isinstance(frame0, torch.Tensor) and isinstance(frame1, torch.Tensor)) or frame0.dim() != 4 or frame0.shape[1] != 3:
            raise ValueError("AMT takes two (B, 3, H, W) frame tensors")
        if tuple(frame0.shape) != tuple(frame1.shape):
            raise ValueError(f"AMT: frame0 is {tuple(frame0.shape)} and frame1 is {tuple(frame1.shape)}")
        if frame0.shape[0] < 1:
            raise ValueError("AMT: an empty batch")
        H, W = frame0.shape[2:]
        if not H or not W or not supported_size(H, W)[0]:
            raise ValueError(size_error(H, W))
        if isinstance(factor, bool) or int(factor) != factor or factor < 2:
            raise ValueError(f"AMT: factor={factor!r}; an integer >= 2 (factor - 1 frames are made per pair)")
        if self.dtype != FP:
            raise ValueError("AMT runs in float32 only")
        if not (frame0.is_cuda and frame1.is_cuda) or frame0.device != frame1.device:
            raise ValueError("flair_amd AMT needs both frames in HBM on one device (device='cuda'); no CPU path exists")

    # ------------------------------------------------------------------------------------------------ per pair
    def _pair(self, f0, f1, scale):
        """amt.py:114-135 on the padded frames (B, 3, H, W) in [-1, 1]."""
        B, _, H, W = f0.shape
        dev = f0.device
        pair = _zeros(B, H, W, 8, dev)
        ops.nchw_to_clip(f0, pair, 0)
        ops.nchw_to_clip(f1, pair, 3)
        ops.affine_channels(pair, 6, 0.5, 0.5, float("-inf"), float("inf"), None, None, pair)      # (frame + 1) / 2
        neg_mean = ops.matmul(ops.global_avgpool(pair), self._pk["wm"])[0]                            # (B, 8)
        ops.add_frame_bias(pair, neg_mean)                                                          # img - mean_
        x = _zeros(2 * B, H, W, K, dev)
        ops.cast_channels(pair[..., 0:3], x[:B], 0)
        ops.cast_channels(pair[..., 3:6], x[B:], 0)
        if scale != 1:
            x = ops.resize(x, (scale * H, scale * W), ops.RESIZE_BILINEAR)
        fmap = self.feat_encoder.run(x)                                                             # (2B, h, w, 128)
        _, h, w, D = fmap.shape
        planar = ops.clip_to_nchw(fmap, D)
        pyr, pyr_t = [ops.corr_volume(fmap[:B], planar[B:])], [ops.corr_volume(fmap[B:], planar[:B])]
        for _ in range(self.corr_levels - 1):
            pyr.append(ops.corr_pool(pyr[-1]))
            pyr_t.append(ops.corr_pool(pyr_t[-1]))
        feats = self.encoder.run(x)
        return dict(pair=pair, neg_mean=neg_mean, fmap=fmap, pyr=pyr, pyr_t=pyr_t, grid=(h, w),
                    f0=[f[:B] for f in feats], f1=[f[B:] for f in feats], scale=scale)

    # ------------------------------------------------------------------------------------------------ per timestep
    def _lookup(self, st, flow, t, downsample):
        """AMT._corr_scale_lookup: -> corr (B, h, w, padc(392)) and the flow at the lookup grid (B, h, w, 16)."""
        h, w = st["grid"]
        B = flow.shape[0]
        if downsample != 1:
            low = ops.resize(flow, (h, w), ops.RESIZE_BILINEAR)
            flow = ops.axpby_nhwc(low, 1.0 / downsample, out=low)
        corr = _zeros(B, h, w, padc(2 * ops.CORR_TAPS * self.corr_levels), flow.device)
        one = torch.ones((), dtype=FP)
        tt = torch.tensor(t, dtype=FP)
        ops.corr_lookup(st["pyr"], st["pyr_t"], flow, float(one / tt), float(one / (one - tt)), corr)
        return corr, flow

    def _update(self, block, ft, c, flow, corr, flow_at_grid):
        """One update block with the residual additions around it.  ft: (B, H, W, >= padc(c)) view, flow: (B, H, W, 16) at
        the decoder's size; corr and flow_at_grid at the block's size (the same for scale_factor None)."""
        s = block.scale_factor
        if s is None:
            return block.deltas(ft, flow, corr, res_net=ft[..., :c], res_flow=flow[..., :4])
        B, H, W, _ = flow.shape
        h, w = flow_at_grid.shape[1:3]
        net = ops.resize(ft, (h, w), ops.RESIZE_BILINEAR, channels=c)
        d_net, d_flow = block.deltas(net, flow_at_grid, corr)
        up_net = ops.resize(d_net, (H, W), ops.RESIZE_BILINEAR)
        new_ft = _zeros(B, H, W, padc(c), flow.device)
        ops.add_act(ft[..., :c], up_net[..., :c], A.ACT_NONE, out=new_ft[..., :c])
        up_flow = ops.resize(d_flow, (H, W), ops.RESIZE_BILINEAR)
        return new_ft, ops.axpby_nhwc(flow, 1.0, up_flow, float(s), out=up_flow)

    @staticmethod
    def _sum4(dec, up):
        """flow + 2.0 * resize(flow_in, 2.0) (ifrnet.py:109-110): dec's channels 0 .. 3 plus twice the enlarged flow."""
        out = torch.zeros_like(up)
        ops.axpby_nhwc(dec[..., :4], 1.0, up[..., :4], 2.0, out=out[..., :4])
        return out

    def _timestep(self, st, t, rec=None):
        """amt.py:137-216 -> (B, H, W, 4) the prediction before the clamp (channel 3 is zero)."""
        c3, c2, c1 = self.channels[2], self.channels[1], self.channels[0]
        (f0_1, f0_2, f0_3, f0_4), (f1_1, f1_2, f1_3, f1_4) = st["f0"], st["f1"]
        keep = (lambda name, x, c, off=0: rec.__setitem__(name, ops.clip_to_nchw(x, c, off))) if rec is not None else (lambda *a: None)
        B, h4, w4, _ = f0_4.shape
        embt = _zeros(B, h4, w4, K, f0_4.device)
        embt[..., 0] = t
        dec = self.decoder4.run(f0_4, f1_4, embt)
        flow, ft = _zeros(*dec.shape[:3], K, dec.device), dec[..., 4:]
        ops.axpby_nhwc(dec[..., :4], 1.0, out=flow[..., :4])
        keep("flow_dec4", flow, 4)
        corr, _ = self._lookup(st, flow, t, 1)
        keep("lookup4", corr, 98 * self.corr_levels)
        ft, flow = self._update(self.update4, ft, c3, flow, corr, flow)
        keep("flow4", flow, 4)

        dec = self.decoder3.run(ft[..., :padc(c3)], f0_3, f1_3, flow)
        flow, ft = self._sum4(dec, ops.resize(flow, dec.shape[1:3], ops.RESIZE_BILINEAR)), dec[..., 4:]
        keep("flow_dec3", flow, 4)
        corr, low = self._lookup(st, flow, t, 2)
        keep("lookup3", corr, 98 * self.corr_levels)
        ft, flow = self._update(self.update3_low, ft, c2, flow, corr, low)
        corr = ops.resize(corr, flow.shape[1:3], ops.RESIZE_BILINEAR)
        ft, flow = self._update(self.update3_high, ft, c2, flow, corr, flow)
        keep("flow3", flow, 4)

        dec = self.decoder2.run(ft[..., :padc(c2)], f0_2, f1_2, flow)
        flow, ft = self._sum4(dec, ops.resize(flow, dec.shape[1:3], ops.RESIZE_BILINEAR)), dec[..., 4:]
        keep("flow_dec2", flow, 4)
        corr, low = self._lookup(st, flow, t, 4)
        keep("lookup2", corr, 98 * self.corr_levels)
        ft, flow = self._update(self.update2_low, ft, c1, flow, corr, low)
        corr = ops.resize(corr, flow.shape[1:3], ops.RESIZE_BILINEAR)
        ft, flow = self._update(self.update2_high, ft, c1, flow, corr, flow)
        keep("flow2", flow, 4)

        dec = self.decoder1.run(ft[..., :padc(c1)], f0_1, f1_1, flow)
        prep = ops.amt_multiflow_prepare(dec, ops.resize(flow, dec.shape[1:3], ops.RESIZE_BILINEAR))
        if st["scale"] != 1:
            s = st["scale"]
            prep = ops.resize(prep, (dec.shape[1] // s, dec.shape[2] // s), ops.RESIZE_BILINEAR)
            ops.axpby_nhwc(prep[..., :20], 1.0 / s, out=prep[..., :20])
        keep("flow1", prep, 20)
        keep("mask", prep, 5, 20)
        x, avg = ops.amt_multiflow_combine(st["pair"], prep, st["neg_mean"])
        y = _run(self._pk["comb0"], x)
        ops.prelu(y, self._pk["slope"], out=y)
        return _run(self._pk["comb2"], y, res0=avg)

    @torch.no_grad()
    def forward(self, frame0, frame1, factor, detail=None):
        """frame0, frame1: (B, 3, H, W) f32 in [-1, 1] -> the factor - 1 frames between them, (B, factor - 1, 3, H, W) f32.
        ``detail``: a list that receives one dict of intermediate NCHW tensors per timestep (tests)."""
        self._check(frame0, frame1, factor)
        factor = int(factor)
        self._ensure_packed(frame0.device)
        B, _, H, W = frame0.shape
        _, (Hp, Wp), scale = supported_size(H, W)
        left, top = (Wp - W) // 2, (Hp - H) // 2
        pad = (left, Wp - W - left, top, Hp - H - top)
        f0 = F.pad(frame0.float(), pad, mode="replicate").contiguous() if (Hp, Wp) != (H, W) else frame0.float().contiguous()
        f1 = F.pad(frame1.float(), pad, mode="replicate").contiguous() if (Hp, Wp) != (H, W) else frame1.float().contiguous()
        out = torch.empty((B, factor - 1, 3, H, W), dtype=FP, device=frame0.device)
        # amt.py:224-228: the reference's f32 timesteps.  For some factors (3, 6, 7 ...) torch.arange counts one step too many
        # and the reference emits an extra frame at t = 1, whose lookup scale is 1 / 0: the first factor - 1 are the frames.
        ts = torch.arange(1 / factor, 1, 1 / factor, dtype=FP).tolist()[:factor - 1]
        recs = [[] for _ in ts]
        # One pair at a time: a pair's frames are the same bits whatever the batch it came in (the convolution kernels pick
        # their tiling, and with it their summation order, from the launch's size), and the two f32 correlation volumes
        # with their pyramids (2 x 85 MiB at 512 x 512) exist for one pair at a time.
        for b in range(B):
            st = None
            for k, t in enumerate(ts):
                if st is None or self._reference_schedule:
                    st = self._pair(f0[b:b + 1], f1[b:b + 1], scale)
                rec = {} if detail is not None else None
                y = self._timestep(st, t, rec)
                ops.affine_channels(y, 3, 1.0, 0.0, 0.0, 1.0, self._pk["half"], self._pk["two"], y)     # clamp(0, 1) * 2 - 1
                out[b, k] = ops.clip_to_nchw(y, 3)[0, :, top:top + H, left:left + W]
                if detail is not None:
                    if k == 0:
                        D = st["fmap"].shape[3]
                        rec.update(fmap0=ops.clip_to_nchw(st["fmap"][:1], D), fmap1=ops.clip_to_nchw(st["fmap"][1:], D),
                                   corr0=st["pyr"][0])
                    recs[k].append(rec)
        if detail is not None:
            detail.extend({name: torch.cat([r[name] for r in per_t], dim=0) for name in per_t[0]} for per_t in recs)
        return out
