"""CPU restatement of AMT-G in plain PyTorch (test infrastructure only).

Written from the formulas of the network (guided_diffusion/amt.py and amt_blocks/ of the reference: a RAFT feature encoder
with instance norms, an IFRNet pyramid encoder with per-channel PReLU, a bidirectional all-pairs correlation pyramid with a
7 x 7 bilinear lookup, three decoders ending in ConvTranspose2d(4, 2, 1), five update blocks, and the multi-flow combine) as
functions over a STATE DICT with the reference's parameter names, so the same weights drive the reference
(tests/golden/make_golden_amt.py), this restatement and the HIP module.  Dtype-generic: in float64 it is the closed form
the GPU tests measure against (the reference itself cannot run in float64: raft.py:199 casts the lookup to float32).  What
depends only on the pair is computed once per pair, as the HIP module does; the values are the reference's.
"""
import torch
import torch.nn.functional as F

from tests.golden.weights import name_seeded_weights

RADIUS, LEVELS, NUM_FLOWS, SKIP = 3, 4, 5, 84


# ------------------------------------------------------------------------------------------------ small pieces
def resize(x, s):
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)


def warp(img, flow):
    """flow_utils.warp: bilinear, border padding, align_corners=True on linspace(-1, 1) + flow / ((size - 1) / 2)."""
    B, _, H, W = flow.shape
    xx = torch.linspace(-1.0, 1.0, W).view(1, 1, 1, W).expand(B, -1, H, -1)
    yy = torch.linspace(-1.0, 1.0, H).view(1, 1, H, 1).expand(B, -1, -1, W)
    grid = torch.cat([xx, yy], 1).to(img)
    flow_ = torch.cat([flow[:, 0:1] / ((W - 1.0) / 2.0), flow[:, 1:2] / ((H - 1.0) / 2.0)], 1)
    return F.grid_sample(img, (grid + flow_).permute(0, 2, 3, 1), mode="bilinear", padding_mode="border", align_corners=True)


def timesteps(factor):
    """The reference's embt values, torch.arange(1 / factor, 1, 1 / factor) in f32 (amt.py:224-228), as a 1-D f32 tensor."""
    return torch.arange(1 / factor, 1, 1 / factor, dtype=torch.float32)


def lookup_scales(t, dtype=torch.float32):
    """t1_scale = 1 / embt and t0_scale = 1 / (1 - embt) (amt.py:101-102) in ``dtype`` from the f32 value t."""
    t = torch.as_tensor(t, dtype=torch.float32).to(dtype)
    return 1.0 / t, 1.0 / (1.0 - t)


def coords_grid(b, h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xs, ys], dim=0).to(dtype)[None].repeat(b, 1, 1, 1)


def conv(sd, name, x, stride=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd[name + ".bias"], stride=stride, padding=(w.shape[2] - 1) // 2)


def convrelu(sd, name, x, stride=1):
    return F.prelu(conv(sd, name + ".0", x, stride), sd[name + ".1.weight"])


def deconv(sd, name, x):
    return F.conv_transpose2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=2, padding=1)


# ------------------------------------------------------------------------------------------------ correlation
def corr_volume(fmap1, fmap2):
    """BidirCorrBlock.corr -> (B, h, w, 1, h, w)."""
    b, d, h, w = fmap1.shape
    corr = torch.bmm(fmap1.view(b, d, h * w).transpose(1, 2), fmap2.view(b, d, h * w)).view(b, h, w, 1, h, w)
    return corr / torch.sqrt(torch.tensor(d).float()).to(fmap1.dtype)


def corr_pyramids(fmap1, fmap2, levels=LEVELS):
    corr = corr_volume(fmap1, fmap2)
    b, h, w = corr.shape[:3]
    corr_t = corr.clone().permute(0, 4, 5, 3, 1, 2).reshape(b * h * w, 1, h, w)
    corr = corr.reshape(b * h * w, 1, h, w)
    pyr, pyr_t = [corr], [corr_t]
    for _ in range(levels - 1):
        corr, corr_t = F.avg_pool2d(corr, 2, stride=2), F.avg_pool2d(corr_t, 2, stride=2)
        pyr.append(corr)
        pyr_t.append(corr_t)
    return pyr, pyr_t


def bilinear_sampler(img, coords):
    H, W = img.shape[-2:]
    xgrid, ygrid = coords.split([1, 1], dim=-1)
    grid = torch.cat([2 * xgrid / (W - 1) - 1, 2 * ygrid / (H - 1) - 1], dim=-1)
    return F.grid_sample(img, grid, align_corners=True)


def corr_lookup(pyr, pyr_t, coords0, coords1, r=RADIUS):
    """BidirCorrBlock.__call__ without its final cast: pyramids of (N, 1, lh, lw) planes, coords (B, 2, h, w) -> two
    (B, levels * 49, h, w) tensors."""
    coords0, coords1 = coords0.permute(0, 2, 3, 1), coords1.permute(0, 2, 3, 1)
    batch, h1, w1, _ = coords0.shape
    d = torch.linspace(-r, r, 2 * r + 1).to(coords0.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out, out_t = [], []
    for i, (corr, corr_t) in enumerate(zip(pyr, pyr_t)):
        c0 = coords0.reshape(batch * h1 * w1, 1, 1, 2) / 2 ** i + delta
        c1 = coords1.reshape(batch * h1 * w1, 1, 1, 2) / 2 ** i + delta
        if corr.shape[-1] <= 1 or corr.shape[-2] <= 1:
            assert corr.shape[-2:] == (1, 1), "the reference raises here"
            corr, corr_t = (v.expand(-1, -1, 2 * r + 1, 2 * r + 1) for v in (corr, corr_t))
        else:
            corr, corr_t = bilinear_sampler(corr, c0), bilinear_sampler(corr_t, c1)
        out.append(corr.reshape(batch, h1, w1, -1))
        out_t.append(corr_t.reshape(batch, h1, w1, -1))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous(), torch.cat(out_t, dim=-1).permute(0, 3, 1, 2).contiguous()


def corr_scale_lookup(pyr, pyr_t, coord, flow0, flow1, t, downsample=1):
    """AMT._corr_scale_lookup -> corr (B, 392, h, w), flow (B, 4, h, w)."""
    t1_scale, t0_scale = lookup_scales(t, flow0.dtype)
    if downsample != 1:
        inv = 1 / downsample
        flow0, flow1 = inv * resize(flow0, inv), inv * resize(flow1, inv)
    corr0, corr1 = corr_lookup(pyr, pyr_t, coord + flow1 * t1_scale, coord + flow0 * t0_scale)
    return torch.cat([corr0, corr1], dim=1), torch.cat([flow0, flow1], dim=1)


# ------------------------------------------------------------------------------------------------ blocks
def residual_block(sd, name, x, stride):
    y = F.relu(F.instance_norm(conv(sd, name + ".conv1", x, stride)))
    y = F.relu(F.instance_norm(conv(sd, name + ".conv2", y)))
    if stride != 1:
        x = F.instance_norm(conv(sd, name + ".downsample.0", x, stride))
    return F.relu(x + y)


def feat_encoder(sd, x, name="feat_encoder"):
    """LargeEncoder(output_dim=128, norm_fn='instance') on (N, 3, H, W) -> (N, 128, H / 8, W / 8)."""
    x = F.relu(F.instance_norm(conv(sd, name + ".conv1", x, 2)))
    for layer, stride in (("layer1", 1), ("layer2", 2), ("layer3", 2), ("layer3_2", 1)):
        x = residual_block(sd, f"{name}.{layer}.0", x, stride)
        x = residual_block(sd, f"{name}.{layer}.1", x, 1)
    return conv(sd, name + ".conv2", x)


def encoder(sd, x, name="encoder"):
    fs = []
    for idx in range(1, 5):
        x = convrelu(sd, f"{name}.pyramid{idx}.1", convrelu(sd, f"{name}.pyramid{idx}.0", x, 2))
        fs.append(x)
    return fs


def res_block(sd, name, x, side=SKIP):
    out = convrelu(sd, name + ".conv1", x)
    out = convrelu(sd, name + ".conv3", torch.cat([out[:, :-side], convrelu(sd, name + ".conv2", out[:, -side:])], 1))
    out = conv(sd, name + ".conv5", torch.cat([out[:, :-side], convrelu(sd, name + ".conv4", out[:, -side:])], 1))
    return F.prelu(x + out, sd[name + ".prelu.weight"])


def convblock(sd, name, x):
    return deconv(sd, name + ".convblock.2", res_block(sd, name + ".convblock.1", convrelu(sd, name + ".convblock.0", x)))


def init_decoder(sd, name, f0, f1, t):
    h, w = f0.shape[2:]
    embt = torch.as_tensor(t, dtype=torch.float32).to(f0.dtype).view(1, 1, 1, 1).expand(f0.shape[0], 1, h, w)
    out = convblock(sd, name, torch.cat([f0, f1, embt], 1))
    return out[:, 0:2], out[:, 2:4], out[:, 4:]


def intermediate_decoder(sd, name, ft_, f0, f1, flow0_in, flow1_in):
    out = convblock(sd, name, torch.cat([ft_, warp(f0, flow0_in), warp(f1, flow1_in), flow0_in, flow1_in], 1))
    return out[:, 0:2] + 2.0 * resize(flow0_in, 2.0), out[:, 2:4] + 2.0 * resize(flow1_in, 2.0), out[:, 4:]


def multi_flow_decoder(sd, name, ft_, f0, f1, flow0, flow1, n=NUM_FLOWS):
    out = convblock(sd, name, torch.cat([ft_, warp(f0, flow0), warp(f1, flow1), flow0, flow1], 1))
    d0, d1, mask, img_res = torch.split(out, [2 * n, 2 * n, n, 3 * n], 1)
    return (d0 + 2.0 * resize(flow0, 2.0).repeat(1, n, 1, 1), d1 + 2.0 * resize(flow1, 2.0).repeat(1, n, 1, 1),
            torch.sigmoid(mask), img_res)


def update_block(sd, name, net, flow, corr, scale_factor=None):
    lrelu = lambda v: F.leaky_relu(v, 0.1)     # noqa: E731
    if scale_factor is not None:
        net = resize(net, 1 / scale_factor)
    cor = lrelu(conv(sd, name + ".convc2", lrelu(conv(sd, name + ".convc1", corr))))
    flo = lrelu(conv(sd, name + ".convf2", lrelu(conv(sd, name + ".convf1", flow))))
    inp = lrelu(conv(sd, name + ".conv", torch.cat([cor, flo], dim=1)))
    out = conv(sd, name + ".gru.2", lrelu(conv(sd, name + ".gru.0", torch.cat([inp, flow, net], dim=1))))
    delta_net = conv(sd, name + ".feat_head.2", lrelu(conv(sd, name + ".feat_head.0", out)))
    delta_flow = conv(sd, name + ".flow_head.2", lrelu(conv(sd, name + ".flow_head.0", out)))
    if scale_factor is not None:
        delta_net = resize(delta_net, scale_factor)
        delta_flow = scale_factor * resize(delta_flow, scale_factor)
    return delta_net, delta_flow


def multi_flow_combine(sd, img0, img1, flow0, flow1, mask, img_res, mean, n=NUM_FLOWS):
    b, _, h, w = flow0.shape
    flow0, flow1 = flow0.reshape(b * n, 2, h, w), flow1.reshape(b * n, 2, h, w)
    mask, img_res = mask.reshape(b * n, 1, h, w), img_res.reshape(b * n, 3, h, w)
    img0 = torch.stack([img0] * n, 1).reshape(-1, 3, h, w)
    img1 = torch.stack([img1] * n, 1).reshape(-1, 3, h, w)
    mean = torch.stack([mean] * n, 1).reshape(-1, 1, 1, 1)
    img_warps = (mask * warp(img0, flow0) + (1 - mask) * warp(img1, flow1) + mean + img_res).reshape(b, n, 3, h, w)
    x = img_warps.view(b, -1, h, w)
    comb = conv(sd, "comb_block.2", F.prelu(conv(sd, "comb_block.0", x), sd["comb_block.1.weight"]))
    return img_warps.mean(1) + comb


# ------------------------------------------------------------------------------------------------ the network
def pad_amounts(h, w, divisor=16):
    """InputPadder: (left, right, top, bottom) of the centred replicate padding."""
    ph = (((h // divisor) + 1) * divisor - h) % divisor
    pw = (((w // divisor) + 1) * divisor - w) % divisor
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def supported(h, w):
    """The sizes the reference runs (raft.py:186-191): with g the 1/8 grid of the padded (and, for padded width <= 64,
    doubled) frame, the coarsest pyramid level g // 8 is >= 2 on both sides or exactly 1 x 1."""
    l, r, t, b = pad_amounts(h, w)
    H, W = h + t + b, w + l + r
    s = 2 if W <= 64 else 1
    gh, gw = s * H // 8 // 8, s * W // 8 // 8
    return (gh >= 2 and gw >= 2) or (gh == 1 and gw == 1)


def pair_state(sd, img0, img1, scale_factor):
    """What depends only on the pair (amt.py:114-135): mean, the mean-free images, both encoder pyramids, the correlation
    pyramids and the coordinate grid."""
    mean_ = torch.cat([img0, img1], 2).mean(1, keepdim=True).mean(2, keepdim=True).mean(3, keepdim=True)
    img0, img1 = img0 - mean_, img1 - mean_
    img0_ = resize(img0, scale_factor) if scale_factor != 1.0 else img0
    img1_ = resize(img1, scale_factor) if scale_factor != 1.0 else img1
    b, _, h, w = img0_.shape
    fmap = feat_encoder(sd, torch.cat([img0_, img1_], dim=0))
    fmap0, fmap1 = fmap[:b], fmap[b:]
    pyr, pyr_t = corr_pyramids(fmap0, fmap1)
    return dict(mean=mean_, img0=img0, img1=img1, fmap0=fmap0, fmap1=fmap1, pyr=pyr, pyr_t=pyr_t,
                coord=coords_grid(b, h // 8, w // 8, img0.dtype), f0=encoder(sd, img0_), f1=encoder(sd, img1_),
                scale_factor=scale_factor)


def timestep(sd, st, t, detail=None):
    """AMT._forward after the per-pair part -> the frame in [0, 1] (before the clamp's companion crop).  ``detail``: a dict
    that receives the three lookups, the flows after each decoder / update and the mask."""
    pyr, pyr_t, coord, sf = st["pyr"], st["pyr_t"], st["coord"], st["scale_factor"]
    (f0_1, f0_2, f0_3, f0_4), (f1_1, f1_2, f1_3, f1_4) = st["f0"], st["f1"]
    rec = detail if detail is not None else {}
    up0_4, up1_4, ft_3 = init_decoder(sd, "decoder4", f0_4, f1_4, t)
    rec["flow_dec4"] = torch.cat([up0_4, up1_4], 1)
    zero = torch.zeros_like(up0_4)
    rec["floor"] = lookup_outside_share(st, zero, zero, t, 1)
    rec["outside"] = [lookup_outside_share(st, up0_4, up1_4, t, 1)]
    rec["outside0"] = [lookup_outside_share(st, up0_4, up1_4, t, 1, [0])]
    corr_4, flow_4 = corr_scale_lookup(pyr, pyr_t, coord, up0_4, up1_4, t, 1)
    rec["lookup4"] = corr_4
    d_ft, d_fl = update_block(sd, "update4", ft_3, flow_4, corr_4)
    up0_4, up1_4, ft_3 = up0_4 + d_fl[:, 0:2], up1_4 + d_fl[:, 2:4], ft_3 + d_ft
    rec["flow4"] = torch.cat([up0_4, up1_4], 1)

    up0_3, up1_3, ft_2 = intermediate_decoder(sd, "decoder3", ft_3, f0_3, f1_3, up0_4, up1_4)
    rec["flow_dec3"] = torch.cat([up0_3, up1_3], 1)
    rec["outside"].append(lookup_outside_share(st, up0_3, up1_3, t, 2))
    rec["outside0"].append(lookup_outside_share(st, up0_3, up1_3, t, 2, [0]))
    corr_3, flow_3 = corr_scale_lookup(pyr, pyr_t, coord, up0_3, up1_3, t, 2)
    rec["lookup3"] = corr_3
    d_ft, d_fl = update_block(sd, "update3_low", ft_2, flow_3, corr_3, 2.0)
    up0_3, up1_3, ft_2 = up0_3 + d_fl[:, 0:2], up1_3 + d_fl[:, 2:4], ft_2 + d_ft
    d_ft, d_fl = update_block(sd, "update3_high", ft_2, torch.cat([up0_3, up1_3], 1), resize(corr_3, 2.0))
    up0_3, up1_3, ft_2 = up0_3 + d_fl[:, 0:2], up1_3 + d_fl[:, 2:4], ft_2 + d_ft
    rec["flow3"] = torch.cat([up0_3, up1_3], 1)

    up0_2, up1_2, ft_1 = intermediate_decoder(sd, "decoder2", ft_2, f0_2, f1_2, up0_3, up1_3)
    rec["flow_dec2"] = torch.cat([up0_2, up1_2], 1)
    rec["outside"].append(lookup_outside_share(st, up0_2, up1_2, t, 4))
    rec["outside0"].append(lookup_outside_share(st, up0_2, up1_2, t, 4, [0]))
    corr_2, flow_2 = corr_scale_lookup(pyr, pyr_t, coord, up0_2, up1_2, t, 4)
    rec["lookup2"] = corr_2
    d_ft, d_fl = update_block(sd, "update2_low", ft_1, flow_2, corr_2, 4.0)
    up0_2, up1_2, ft_1 = up0_2 + d_fl[:, 0:2], up1_2 + d_fl[:, 2:4], ft_1 + d_ft
    d_ft, d_fl = update_block(sd, "update2_high", ft_1, torch.cat([up0_2, up1_2], 1), resize(corr_2, 4.0))
    up0_2, up1_2, ft_1 = up0_2 + d_fl[:, 0:2], up1_2 + d_fl[:, 2:4], ft_1 + d_ft
    rec["flow2"] = torch.cat([up0_2, up1_2], 1)

    up0_1, up1_1, mask, img_res = multi_flow_decoder(sd, "decoder1", ft_1, f0_1, f1_1, up0_2, up1_2)
    if sf != 1.0:
        up0_1, up1_1 = resize(up0_1, 1.0 / sf) * (1.0 / sf), resize(up1_1, 1.0 / sf) * (1.0 / sf)
        mask, img_res = resize(mask, 1.0 / sf), resize(img_res, 1.0 / sf)
    rec["flow1"] = torch.cat([up0_1, up1_1], 1)
    rec["mask"] = mask
    pred = multi_flow_combine(sd, st["img0"], st["img1"], up0_1, up1_1, mask, img_res, st["mean"])
    return torch.clamp(pred, 0, 1)


@torch.no_grad()
def amt_forward(sd, frame0, frame1, factor, detail=None):
    """AMT.forward: frames (B, 3, H, W) in [-1, 1] -> (B, factor - 1, 3, H, W).  ``detail``: a list that receives one dict
    per timestep (see ``timestep``) plus, in its first dict, the two feature maps and the level-0 volume."""
    i0, i1 = (frame0 + 1) / 2, (frame1 + 1) / 2
    h, w = i0.shape[-2:]
    pad = pad_amounts(h, w)
    i0, i1 = F.pad(i0, pad, mode="replicate"), F.pad(i1, pad, mode="replicate")
    st = pair_state(sd, i0, i1, 2.0 if i0.shape[-1] <= 64 else 1.0)
    frames = []
    for k, t in enumerate(timesteps(factor)):
        rec = {} if detail is not None else None
        pred = timestep(sd, st, t, rec)
        if detail is not None:
            if k == 0:
                rec.update(fmap0=st["fmap0"], fmap1=st["fmap1"], corr0=st["pyr"][0])
            detail.append(rec)
        frames.append(pred[..., pad[2]:pred.shape[-2] - pad[3], pad[0]:pred.shape[-1] - pad[1]])
    return torch.stack(frames, dim=1) * 2 - 1


# ------------------------------------------------------------------------------------------------ weights and inputs
# Name-seeded weights alone give final flows of 20 .. 60 px (nearly every lookup sample and warp leaves the frame) and a
# mask that stays near 1/2: the flow channels of the transposed convolution that ends each decoder and the last convolution
# of every flow_head are scaled down, the mask channels of decoder1 up.  The fixture stores the factors.
SCALES = dict(flow=0.15, head=0.1, mask=1.5)
DECODERS = ("decoder4", "decoder3", "decoder2", "decoder1")
UPDATES = ("update4", "update3_low", "update2_low", "update3_high", "update2_high")


def seeded_state_dict(net, scales=None):
    """Name-seeded weights of ``net`` (the reference module or ours) as a CPU f32 state dict, scaled as SCALES says."""
    sc = dict(SCALES, **(scales or {}))
    sd = {k: v.detach().float().cpu().clone() for k, v in name_seeded_weights(net).state_dict().items()}
    n = NUM_FLOWS
    for d in DECODERS:
        w, b = sd[f"{d}.convblock.2.weight"], sd[f"{d}.convblock.2.bias"]       # (Cin, Cout, 4, 4), (Cout,)
        nf = 4 * n if d == "decoder1" else 4
        w[:, :nf] *= sc["flow"]
        b[:nf] *= sc["flow"]
        if d == "decoder1":
            w[:, 4 * n:5 * n] *= sc["mask"]
            b[4 * n:5 * n] *= sc["mask"]
    for u in UPDATES:
        sd[f"{u}.flow_head.2.weight"] *= sc["head"]
        sd[f"{u}.flow_head.2.bias"] *= sc["head"]
    return sd


def lookup_outside_share(st, flow0, flow1, t, downsample, levels=None):
    """Share of the lookup's bilinear corner samples (both directions, the sampled levels among ``levels`` (default: all),
    49 taps, 4 corners) that fall outside their plane, for the flows at the decoder's size."""
    t1, t0 = lookup_scales(t, flow0.dtype)
    if downsample != 1:
        inv = 1 / downsample
        flow0, flow1 = inv * resize(flow0, inv), inv * resize(flow1, inv)
    d = torch.arange(-RADIUS, RADIUS + 1, dtype=flow0.dtype)
    n = hit = 0
    for c in (st["coord"] + flow1 * t1, st["coord"] + flow0 * t0):
        for i, plane in enumerate(st["pyr"]):
            H, W = plane.shape[-2:]
            if (H, W) == (1, 1) or (levels is not None and i not in levels):
                continue
            x0 = (c[:, 0, :, :, None] / 2 ** i + d).floor()
            y0 = (c[:, 1, :, :, None] / 2 ** i + d).floor()
            ox = ((x0 < 0) | (x0 > W - 1)).float() + ((x0 + 1 < 0) | (x0 + 1 > W - 1)).float()        # of 2 columns
            oy = ((y0 < 0) | (y0 > H - 1)).float() + ((y0 + 1 < 0) | (y0 + 1 > H - 1)).float()
            inside = (2 - ox)[..., :, None] * (2 - oy)[..., None, :]                                  # corners inside, of 4
            n += inside.numel() * 4
            hit += float((4 - inside).sum())
    return hit / n


CASES = {"s32": dict(B=1, H=32, W=32, factor=2, seed=181),          # x2 scale path, 8 x 8 grid, coarsest level 1 x 1
         "s64": dict(B=1, H=64, W=64, factor=2, seed=182),          # x2 scale path, 16 x 16 grid, coarsest level 2 x 2
         "rect": dict(B=2, H=120, W=140, factor=4, seed=183)}       # padded to 128 x 144 (centred), 16 x 18 grid, floored 4 x 4


def input_u8(case):
    """(2, B, 3, H, W) uint8: frame0 a seeded smooth image, frame1 a copy of it shifted by (3, -2) pixels with noise."""
    c = CASES[case]
    g = torch.Generator().manual_seed(c["seed"])
    low = 0.25 + 0.5 * torch.rand(c["B"], 3, c["H"] // 16 + 3, c["W"] // 16 + 3, generator=g)
    big = F.interpolate(low, scale_factor=16, mode="bicubic", align_corners=False).clamp(0, 1)
    f0 = big[:, :, 16:16 + c["H"], 16:16 + c["W"]]
    f1 = big[:, :, 13:13 + c["H"], 18:18 + c["W"]] + 0.02 * torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    return torch.stack([f0, f1.clamp(0, 1)]).mul(255).round().to(torch.uint8)


def frames(u8):
    x = torch.as_tensor(u8).float() / 127.5 - 1.0
    return x[0].contiguous(), x[1].contiguous()


# ------------------------------------------------------------------------------------------------ what the fixture keeps
QUANTITIES = ("fmap0", "fmap1", "corr0", "lookup4", "lookup3", "lookup2", "flow_dec4", "flow4", "flow_dec3", "flow3",
              "flow_dec2", "flow2", "flow1", "mask", "out")
BLOCK_CASE = "s32"                           # the case whose decoder4 / update4 inputs and outputs are stored in full
BLOCK_INPUTS = ("blk_f0_4", "blk_f1_4", "blk_net", "blk_flow", "blk_corr")
GRID_PIXELS, LOOKUP_PIXELS, OUT_PIXELS = 16, 8, 64
STRIDE = dict(flow_dec3=2, flow3=2, flow_dec2=4, flow2=4, flow1=8, mask=8)


def grid_size(case):
    """(h, w) of the lookup grid: 1/8 of the padded (and, up to 64 wide, doubled) frame."""
    c = CASES[case]
    l, r, t, b = pad_amounts(c["H"], c["W"])
    H, W = c["H"] + t + b, c["W"] + l + r
    s = 2 if W <= 64 else 1
    return s * H // 8, s * W // 8


def sample_pixels(case, hw, n, salt):
    """n seeded flat positions into an h x w grid per frame of the batch, sorted: (B, n) int64."""
    c = CASES[case]
    g = torch.Generator().manual_seed(c["seed"] + salt)
    return torch.stack([torch.randperm(hw[0] * hw[1], generator=g)[:n].sort()[0] for _ in range(c["B"])])


def gather_pixels(t, pix):
    """(B, ..., H, W), (B, K) flat positions -> (B, ..., K)."""
    return torch.stack([t[b].flatten(-2)[..., pix[b]] for b in range(t.shape[0])])


def stored(case, name, t):
    """What the fixture keeps of quantity ``name`` (the first timestep's, except ``out``): feature maps and lookups at
    seeded pixels of the lookup grid, the level-0 volume as the whole planes of LOOKUP_PIXELS queries, the coarse flows in
    full and the finer ones on a strided grid, the output in full or (case rect) on a 4-strided grid plus OUT_PIXELS seeded
    pixels per frame, concatenated."""
    B = CASES[case]["B"]
    hw = grid_size(case)
    pix = sample_pixels(case, hw, GRID_PIXELS, 1000)
    if name in ("fmap0", "fmap1"):
        return gather_pixels(t, pix)
    if name.startswith("lookup"):
        return gather_pixels(t, pix[:, :LOOKUP_PIXELS])
    if name == "corr0":                          # (B h w, h, w) planes (a leading singleton channel axis is dropped)
        t = t.reshape(B, hw[0] * hw[1], *hw)
        return torch.stack([t[b, pix[b, :LOOKUP_PIXELS]] for b in range(B)])
    if name in STRIDE:
        return t[..., ::STRIDE[name], ::STRIDE[name]].contiguous()
    if name == "out" and case == "rect":
        c = CASES[case]
        op = sample_pixels(case, (c["H"], c["W"]), OUT_PIXELS, 2000)
        return torch.cat([t[..., ::4, ::4].flatten(-2), gather_pixels(t.flatten(1, 2), op).view(*t.shape[:3], -1)], dim=-1)
    return t
