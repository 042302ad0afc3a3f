"""CPU restatement of SuperSloMo in plain PyTorch (test infrastructure only).

Written from the formulas of the network (two UNets of plain convolutions with LeakyReLU(0.1), 2x2 average pooling, bilinear
x2 enlargement and skip concatenation; back-warping by ``grid_sample`` with its defaults on x = w + u, gx = 2 (x / W - 0.5);
the time-weighted flow combinations, the visibility-weighted blend and the de-normalisation) as functions over a STATE
DICT with the reference's parameter names, so the same weights drive the reference (tests/golden/make_golden_superslomo.py),
this restatement and the HIP module.  Pinned to g17_superslomo.npz by tests/test_superslomo_cpu.py.  Also holds what the
fixture generator and the tests share: the inputs, the weights and the stored positions.
"""
import torch
import torch.nn.functional as F

from tests.golden.weights import name_seeded_weights

MEAN = (0.429, 0.431, 0.397)
CASES = {"small": dict(B=1, H=32, W=32, factor=2, seed=171),        # the UNet bottom is a 1 x 1 map
         "big": dict(B=2, H=64, W=96, factor=4, seed=172)}          # bottom 2 x 3, W no power of two
# Name-seeded weights alone give flows of 0.01 px (a test would pass with the flows ignored): the last convolution of each
# UNet is scaled.  The fixture stores the two factors.
S1, S2 = 85.0, 40.0
GRID = 2                                                            # stride of the stored grid of case "big"
PIXELS = 64                                                         # and seeded positions per frame of the batch


def input_u8(case):
    """(2, B, 3, H, W) uint8: frame0 a seeded smooth image, frame1 a copy of it shifted by (3, -2) pixels with noise."""
    c = CASES[case]
    g = torch.Generator().manual_seed(c["seed"])
    low = 0.25 + 0.5 * torch.rand(c["B"], 3, c["H"] // 16 + 2, c["W"] // 16 + 2, generator=g)
    big = F.interpolate(low, scale_factor=16, mode="bicubic", align_corners=False).clamp(0, 1)
    f0 = big[:, :, 16:16 + c["H"], 16:16 + c["W"]]
    f1 = big[:, :, 13:13 + c["H"], 18:18 + c["W"]] + 0.02 * torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    return torch.stack([f0, f1.clamp(0, 1)]).mul(255).round().to(torch.uint8)


def frames(u8):
    """(2, B, 3, H, W) uint8 -> frame0, frame1 as f32 in [-1, 1]."""
    x = torch.as_tensor(u8).float() / 127.5 - 1.0
    return x[0].contiguous(), x[1].contiguous()


def seeded_state_dict(net, s1=S1, s2=S2):
    """Name-seeded weights of ``net`` (the reference module or ours) as a CPU f32 state dict, conv3 of the two UNets scaled."""
    sd = {k: v.detach().float().cpu().clone() for k, v in name_seeded_weights(net).state_dict().items()}
    for prefix, s in (("flow_estimator", s1), ("interp", s2)):
        for leaf in ("weight", "bias"):
            sd[f"{prefix}.conv3.{leaf}"] = sd[f"{prefix}.conv3.{leaf}"] * s
    return sd


def sample_pixels(case):
    """PIXELS seeded flat positions into the H x W grid per frame of the batch, sorted: (B, PIXELS) int64."""
    c = CASES[case]
    g = torch.Generator().manual_seed(c["seed"] + 1000)
    return torch.stack([torch.randperm(c["H"] * c["W"], generator=g)[:PIXELS].sort()[0] for _ in range(c["B"])])


def gather_pixels(t, pix):
    """(B, ..., H, W), (B, K) flat positions -> (B, ..., K)."""
    return torch.stack([t[b].flatten(-2)[..., pix[b]] for b in range(t.shape[0])])


def stored(case, t):
    """What the fixture keeps of a (B, ..., H, W) tensor: all of it (small), or the GRID-strided grid (big)."""
    return t if case == "small" else t[..., ::GRID, ::GRID].contiguous()


# ------------------------------------------------------------------------------------------------ the network
def _conv(sd, name, x):
    w = sd[name + ".weight"]
    return F.leaky_relu(F.conv2d(x, w, sd[name + ".bias"], stride=1, padding=(w.shape[2] - 1) // 2), negative_slope=0.1)


def _down(sd, name, x):
    return _conv(sd, name + ".conv2", _conv(sd, name + ".conv1", F.avg_pool2d(x, 2)))


def _up(sd, name, x, skip):
    x = _conv(sd, name + ".conv1", F.interpolate(x, scale_factor=2, mode="bilinear"))
    return _conv(sd, name + ".conv2", torch.cat((x, skip), 1))


def unet(sd, name, x):
    x = _conv(sd, name + ".conv1", x)
    s1 = _conv(sd, name + ".conv2", x)
    s2 = _down(sd, name + ".down1", s1)
    s3 = _down(sd, name + ".down2", s2)
    s4 = _down(sd, name + ".down3", s3)
    s5 = _down(sd, name + ".down4", s4)
    x = _down(sd, name + ".down5", s5)
    x = _up(sd, name + ".up1", x, s5)
    x = _up(sd, name + ".up2", x, s4)
    x = _up(sd, name + ".up3", x, s3)
    x = _up(sd, name + ".up4", x, s2)
    x = _up(sd, name + ".up5", x, s1)
    return _conv(sd, name + ".conv3", x)


def back_warp(img, flow):
    """img sampled at w + u, h + v through grid_sample's defaults (bilinear, zeros, align_corners=False): the sample sits
    half a pixel up-left of that position."""
    H, W = img.shape[2:]
    x = torch.arange(W, dtype=flow.dtype).view(1, 1, W) + flow[:, 0]
    y = torch.arange(H, dtype=flow.dtype).view(1, H, 1) + flow[:, 1]
    grid = torch.stack((2 * (x / W - 0.5), 2 * (y / H - 0.5)), dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def normalised(frame):
    return (frame + 1) / 2 - torch.tensor(MEAN, dtype=frame.dtype).view(1, 3, 1, 1)


def coefficients(k, factor):
    t = k / factor
    temp = -t * (1 - t)
    return t, [temp, t * t, (1 - t) * (1 - t), temp]


def stage_a(i0, i1, f01, f10, coef):
    """-> the interpolation UNet's 20-channel input, and ft0, ft1."""
    ft0 = coef[0] * f01 + coef[1] * f10
    ft1 = coef[2] * f01 + coef[3] * f10
    g0 = back_warp(i0, ft0)
    g1 = back_warp(i1, ft1)
    return torch.cat((i0, i1, f01, f10, ft1, ft0, g1, g0), dim=1), ft0, ft1


def stage_b(i0, i1, ft0, ft1, io, t):
    """-> the frame in [-1, 1], the visibility map, the final flows."""
    ft0f = io[:, :2] + ft0
    ft1f = io[:, 2:4] + ft1
    v0 = torch.sigmoid(io[:, 4:5])
    v1 = 1 - v0
    g0 = back_warp(i0, ft0f)
    g1 = back_warp(i1, ft1f)
    p = ((1 - t) * v0 * g0 + t * v1 * g1) / ((1 - t) * v0 + t * v1)
    p = (p + torch.tensor(MEAN, dtype=p.dtype).view(1, 3, 1, 1)) * 2 - 1
    return p, v0, ft0f, ft1f


@torch.no_grad()
def superslomo_forward(sd, frame0, frame1, factor, detail=None):
    """-> (B, factor - 1, 3, H, W), f01, f10.  ``detail``: a list that receives per timestep dict(v0=, ft0f=, ft1f=)."""
    i0, i1 = normalised(frame0), normalised(frame1)
    flow = unet(sd, "flow_estimator", torch.cat([i0, i1], dim=1))
    f01, f10 = flow[:, :2], flow[:, 2:]
    out = []
    for k in range(1, factor):
        t, coef = coefficients(k, factor)
        iy, ft0, ft1 = stage_a(i0, i1, f01, f10, coef)
        p, v0, ft0f, ft1f = stage_b(i0, i1, ft0, ft1, unet(sd, "interp", iy), t)
        out.append(p)
        if detail is not None:
            detail.append(dict(v0=v0, ft0f=ft0f, ft1f=ft1f))
    return torch.stack(out, dim=1), f01, f10
