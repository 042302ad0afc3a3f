"""Closed forms of the AMT-G tail and of the split instance norm (csrc/amt.hip), written out per element.

  prepare64   flair_amt_multiflow_prepare: MultiFlowDecoder.forward behind its convblock (tests/amt_cpu.py:171-175)
  combine64   flair_amt_multiflow_combine: multi_flow_combine up to comb_block (tests/amt_cpu.py:194-202)
  axpby64     flair_axpby_nhwc
  instnorm64  flair_instnorm_nhwc

All of them work in PIXEL coordinates, as the kernels do; tests/amt_cpu.warp goes through a linspace grid that it builds in
f32 whatever it is handed, so in float64 it is NOT the closed form (it is off by 4.5e-7 at 5 x 7 and by 2.8e-6 at 24 x 40).
reference_combine / reference_prepare call the restated network's own functions (with the convolutions around them stubbed
and, when asked, a float64 warp), which ties the closed forms to the reference in tests/test_amt_tail_cpu.py.

The same code run in float32 is the EMULATION of a kernel: every operation in the kernel's documented order, each rounded
(amt.hip is compiled without contraction).  `fault=` turns a closed form into one of its mutants, a plausible kernel bug;
tests/test_amt_tail_cpu.py shows that the comparisons of tests/test_gpu_amt_tail.py reject every one of them.

The inputs of both test files are made here, seeded and cached, so the CPU companion proves things about the very tensors
the GPU tests use.
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

from tests import amt_cpu as ac
from tests.util import balanced_signs, int_tensor

F64, F32 = torch.float64, torch.float32
N = ac.NUM_FLOWS                    # 5 flows per image
MF_C = 8 * N                        # delta_flow0 (2 n) | delta_flow1 (2 n) | mask (n) | img_res (3 n)

COMBINE_FAULTS = ("swap_xy", "flow0_for_img1", "pair345_both", "mask_other", "zeros", "unclamped", "plus_neg_mean",
                  "mean_frame0", "res_i5c", "mean_of_4", "div_4", "ch15")
PREPARE_FAULTS = ("factor1", "up01_both", "up_swap", "sig_19_23", "res_altered")
INSTNORM_FAULTS = ("var_n1", "eps_outside", "drop_remainder", "double_count", "neighbour_channel", "neighbour_frame",
                   "one_pass_f32")


# ------------------------------------------------------------------------------------------------ the tail
def _prepare(dec, up, dtype, fault=None):
    d, u = dec[..., :MF_C].to(dtype), up[..., :4].to(dtype)
    u2 = (1.0 if fault == "factor1" else 2.0) * u
    idx = [(c & 1) + (2 if c >= 2 * N else 0) for c in range(4 * N)]
    if fault == "up01_both":
        idx = [c & 1 for c in range(4 * N)]
    if fault == "up_swap":
        idx = [j ^ 1 for j in idx]
    out = d.clone()
    out[..., :4 * N] = d[..., :4 * N] + u2[..., idx]
    lo, hi = {"sig_19_23": (4 * N - 1, 5 * N - 1), "res_altered": (4 * N, 5 * N + 1)}.get(fault, (4 * N, 5 * N))
    out[..., lo:hi] = 1.0 / (1.0 + torch.exp(-out[..., lo:hi]))
    return out


def prepare64(dec, up, fault=None):
    """dec (B, H, W, >= 40), up (B, H, W, >= 4) -> (B, H, W, 40) float64: flows + 2 up | sigmoid(mask) | img_res."""
    return _prepare(dec, up, F64, fault)


def prepare_emul32(dec, up):
    return _prepare(dec, up, F32)


def border_warp(img, px, py, fault=None):
    """img (B, H, W, 3), px and py (B, H, W) pixel coordinates of img's dtype -> (B, H, W, 3): clamp the coordinate to the
    frame, floor, clamp the + 1 neighbour to the edge, weights (1 - fx)(1 - fy), ..., summed nw, ne, sw, se.  The image is
    read through flat pixel indices with NaN behind the last frame, which is what a neighbour that is NOT clamped finds
    behind a guarded view."""
    B, H, W, _ = img.shape
    flat = torch.cat([img.reshape(B * H * W, 3), torch.full((W + 2, 3), float("nan"), dtype=img.dtype)])
    base = (torch.arange(B) * (H * W)).view(B, 1, 1)
    zeros = fault == "zeros"
    ix, iy = (px, py) if zeros else (px.clamp(0, W - 1), py.clamp(0, H - 1))
    x0f, y0f = ix.floor(), iy.floor()
    ex, ey = x0f + 1.0, y0f + 1.0
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = x0 + 1, y0 + 1
    if fault != "unclamped" and not zeros:
        x1, y1 = x1.clamp(max=W - 1), y1.clamp(max=H - 1)
    out = None
    for yy, xx, wt in ((y0, x0, (ex - ix) * (ey - iy)), (y0, x1, (ix - x0f) * (ey - iy)), (y1, x0, (ex - ix) * (iy - y0f)),
                       (y1, x1, (ix - x0f) * (iy - y0f))):
        if zeros:
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            v = flat[base + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)]
            term = torch.where(ok[..., None], v * wt[..., None], torch.zeros((), dtype=img.dtype))
        else:
            term = flat[base + yy * W + xx] * wt[..., None]
        out = term if out is None else out + term
    return out


def _combine(pair, prep, neg_mean, dtype, fault=None):
    pair, prep = pair[..., :6].to(dtype), prep[..., :MF_C].to(dtype)
    nm = neg_mean.to(dtype).reshape(neg_mean.shape[0], -1)[:, 0]
    B, H, W, _ = pair.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xs, ys = xs.to(dtype).expand(B, H, W), ys.to(dtype).expand(B, H, W)
    mean = nm if fault == "plus_neg_mean" else -nm
    if fault == "mean_frame0":
        mean = mean[:1].expand(B)
    mean = mean.view(B, 1, 1, 1)
    img0, img1 = pair[..., 0:3], pair[..., 3:6]
    if fault == "pair345_both":
        img0 = img1
    x = torch.zeros(B, H, W, 16, dtype=dtype)
    s = None
    for i in range(N):
        f0, f1 = prep[..., 2 * i:2 * i + 2], prep[..., 2 * N + 2 * i:2 * N + 2 * i + 2]
        if fault == "flow0_for_img1":
            f1 = f0
        if fault == "swap_xy":
            f0, f1 = f0.flip(-1), f1.flip(-1)
        g0 = border_warp(img0, xs + f0[..., 0], ys + f0[..., 1], fault)
        g1 = border_warp(img1, xs + f1[..., 0], ys + f1[..., 1], fault)
        m = prep[..., 4 * N + i:4 * N + i + 1]
        if fault == "mask_other":
            g0, g1 = g1, g0
        res = prep[..., [5 * N + i, 6 * N + i, 7 * N + i]] if fault == "res_i5c" else prep[..., 5 * N + 3 * i:5 * N + 3 * i + 3]
        t = m * g0 + (1.0 - m) * g1 + mean + res
        x[..., 3 * i:3 * i + 3] = t
        if not (fault == "mean_of_4" and i == N - 1):
            s = t if s is None else s + t
    if fault == "ch15":
        x[..., 15] = 1.0
    avg = torch.zeros(B, H, W, 4, dtype=dtype)
    avg[..., :3] = s / (4.0 if fault in ("mean_of_4", "div_4") else 5.0)
    return x, avg, s


def combine64(pair, prep, neg_mean, fault=None, with_sum=False):
    """pair (B, H, W, >= 6) the two mean-free images, prep (B, H, W, >= 40) as prepare64 leaves it, neg_mean (B,) or
    (B, k) with -mean in its first column -> x (B, H, W, 16), avg (B, H, W, 4) float64 (and the five-term sum that avg
    divides): per flow i, t = m g0 + (1 - m) g1 + mean + img_res[3 i + c], x[3 i + c] = t, avg[c] = (sum_i t) / 5;
    channel 15 of x and channel 3 of avg are zero."""
    x, avg, s = _combine(pair, prep, neg_mean, F64, fault)
    return (x, avg, s) if with_sum else (x, avg)


def combine_emul32(pair, prep, neg_mean):
    return _combine(pair, prep, neg_mean, F32)[:2]


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def warp64(img, flow):
    """tests/amt_cpu.warp with its linspace grid in float64 (the reference's formula, not its f32 grid)."""
    B, _, H, W = flow.shape
    xx = torch.linspace(-1.0, 1.0, W, dtype=F64).view(1, 1, 1, W).expand(B, -1, H, -1)
    yy = torch.linspace(-1.0, 1.0, H, dtype=F64).view(1, 1, H, 1).expand(B, -1, -1, W)
    flow_ = torch.cat([flow[:, 0:1] / ((W - 1.0) / 2.0), flow[:, 1:2] / ((H - 1.0) / 2.0)], 1)
    return F.grid_sample(img, (torch.cat([xx, yy], 1) + flow_).permute(0, 2, 3, 1), mode="bilinear", padding_mode="border",
                         align_corners=True)


@contextlib.contextmanager
def _stubbed(**names):
    old = {k: getattr(ac, k) for k in names}
    for k, v in names.items():
        setattr(ac, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ac, k, v)


def reference_combine(pair, prep, neg_mean, dtype=F32, warp=None):
    """tests/amt_cpu.multi_flow_combine itself in ``dtype`` on NCHW copies of the inputs, with comb_block's convolutions
    stubbed to zero: -> img_warps as (B, H, W, 15) and its mean over the flows as (B, H, W, 3).  warp=None keeps the
    reference's own warp (f32 ATen arithmetic when dtype is f32)."""
    B = pair.shape[0]
    p, q = nchw(pair[..., :6]).to(dtype), nchw(prep[..., :MF_C]).to(dtype)
    mean = -neg_mean.to(dtype).reshape(B, -1)[:, :1].reshape(B, 1, 1, 1)
    seen = []

    def conv(sd, name, x, stride=1):
        seen.append(x)
        return torch.zeros(x.shape[0], 3, *x.shape[2:], dtype=x.dtype)

    with _stubbed(conv=conv, **({"warp": warp} if warp is not None else {})):
        avg = ac.multi_flow_combine({"comb_block.1.weight": torch.zeros(1, dtype=dtype)}, p[:, 0:3], p[:, 3:6], q[:, :2 * N],
                                    q[:, 2 * N:4 * N], q[:, 4 * N:5 * N], q[:, 5 * N:], mean)
    return nhwc(seen[0]).contiguous(), nhwc(avg).contiguous()


def reference_prepare(dec, flow_half, dtype=F64):
    """tests/amt_cpu.multi_flow_decoder itself with its convblock stubbed to return ``dec``: dec (B, 2 h, 2 w, 40), flow_half
    (B, h, w, 4) the flows it enlarges -> (B, 2 h, 2 w, 40), and the enlarged flows (B, 2 h, 2 w, 4) that the kernel is given."""
    d, fl = nchw(dec).to(dtype), nchw(flow_half).to(dtype)
    one = fl[:, :1]
    with _stubbed(convblock=lambda sd, name, x: d, warp=lambda img, flow: img):
        out = ac.multi_flow_decoder({}, "decoder1", one, one, one, fl[:, 0:2], fl[:, 2:4])
    return nhwc(torch.cat(out, 1)).contiguous(), nhwc(ac.resize(fl, 2.0)).contiguous()


# ------------------------------------------------------------------------------------------------ axpby
def f32_scalar(v):
    return torch.tensor(v, dtype=F32)


def axpby64(x0, a, x1=None, b=0.0):
    """a x0 + b x1 in float64, a and b the f32 values that the entry receives."""
    y = f32_scalar(a).double() * x0.double()
    return y if x1 is None else y + f32_scalar(b).double() * x1.double()


def axpby_emul32(x0, a, x1=None, b=0.0, fault=None):
    """The kernel's order in f32: a x0 rounded, b x1 rounded, then the sum.  fault="fma": the sum takes b x1 unrounded, as
    a contracted `v += b * u` would (the exact product and sum in float64, rounded once)."""
    y = x0 * f32_scalar(a)
    if x1 is None:
        return y
    if fault == "fma":
        return (y.double() + f32_scalar(b).double() * x1.double()).float()
    return y + x1 * f32_scalar(b)


# ------------------------------------------------------------------------------------------------ instance norm
IN_MAX_SPLIT = 64


def in_split(HW):
    """How many chunks amt.hip sums a plane in: HW / 512, at least 1 and at most 64; a chunk is ceil(HW / S) pixels."""
    return 1 if HW <= 512 else min(HW // 512, IN_MAX_SPLIT)


def chunks(HW):
    S = in_split(HW)
    c = -(-HW // S)
    return [min(c, HW - s * c) for s in range(S)]


def _pixel_counts(HW, fault):
    """How often each pixel of a plane enters the sums: once, unless a chunk fault drops or repeats some."""
    S = in_split(HW)
    n = torch.ones(HW, dtype=F64)
    if fault == "drop_remainder":                   # chunk = HW / S rounded down, nothing after S chunks
        n[S * (HW // S):] = 0
    if fault == "double_count":                     # every chunk but the first starts one pixel early
        c = -(-HW // S)
        for s in range(1, S):
            n[s * c - 1] += 1
    return n.view(1, HW, 1)


def _neighbour(stat, fault):
    if fault == "neighbour_channel":
        return stat.roll(1, dims=2)
    if fault == "neighbour_frame":
        return stat.roll(1, dims=0)
    return stat


def instnorm64(x, eps=1e-5, relu=False, fault=None):
    """x (F, H, W, C) -> float64: (x - mean) / sqrt(var + eps) with the biased variance of each (frame, channel) plane."""
    F_, H, W, C = x.shape
    HW = H * W
    v = x.double().reshape(F_, HW, C)
    n = _pixel_counts(HW, fault)
    mean = (n * v).sum(1, keepdim=True) / HW
    var = (n * (v - mean) ** 2).sum(1, keepdim=True) / (HW - 1 if fault == "var_n1" else HW)
    if fault == "one_pass_f32":
        m32 = mean.float()
        var = ((v * v).sum(1, keepdim=True) / HW).float().sub(m32 * m32).clamp_min(0.0).double()
    mean, var = _neighbour(mean, fault), _neighbour(var, fault)
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    y = ((v - mean) * rstd).reshape(F_, H, W, C)
    return y.clamp_min(0.0) if relu else y


def instnorm_emul32(x, eps=1e-5, relu=False):
    """The kernel's order: the mean summed in double and rounded to f32, the variance of the values centred IN F32 on that
    mean summed in double, 1 / sqrt(var + eps) in double rounded to f32, then (x - mean) * rstd in f32."""
    F_, H, W, C = x.shape
    v = x.reshape(F_, H * W, C)
    mean = v.double().mean(1, keepdim=True).float()
    var = ((v - mean).double() ** 2).mean(1, keepdim=True)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    y = ((v - mean) * rstd).reshape(F_, H, W, C)
    return y.clamp_min(0.0) if relu else y


def aten_instnorm32(x, eps=1e-5, relu=False):
    y = nhwc(F.instance_norm(nchw(x), eps=eps))
    return (F.relu(y) if relu else y).contiguous()


# ------------------------------------------------------------------------------------------------ inputs
TAIL_SHAPES = [(2, 5, 7),           # the smallest with two frames
               (2, 17, 19),         # 646 pixels: three workgroups, the last one partial, and the second frame's base
               (1, 1, 9), (1, 9, 1)]    # an extent of one pixel: both neighbours clamp
AXPBY_C = [4, 20, 40]
AXPBY_P = [(2, 5, 7), (2, 17, 19)]
AXPBY_COEFS = [(1.0, 2.0), (1.0 / 3.0, 1.7)]
CORR_SCALE_N = [1, 3, 4, 5, 1027]
# (F, H, W, C): see tests/test_gpu_amt_tail.py for what each one reaches
INSTNORM_SHAPES = [(2, 32, 32, 64), (2, 33, 36, 112), (1, 40, 41, 4), (1, 182, 182, 64), (2, 33, 35, 64)]
INSTNORM_OFFSETS = [1, 30, 300]
ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _gen(*key):
    seed = 20240
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _neg_mean(values):
    """(B, 8) with -mean in column 0 and NaN in the rest, so that its row stride is 8 and only column 0 may be read."""
    t = torch.full((len(values), 8), float("nan"))
    t[:, 0] = torch.tensor(values)
    return t


def pinned_pixels(B, H, W):
    """name -> (frame, h, w) of the pixels whose ten flows are pinned; distinct at every shape of TAIL_SHAPES."""
    at = lambda f, p: (f, (p % (H * W)) // W, (p % (H * W)) % W)
    return {"far_up_left": at(0, 1), "on_last": at(0, 2), "on_zero": at(0, 3), "fraction_below_zero": at(B - 1, 0),
            "far_down_right": at(B - 1, H * W - 1)}


@functools.lru_cache(maxsize=None)
def combine_exact_case(B, H, W):
    """Integer images in [-8, 8], flows on a quarter-pixel grid in [-4, 4], masks k / 8, img_res k / 4, integer means:
    every product and sum of the kernel is exact in f32 (tests/test_amt_tail_cpu.py checks it)."""
    g = _gen(1, B, H, W)
    pair = int_tensor((B, H, W, 6), -8, 8, g)
    prep = torch.cat([int_tensor((B, H, W, 4 * N), -16, 16, g) / 4, int_tensor((B, H, W, N), 0, 8, g) / 8,
                      int_tensor((B, H, W, 3 * N), -8, 8, g) / 4], dim=-1)
    pins = pinned_pixels(B, H, W)
    both = lambda fx, fy: torch.tensor([fx, fy] * (2 * N), dtype=F32)
    prep[pins["far_up_left"]][:4 * N] = -40.0
    prep[pins["far_down_right"]][:4 * N] = 40.0
    _, h, w = pins["on_last"]
    prep[pins["on_last"]][:4 * N] = both(W - 1 - w, H - 1 - h)
    _, h, w = pins["on_zero"]
    prep[pins["on_zero"]][:4 * N] = both(-w, -h)
    prep[pins["fraction_below_zero"]][:4 * N] = both(-0.25, -0.5)
    return dict(pair=pair, prep=prep, neg_mean=_neg_mean([-3.0, 5.0][:B]))


def landings(prep, H, W):
    """-> px, py (B, H, W, 2 N): where the ten flows of each pixel land."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    fl = prep[..., :4 * N].double()
    return xs[None, :, :, None] + fl[..., 0::2], ys[None, :, :, None] + fl[..., 1::2]


def landing_classes(prep, H, W):
    px, py = landings(prep, H, W)
    return {"far_up_left": bool(((px <= -30) & (py <= -30)).any()),
            "far_down_right": bool(((px >= W + 30) & (py >= H + 30)).any()),
            "on_last": bool(((px == W - 1) & (py == H - 1)).any()),
            "on_zero": bool(((px == 0) & (py == 0)).any()),
            "fraction_below_zero": bool(((px > -1) & (px < 0) & (py > -1) & (py < 0)).any())}


@functools.lru_cache(maxsize=None)
def combine_seeded_case(B, H, W):
    """Normal images, flows of sigma 3, masks uniform in (0, 1), img_res of sigma 0.1, means near 0.45."""
    g = _gen(2, B, H, W)
    pair = torch.randn(B, H, W, 6, generator=g)
    prep = torch.cat([3.0 * torch.randn(B, H, W, 4 * N, generator=g), torch.rand(B, H, W, N, generator=g),
                      0.1 * torch.randn(B, H, W, 3 * N, generator=g)], dim=-1)
    return dict(pair=pair, prep=prep, neg_mean=_neg_mean([-0.4375, -0.53][:B]))


@functools.lru_cache(maxsize=None)
def prepare_case(B, H, W):
    """dec and up on a quarter grid, |v| <= 64 (dec + 2 up is exact); the mask channels normal of sigma 4."""
    g = _gen(3, B, H, W)
    dec = int_tensor((B, H, W, MF_C), -256, 256, g) / 4
    dec[..., 4 * N:5 * N] = 4.0 * torch.randn(B, H, W, N, generator=g)
    up = int_tensor((B, H, W, 4), -256, 256, g) / 4
    return dict(dec=dec, up=up)


SATURATION = [-100.0, -88.0, -20.0, 0.0, 20.0, 88.0, 100.0]


def saturation_case():
    """(1, 1, 7, 40) and (1, 1, 7, 4): pixel j holds SATURATION[j] in all five mask channels, zeros elsewhere."""
    dec = torch.zeros(1, 1, len(SATURATION), MF_C)
    dec[0, 0, :, 4 * N:5 * N] = torch.tensor(SATURATION)[:, None]
    return dict(dec=dec, up=torch.zeros(1, 1, len(SATURATION), 4))


@functools.lru_cache(maxsize=None)
def axpby_case(shape, C):
    g = _gen(4, *shape, C)
    return torch.randn(*shape, C, generator=g), torch.randn(*shape, C, generator=g)


@functools.lru_cache(maxsize=None)
def corr_scale_case(n):
    return 10.0 * torch.randn(n, generator=_gen(5, n))


@functools.lru_cache(maxsize=None)
def instnorm_balanced_case(shape):
    F_, H, W, C = shape
    return balanced_signs(F_, H, W, C, 1, C, _gen(6, *shape))


@functools.lru_cache(maxsize=None)
def instnorm_seeded_case(shape, offset):
    """Per channel a scale in [0.5, 1.5] and a mean of +-(0.75 .. 1.25) * offset standard deviations; the frames after the
    first are scaled by 3, so no two frames and no two channels share their statistics."""
    F_, H, W, C = shape
    g = _gen(7, *shape, offset)
    scale = 0.5 + torch.rand(C, generator=g)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    x = (torch.randn(F_, H, W, C, generator=g) + offset * sign * (0.75 + 0.5 * torch.rand(C, generator=g))) * scale
    x[1:] *= 3.0
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _instnorm_seeded_pair(shape, offset):
    x = instnorm_seeded_case(shape, offset)
    return instnorm64(x), aten_instnorm32(x).double()


def instnorm_seeded_reference(shape, offset, relu=False):
    """-> want (float64), and the deviation of F.instance_norm (+ ReLU) in f32 from it."""
    want, aten = _instnorm_seeded_pair(shape, offset)
    if relu:
        want, aten = want.clamp_min(0.0), aten.clamp_min(0.0)
    return want, (aten - want).abs().max().item()


@functools.lru_cache(maxsize=None)
def combine_exact_reference(B, H, W):
    """-> x, avg, and the five-term sum behind avg, float64."""
    return combine64(**combine_exact_case(B, H, W), with_sum=True)


@functools.lru_cache(maxsize=None)
def combine_seeded_reference(B, H, W):
    """-> want x, want avg (float64) and, for each, the deviation of the reference's own f32 ATen arithmetic from it.  (On
    an extent of one pixel the reference divides the flow by (size - 1) / 2 = 0; the infinite coordinate clamps to the one
    pixel there is, so the answer is finite as long as no flow is exactly 0.)"""
    d = combine_seeded_case(B, H, W)
    x, avg = combine64(**d)
    x32, avg32 = reference_combine(**d)
    return x, avg, max_err(x32, x[..., :3 * N]), max_err(avg32, avg[..., :3])


@functools.lru_cache(maxsize=None)
def prepare_reference(B, H, W):
    """-> want (float64) and the deviation of torch.sigmoid in f32 from float64 on the case's mask values."""
    d = prepare_case(B, H, W)
    m = d["dec"][..., 4 * N:5 * N]
    return prepare64(**d), max_err(torch.sigmoid(m), torch.sigmoid(m.double()))


def not_mask(t):
    """The channels of a prepare output that are exact: flows and img_res."""
    return torch.cat([t[..., :4 * N], t[..., 5 * N:]], dim=-1)


def max_err(got, want):
    """Largest |got - want| with NaN counted as infinite."""
    d = (got.double() - want).abs()
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).max().item()


def same_bits(a, b):
    """a and b (f32) agree in every element, signed zeros taken as equal (tests/util.assert_bits_equal's rule)."""
    return bool((a == b).all())
