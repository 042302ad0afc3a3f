"""Float64 closed forms of the resampling operations of csrc/warp.hip, and the cases that tests/test_resample_exact_cpu.py
and tests/test_gpu_resample_exact.py share.

Every function is written from the operation's definition (mmedit's flow_warp = grid_sample(bilinear, align_corners=True)
on pixel coordinates + flow; F.interpolate bilinear / bicubic / nearest; F.avg_pool2d), not from the kernels.  Tensors are
clips (F, H, W, C); flows are (F, H, W, 2) with (dx, dy) innermost.

`fault=` turns a closed form into one of its mutants (a plausible kernel bug); tests/test_resample_exact_cpu.py shows that
the cases and the bound see every one of them.

Data.  Sources are integers in [-8, 8] (exact in bf16 and f32), so D = 16 bounds the difference of two neighbouring samples
(and of a sample and the zero padding).  Flows are multiples of 1, 0.5 and 0.25, so that the bilinear weights are multiples
of 1/16 and the exact result, a multiple of 1/16 below 16, is a bf16 number.

Bound.  |got - ref64| <= out_rounding(ref64, dtype) + COORD_FACTOR * D * 2^-24 * m per element, m the largest extent.  The
second term: a sampling coordinate below m computed in f32 is off by a few 2^-24 * m, and moving a bilinear sample by e
moves the result by at most D * e per axis.  The f32 reference on the CPU stays below 1.0 * D * 2^-24 * m (asserted against
the whole bound in test_resample_exact_cpu.py), so the factor 4 leaves it 4x headroom.
"""
import numpy as np
import torch

from tests.util import int_tensor, out_rounding

D = 16.0
COORD_FACTOR = 4.0
U24 = 2.0 ** -24


def coord_term(m):
    return COORD_FACTOR * D * U24 * m


def bound(ref64, dtype, m):
    return out_rounding(ref64, dtype) + coord_term(m)


def worst_ratio(got, ref64, dtype, m):
    """-> (largest err / bound, flat index of it); NaN counts as infinite."""
    err = (got.detach().cpu().double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    r = err / bound(ref64, dtype, m)
    i = int(r.flatten().argmax())
    return r.flatten()[i].item(), i


def assert_within(got, ref64, dtype, m, what):
    """Per element |got - ref64| <= bound.  -> the largest err / bound."""
    assert ref64.dtype == torch.float64 and tuple(got.shape) == tuple(ref64.shape), (what, got.shape, ref64.shape)
    ratio, i = worst_ratio(got, ref64, dtype, m)
    if not ratio <= 1.0:
        idx = np.unravel_index(i, tuple(ref64.shape))
        g = got.detach().cpu().double()
        bad = ((g - ref64).abs() > bound(ref64, dtype, m)) | torch.isnan(g)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} element(s) beyond the bound; worst err / bound = "
                             f"{ratio:.3g} at {[int(v) for v in idx]}: got {g.flatten()[i].item()!r}, expected "
                             f"{ref64.flatten()[i].item()!r}, bound {bound(ref64, dtype, m).flatten()[i].item():.3e}")
    return ratio


# ------------------------------------------------------------------------------------------------------------- warps
def _landing(px, py, H, W, fault=None):
    """Sampling coordinates of grid_sample(align_corners=True) after flow_warp's normalisation: the pixel coordinate itself,
    and 0 on an axis of size 1 (the round trip multiplies by size - 1 = 0)."""
    ix = px if (W > 1 or fault == "size1_follows") else torch.zeros_like(px)
    iy = py if (H > 1 or fault == "size1_follows") else torch.zeros_like(py)
    return ix, iy


def bilinear64(x, px, py, border, fault=None):
    """x (F, H, W, C) sampled at pixel coordinates px, py (F, H, W) float64 -> (F, H, W, C) float64."""
    F_, H, W, C = x.shape
    xd = x.double()
    if fault == "swap_xy":
        px, py = py, px
    ix, iy = _landing(px, py, H, W, fault)
    if border and fault != "clamp_after_floor":
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    ax, ay = ix - x0, iy - y0
    if border and fault == "clamp_after_floor":
        x0, y0 = x0.clamp(0, W - 1), y0.clamp(0, H - 1)
    if fault == "weights":
        ax = 1.0 - ax
    if fault == "corner_x":
        x0 = x0 + 1
    if fault == "corner_y":
        y0 = y0 + 1
    f = torch.arange(F_).view(F_, 1, 1).expand_as(px)
    out = torch.zeros(F_, px.shape[1], px.shape[2], C, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            inside = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            v = xd[f, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()]
            out += torch.where(inside, wgt, torch.zeros_like(wgt))[..., None] * v
    return out


def _pixel_coords(flow):
    F_, H, W, _ = flow.shape
    fd = flow.double()
    return (torch.arange(W, dtype=torch.float64).view(1, 1, W) + fd[..., 0],
            torch.arange(H, dtype=torch.float64).view(1, H, 1) + fd[..., 1])


def warp_ref64(x, flow, border, fault=None):
    px, py = _pixel_coords(flow)
    return bilinear64(x, px, py, border, fault)


def compose_ref64(f1, f2, fault=None):
    w = warp_ref64(f2, f1, False, None if fault == "no_add" else fault)
    return w if fault == "no_add" else f1.double() + w


def prep_ref64(prop, feat2, flow1, flow_prev, dtype, flow2=None, fault=None):
    """-> dict(cond1, flow2, cond2, flowpad) of flair_vsrpp_prep; flow2, cond2 are None and flowpad[..., 2:4] is 0 without
    flow_prev.  cond2 is feat2 warped by the composed flow -- or by `flow2` when one is given: the f32 flow that the
    implementation under test reported (itself compared with the composed flow), so that the f32 rounding of a flow is
    not charged a second time, multiplied by D, to the warp that uses it.  flowpad is (flow1, that flow) rounded to dtype."""
    out = dict(cond1=warp_ref64(prop, flow1, False), flow2=None, cond2=None)
    pad = torch.zeros(*flow1.shape[:3], 4, dtype=torch.float64)
    pad[..., 0:2] = flow1.double()
    if flow_prev is not None:
        out["flow2"] = compose_ref64(flow1, flow_prev, fault)
        used = out["flow2"] if flow2 is None else flow2.double()
        out["cond2"] = warp_ref64(feat2, used, False)
        pad[..., 2:4] = used
    out["flowpad"] = pad.to(dtype).double()         # flows are f32 numbers (or f32 sums): one rounding
    return out


def corner_shares(flow, H, W):
    """-> (share of output pixels whose corners with a non-zero weight ALL lie outside the frame, share with some but not
    all of them outside).  A corner of weight 0 (an integer landing's right neighbour) contributes nothing wherever it is."""
    px, py = _pixel_coords(flow)
    ix, iy = _landing(px, py, H, W)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    ax, ay = ix - x0, iy - y0
    n_out = torch.zeros_like(ix)
    n_all = torch.zeros_like(ix)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            live = ((ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)) > 0
            outside = ~((xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1))
            n_all += live
            n_out += live & outside
    return (n_out == n_all).double().mean().item(), ((n_out > 0) & (n_out < n_all)).double().mean().item()


# ------------------------------------------------------------------------------------------------------------ resize
def _cubic_weights(t, A):
    c1 = lambda v: ((A + 2.0) * v - (A + 3.0)) * v * v + 1.0
    c2 = lambda v: ((A * v - 5.0 * A) * v + 8.0 * A) * v - 4.0 * A
    return [c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)]


def _axis_taps(mode, n_in, n_out, fault=None):
    """The taps of one axis -> list of (index (n_out,) long, weight (n_out,) float64)."""
    o = torch.arange(n_out, dtype=torch.float64)
    if mode == 3:
        assert n_in == 2 * n_out
        return [((2 * o).long(), torch.full_like(o, 0.5)), ((2 * o + 1).long(), torch.full_like(o, 0.5))]
    s = n_in / n_out
    if mode in (0, 1):
        if mode == 1:
            s = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        half = (mode == 0) != (fault in ("no_half_pixel", "half_pixel_ac"))
        r = (s * (o + 0.5) - 0.5).clamp_min(0.0) if half else s * o
        i0 = torch.floor(r).clamp_max(n_in - 1)
        a = (r - i0).clamp(0.0, 1.0)
        return [(i0.long(), 1.0 - a), ((i0 + 1).clamp_max(n_in - 1).long(), a)]
    assert mode == 2
    r = s * (o + 0.5) - 0.5
    i0 = torch.floor(r)
    w = _cubic_weights(r - i0, -0.5 if fault == "cubic_a05" else -0.75)
    taps = []
    for k in range(4):
        i = i0 - 1 + k
        wk = w[k]
        if fault == "cubic_unclamped":
            wk = torch.where((i >= 0) & (i <= n_in - 1), wk, torch.zeros_like(wk))
        taps.append((i.clamp(0, n_in - 1).long(), wk))
    return taps


def resize_ref64(x, size, mode, scale_c0=1.0, scale_c1=1.0, fault=None):
    """Modes 0 to 3 of flair_resize_nhwc on a clip (F, Hi, Wi, C) -> (F, Ho, Wo, C) float64: bilinear with align_corners
    False / True, bicubic (A = -0.75, taps clamped to the border), 2x2 mean; channel 0 * scale_c0, channel 1 * scale_c1."""
    F_, Hi, Wi, C = x.shape
    Ho, Wo = size
    xd = x.double()
    out = torch.zeros(F_, Ho, Wo, C, dtype=torch.float64)
    for iy, wy in _axis_taps(mode, Hi, Ho, fault):
        for ix, wx in _axis_taps(mode, Wi, Wo, fault):
            out += (wy.view(1, Ho, 1, 1) * wx.view(1, 1, Wo, 1)) * xd[:, iy][:, :, ix]
    sc = [scale_c0, scale_c1]
    if fault == "scale_swap":
        sc = [scale_c1, scale_c0]
    for c in range(min(C, 2)):
        out[..., c] *= sc[c]
    if fault == "scale_c2" and C > 2:
        out[..., 2] *= scale_c1
    return out


def nearest_index(n_in, n_out, fault=None):
    """Source index of F.interpolate(mode="nearest"): floor(dst * scale) with the scale and the product in float32, which is
    not the exact rational at small sizes (n_in = 2, n_out = 82: 41 * float32(2 / 82) < 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    v = np.arange(n_out, dtype=np.float32) * scale
    if fault == "round":
        v = v + np.float32(0.5)
    return torch.from_numpy(np.minimum(np.floor(v).astype(np.int64), n_in - 1))


def nearest_ref(x, size, fault=None):
    """Mode 4: a gather, so the result has x's dtype and is compared bit for bit."""
    return x[:, nearest_index(x.shape[1], size[0], fault)][:, :, nearest_index(x.shape[2], size[1], fault)]


# ------------------------------------------------------------------------------------------------------------- cases
def source(F_, H, W, C, g):
    """Integers in [-8, 8], every frame and channel drawn on its own."""
    return int_tensor((F_, H, W, C), -8, 8, g)


def ramp(F_, H, W, C):
    """A large source without a large random draw: (((3 + c div 17) h + 5 w + 7 c + 11 f) mod 17) - 8, integers in [-8, 8]
    that differ from pixel to pixel, from channel to channel and from frame to frame."""
    c = torch.arange(C).view(1, 1, 1, C)
    v = ((3 + c // 17) * torch.arange(H).view(1, H, 1, 1) + 5 * torch.arange(W).view(1, 1, W, 1) + 7 * c
         + 11 * torch.arange(F_).view(F_, 1, 1, 1))
    return (v % 17 - 8).float()


def pinned_flows(H, W):
    """(landing x or None, landing y or None, flow) triples; a landing is turned into flow = landing - coordinate, `flow`
    is used as it stands.  Landings exactly on -1 (the last position where zeros padding still contributes: weight 0),
    0, size - 1 and size on each axis with the other axis half a pixel off, both axes on -1 and on size - 1, and flows far
    outside, the last pair beyond int32."""
    pins = []
    for t in (-1.0, 0.0, W - 1.0, float(W)):
        pins.append((t, None, (0.0, 0.5)))
    for t in (-1.0, 0.0, H - 1.0, float(H)):
        pins.append((None, t, (0.5, 0.0)))
    pins.append((-1.0, -1.0, (0.0, 0.0)))
    pins.append((W - 1.0, H - 1.0, (0.0, 0.0)))
    for v in (1e4, -1e4, 3e9, -3e9):
        pins.append((None, None, (v, v)))
    return pins


def flow_field(F_, H, W, g, edge_share=0.2, span=None):
    """(F, H, W, 2) float32: per pixel and axis a multiple of 1, 0.5 or 0.25 within +-span (3 pixels; 2 where an axis has
    fewer than 8 samples, or more than half of the landings would miss the frame); a share of the pixels is sent
    to a landing 0.25, 0.5 or 0.75 outside the first or last sample of one axis (one to three corners outside, at any frame
    size); then the pinned pixels, spread evenly over the field.  Needs F * H * W >= 14."""
    if span is None:
        span = 3 if min(v for v in (H, W, 1 << 30) if v > 1) >= 8 else 2
    step = torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (F_, H, W, 2), generator=g)]
    k = torch.floor((torch.rand(F_, H, W, 2, generator=g) * 2 - 1) * (span / step + 1)).clamp(-span / step, span / step)
    flow = k * step
    coords = torch.stack([torch.arange(W).view(1, 1, W).expand(F_, H, W),
                          torch.arange(H).view(1, H, 1).expand(F_, H, W)], -1).float()
    size = torch.tensor([float(W), float(H)])
    edge = torch.rand(F_, H, W, generator=g) < edge_share
    axis = torch.randint(0, 2, (F_, H, W), generator=g)
    if W == 1:
        axis[:] = 1
    if H == 1:
        axis[:] = 0
    high = torch.randint(0, 2, (F_, H, W), generator=g).bool()
    frac = torch.randint(1, 4, (F_, H, W), generator=g).float() / 4
    land = torch.where(high, size[axis] - 1 + frac, -frac)
    sel = torch.nn.functional.one_hot(axis, 2).bool() & edge[..., None]
    flow = torch.where(sel, land[..., None] - coords, flow)
    pins = pinned_flows(H, W)
    n = F_ * H * W
    assert n >= len(pins), (F_, H, W)
    flat, cflat = flow.view(n, 2), coords.reshape(n, 2)
    for j, (lx, ly, fl) in enumerate(pins):
        p = j * (n // len(pins))
        flat[p, 0] = fl[0] if lx is None else lx - cflat[p, 0]
        flat[p, 1] = fl[1] if ly is None else ly - cflat[p, 1]
    return flow.contiguous()


def warp_frames(H, W):
    """Frames of a case: 3 (flow_warp takes the clip; the one-frame entries, vsrpp_*, run frame by frame), more for the
    six-pixel frames so that the 14 pinned pixels leave room for ordinary ones."""
    return max(3, -(-60 // (H * W)))


# (H, W, C): not square, so that an axis swap shows; axes of size 1; W = 64
WARP_CASES = [(5, 7, 64), (12, 10, 32), (9, 33, 64), (1, 6, 32), (6, 1, 64), (17, 64, 32)]
BIG_WARP = (520, 520, 32)          # 520 * 520 * (32 / 8) 16-byte chunks of bf16 > 4096 * 256 threads: the grid-stride loop
BIG_COMPOSE = (1030, 1030)         # > 4096 * 256 pixels
FLOW_PREV_SPAN = 2                 # |flow_prev| <= 2, so DP bounds its neighbour difference
DP = 4.0


def _seed(*key):
    s = 1
    for v in key:
        s = s * 1009 + int(v) + 7
    return torch.Generator().manual_seed(s % (2 ** 31))


_CACHE = {}


def warp_case(H, W, C):
    """-> dict(x, x2 sources (F, H, W, C) f32; flow, flow2 displacing fields with the pins, flow_prev a sampled field,
    (F, H, W, 2) f32); cached, never modified by a test."""
    key = ("warp", H, W, C)
    if key not in _CACHE:
        g = _seed(H, W, C)
        big = (H, W, C) == BIG_WARP
        F_ = 1 if big else warp_frames(H, W)
        # flow_prev is a field that is sampled, not one that displaces: quarter-pixel values, no pins
        _CACHE[key] = dict(x=ramp(F_, H, W, C) if big else source(F_, H, W, C, g),
                           x2=ramp(F_, H, W, C).flip(3).contiguous() if big else source(F_, H, W, C, g),
                           flow=flow_field(F_, H, W, g), flow2=flow_field(F_, H, W, g),
                           flow_prev=int_tensor((F_, H, W, 2), -4 * FLOW_PREV_SPAN, 4 * FLOW_PREV_SPAN, g) / 4)
    return _CACHE[key]


def compose_case(H, W):
    """-> dict(f1 quarter-pixel flows with the pins, f2 integer-valued in [-8, 8]), one frame for the large case."""
    key = ("compose", H, W)
    if key not in _CACHE:
        g = _seed(H, W, 2)
        big = (H, W) == BIG_COMPOSE
        F_ = 1 if big else warp_frames(H, W)
        _CACHE[key] = dict(f1=flow_field(F_, H, W, g), f2=ramp(F_, H, W, 2) if big else source(F_, H, W, 2, g))
    return _CACHE[key]


RESIZE_IN = [(7, 9), (1, 6), (6, 1), (2, 3), (16, 12), (33, 5)]
RESIZE_OUT = [(13, 11), (3, 4), (1, 1), (14, 18), (40, 30), (5, 64)]
RESIZE_FRAMES = 2
SCALED_CASES = [((7, 9), (13, 11)), ((16, 12), (3, 4))]     # scale_c0 = 1.5, scale_c1 = 0.75 on three channels
# mode 0 on 16-byte-aligned dense clips of 16 / 32 channels (bilinear_vec_kernel), up and down at non-integer ratios
VEC_CASES = [((7, 9), (13, 11)), ((16, 12), (5, 7)), ((1, 6), (3, 4)), ((33, 5), (14, 18)), ((6, 1), (5, 64))]
# mode 4: (Hi, Wi), (Ho, Wo), C
NEAREST_CASES = [((7, 9), (14, 18), 16), ((7, 9), (14, 18), 3), ((7, 9), (10, 13), 16), ((16, 12), (5, 7), 3),
                 ((2, 3), (82, 7), 3), ((4, 3), (82, 5), 16), ((3, 2), (6, 82), 3), ((1, 6), (2, 12), 16)]
BIG_RESIZE = ((37, 53), (600, 601), 3)      # 600 * 601 * 3 scalar-kernel threads > 4096 * 256
BIG_RESIZE_VEC = ((300, 200), (728, 724), 16)    # 728 * 724 * (16 / 8) chunks of bf16 > 4096 * 256


def resize_extent(hw_in, hw_out):
    return max(*hw_in, *hw_out)


def resize_source(F_, Hi, Wi, C, big=False):
    key = ("resize", F_, Hi, Wi, C, big)
    if key not in _CACHE:
        _CACHE[key] = ramp(F_, Hi, Wi, C) if big else source(F_, Hi, Wi, C, _seed(F_, Hi, Wi, C))
    return _CACHE[key]
