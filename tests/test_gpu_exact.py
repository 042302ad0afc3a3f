"""Bit-exact parity of the matrix-core kernels (conv.hip, chain.hip, dcn.hip) and of the depthwise kernels on integer data.

On integer-valued inputs every product and every partial sum of a convolution is an integer below 2^24, so f32 holds all
of them exactly: the result does not depend on accumulation order, tile shape, split-K or the MFMA instruction, and the
kernel's output has to equal the reference BIT FOR BIT -- the exact value in f32, its round-to-nearest-even in bf16.
One wrong or missing (tap, channel) product, a bias taken from the neighbouring cout, truncation instead of RNE or an
error confined to one row of one tile changes bits, where the randn / 1.6 % tests (test_gpu_kernels.py) see nothing.

Data: weights in [-3, 3], bias and frame_bias in [-8, 8], residuals in [-64, 64], inputs in [-R, R] (R per case),
out_scale a power of two.  Reference: F.conv2d / F.conv3d in float64 on the CPU, cast to f32 (exact: every test calls
assert_exact_headroom on its own data), epilogue in f32 in the documented order
(act(conv + bias + frame_bias) + res0 + res1) * out_scale, then .to(dtype).  Every bf16 case asserts that at least 5 %
of its outputs were NOT representable in bf16 before that cast, so the rounding is exercised.
Exact activations: none and ReLU with any residuals, the leaky ReLUs (one IEEE f32 product v * slope) with at most one.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_bits_equal, assert_exact_headroom, int_tensor

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float32
NONE, RELU, LRELU01, LRELU02 = 0, 1, 2, 5


def _ops():
    from flair_amd import ops
    return ops


def _name(dtype):
    return "bf16" if dtype == BF else "f32"


def act_f32(v, act):
    """The activation in f32, one IEEE product for the leaky slopes (= F.leaky_relu = the kernels' fmaxf(v, v * slope))."""
    assert v.dtype == FP
    if act == NONE:
        return v
    if act == RELU:
        return torch.relu(v)
    slope = torch.tensor({LRELU01: 0.1, LRELU02: 0.2}[act], dtype=FP)
    return torch.where(v > 0, v, v * slope)


def epilogue_f32(conv, bias, fb, act, res, scale):
    """conv: exact f32 (T, C, H, W); -> f32 (act(conv + bias + frame_bias) + res0 + res1) * out_scale."""
    add = bias.view(1, -1, 1, 1)
    if fb is not None:
        add = add + fb[:, :conv.shape[1], None, None]       # integers: exact, in either association
    v = act_f32(conv + add, act)
    for r in res:
        v = v + r
    return v * torch.tensor(scale, dtype=FP)


def unrepresentable_share(pre, dtype):
    """Share of the f32 values that the cast to `dtype` changes."""
    return (pre.to(dtype).float() != pre).float().mean().item()


def assert_rounding_exercised(pre, dtype, what, least=0.05):
    if dtype == BF:
        s = unrepresentable_share(pre, dtype)
        assert s >= least, f"{what}: only {100 * s:.1f} % of the outputs need rounding to bf16 (want >= {100 * least:.0f} %)"


def nhwc(t, dtype, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


def conv64(x, w, k, *, stride=1, asym_pad=False, reflect_pad=False):
    """float64 convolution of (T, Cin, H, W) with (Cout, Cin, *k), the padding rules of flair_conv_nhwc."""
    if reflect_pad:
        return F.conv2d(F.pad(x, (k[2] // 2,) * 2 + (k[1] // 2,) * 2, mode="reflect"), w[:, :, 0])
    if asym_pad:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w[:, :, 0], stride=2)
    if k[0] == 1:
        return F.conv2d(x, w[:, :, 0], padding=(k[1] // 2, k[2] // 2), stride=stride)
    return F.conv3d(x.permute(1, 0, 2, 3)[None], w, padding=tuple(v // 2 for v in k))[0].permute(1, 0, 2, 3)


# ------------------------------------------------------------------------------------------------ flair_conv_nhwc
@functools.lru_cache(maxsize=2)
def conv_data(T, H, W, segs, cout, k, R, stride=1, asym_pad=False, reflect_pad=False):
    """Integer data of one geometry and its exact convolution, shared by the dtypes and epilogues run on it (read only):
    x, w, bias, two residuals, a frame bias 4 columns wider than Cout, conv (f32, exact) and conv(|x|, |w|) (f64)."""
    g = torch.Generator().manual_seed(T * 1009 + H * 31 + W * 7 + cout * 3 + sum(segs) + k[0] + 5 * k[1] + stride + R)
    cin = sum(segs)
    x = int_tensor((T, cin, H, W), -R, R, g)
    w = int_tensor((cout, cin, *k), -3, 3, g)
    bias = int_tensor((cout,), -8, 8, g)
    kw = dict(stride=stride, asym_pad=asym_pad, reflect_pad=reflect_pad)
    conv = conv64(x.double(), w.double(), k, **kw)
    mag = conv64(x.double().abs(), w.double().abs(), k, **kw)
    res = [int_tensor(conv.shape, -64, 64, g) for _ in range(2)]
    fb = int_tensor((T, cout + 4), -8, 8, g)
    assert_exact_headroom(mag)
    return dict(x=x, w=w, bias=bias, res=res, fb=fb, conv=conv.float(), mag=mag)


def C(T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, **ex):
    return (T, H, W, tuple(segs), cout, k, act, nres, R, scale, bf, fp, ex)


# T, H, W, segs, cout, kernel, act, residuals, R, out_scale, variant reached in bf16, in f32 (None: not run in f32), extras
CONV_EXACT = [
    # ---- variants 0..2, im2col.  Geometries of test_gpu_strides.CONV_CASES (K deepened where 64 products of +-16 * +-3
    # leave bf16 nothing to round), then what that list does not cross
    C(1, 256, 256, [96, 32], 72, (1, 1, 1), RELU, 2, 16, 0.5, 0, 0),             # 128 x 128 tiles, bf16 32-channel K step
    C(1, 256, 256, [32, 32], 64, (1, 1, 1), LRELU01, 1, 16, 2.0, 1, 1),          # 64 x 128 tiles
    C(2, 16, 16, [32, 32], 64, (1, 3, 3), LRELU01, 1, 8, 0.5, 2, 2),             # 64 x 64 tiles
    C(2, 16, 16, [64, 128], 64, (1, 3, 3), NONE, 0, 8, 1.0, 2, 2),               # bf16 64-channel K step (launch_pd<.., 2, 2>)
    C(2, 16, 16, [96, 32], 64, (1, 3, 3), RELU, 1, 8, 2.0, 2, 2),                # bf16 32-channel K step, a 96-channel segment
    C(8, 16, 16, [256], 256, (3, 3, 3), RELU, 1, 3, 0.5, 0, 0, splitk=True),     # split-K reduction: the deep-K geometries
    C(16, 8, 8, [256, 256], 384, (1, 3, 3), NONE, 2, 3, 1.0, 0, 0, splitk=True),
    C(16, 4, 4, [512], 512, (3, 3, 3), NONE, 1, 3, 2.0, 2, 2, splitk=True),
    C(1, 9, 7, [32], 16, (1, 7, 7), RELU, 0, 8, 1.0, 2, 2),                      # 7x7
    C(5, 6, 6, [64, 64], 8, (1, 1, 1), LRELU02, 1, 16, 0.5, 2, 2),               # 1x1 on few pixels
    C(2, 32, 64, [32, 32], 64, (1, 3, 3), LRELU01, 1, 8, 1.0, 2, 2, stride=2),
    C(2, 32, 32, [32, 32], 64, (1, 3, 3), NONE, 1, 8, 0.5, 2, 2, stride=2, asym_pad=True),
    C(2, 20, 24, [32, 32], 64, (1, 3, 3), RELU, 1, 8, 2.0, 2, 2, reflect_pad=True),
    C(5, 16, 16, [64], 64, (1, 3, 3), NONE, 0, 8, 1.0, 2, 2, frame_bias=True),
    # bf16 Cout = 4 (mod 8): the only outputs stored as 8-byte quads
    C(1, 256, 256, [96], 68, (1, 1, 1), NONE, 1, 16, 1.0, 0, None),
    C(1, 256, 256, [96], 36, (1, 1, 1), LRELU01, 1, 16, 0.5, 1, None),
    C(2, 16, 16, [32], 36, (1, 3, 3), RELU, 2, 16, 2.0, 2, None),
    # ---- variants 3..7, halo and K-split kernels (8 / 4 / 2 rows; the last row of tiles of 250 and 125 rows hangs over)
    C(4, 136, 128, [32, 32], 8, (1, 3, 3), NONE, 1, 8, 0.5, 3, 3),
    C(2, 136, 128, [32, 32], 8, (1, 3, 3), LRELU01, 1, 8, 2.0, 4, 4),
    C(3, 30, 32, [32, 32, 32], 64, (3, 3, 3), RELU, 2, 8, 0.5, 5, 5),
    C(1, 250, 256, [32, 32], 8, (1, 3, 3), NONE, 2, 8, 1.0, 6, 6),
    C(1, 125, 128, [32, 32], 72, (1, 3, 3), LRELU02, 1, 8, 0.5, 7, 7),
    C(1, 128, 128, [128], 128, (1, 3, 3), RELU, 1, 8, 1.0, 7, 7, frame_bias=True),
    C(1, 256, 256, [32], 36, (1, 3, 3), RELU, 1, 16, 0.5, 3, None),
    C(1, 256, 128, [32], 36, (1, 3, 3), NONE, 2, 8, 2.0, 4, None),
    C(2, 16, 32, [32], 36, (1, 3, 3), LRELU01, 1, 8, 1.0, 5, None),
    C(2, 16, 32, [32], 68, (1, 3, 3), NONE, 0, 8, 0.5, 5, None),
    # ---- variant 8, persistent LDS-DMA kernel (bf16).  Every copy of its epilogue (conv.hip, epilogue_as): ACT == 0 with
    # slope 1 and out_scale != 1, slope 0, slope 0.1; ACT == 3 (no activation, out_scale == 1) with and without residual;
    # HASRES with res0 only and with res0 + res1 -- spread over temporal taps at the clip edges and 1.5 tiles per
    # workgroup, 64-channel chunks, and 8 couts (half of each 16-cout store group is padding)
    C(6, 64, 128, [32, 32], 128, (3, 3, 3), NONE, 2, 8, 0.5, 8, None),
    C(6, 64, 128, [32, 32], 128, (3, 3, 3), RELU, 0, 8, 2.0, 8, None),
    C(4, 128, 128, [64], 128, (1, 3, 3), NONE, 1, 8, 1.0, 8, None),
    C(4, 128, 128, [64], 128, (1, 3, 3), NONE, 0, 8, 1.0, 8, None),
    C(4, 128, 128, [64], 128, (1, 3, 3), RELU, 0, 8, 1.0, 8, None, frame_bias=True),
    C(3, 256, 256, [32], 8, (1, 3, 3), LRELU01, 1, 8, 0.5, 8, None),
    C(3, 256, 256, [32], 8, (1, 3, 3), NONE, 2, 8, 1.0, 8, None),
    # ---- variant 9 (bf16): conv_frame_kernel (256^2, Cout <= 64, padded couts) and conv3x3_dma_kernel<8, 1, 2> (Cout = 128,
    # or a frame bias), each with 0, 1 and 2 residuals
    C(1, 256, 256, [32], 64, (1, 3, 3), RELU, 0, 16, 0.5, 9, None, frame=True),
    C(1, 256, 256, [32], 64, (1, 3, 3), LRELU01, 1, 16, 2.0, 9, None, frame=True),
    C(1, 256, 256, [32], 64, (1, 3, 3), NONE, 2, 16, 1.0, 9, None, frame=True),
    C(1, 256, 256, [32], 24, (1, 3, 3), NONE, 2, 8, 0.5, 9, None, frame=True),
    C(1, 128, 256, [32], 128, (1, 3, 3), NONE, 0, 16, 1.0, 9, None, frame=False),
    C(1, 128, 256, [32], 128, (1, 3, 3), LRELU02, 1, 16, 0.5, 9, None, frame=False),
    C(1, 128, 256, [32], 128, (1, 3, 3), RELU, 2, 16, 2.0, 9, None, frame=False),
    C(1, 256, 256, [64], 64, (1, 3, 3), NONE, 1, 8, 1.0, 9, None, frame=False, frame_bias=True),
]
CONV_RUNS = [(dt, c) for c in CONV_EXACT for dt in (BF, FP) if dt == BF or c[11] is not None]


def frame_kernel_takes(case):
    """conv.hip's frame_kernel_ok for the variant-9 cases here (bf16, 3x3, stride 1, segments of 32 k channels, plain acts)."""
    T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, ex = case
    return not ex.get("frame_bias") and cout <= 64 and cout % 8 == 0 and W % 32 == 0 and H % 8 == 0


def _conv_id(v):
    if isinstance(v, torch.dtype):
        return _name(v)
    T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, ex = v
    return (f"v{bf}-{T}x{H}x{W}-{'+'.join(map(str, segs))}-o{cout}-k{''.join(map(str, k))}-a{act}-r{nres}-s{scale}"
            + "".join(f"-{n}" for n in sorted(ex) if ex[n] is True and n != "frame"))


def conv_reference(case, dtype):
    """-> (data, fb or None, residual list, f32 value before the cast, reference in dtype (T, C, H, W))."""
    T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, ex = case
    assert act in (NONE, RELU) or nres <= 1, "a leaky ReLU with two residuals adds two inexact values: order dependent"
    d = conv_data(T, H, W, segs, cout, k, R, ex.get("stride", 1), ex.get("asym_pad", False), ex.get("reflect_pad", False))
    fb = d["fb"] if ex.get("frame_bias") else None
    res = d["res"][:nres]
    mag = d["mag"] + d["bias"].abs().double().view(1, -1, 1, 1)
    if fb is not None:
        mag = mag + fb[:, :cout, None, None].abs().double()
    for r in res:
        mag = mag + r.abs().double()
    assert_exact_headroom(mag)
    pre = epilogue_f32(d["conv"], d["bias"], fb, act, res, scale)
    assert_rounding_exercised(pre, dtype, f"conv {_conv_id(case)}")
    return d, fb, res, pre, pre.to(dtype)


def test_conv_exact_cases_reach_every_variant():
    """Each case is listed under the variant flair_conv_variant gives it; bf16 reaches 0..9, f32 0..7; variant 9 runs on
    conv_frame_kernel and on conv3x3_dma_kernel<8, 1, 2>; the split-K cases do split."""
    ops = _ops()
    for dtype, col in ((BF, 10), (FP, 11)):
        seen = set()
        for c in CONV_EXACT:
            if c[col] is None:
                continue
            T, H, W, segs, cout, k = c[:6]
            v = ops.conv_variant(T, H, W, list(segs), cout, k, dtype=dtype, stride=c[12].get("stride", 1))
            assert v == c[col], (_conv_id(c), dtype, v)
            seen.add(v)
        assert seen == set(range(10) if dtype == BF else range(8)), (dtype, seen)
    assert {frame_kernel_takes(c) for c in CONV_EXACT if c[10] == 9} == {True, False}
    for c in CONV_EXACT:
        if c[10] == 9:
            assert frame_kernel_takes(c) == c[12]["frame"], _conv_id(c)


@pytest.mark.parametrize("dtype,case", CONV_RUNS, ids=_conv_id)
def test_conv_exact(dev, dtype, case):
    ops = _ops()
    T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, ex = case
    stride = ex.get("stride", 1)
    assert ops.conv_variant(T, H, W, list(segs), cout, k, dtype=dtype, stride=stride) == (bf if dtype == BF else fp)
    d, fb, res, pre, ref = conv_reference(case, dtype)
    xs, o = [], 0
    for c in segs:
        xs.append(nhwc(d["x"][:, o:o + c], dtype, dev))
        o += c
    wp = ops.pack_conv_weight(d["w"], [(c, c) for c in segs], dtype).to(dev)
    rs = [nhwc(r, dtype, dev) for r in res] + [None, None]
    if ex.get("splitk"):
        p = ops.ConvParams()
        p.dtype = 1 if dtype == BF else 0
        p.T, p.H, p.W = T, H, W
        p.KT, p.KH, p.KW = k
        p.Cout, p.nseg, p.stride, p.y_ld = cout, len(segs), 1, cout
        for i, c in enumerate(segs):
            p.seg_c[i] = p.seg_ld[i] = c
        assert ops._conv_ws_bytes(p) > 0, "the deep-K geometry no longer splits K"
    y = ops.conv(xs, wp, d["bias"].to(dev), cout, k, act=act, res0=rs[0], res1=rs[1], out_scale=scale, stride=stride,
                 frame_bias=fb.to(dev) if fb is not None else None, asym_pad=ex.get("asym_pad", False),
                 reflect_pad=ex.get("reflect_pad", False))
    torch.cuda.synchronize()
    rows = {3: 8, 4: 4, 5: 2, 6: 8, 7: 4, 8: 16, 9: 8}.get(bf if dtype == BF else fp, 8)
    assert_bits_equal(y.cpu(), ref.permute(0, 2, 3, 1).contiguous(), f"conv {_conv_id(case)} {_name(dtype)}",
                      tile=(rows, 32, min(64, cout)))


def test_conv_exact_sees_one_wrong_weight(dev):
    """The comparison is as sharp on the GPU as tests/test_exact_cpu.py shows it to be on the CPU: the kernel run with ONE
    weight off by one, of 64 * 9 * 64, fails it, and the tile histogram names the cout."""
    ops = _ops()
    case = C(2, 16, 16, [32, 32], 64, (1, 3, 3), NONE, 1, 8, 0.5, 2, 2)
    T, H, W, segs, cout, k, act, nres, R, scale, bf, fp, ex = case
    d, fb, res, pre, ref = conv_reference(case, BF)
    w = d["w"].clone()
    w[37, 11, 0, 2, 1] += 1.0
    xs = [nhwc(d["x"][:, :32], BF, dev), nhwc(d["x"][:, 32:], BF, dev)]
    wp = ops.pack_conv_weight(w, [(32, 32), (32, 32)], BF).to(dev)
    y = ops.conv(xs, wp, d["bias"].to(dev), cout, k, act=act, res0=nhwc(res[0], BF, dev), out_scale=scale)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="differ in bits") as e:
        assert_bits_equal(y.cpu(), ref.permute(0, 2, 3, 1).contiguous(), "one wrong weight", tile=(8, 32, 64))
    hist = [int(v) for v in str(e.value).split("by c % 64: [")[1].split("]")[0].split(",")]
    assert hist[37] > 0 and sum(hist) == hist[37], hist


# ------------------------------------------------------------------------------------------------ flair_conv_chain
# T, H, W, segs (None: no stage A), c_mid, coutB, actA, actB, residuals, out_scale
CHAIN_EXACT = [
    (1, 64, 64, None, 64, 72, NONE, RELU, 0, 0.5),         # conv_resident_kernel (bf16; takes no residuals)
    (1, 64, 64, (64,), 64, 64, RELU, NONE, 2, 0.5),        # conv_pair_kernel (bf16), both residuals
    (2, 32, 32, (64, 32), 64, 64, RELU, LRELU01, 1, 2.0),  # general chain, c = 64; leaky ReLU with its one residual
    (1, 32, 64, (128,), 128, 128, RELU, NONE, 2, 1.0),     # general chain, c = 128
    (1, 20, 32, None, 128, 72, NONE, RELU, 1, 0.5),        # no stage A at c = 128; tiles hang over the image bottom
    (1, 8, 32, (64,), 64, 64, NONE, RELU, 1, 2.0),         # one tile: every border of the halo and of the intermediate is padding
    (2, 20, 40, (64,), 64, 64, RELU, NONE, 2, 0.5),        # W % 32 != 0, tiles hang over the bottom
]


@functools.lru_cache(maxsize=2)
def chain_data(T, H, W, segs, cm, coutB):
    g = torch.Generator().manual_seed(T * 977 + H * 13 + W + coutB + cm)
    cin = sum(segs) if segs else cm
    R = 3 if segs else 16      # one stage of K = 9 c products of +-3 * +-3 stays within bf16's 8 bits: a wider input there
    d = dict(x=int_tensor((T, cin, H, W), -R, R, g), wB=int_tensor((coutB, cm, 3, 3), -3, 3, g),
             bB=int_tensor((coutB,), -8, 8, g), res=[int_tensor((T, coutB, H, W), -64, 64, g) for _ in range(2)])
    if segs:
        d["wA"] = int_tensor((cm, cin, 3, 3), -3, 3, g)
        d["bA"] = int_tensor((cm,), -8, 8, g)
        d["convA"] = F.conv2d(d["x"].double(), d["wA"].double(), padding=1).float()
        d["magA"] = F.conv2d(d["x"].double().abs(), d["wA"].double().abs(), padding=1) + d["bA"].abs().double().view(1, -1, 1, 1)
        assert_exact_headroom(d["magA"])
    return d


def chain_reference(case, dtype):
    """The intermediate is act_A(conv_A + bias_A) in f32 cast with .to(dtype): an integer after RNE, so stage B is exact again."""
    T, H, W, segs, cm, coutB, actA, actB, nres, scale = case
    assert actA in (NONE, RELU) and (actB in (NONE, RELU) or nres <= 1)
    d = chain_data(T, H, W, segs, cm, coutB)
    if segs:
        mid = act_f32(d["convA"] + d["bA"].view(1, -1, 1, 1), actA).to(dtype).float()
    else:
        mid = d["x"]
    res = d["res"][:nres]
    convB = F.conv2d(mid.double(), d["wB"].double(), padding=1)
    mag = F.conv2d(mid.double().abs(), d["wB"].double().abs(), padding=1) + d["bB"].abs().double().view(1, -1, 1, 1)
    for r in res:
        mag = mag + r.abs().double()
    assert_exact_headroom(mag)
    pre = epilogue_f32(convB.float(), d["bB"], None, actB, res, scale)
    assert_rounding_exercised(pre, dtype, f"conv_chain {case}")
    return d, res, pre.to(dtype)


@pytest.mark.parametrize("dtype", [BF, FP], ids=_name)
@pytest.mark.parametrize("case", CHAIN_EXACT, ids=lambda c: "-".join(str(v) for v in c).replace(" ", ""))
def test_conv_chain_exact(dev, dtype, case):
    ops = _ops()
    T, H, W, segs, cm, coutB, actA, actB, nres, scale = case
    d, res, ref = chain_reference(case, dtype)
    xs, o = [], 0
    for c in (segs or (cm,)):
        xs.append(nhwc(d["x"][:, o:o + c], dtype, dev))
        o += c
    wAp = ops.pack_conv_weight(d["wA"][:, :, None], [(c, c) for c in segs], dtype).to(dev) if segs else None
    wBp = ops.pack_conv_weight(d["wB"][:, :, None], [(cm, cm)], dtype).to(dev)
    rs = [nhwc(r, dtype, dev) for r in res] + [None, None]
    # 8 channels wider than needed (conv_resident_kernel's store groups are 16 couts wide): the pad channels stay untouched
    out = torch.full((T, H, W, coutB + 8), 7.0, dtype=dtype, device=dev)
    ops.conv_chain(xs, wAp, d["bA"].to(dev) if segs else None, actA, wBp, d["bB"].to(dev), actB, cm, coutB,
                   res0=rs[0], res1=rs[1], out_scale=scale, out=out)
    torch.cuda.synchronize()
    assert torch.all(out[..., coutB:] == 7.0), "pad channels of the output buffer were written"
    assert_bits_equal(out[..., :coutB].cpu(), ref.permute(0, 2, 3, 1).contiguous(), f"conv_chain {case} {_name(dtype)}",
                      tile=(8, 32 if W % 32 == 0 else 8, 64))


# ------------------------------------------------------------------------------------------------ flair_dcn_align
def dcn_gather_ref(x, offset, mask, w, b, G):
    """Modulated deformable 3x3 convolution (stride 1, padding 1, dilation 1) for INTEGER sampling positions, float64:
    the bilinear weights are {1, 0, 0, 0}, so each (pixel, tap, group) sample is x at one integer position, or 0 outside
    the image, times the mask -- a gathered integer convolution with no inexact step (a grid_sample formulation
    normalises the positions inexactly even in float64).
    x (N, C, H, W); offset (N, 2 * G * 9, H, W), channel 2 * (g * 9 + k) the row and + 1 the column displacement;
    mask (N, G * 9, H, W); w (Cout, C, 3, 3); b (Cout,) or None.
    -> (out (N, Cout, H, W), inside (N, G, 9, H, W) bool, numbers of samples exactly on row -1, row H, column -1, column W)."""
    N, Cin, H, W = x.shape
    cpg = Cin // G
    x, w = x.double(), w.double()
    off = offset.double().view(N, G, 9, 2, H, W)
    assert torch.equal(off, off.round()), "integer sampling positions only"
    msk = mask.double().view(N, G, 9, H, W)
    hh = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    ww = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    xp = F.pad(x, (1, 1, 1, 1)).reshape(N, Cin, (H + 2) * (W + 2))           # the frame with a border of zeros
    out = torch.zeros(N, w.shape[0], H * W, dtype=torch.float64)
    inside = torch.empty(N, G, 9, H, W, dtype=torch.bool)
    edge = [0, 0, 0, 0]
    for k in range(9):
        i, j = divmod(k, 3)
        py = hh - 1 + i + off[:, :, k, 0]                                    # (N, G, H, W)
        px = ww - 1 + j + off[:, :, k, 1]
        ok = (py >= 0) & (py <= H - 1) & (px >= 0) & (px <= W - 1)
        inside[:, :, k] = ok
        for n, hit in enumerate((py == -1, py == H, px == -1, px == W)):
            edge[n] += int(hit.sum())
        idx = ((py.clamp(-1, H) + 1) * (W + 2) + px.clamp(-1, W) + 1).long()
        idx = idx.repeat_interleave(cpg, dim=1).reshape(N, Cin, H * W)
        m = (ok.double() * msk[:, :, k]).repeat_interleave(cpg, dim=1).reshape(N, Cin, H * W)
        col = torch.gather(xp, 2, idx) * m
        out += torch.einsum("oc,ncp->nop", w[:, :, i, j], col)
    if b is not None:
        out += b.double().view(1, -1, 1)
    return out.view(N, -1, H, W), inside, tuple(edge)


def dcn_activated_cases():
    from tests.test_gpu_strides import DCN_CASES
    return [c for c in DCN_CASES if c[7]]


def dcn_int_data(case):
    """Integer offsets in [-4, 4], integer flows in [-3, 3], masks in {0, 0.5, 1}, w in [-3, 3], bias in [-8, 8]."""
    dtype, Fr, H, W, half, cout, G, _ = case
    g = torch.Generator().manual_seed(21 + half + cout + H + Fr)
    # x in [-3, 3] at K = 9 * 256; at K = 9 * 128, where the sums of +-3 * +-3 * mask products on a small frame (two samples in
    # five outside) seldom leave bf16's 8 bits, in [-8, 8] (x * mask is still exact in bf16)
    R = 3 if half == 128 else 8
    x = int_tensor((Fr, 2 * half, H, W), -R, R, g)
    w = int_tensor((cout, 2 * half, 3, 3), -3, 3, g)
    b = int_tensor((cout,), -8, 8, g)
    offset = int_tensor((Fr, 18 * G, H, W), -4, 4, g)                        # the reference's order (o1 | o2), (g * 9 + k) * 2 + (y, x)
    mask = int_tensor((Fr, 9 * G, H, W), 0, 2, g) * 0.5
    f1 = int_tensor((Fr, H, W, 2), -3, 3, g)
    f2 = int_tensor((Fr, H, W, 2), -3, 3, g)
    return x, w, b, offset, mask, f1, f2


def dcn_total_offset(offset, f1, f2):
    """Residues plus flows: groups of the first input half take flow1, the others flow2 (flow channel 0 is x, 1 is y)."""
    off1, off2 = offset.chunk(2, dim=1)
    off1 = off1 + f1.permute(0, 3, 1, 2).flip(1).repeat(1, off1.shape[1] // 2, 1, 1)
    off2 = off2 + f2.permute(0, 3, 1, 2).flip(1).repeat(1, off2.shape[1] // 2, 1, 1)
    return torch.cat([off1, off2], dim=1)


# Share of the (pixel, tap, group) samples that must fall outside the image.  A displacement is offset + flow + tap:
# uniform integers in [-4, 4], [-3, 3] and [-1, 1], mean |d| = 2.74 pixels, so about 2.74 / H + 2.74 / W of the samples
# leave an H x W frame: 20 % .. 50 % of the frames of up to 16 x 32 pixels, where 10 % is asserted; 6.4 % at 64 x 128,
# 4.8 % at 121 x 109 and 4.3 % at 128 x 128, which these ranges cannot raise to 10 %: there 3 % (tens of thousands of
# samples), with every edge crossed and the positions -1, H and W hit exactly.
def dcn_outside_floor(H, W):
    return 0.10 if H * W <= 16 * 32 else 0.03


@pytest.mark.parametrize("case", dcn_activated_cases(),
                         ids=lambda c: f"{_name(c[0])}-{c[1]}x{c[2]}x{c[3]}-h{c[4]}-o{c[5]}-G{c[6]}")
def test_dcn_exact(dev, case):
    """flair_dcn_align, raw_activated = 1, every activated instantiation (ONEFRAME with its dot2 blend in bf16, and
    batched): with integer positions the blend weights are {mask, 0, 0, 0} in f32 and in bf16 alike (0, 0.5, 1), so the
    output is a gathered integer convolution -- compared bit for bit on every frame."""
    ops = _ops()
    dtype, Fr, H, W, half, cout, G, _ = case
    x, w, b, offset, mask, f1, f2 = dcn_int_data(case)
    ref, inside, edge = dcn_gather_ref(x, dcn_total_offset(offset, f1, f2), mask, w, b, G)
    share = inside.float().mean().item()
    print(f"dcn {case[1:]} {_name(dtype)}: {100 * (1 - share):.1f} % of the samples outside; on row -1, row H, column -1, column W: {edge}")
    assert 1 - share >= dcn_outside_floor(H, W) and share >= 0.10 and min(edge) > 0, (1 - share, share, edge)
    mag, _, _ = dcn_gather_ref(x.abs(), dcn_total_offset(offset, f1, f2), mask, w.abs(), b.abs(), G)
    assert_exact_headroom(mag)
    pre = ref.float()
    assert torch.equal(pre.double(), ref)
    assert_rounding_exercised(pre, dtype, f"dcn {case}")
    raw = torch.cat([offset, mask], dim=1)[:, ops.dcn_raw_permutation(G)]
    wp = ops.pack_conv_weight(w, [(2 * half, 2 * half)], dtype).to(dev)
    y = ops.dcn_align(nhwc(x[:, :half], dtype, dev), nhwc(x[:, half:], dtype, dev), nhwc(raw, dtype, dev), f1.to(dev),
                      f2.to(dev), wp, b.to(dev), cout, groups=G, raw_activated=True)
    torch.cuda.synchronize()
    assert_bits_equal(y.cpu(), pre.to(dtype).permute(0, 2, 3, 1).contiguous(), f"dcn {case}", tile=(1, 32, 32))


def test_dcn_exact_sees_one_wrong_offset(dev):
    """One residue of one (pixel, tap, group) off by one pixel, of 2 * 11 * 13 * 9 * 8 samples, fails the comparison."""
    ops = _ops()
    case = (BF, 2, 11, 13, 64, 32, 8, True)
    dtype, Fr, H, W, half, cout, G, _ = case
    x, w, b, offset, mask, f1, f2 = dcn_int_data(case)
    mask[1, 3 * 9 + 4, 5, 6] = 1.0                                           # group 3, centre tap, pixel (5, 6) of frame 1: inside
    offset[1, 2 * (3 * 9 + 4)] = 0.0
    offset[1, 2 * (3 * 9 + 4) + 1] = 0.0
    f1[1] = 0.0
    ref, _, _ = dcn_gather_ref(x, dcn_total_offset(offset, f1, f2), mask, w, b, G)
    wrong = offset.clone()
    wrong[1, 2 * (3 * 9 + 4) + 1, 5, 6] = 1.0
    wp = ops.pack_conv_weight(w, [(2 * half, 2 * half)], dtype).to(dev)
    outs = []
    for off in (offset, wrong):
        raw = torch.cat([off, mask], dim=1)[:, ops.dcn_raw_permutation(G)]
        outs.append(ops.dcn_align(nhwc(x[:, :half], dtype, dev), nhwc(x[:, half:], dtype, dev), nhwc(raw, dtype, dev),
                                  f1.to(dev), f2.to(dev), wp, b.to(dev), cout, groups=G, raw_activated=True).cpu())
    torch.cuda.synchronize()
    want = ref.float().to(dtype).permute(0, 2, 3, 1).contiguous()
    assert_bits_equal(outs[0], want, "right offsets")
    assert not torch.equal(x[1, 48:64, 5, 6], x[1, 48:64, 5, 7])             # group 3 = channels [48, 64): the two positions differ
    with pytest.raises(AssertionError, match="first at \\[1, 5, 6, "):
        assert_bits_equal(outs[1], want, "one wrong offset")


# ------------------------------------------------------------------------------------------------ depthwise kernels
@pytest.mark.parametrize("dtype", [FP, BF], ids=_name)
@pytest.mark.parametrize("shape", [(2, 9, 13, 32), (1, 16, 16, 64)])
def test_dwconv7_exact(dev, dtype, shape):
    """Depthwise 7x7 with integer taps in [-3, 3] on x in [-16, 16], into a channel slice of a wider output.  49 products
    of up to 48: about 3 % of the sums leave bf16's 8 bits (at least 1 % asserted)."""
    ops = _ops()
    T, H, W, Cc = shape
    g = torch.Generator().manual_seed(H * W + Cc)
    x = int_tensor((T, Cc, H, W), -16, 16, g)
    w = int_tensor((Cc, 1, 7, 7), -3, 3, g)
    b = int_tensor((Cc,), -8, 8, g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=3, groups=Cc)
    assert_exact_headroom(F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=3, groups=Cc))
    pre = ref.float()
    assert_rounding_exercised(pre, dtype, f"dwconv7 {shape}", least=0.01)
    out = torch.full((T, H, W, Cc + 16), 7.0, dtype=dtype, device=dev)
    ops.dwconv7(nhwc(x, dtype, dev), w.reshape(Cc, 49).t().contiguous().to(dev), b.to(dev), out=out[..., 8:8 + Cc])
    torch.cuda.synchronize()
    assert (out[..., :8] == 7.0).all() and (out[..., 8 + Cc:] == 7.0).all()
    assert_bits_equal(out[..., 8:8 + Cc].cpu(), pre.to(dtype).permute(0, 2, 3, 1).contiguous(), f"dwconv7 {shape} {_name(dtype)}")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pw", [False, True], ids=["dw", "dw+pw"])
@pytest.mark.parametrize("shape", [(2, 9, 11, 16), (1, 16, 16, 32)])
def test_dwconv_exact(dev, stride, pw, shape):
    """MobileNet depthwise 3x3 (+ fused 1x1 onto 24 channels) in f32 with ReLU, so that the intermediate stays an integer."""
    ops = _ops()
    T, H, W, Cc = shape
    cout = 24
    g = torch.Generator().manual_seed(10 + stride + Cc)
    x = int_tensor((T, Cc, H, W), -8, 8, g)
    w_dw = int_tensor((9, Cc), -3, 3, g)
    b_dw = int_tensor((Cc,), -8, 8, g)
    w_pw = int_tensor((cout, Cc), -3, 3, g)
    b_pw = int_tensor((cout,), -8, 8, g)
    wd = w_dw.double().t().reshape(Cc, 1, 3, 3)
    ref = torch.relu(F.conv2d(x.double(), wd, b_dw.double(), stride=stride, padding=1, groups=Cc))
    mag = F.conv2d(x.double().abs(), wd.abs(), b_dw.double().abs(), stride=stride, padding=1, groups=Cc)
    assert_exact_headroom(mag)
    if pw:
        assert_exact_headroom(F.conv2d(ref, w_pw.double().abs()[:, :, None, None], b_pw.double().abs()))
        ref = torch.relu(F.conv2d(ref, w_pw.double()[:, :, None, None], b_pw.double()))
    co = cout if pw else Cc
    out = torch.full((T, ref.shape[2], ref.shape[3], co + 8), 7.0, dtype=FP, device=dev)
    ops.dwconv(nhwc(x, FP, dev), w_dw.to(dev), b_dw.to(dev), stride=stride, pw=(w_pw.to(dev), b_pw.to(dev)) if pw else None,
               act=ops.ACT_RELU, out=out[..., 4:4 + co])
    torch.cuda.synchronize()
    assert (out[..., :4] == 7.0).all() and (out[..., 4 + co:] == 7.0).all()
    assert_bits_equal(out[..., 4:4 + co].cpu(), ref.float().permute(0, 2, 3, 1).contiguous(), f"dwconv {shape} s{stride} pw={pw}")
