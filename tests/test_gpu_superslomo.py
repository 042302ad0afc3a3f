"""SuperSloMo frame interpolation on the GPU: the two entries of slomo.hip against a float64 closed form (dense and on strided
channel views with guarded neighbours), bit for bit on half-pixel cases and with a saturated visibility map; the network
against the reference's own output (tests/golden/g17_superslomo.npz); the convolution geometries the network adds, bit for
bit on integer data; bf16; the files and the command line."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import superslomo_cpu as sc
from tests.test_gpu_exact import C, LRELU01, conv_reference, nhwc
from tests.test_gpu_strides import run_both
from tests.test_superslomo_cpu import GOLD, compare
from tests.util import IN_FILL, OUT_FILL, assert_bits_equal, assert_untouched, guarded, rb

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float32
SHAPES = [(2, 9, 11), (1, 32, 32), (1, 5, 40)]
# (k, factor) of the coefficients a case runs with: the midpoint and a late, asymmetric timestep
TIMES = {(2, 9, 11): (1, 2), (1, 32, 32): (3, 4), (1, 5, 40): (1, 3)}


def _ops():
    from flair_amd import ops
    return ops


def _g(dtype):
    return 16 // torch.tensor([], dtype=dtype).element_size()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def clip(t):
    return t.permute(0, 2, 3, 1)


def outside_share(flows):
    """Share of the samples of back_warp(., flow), over all the given (B, 2, H, W) flows, with a corner outside the frame."""
    n = hit = 0
    for fl in flows:
        H, W = fl.shape[2:]
        x0 = (torch.arange(W).view(1, 1, W) + fl[:, 0].double() - 0.5).floor()
        y0 = (torch.arange(H).view(1, H, 1) + fl[:, 1].double() - 0.5).floor()
        out = (x0 < 0) | (x0 + 1 > W - 1) | (y0 < 0) | (y0 + 1 > H - 1)
        n, hit = n + out.numel(), hit + int(out.sum())
    return hit / n


@functools.lru_cache(maxsize=None)
def kernel_data(shape, dtype):
    """Inputs of one shape, rounded through dtype (read only), each 8 channels wide with NaN in the channels no entry may
    use: pair (6 channels, in the range of normalised frames), flows (4) and the interpolation UNet's output (5: flow
    residuals ~ N(0, 1.5 px), visibility logits ~ N(0, 2)).  The flows are ~ N(0, 2.5 px) / the largest coefficient, so
    that the warps of stage A move by up to ~ N(0, 2.5 px) and those of stage B, which add the residuals, by ~ N(0, 3 px)."""
    B, H, W = shape
    k, factor = TIMES[shape]
    t, coef = sc.coefficients(k, factor)
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W)
    pair, flow, io = (torch.full((B, H, W, 8), float("nan")) for _ in range(3))
    pair[..., :6] = rb(torch.rand(B, H, W, 6, generator=g) - 0.42, dtype)
    flow[..., :4] = rb(torch.randn(B, H, W, 4, generator=g) * (2.5 / max(abs(c) for c in coef)), dtype)
    io[..., :4] = rb(torch.randn(B, H, W, 4, generator=g) * 1.5, dtype)
    io[..., 4] = rb(torch.randn(B, H, W, generator=g) * 2.0, dtype)
    return dict(pair=pair, flow=flow, io=io, t=t, coef=coef)


def closed_form(d, io=None, prec=torch.float64):
    """Stage A and stage B of tests/superslomo_cpu.py on the data of kernel_data in ``prec`` -> (iy (B, H, W, 20), frame
    (B, 3, H, W) in [-1, 1], [ft0, ft1], [ft0f, ft1f])."""
    pair, flow = nchw(d["pair"]).to(prec), nchw(d["flow"]).to(prec)
    io = nchw(d["io"] if io is None else io).to(prec)
    i0, i1, f01, f10 = pair[:, :3], pair[:, 3:6], flow[:, :2], flow[:, 2:4]
    iy, ft0, ft1 = sc.stage_a(i0, i1, f01, f10, d["coef"])
    p, _, ft0f, ft1f = sc.stage_b(i0, i1, ft0, ft1, io, d["t"])
    return clip(iy).contiguous(), p, [ft0, ft1], [ft0f, ft1f]


# ------------------------------------------------------------------------------------------------ 1. the kernels
# Bound: 4 x the deviation of the same closed form evaluated in f32 ATen from its float64 evaluation on the same inputs
# (3e-7 .. 3e-6 here); the margin covers FMA contraction and summation order.  Measured on one MI355X, error / deviation:
#   stage A  f32 1.00, 1.00, 1.01 (9 x 11, 32 x 32, 5 x 40); bf16: within the output's rounding, worst error / bound 0.98, 0.99, 0.93
#   stage B  f32 1.00 on the three shapes, bf16 inputs 1.00 (the output is f32); saturated visibility 0.95 .. 1.00
# i.e. the kernels land on the f32 ATen result itself to within its last bits.  An error above 4 is a finding to explain,
# not a bound to raise.
@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_a_against_float64(dev, dtype, shape):
    ops = _ops()
    B, H, W = shape
    d = kernel_data(shape, dtype)
    ref, _, fts, _ = closed_form(d)
    share = outside_share(fts)
    assert 0.10 <= share <= 0.60, share
    dev32 = (closed_form(d, prec=torch.float32)[0].double() - ref).abs().max().item()
    assert dev32 > 0
    gv, oc = _g(dtype), ops.pad_channels(20, dtype)
    out = run_both(dev, {"pair": (d["pair"], dtype, gv, 8 + 2 * gv), "flow": (d["flow"], dtype, 2 * gv, 4 * gv)},
                   {"y": ((B, H, W, oc), dtype, gv, oc + 3 * gv)},
                   lambda pair, flow, y: ops.slomo_warp_pack(pair, flow, d["coef"], out=y), f"stage A {shape}")["y"]
    assert (out[..., 20:] == 0).all()                                           # pad channels come back as zero
    err = (out[..., :20] - ref).abs()
    bound = 4 * dev32 * (1 + 2.0 ** -8) + (ref.abs() * 2.0 ** -8 if dtype == BF else 0.0)
    print(f"stage A {shape} {dtype}: outside share {share:.2f}, f32-vs-f64 deviation {dev32:.2e}, "
          f"max err {err.max().item():.2e}, worst err / bound {(err / bound).max().item():.2f}")
    assert (err <= bound).all(), (err / bound).max().item()
    if dtype == FP:                                                             # the pass-through channels are copies
        assert torch.equal(out[..., :6].float(), d["pair"][..., :6]) and torch.equal(out[..., 6:10].float(), d["flow"][..., :4])


def run_stage_b(dev, d, dtype, io=None, what=""):
    """flair_slomo_blend dense and on guarded strided views -> (B, 3, H, W) f64 cpu.  The result goes to slot [:, 1] of a
    (B, 3, 3, H, W) tensor of sentinels: the strided output equals the dense one bit for bit, the other slots and every
    input buffer stay as they were."""
    ops = _ops()
    io = d["io"] if io is None else io
    B, H, W, _ = d["pair"].shape
    gv = _g(dtype)
    dense = torch.full((B, 3, H, W), OUT_FILL, dtype=FP, device=dev)
    ops.slomo_blend(d["pair"].to(dev, dtype), d["flow"].to(dev, dtype), io.to(dev, dtype), d["coef"], d["t"], dense)
    views = {}
    for name, t, coff, ld in (("pair", d["pair"], gv, 8 + 2 * gv), ("flow", d["flow"], 2 * gv, 4 * gv),
                              ("io", io, gv, 3 * gv)):
        buf, v = guarded(*t.shape, dtype, dev, coff=coff, ld=ld, fill=IN_FILL)
        v.copy_(t.to(dev, dtype))
        views[name] = (buf, v, buf.clone())
    slots = torch.full((B, 3, 3, H, W), OUT_FILL, dtype=FP, device=dev)
    ops.slomo_blend(views["pair"][1], views["flow"][1], views["io"][1], d["coef"], d["t"], slots[:, 1])
    torch.cuda.synchronize()
    assert_bits_equal(slots[:, 1].cpu(), dense.cpu(), f"{what}: slot output against the dense call")
    assert (slots[:, 0] == OUT_FILL).all() and (slots[:, 2] == OUT_FILL).all(), f"{what}: a neighbouring slot changed"
    for name, (buf, _, before) in views.items():
        assert_untouched(buf, before, None, f"{what}: input {name}")
    return dense.double().cpu()


@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_b_against_float64(dev, dtype, shape):
    d = kernel_data(shape, dtype)
    _, ref, _, ftf = closed_form(d)
    share = outside_share(ftf)
    assert 0.10 <= share <= 0.60, share
    dev32 = (closed_form(d, prec=torch.float32)[1].double() - ref).abs().max().item()
    assert dev32 > 0
    got = run_stage_b(dev, d, dtype, what=f"stage B {shape}")
    err = (got - ref).abs().max().item()
    print(f"stage B {shape} {dtype}: outside share {share:.2f}, f32-vs-f64 deviation {dev32:.2e}, max err {err:.2e}, "
          f"err / deviation {err / dev32:.2f} (bound 4)")
    assert err <= 4 * dev32, (err, dev32)                                        # the output is f32 in either mode


# ------------------------------------------------------------------------------------------------ 2. half-pixel cases
def four_neighbour_mean(img, flow):
    """img (B, 3, H, W) and integer flow (B, 2, H, W): the mean of the four pixels (y - 1 .. y, x - 1 .. x) + flow, zeros
    outside -- what back_warp gives for an integer flow (the sample sits half a pixel up-left), exact in f32."""
    B, _, H, W = img.shape
    out = torch.zeros_like(img)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for b in range(B):
        for dy in (-1, 0):
            for dx in (-1, 0):
                yy, xx = ys + flow[b, 1].long() + dy, xs + flow[b, 0].long() + dx
                ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                out[b] += torch.where(ok, img[b][:, yy.clamp(0, H - 1), xx.clamp(0, W - 1)], torch.zeros(()))
    return out * 0.25


@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("size", [16, 32])
@pytest.mark.parametrize("flows", ["zero", "integer"])
def test_stage_a_half_pixel_cases_bit_for_bit(dev, dtype, size, flows):
    """Powers of two: the coordinate round trip is exact and every weight is 1/4.  Fails if the half-pixel shift or the
    zeros rule is lost (align_corners=True would return the image itself for a zero flow)."""
    ops = _ops()
    B = 2
    g = torch.Generator().manual_seed(size + len(flows))
    pair = torch.randint(-8, 9, (B, size, size, 6), generator=g).float()
    flow = torch.zeros(B, size, size, 4) if flows == "zero" else torch.randint(-3, 4, (B, size, size, 4), generator=g).float()
    x = torch.zeros(B, size, size, 8, dtype=dtype, device=dev)
    x[..., :6] = pair.to(dev, dtype)
    fl = torch.zeros(B, size, size, 8, dtype=dtype, device=dev)
    fl[..., :4] = flow.to(dev, dtype)
    iy = ops.slomo_warp_pack(x, fl, [1.0, 0.0, 0.0, 1.0])                       # ft0 = f01, ft1 = f10
    want0 = four_neighbour_mean(nchw(pair[..., :3]), nchw(flow[..., :2]))
    want1 = four_neighbour_mean(nchw(pair[..., 3:]), nchw(flow[..., 2:]))
    assert (want0 != nchw(pair[..., :3])).float().mean().item() > 0.5           # the shift is visible in the data
    assert_bits_equal(iy[..., 17:20].cpu(), clip(want0).contiguous().to(dtype), f"warp(i0, ft0) {size} {flows}")
    assert_bits_equal(iy[..., 14:17].cpu(), clip(want1).contiguous().to(dtype), f"warp(i1, ft1) {size} {flows}")
    assert_bits_equal(iy[..., 10:12].cpu(), flow[..., 2:].to(dtype), "ft1")
    assert_bits_equal(iy[..., 12:14].cpu(), flow[..., :2].to(dtype), "ft0")


# ------------------------------------------------------------------------------------------------ 3. saturated visibility
@pytest.mark.parametrize("sign", [100.0, -100.0])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_stage_b_saturated_visibility(dev, shape, sign):
    """io[4] = +-100: sigmoid is 1 or 0 (exp(100) overflows f32), the blend's divisor keeps one term, and the output is the
    de-normalised warp of the one visible frame."""
    d = kernel_data(shape, FP)
    io = d["io"].clone()
    io[..., 4] = sign
    pair = nchw(d["pair"]).double()
    _, ref, _, ftf = closed_form(d, io=io)
    one = sc.back_warp(pair[:, :3], ftf[0]) if sign > 0 else sc.back_warp(pair[:, 3:6], ftf[1])
    want = (one + torch.tensor(sc.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) * 2 - 1
    assert (ref - want).abs().max().item() < 1e-12
    dev32 = (closed_form(d, io=io, prec=torch.float32)[1].double() - ref).abs().max().item()
    got = run_stage_b(dev, d, FP, io=io, what=f"saturated {sign}")
    assert torch.isfinite(got).all()
    err = (got - want).abs().max().item()
    print(f"saturated visibility {shape} {sign:+.0f}: max err {err:.2e}, err / f32-vs-f64 deviation {err / dev32:.2f} (bound 4)")
    assert err <= 4 * dev32, (err, dev32)


# ------------------------------------------------------------------------------------------------ 4. the network
@functools.lru_cache(maxsize=1)
def _state_dict():
    from flair_amd.guided_diffusion.superslomo import SuperSloMo
    return sc.seeded_state_dict(SuperSloMo())


@functools.lru_cache(maxsize=1)
def _net(dev):
    from flair_amd.guided_diffusion.superslomo import SuperSloMo
    net = SuperSloMo().eval()
    net.load_state_dict(_state_dict())
    return net.to(dev)


# f32 HIP network against the fixture, error / the reference's own f32-vs-float64 deviation of that quantity (3e-6 .. 2e-5),
# measured on one MI355X: f01 1.34, f10 1.31, frames 1.68 (32 x 32, factor 2) and 0.99, 1.35, 1.15 (64 x 96, factor 4).
# Bound 8: the HIP convolutions sum up to 9216 products in another order than ATen.
@pytest.mark.parametrize("case", ["small", "big"])
def test_network_matches_reference_fixture(dev, case):
    g = np.load(GOLD)
    c = sc.CASES[case]
    f0, f1 = sc.frames(torch.from_numpy(g[f"{case}_u8"]))
    net = _net(dev)
    out, f01, f10 = net(f0.to(dev), f1.to(dev), c["factor"], return_flow=True)
    assert tuple(out.shape) == (c["B"], c["factor"] - 1, 3, c["H"], c["W"]) and out.dtype == FP
    for fl in (f01, f10):
        assert tuple(fl.shape) == (c["B"], 2, c["H"], c["W"]) and fl.dtype == FP and fl.is_contiguous()
    only = net(f0.to(dev), f1.to(dev), c["factor"])
    assert torch.equal(only, out)
    worst = compare(case, g, dict(f01=f01.cpu(), f10=f10.cpu(), out=out.cpu()), 8.0, "network")
    print(f"network {case}: worst error / deviation {worst:.2f} (bound 8)")


def test_network_refusals(dev):
    net = _net(dev)
    x = torch.zeros(1, 3, 64, 64, device=dev)
    with pytest.raises(ValueError, match="factor"):
        net(x, x, 1)
    y = torch.zeros(1, 3, 40, 64, device=dev)
    with pytest.raises(ValueError, match="multiples of 32"):
        net(y, y, 2)
    with pytest.raises(ValueError, match="no CPU path"):
        net(x.cpu(), x.cpu(), 2)
    with pytest.raises(ValueError, match="no CPU path"):
        net(x, x.cpu(), 2)
    with pytest.raises(ValueError, match="frame1 is"):
        net(x, torch.zeros(1, 3, 64, 96, device=dev), 2)


# ------------------------------------------------------------------------------------------------ 5. convolution geometries
SLOMO_CONVS = [
    C(1, 16, 16, [32], 64, (1, 5, 5), LRELU01, 0, 8, 1.0, None, None),          # down1.conv1 of case "small"
    C(2, 9, 11, [64], 64, (1, 5, 5), LRELU01, 0, 8, 1.0, None, None),           # 5x5 on odd sizes, two frames
    C(1, 32, 48, [64], 64, (1, 5, 5), LRELU01, 0, 8, 1.0, None, None),          # down1.conv2 of case "big"
    C(1, 1, 1, [512], 512, (1, 3, 3), LRELU01, 0, 3, 1.0, None, None),          # down5 on the 1 x 1 bottom of case "small"
    C(2, 2, 3, [512], 512, (1, 3, 3), LRELU01, 0, 3, 1.0, None, None),          # and on the 2 x 3 bottom of case "big"
    C(1, 2, 2, [512, 512], 512, (1, 3, 3), LRELU01, 0, 3, 1.0, None, None),     # up1.conv2 of case "small": two segments
]


@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", SLOMO_CONVS, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{'+'.join(map(str, c[3]))}-k{c[5][1]}")
def test_new_conv_geometries_bit_for_bit(dev, dtype, case):
    """5x5 stride-1 convolutions and 3x3 convolutions on 1 x 1 and 2 x 3 maps on integer data against float64, in the
    manner of tests/test_gpu_exact.py (every partial sum is an integer below 2^24)."""
    ops = _ops()
    T, H, W, segs, cout, k, act, nres, R, scale, _, _, ex = case
    d, fb, res, pre, ref = conv_reference(case, dtype)
    xs, o = [], 0
    for c in segs:
        x = torch.empty((T, H, W, c), dtype=dtype, device=dev)       # fresh strides: permute().contiguous() of a 1 x 1 map
        xs.append(x.copy_(nhwc(d["x"][:, o:o + c], dtype, dev)))      # keeps the NCHW ones, which name no pixel stride
        o += c
    wp = ops.pack_conv_weight(d["w"], [(c, c) for c in segs], dtype).to(dev)
    y = ops.conv(xs, wp, d["bias"].to(dev), cout, k, act=act, out_scale=scale)
    torch.cuda.synchronize()
    assert_bits_equal(y.cpu(), ref.permute(0, 2, 3, 1).contiguous(), f"conv {case[:6]} {dtype}", tile=(8, 32, 64))


# ------------------------------------------------------------------------------------------------ 6. bf16
def test_bf16_runs_and_fp32_comes_back(dev):
    """convert_to_bf16(): shapes kept, agreement with the f32 run reported (not gated); convert_to_fp32() afterwards gives
    the f32 output again, bit for bit."""
    from flair_amd.guided_diffusion.superslomo import SuperSloMo
    g = np.load(GOLD)
    c = sc.CASES["big"]
    f0, f1 = (t.to(dev) for t in sc.frames(torch.from_numpy(g["big_u8"])))
    net = SuperSloMo().eval()
    net.load_state_dict(_state_dict())
    net = net.to(dev)
    out32, a32, b32 = net(f0, f1, c["factor"], return_flow=True)
    out16, a16, b16 = net.convert_to_bf16()(f0, f1, c["factor"], return_flow=True)
    assert out16.shape == out32.shape and out16.dtype == FP and a16.shape == a32.shape and b16.shape == b32.shape
    assert torch.isfinite(out16).all()
    print(f"superslomo bf16 against f32 (64 x 96, factor 4): flows differ by up to {(a16 - a32).abs().max().item():.3f} / "
          f"{(b16 - b32).abs().max().item():.3f} px, frames by {(out16 - out32).abs().max().item():.3f} at most and "
          f"{(out16 - out32).abs().mean().item():.4f} on average (range [-1, 1])")
    again = net.convert_to_fp32()(f0, f1, c["factor"])
    assert torch.equal(again, out32)


# ------------------------------------------------------------------------------------------------ 7. files and command line
def test_files_and_command_line(dev, tmp_path):
    from flair_amd import __main__ as cli
    from flair_amd import interpolate as fi
    from flair_amd import io as fio
    h, w, T, factor = 48, 80, 5, 3
    src, out, wdir = tmp_path / "src", tmp_path / "out", tmp_path / "weights"
    src.mkdir()
    wdir.mkdir()
    gen = torch.Generator().manual_seed(48)
    low = torch.rand(T, 3, h // 8, w // 8, generator=gen)
    frames = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    u8 = (frames * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    for i in range(T):
        fio.write_frame(str(src / f"{i:03d}.png"), u8[i].numpy())
    sd = _state_dict()
    torch.save({"state_dictFC": {k[len("flow_estimator."):]: v for k, v in sd.items() if k.startswith("flow_estimator.")},
                "state_dictAT": {k[len("interp."):]: v for k, v in sd.items() if k.startswith("interp.")}},
               wdir / "SuperSloMo.ckpt")
    net = fi.load_interpolator(wdir, dev)
    n = fi.interpolate_video_files(str(src), str(out), factor, net=net, device=dev)
    names = sorted(os.listdir(out))
    assert n == 13 and names == [f"{i:04d}.png" for i in range(13)]
    got = np.stack([fio.decode_frame_hwc(str(out / name)) for name in names])
    assert got.shape == (13, h, w, 3)
    for i in range(T):
        assert np.array_equal(got[i * factor], u8[i].numpy()), i                 # originals: byte-identical
    # the others: the module called directly on the edge-padded pairs (all four in one batch, as the files path sends
    # them), cropped, through io.to_bytes
    x = fi.pad_frames(u8.to(dev).permute(0, 3, 1, 2).float() / 255.0)
    assert tuple(x.shape[2:]) == (64, 96)
    mid = _net(dev)((x[:-1] * 2 - 1).contiguous(), (x[1:] * 2 - 1).contiguous(), factor)
    want = fio.to_bytes(((mid[..., :h, :w] + 1) / 2).clamp(0, 1).flatten(0, 1)).view(T - 1, factor - 1, h, w, 3).cpu().numpy()
    for p in range(T - 1):
        for k in range(factor - 1):
            assert np.array_equal(got[p * factor + 1 + k], want[p, k]), (p, k)
    assert any(not np.array_equal(want[p, 0], u8[p].numpy()) for p in range(T - 1))
    # the same through interpolate_frames, and the command line with its scores
    again = fi.interpolate_frames(net, u8.to(dev).permute(0, 3, 1, 2).float() / 255.0, factor)
    assert np.array_equal(fio.to_bytes(again).cpu().numpy(), got)
    out2, js = tmp_path / "out2", tmp_path / "m.json"
    with torch.enable_grad():                     # main() turns autograd off for the process; keep it to this test
        assert cli.main(["interpolate", str(src), str(out2), "--factor", str(factor), "--weights", str(wdir), "--device", str(dev),
                         "--ground-truth", str(out), "--json", str(js)]) == 0
    assert sorted(os.listdir(out2)) == names
    result = json.loads(js.read_text())
    assert result["count"] == 13 and len(result["frames"]) == 13 and result["mean"]["ssim"] > 0.9999
