"""AMT-G on the GPU (amt.hip, ABI 17).  The entries: the correlation lookup against a float64 closed form (volume entries
bit for bit at integer coordinates, dyadic coordinates on integer volumes bit for bit, seeded coordinates within the f32
ATen deviation, guarded strided destinations), the pyramid pooling, the volume itself, per-channel PReLU, the transposed
convolution as a repacked 3x3 convolution plus depth-to-space, and InstanceNorm + ReLU.  The network: the feature encoder,
one decoder and one update block on the reference's own inputs, the three cases end to end with their intermediate flows
(tests/golden/g18_amt.npz), batch and factor invariance bit for bit, and the driver on an uneven size.  The tail of the
network (multi-flow prepare and combine, axpby, corr_scale) and the instance norm on planes large enough to be summed in
chunks have their per-element tests in tests/test_gpu_amt_tail.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import amt_cpu as ac
from tests.test_amt_cpu import GOLD, ratios
from tests.test_gpu_strides import run_both
from tests.util import (assert_bits_equal, assert_flat_untouched, balanced_signs, flat_guarded, gn_fold_f32, int_tensor,
                        OUT_FILL)

pytestmark = pytest.mark.gpu
FP = torch.float32
# query grid (B, h, w) and the planes of each pyramid level
LOOKUPS = {"6x5": ((2, 6, 5), [(6, 5), (3, 2), (1, 1)]),
           "12x10": ((1, 12, 10), [(12, 10), (6, 5), (3, 2), (1, 1)])}


def _ops():
    from flair_amd import ops
    return ops


def nchw(t):
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ 1. the lookup
def pyramids(name, kind, seed):
    """Two lists of (B h w, lh, lw) f32 planes: seeded normal values or integers in [-8, 8]; every level is seeded on its
    own (no level is the pooling of another: the lookup must not care)."""
    (B, h, w), levels = LOOKUPS[name]
    g = torch.Generator().manual_seed(seed)
    make = (lambda s: torch.randn(s, generator=g)) if kind == "randn" else (lambda s: int_tensor(s, -8, 8, g))
    return [make((B * h * w, lh, lw)) for lh, lw in levels], [make((B * h * w, lh, lw)) for lh, lw in levels]


def bilinear_zeros64(planes, x, y):
    """planes (N, H, W), x and y (N, K) float64 pixel coordinates -> (N, K) float64: bilinear, zeros outside, written out."""
    N, H, W = planes.shape
    p = planes.double()
    x0, y0 = x.floor(), y.floor()
    out = torch.zeros_like(x)
    n = torch.arange(N).view(N, 1).expand_as(x)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = (1 - (x - xx).abs()) * (1 - (y - yy).abs())
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            v = p[n, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()]
            out += torch.where(ok, v * wgt, torch.zeros_like(v))
    return out


def lookup64(name, pyr, pyr_t, flow, s_corr, s_corr_t):
    """The closed form in float64 -> (B, h, w, 98 levels), and per output element whether its coordinate is an integer."""
    (B, h, w), levels = LOOKUPS[name]
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    base = torch.stack([xs, ys], dim=-1).double().view(1, h, w, 2)
    a = torch.arange(49) // 7 - 3           # the first tap axis moves x
    b = torch.arange(49) % 7 - 3
    outs, whole = [], []
    for vols, fl, s in ((pyr, flow[..., 2:4], s_corr), (pyr_t, flow[..., 0:2], s_corr_t)):
        # the centre is an f32 quantity in the reference and the kernel: product and sum rounded
        c = (base.float() + fl * torch.tensor(s, dtype=FP)).double().view(B * h * w, 2)
        for l, v in enumerate(vols):
            x = c[:, 0:1] / 2 ** l + a.view(1, 49)
            y = c[:, 1:2] / 2 ** l + b.view(1, 49)
            if tuple(v.shape[1:]) == (1, 1):
                outs.append(v.double().view(-1, 1).expand(-1, 49))
                whole.append(torch.ones_like(x, dtype=torch.bool))
            else:
                outs.append(bilinear_zeros64(v, x, y))
                whole.append((x == x.floor()) & (y == y.floor()))
    n = len(levels)
    return torch.cat(outs, dim=1).view(B, h, w, 98 * n), torch.cat(whole, dim=1).view(B, h, w, 98 * n)


def lookup_aten32(name, pyr, pyr_t, flow, s_corr, s_corr_t):
    """The reference's own f32 ATen calls (tests/amt_cpu.py: grid_sample behind bilinear_sampler's normalisation)."""
    (B, h, w), _ = LOOKUPS[name]
    coord = ac.coords_grid(B, h, w, FP)
    fl = nchw(flow)
    c0, c1 = ac.corr_lookup([v[:, None] for v in pyr], [v[:, None] for v in pyr_t], coord + fl[:, 2:4] * torch.tensor(s_corr),
                            coord + fl[:, 0:2] * torch.tensor(s_corr_t))
    return torch.cat([c0, c1], dim=1).permute(0, 2, 3, 1).contiguous()


def run_lookup(dev, name, pyr, pyr_t, flow, s_corr, s_corr_t, what):
    """Dense and on guarded strided views (flow at channel 4 of 12, the destination at channel 4 of a pixel stride of at least 98 levels + 12)."""
    ops = _ops()
    (B, h, w), levels = LOOKUPS[name]
    C = 98 * len(levels)
    ld = (C + 12 + 3) // 4 * 4
    dp, dpt = [v.to(dev) for v in pyr], [v.to(dev) for v in pyr_t]
    before = [v.clone() for v in dp + dpt]
    out = run_both(dev, {"flow": (flow, FP, 4, 12)}, {"y": ((B, h, w, C), FP, 4, ld)},
                   lambda flow, y: ops.corr_lookup(dp, dpt, flow, s_corr, s_corr_t, y), what)["y"]
    for v, b4 in zip(dp + dpt, before):
        assert torch.equal(v, b4), f"{what}: a volume changed"
    return out


def exact_flows(name, seed, step):
    """Flows on a grid of ``step`` pixels in [-3, 3]; query 1 is sent far up-left and the last query far down-right, so their
    windows lie wholly outside the sampled planes."""
    (B, h, w), _ = LOOKUPS[name]
    g = torch.Generator().manual_seed(seed)
    flow = torch.randint(-3 * int(1 / step), 3 * int(1 / step) + 1, (B, h, w, 4), generator=g).float() * step
    flow[0, 0, 1] = -40.0
    flow[-1, -1, -1] = 40.0
    return flow


@pytest.mark.parametrize("name", list(LOOKUPS))
def test_lookup_integer_coordinates_return_volume_entries(dev, name):
    """Seeded normal volumes, integer flows, scale 1: wherever a level's coordinate is an integer the output is that volume
    entry (or zero outside the plane), bit for bit, and a 1 x 1 level gives its value to all 49 taps."""
    pyr, pyr_t = pyramids(name, "randn", 11)
    flow = exact_flows(name, 12, 1.0)
    want, whole = lookup64(name, pyr, pyr_t, flow, 1.0, 1.0)
    got = run_lookup(dev, name, pyr, pyr_t, flow, 1.0, 1.0, f"lookup {name} integer").float()
    n = len(LOOKUPS[name][1])
    assert whole[..., :49].all() and whole[..., 49 * n:49 * n + 49].all()       # level 0: every tap
    assert whole.float().mean().item() > 0.4
    assert_bits_equal(torch.where(whole, got, torch.zeros(())), torch.where(whole, want.float(), torch.zeros(())),
                      f"lookup {name}: integer coordinates")
    # the window of every query leaves its 6 x 5 (12 x 10) plane; the two far queries read zeros at every sampled level
    sampled = torch.tensor([lv != (1, 1) for lv in LOOKUPS[name][1]]).repeat_interleave(49).repeat(2)
    if name == "6x5":
        assert (want[..., :49] == 0).any(dim=-1).all()
    for q in ((0, 0, 1), (-1, -1, -1)):
        assert (got[q][sampled] == 0).all() and (got[q][~sampled] != 0).all()
    err = (got.double() - want).abs().max().item()
    assert err < 1e-5, err                                                      # the other coordinates: dyadic weights


@pytest.mark.parametrize("name", list(LOOKUPS))
@pytest.mark.parametrize("step", [0.5, 0.25])
def test_lookup_dyadic_coordinates_on_integer_volumes(dev, name, step):
    """Integer volumes, flows on a half (quarter) pixel grid, scale 1 and 2: every weight is a dyadic fraction of a few bits
    and every product and sum is exact in f32, so the float64 closed form is the one correct answer."""
    pyr, pyr_t = pyramids(name, "int", 21)
    flow = exact_flows(name, 22, step)
    s_corr, s_corr_t = 2.0, 1.0
    want, _ = lookup64(name, pyr, pyr_t, flow, s_corr, s_corr_t)
    assert torch.equal(want.float().double(), want)
    got = run_lookup(dev, name, pyr, pyr_t, flow, s_corr, s_corr_t, f"lookup {name} step {step}").float()
    n = 49 * len(LOOKUPS[name][1])
    assert not torch.equal(want[..., :n], want[..., n:])                        # the halves differ: a swap would show
    assert_bits_equal(got, want.float(), f"lookup {name}: coordinates on a {step} grid")


# Bound: 4 x the deviation of the reference's f32 ATen calls from the float64 closed form on the same inputs, the project's
# bound for its warp kernels.
@pytest.mark.parametrize("name", list(LOOKUPS))
def test_lookup_seeded_coordinates_against_float64(dev, name):
    (B, h, w), levels = LOOKUPS[name]
    pyr, pyr_t = pyramids(name, "randn", 31)
    g = torch.Generator().manual_seed(32)
    flow = torch.randn(B, h, w, 4, generator=g) * 1.5
    s_corr, s_corr_t = (float(v) for v in ac.lookup_scales(ac.timesteps(4)[0]))      # t = 0.25: 4 and 4 / 3
    want, _ = lookup64(name, pyr, pyr_t, flow, s_corr, s_corr_t)
    dev32 = (lookup_aten32(name, pyr, pyr_t, flow, s_corr, s_corr_t).double() - want).abs().max().item()
    assert dev32 > 0
    got = run_lookup(dev, name, pyr, pyr_t, flow, s_corr, s_corr_t, f"lookup {name} seeded")
    outside = (want == 0).double().mean().item()
    err = (got - want).abs().max().item()
    print(f"lookup {name}: zero samples {outside:.2f}, f32 ATen deviation {dev32:.2e}, max err {err:.2e}, "
          f"err / deviation {err / dev32:.2f} (bound 4)")
    assert 0.05 < outside < 0.95
    assert err <= 4 * dev32, (err, dev32)


def test_lookup_refuses_what_the_reference_raises_on(dev):
    ops = _ops()
    from flair_amd._lib import FlairHipError
    flow = torch.zeros(1, 2, 2, 4, device=dev)
    out = torch.zeros(1, 2, 2, 98, device=dev)
    with pytest.raises(FlairHipError, match="1 x 1"):
        ops.corr_lookup([torch.zeros(4, 1, 2, device=dev)], [torch.zeros(4, 1, 2, device=dev)], flow, 1.0, 1.0, out)
    with pytest.raises(FlairHipError, match="flow stride/alignment"):
        ops.corr_lookup([torch.zeros(4, 2, 2, device=dev)], [torch.zeros(4, 2, 2, device=dev)],
                        torch.zeros(1, 2, 2, 8, device=dev)[..., 1:5], 1.0, 1.0, out)


# ------------------------------------------------------------------------------------------------ 2. the pyramid and the volume
@pytest.mark.parametrize("hw", [(6, 5), (5, 7), (2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_pool_bit_for_bit(dev, hw):
    ops = _ops()
    h, w = hw
    g = torch.Generator().manual_seed(h * 10 + w)
    vol = int_tensor((2 * h * w, h, w), -64, 64, g)
    want = F.avg_pool2d(vol.double()[:, None], 2, stride=2)[:, 0].float()
    buf, out, before = flat_guarded(tuple(want.shape), FP, dev, OUT_FILL)
    src = vol.to(dev)
    ops.corr_pool(src, out=out)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2 * h * w, h // 2, w // 2)
    assert_bits_equal(out.cpu(), want, f"pool {hw}")
    assert_flat_untouched(buf, before, out, f"pool {hw}")
    assert torch.equal(src.cpu(), vol)


def test_volume_both_directions(dev):
    """corr = fmap0^T fmap1 / sqrt(128) and corr_T from the swapped product, on integer features (exact sums, one rounded
    division): bit for bit against float64 divided by the f32 sqrt(128) and rounded once."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    B, h, w, D = 2, 3, 5, 128
    f0, f1 = int_tensor((B, D, h, w), -4, 4, g), int_tensor((B, D, h, w), -4, 4, g)
    ref = ac.corr_volume(f0.double(), f1.double()).view(B * h * w, h, w)
    div = torch.sqrt(torch.tensor(128).float()).double()
    prod = torch.bmm(f0.double().view(B, D, -1).transpose(1, 2), f1.double().view(B, D, -1))
    want = (prod / div).float().view(B * h * w, h, w)
    assert (want.double() - ref).abs().max().item() < 1e-5
    a0, a1 = (t.permute(0, 2, 3, 1).contiguous().to(dev) for t in (f0, f1))
    corr = ops.corr_volume(a0, f1.to(dev))
    corr_t = ops.corr_volume(a1, f0.to(dev))
    assert_bits_equal(corr.cpu(), want, "corr")
    assert_bits_equal(corr_t.cpu(), want.view(B, h * w, h * w).transpose(1, 2).reshape(B * h * w, h, w).contiguous(), "corr_T")


# ------------------------------------------------------------------------------------------------ 3. PReLU
@pytest.mark.parametrize("C", [84, 256])
@pytest.mark.parametrize("addend", [False, True], ids=["x", "x+y"])
def test_prelu_bit_for_bit(dev, C, addend):
    ops = _ops()
    g = torch.Generator().manual_seed(C + addend)
    T, H, W = 2, 5, 7
    x0, x1 = torch.randn(T, H, W, C, generator=g), torch.randn(T, H, W, C, generator=g)
    slope = torch.randn(C, generator=g) * 0.5
    v = x0 + x1 if addend else x0
    want = F.prelu(nchw(v), slope).permute(0, 2, 3, 1).contiguous()
    assert (v < 0).any() and (want != v).any()
    ds = slope.to(dev)
    ins = {"x0": (x0, FP, 4, C + 12)}
    if addend:
        ins["x1"] = (x1, FP, 8, C + 8)
    got = run_both(dev, ins, {"y": ((T, H, W, C), FP, 4, C + 8)},
                   lambda x0, y, x1=None: ops.prelu(x0, ds, x1, out=y), f"prelu {C} {addend}")["y"]
    assert_bits_equal(got.float(), want, f"prelu {C} {addend}")
    inplace = x0.to(dev)
    ops.prelu(inplace, ds, x1.to(dev) if addend else None, out=inplace)
    assert_bits_equal(inplace.cpu(), want, "prelu in place")


# ------------------------------------------------------------------------------------------------ 4. ConvTranspose2d(4, 2, 1)
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cout", [40, 116])
def test_transposed_convolution_path_bit_for_bit(dev, hw, cout):
    """The repacked 3x3 convolution + depth-to-space against float64 conv_transpose2d on integer data (every partial sum is
    an integer below 2^24)."""
    ops = _ops()
    h, w = hw
    cin, B = 48, 2
    g = torch.Generator().manual_seed(cout + h)
    x = int_tensor((B, cin, h, w), -4, 4, g)
    wt, b = int_tensor((cin, cout, 4, 4), -3, 3, g), int_tensor((cout,), -8, 8, g)
    want = F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1)
    assert want.abs().max().item() < 2 ** 24
    w3, b3 = ops.deconv_as_conv3x3(wt, b)
    wp = ops.pack_conv_weight(w3, [(cin, cin)], FP).to(dev)
    xc = torch.empty((B, h, w, cin), dtype=FP, device=dev).copy_(x.permute(0, 2, 3, 1))
    y4 = ops.conv(xc, wp, b3.to(dev), 4 * cout, (1, 3, 3))
    buf, out, before = flat_guarded((B, 2 * h, 2 * w, cout), FP, dev, OUT_FILL)
    ops.depth_to_space2(y4, cout, out=out)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu(), want.float().permute(0, 2, 3, 1).contiguous(), f"deconv {hw} {cout}")
    assert_flat_untouched(buf, before, out, f"deconv {hw} {cout}")


# ------------------------------------------------------------------------------------------------ 5. InstanceNorm + ReLU
def instance_norm_relu(ops, x):
    """flair_instnorm_nhwc.  (flair_groupnorm_nhwc with groups = C, frames_per_stat = 1 passes the balanced planes bit for
    bit but measured 14.9 x the f32 ATen deviation on the seeded 4 x 4 map at C = 64: var = E[x^2] - mean^2.)"""
    return ops.instance_norm(x, ops.ACT_RELU, 1e-5)


@pytest.mark.parametrize("C", [64, 112, 160])
@pytest.mark.parametrize("hw", [(4, 4), (16, 18)], ids=lambda s: "x".join(map(str, s)))
def test_instance_norm_balanced_planes_bit_for_bit(dev, C, hw):
    """Every (frame, channel) plane holds as many +1 as -1: mean 0 and variance 1 in any summation order, so the output is
    relu(+-1 * f32(1 / sqrt(1 + eps))), bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(C + hw[0])
    x = balanced_signs(2, *hw, C, 1, C, g)
    assert (x.sum((1, 2)) == 0).all()
    zero, one = torch.zeros(1, 1, 1, 1, dtype=torch.float64), torch.ones(1, 1, 1, 1, dtype=torch.float64)
    want = F.relu(gn_fold_f32(x, zero, one, torch.ones(C), torch.zeros(C), 1e-5))
    got = instance_norm_relu(ops, x.to(dev))
    assert_bits_equal(got.cpu(), want, f"instance norm {C} {hw}")


@pytest.mark.parametrize("C", [64, 112, 160])
@pytest.mark.parametrize("hw", [(4, 4), (16, 18)], ids=lambda s: "x".join(map(str, s)))
def test_instance_norm_against_float64(dev, C, hw):
    """Seeded data with per-channel offsets and scales: within 4 x the deviation of F.instance_norm in f32 ATen from its
    float64 evaluation."""
    ops = _ops()
    g = torch.Generator().manual_seed(1000 + C + hw[0])
    x = torch.randn(2, *hw, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    want = F.relu(F.instance_norm(nchw(x).double(), eps=1e-5)).permute(0, 2, 3, 1)
    dev32 = (F.relu(F.instance_norm(nchw(x), eps=1e-5)).permute(0, 2, 3, 1).double() - want).abs().max().item()
    got = instance_norm_relu(ops, x.to(dev)).cpu().double()
    err = (got - want).abs().max().item()
    print(f"instance norm C = {C} {hw}: f32 ATen deviation {dev32:.2e}, max err {err:.2e}, err / deviation {err / dev32:.2f} (bound 4)")
    assert err <= 4 * dev32, (err, dev32)


# ------------------------------------------------------------------------------------------------ 6. the network
@functools.lru_cache(maxsize=1)
def _state_dict():
    from flair_amd.guided_diffusion.amt import AMT
    return ac.seeded_state_dict(AMT())


@functools.lru_cache(maxsize=1)
def _net(dev):
    from flair_amd.guided_diffusion.amt import AMT
    net = AMT().eval()
    net.load_state_dict(_state_dict())
    net = net.to(dev)
    net._ensure_packed(dev)
    return net


def to_nhwc(t, dev, width=None):
    """(B, C, H, W) cpu -> (B, H, W, width) on the device, zeros past C."""
    B, C, H, W = t.shape
    x = torch.zeros((B, H, W, width or C), dtype=FP, device=dev)
    x[..., :C] = t.permute(0, 2, 3, 1).to(dev)
    return x


# Per block, the inputs are the reference's own stored values, so errors do not compound.  Bound: 8 x the stored deviation
# of that block, the SuperSloMo network bound (a different summation order over up to thousands of products).
def test_feat_encoder_against_fixture(dev):
    g = np.load(GOLD)
    net = _net(dev)
    for case in ac.CASES:
        f0, f1 = ac.frames(torch.from_numpy(g[f"{case}_u8"]))
        i0, i1 = (f0 + 1) / 2, (f1 + 1) / 2
        pad = ac.pad_amounts(*i0.shape[-2:])
        i0, i1 = F.pad(i0, pad, mode="replicate"), F.pad(i1, pad, mode="replicate")
        mean_ = torch.cat([i0, i1], 2).mean(1, keepdim=True).mean(2, keepdim=True).mean(3, keepdim=True)
        x = torch.cat([i0 - mean_, i1 - mean_], dim=0)
        if x.shape[-1] <= 64:
            x = ac.resize(x, 2.0)
        fmap = net.feat_encoder.run(to_nhwc(x, dev, 16)).permute(0, 3, 1, 2).cpu()
        B = f0.shape[0]
        r = ratios(case, g, dict(fmap0=fmap[:B], fmap1=fmap[B:]), "feat_encoder", ("fmap0", "fmap1"))
        assert max(r.values()) <= 8.0, r


def test_decoder_and_update_block_against_fixture(dev):
    g = np.load(GOLD)
    net = _net(dev)
    case = ac.BLOCK_CASE
    t = ac.timesteps(ac.CASES[case]["factor"])[0].item()
    f0, f1 = (torch.from_numpy(g[f"{case}_blk_{n}"]) for n in ("f0_4", "f1_4"))
    embt = torch.zeros(*f0.shape[:1], *f0.shape[2:], 16, device=dev)
    embt[..., 0] = t
    dec = net.decoder4.run(to_nhwc(f0, dev), to_nhwc(f1, dev), embt)
    want = torch.from_numpy(g[f"{case}_blk_dec4"])
    assert (dec[..., want.shape[1]:] == 0).all()                                # the pad channels of the next segment
    err = (dec[..., :want.shape[1]].permute(0, 3, 1, 2).cpu() - want).abs().max().item()
    d = float(g[f"{case}_dev_blk_dec4"])
    print(f"decoder4: max|err| {err:.3e} = {err / d:.2f} x the block's deviation {d:.2e} (bound 8)")
    assert err <= 8 * d, (err, d)
    ins = [torch.from_numpy(g[f"{case}_blk_{n}"]) for n in ("net", "flow", "corr")]
    d_net, d_flow = net.update4.deltas(to_nhwc(ins[0], dev), to_nhwc(ins[1], dev, 16), to_nhwc(ins[2], dev, 400))
    for name, got, c in (("dnet", d_net, 112), ("dflow", d_flow, 4)):
        want = torch.from_numpy(g[f"{case}_blk_{name}"])
        assert (got[..., c:] == 0).all()
        err = (got[..., :c].permute(0, 3, 1, 2).cpu() - want).abs().max().item()
        d = float(g[f"{case}_dev_blk_{name}"])
        print(f"update4 {name}: max|err| {err:.3e} = {err / d:.2f} x the block's deviation {d:.2e} (bound 8)")
        assert err <= 8 * d, (name, err, d)


# End to end the network feeds its flows back into lookups and warps, so no bound is derived: the gate per quantity is twice
# the measured error / stored deviation, rounded up.  Measured on one MI355X (the largest over the three cases):
#   fmap0 1.11, fmap1 1.28, corr0 1.34, lookup4 0.97, lookup3 1.06, lookup2 0.75, flow_dec4 1.62, flow4 1.58, flow_dec3 1.27,
#   flow3 1.30, flow_dec2 1.59, flow2 1.42, flow1 1.13, mask 1.29, out 2.40
# -- the size of the per-block ratios (feat_encoder 1.0 - 1.3, decoder4 and update4 below 2): nothing compounds visibly.
GATES = dict(fmap0=3, fmap1=3, corr0=3, lookup4=2, lookup3=3, lookup2=2, flow_dec4=4, flow4=4, flow_dec3=3, flow3=3,
             flow_dec2=4, flow2=3, flow1=3, mask=3, out=5)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_network_against_reference_fixture(dev, case):
    g = np.load(GOLD)
    c = ac.CASES[case]
    f0, f1 = ac.frames(torch.from_numpy(g[f"{case}_u8"]))
    net = _net(dev)
    detail = []
    out = net(f0.to(dev), f1.to(dev), c["factor"], detail=detail)
    assert tuple(out.shape) == (c["B"], c["factor"] - 1, 3, c["H"], c["W"]) and out.dtype == FP
    assert len(detail) == c["factor"] - 1
    got = {k: v.cpu() for k, v in detail[0].items()}
    got["out"] = out.cpu()
    r = ratios(case, g, got, "network")
    print(f"network {case} ratios: " + ", ".join(f"{k} {v:.2f}" for k, v in r.items()))
    for q, v in r.items():
        assert v <= GATES[q], (case, q, v, GATES[q])
    assert torch.equal(net(f0.to(dev), f1.to(dev), c["factor"]), out)          # the same bits without the record


def test_batch_and_factor(dev):
    """Batch 2 equals two batch-1 runs bit for bit; the frame of factor 4 at t = 0.5 equals that of factor 2."""
    g = np.load(GOLD)
    f0, f1 = (t.to(dev) for t in ac.frames(torch.from_numpy(g["rect_u8"])))
    net = _net(dev)
    both = net(f0, f1, 4)
    for b in range(2):
        one = net(f0[b:b + 1].contiguous(), f1[b:b + 1].contiguous(), 4)
        assert_bits_equal(one.cpu(), both[b:b + 1].cpu(), f"batch item {b}")
    half = net(f0, f1, 2)
    assert_bits_equal(half[:, 0].cpu(), both[:, 1].cpu(), "t = 0.5 of factor 4 and of factor 2")
    assert not torch.equal(both[:, 0], both[:, 1])
    net._reference_schedule = True              # the per-pair work repeated per timestep: the same frames
    try:
        assert_bits_equal(net(f0, f1, 4).cpu(), both.cpu(), "reference schedule")
    finally:
        net._reference_schedule = False


def test_driver_keeps_originals_and_pads_inside_the_module(dev):
    """An uneven size through interpolate_frames: MULTIPLE = 1, so the driver pads nothing, the module pads to multiples of
    16 itself (centred) and crops; originals come back bit for bit and the new frames are the module's."""
    from flair_amd import interpolate as fi
    net = _net(dev)
    assert net.MULTIPLE == 1
    T, h, w, factor = 3, 121, 139, 3
    gen = torch.Generator().manual_seed(7)
    low = torch.rand(T, 3, h // 8 + 1, w // 8 + 1, generator=gen)
    frames = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False).to(dev)
    assert fi.pad_frames(frames, net.MULTIPLE) is frames
    out = fi.interpolate_frames(net, frames, factor, batch=2)
    assert tuple(out.shape) == (factor * (T - 1) + 1, 3, h, w)
    assert torch.equal(out[::factor], frames)
    mid = net((frames[:-1] * 2 - 1).contiguous(), (frames[1:] * 2 - 1).contiguous(), factor)
    want = ((mid + 1) / 2).clamp(0, 1)
    for p in range(T - 1):
        for k in range(factor - 1):
            assert torch.equal(out[p * factor + 1 + k], want[p, k]), (p, k)
    assert not torch.equal(out[1], out[0])
    with pytest.raises(ValueError, match="coarsest pyramid level"):
        fi.interpolate_frames(net, frames[..., :72, :], factor)
