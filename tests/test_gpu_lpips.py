"""GPU: the LPIPS kernels (csrc/lpips.hip, include/flair_eval.h) and flair_amd.lpips against tests/lpips_ref.py.

The tap kernel is compared bit for bit on features whose every norm, quotient and partial sum is exactly representable, and
per element on random features; the whole metric on both trunks with seeded weights.  Where a comparison is not exact its
bound is 4 x the deviation of the float32 CPU restatement from float64 on the same inputs, computed here and logged."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_ref as lr
from tests import util

pytestmark = pytest.mark.gpu

WIDTHS = (64, 128, 192, 256, 384, 512)


def run_tap(fa, fb, w, acc_before, dev):
    """One flair_lpips_tap call through the typed binding with the accumulator and the workspace inside guarded
    allocations -> the (F,) float64 accumulator on the host."""
    from flair_amd import _lib, ops
    Fr, H, W, C = fa.shape
    abuf, av, _ = util.flat_guarded((Fr,), torch.float64, dev, util.OUT_FILL, src=acc_before)
    a0 = abuf.clone()
    n = Fr * ops.LPIPS_TAP_PARTS
    wbuf, wv, w0 = util.flat_guarded((n,), torch.float64, dev, util.OUT_FILL)
    _lib.call.flair_lpips_tap(fa, fa.stride(2), fb, fb.stride(2), Fr, H * W, C, w, av, wv, 8 * n)
    torch.cuda.synchronize()
    util.assert_flat_untouched(abuf, a0, view=av, what="acc")
    util.assert_flat_untouched(wbuf, w0, view=wv, what="workspace")
    return av.cpu().clone()


def place(t, layout, dev):
    """(F, P, C) cpu f32 -> a (F, 1, P, C) clip tensor on the device: dense, or a channel slice of a wider buffer between
    guard frames, NaN all around.  -> (buffer or None, view)."""
    Fr, P, C = t.shape
    if layout == "dense":
        return None, t.view(Fr, 1, P, C).to(dev).contiguous()
    buf, v = util.guarded(Fr, 1, P, C, torch.float32, dev, coff=16, ld=C + 32, fill=util.IN_FILL)
    v.copy_(t.view(Fr, 1, P, C))
    return buf, v


def exact_features(Fr, P, C, g):
    """+-1 on 4^k channels (k = 0 .. 3, seeded per pixel), 0 elsewhere: every norm is 2^k.  Pixel 0 of a is all zero; pixel 1
    (frame 0's only pixel shares the first case) is all zero on both sides."""
    def one():
        x = torch.zeros(Fr, P, C)
        k = torch.randint(0, 4, (Fr, P), generator=g)
        order = torch.rand(Fr, P, C, generator=g).argsort(-1)
        on = order < (4 ** k)[..., None]
        return torch.where(on, torch.randint(0, 2, (Fr, P, C), generator=g).float() * 2 - 1, x)
    a, b = one(), one()
    a[:, 0] = 0
    if P > 1:
        a[:, 1] = 0
        b[:, 1] = 0
    else:
        b[-1, 0] = 0
    return a, b


def exact_tap(a, b, w):
    """(sum_p d_p) / P of exact_features in float64, where every step is exact but the last division.  In f32 the norm 2^k
    absorbs the 1e-10 and a zero vector divided by 1e-10 is zero, so the kernel's d is this d; the float64 reference, in
    which the eps survives, agrees to 1e-9."""
    def unit(t):
        return t.double() / t.double().pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1.0)
    d = ((unit(a) - unit(b)).pow(2) * w.double()).sum(-1)
    assert d.max() < 512 and torch.equal(d * 512, (d * 512).round())
    want = d.sum(-1) / a.shape[1]
    assert (want - lr.tap_distance(a.double(), b.double(), w.double())).abs().max() < 1e-9
    return want


@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("Fr", [1, 3])
@pytest.mark.parametrize("C", WIDTHS)
def test_tap_exact(dev, C, Fr, layout):
    """Norms 1, 2, 4, 8, quotients +-2^-k, weights 2^0 .. 2^-3: every product is a multiple of 2^-9 below 4 and a pixel's (at
    most 128 non-zero) terms sum below 2^9, so every f32 partial in any order is exact, as is every double after it.  The one
    correct per-frame value is (sum_p d_p) / HW rounded once; a second call accumulates onto the first."""
    g = torch.Generator().manual_seed(7 * C + Fr)
    w = 2.0 ** -torch.randint(0, 4, (C,), generator=g).float()
    for P in (1, 15, 323):
        a, b = exact_features(Fr, P, C, g)
        a2, b2 = exact_features(Fr, P, C, g)
        want1 = exact_tap(a, b, w)
        want2 = want1 + exact_tap(a2, b2, w)
        (abuf, av), (bbuf, bv) = place(a, layout, dev), place(b, layout, dev)
        keep = [None if x is None else x.clone() for x in (abuf, bbuf)]
        got1 = run_tap(av, bv, w.to(dev), torch.zeros(Fr, dtype=torch.float64), dev)
        av.copy_(a2.view_as(av))
        bv.copy_(b2.view_as(bv))
        got2 = run_tap(av, bv, w.to(dev), got1, dev)
        assert torch.equal(util.bits(got1), util.bits(want1)), (C, Fr, P, got1.tolist(), want1.tolist())
        assert torch.equal(util.bits(got2), util.bits(want2)), (C, Fr, P, got2.tolist(), want2.tolist())
        for buf, before, view in ((abuf, keep[0], av), (bbuf, keep[1], bv)):
            if buf is not None:
                util.assert_untouched(buf, before, view=view, what="features")


@pytest.mark.parametrize("C", WIDTHS)
def test_tap_random_features_within_4x_the_f32_restatement(dev, C):
    """Per pixel (64 frames of one pixel) and per frame (3 frames of 323 pixels) against float64."""
    for P, Fr in ((1, 64), (323, 3)):
        fa, fb, w = lr.random_tap_case(C, P, Fr)
        ref = lr.tap_distance(fa.double(), fb.double(), w.double())
        f32 = lr.tap_distance(fa, fb, w)
        bound = lr.bound_4x(ref, f32)
        _, av = place(fa, "strided", dev)
        _, bv = place(fb, "dense", dev)
        got = run_tap(av, bv, w.to(dev), torch.zeros(Fr, dtype=torch.float64), dev)
        err = (got - ref).abs().max().item()
        util.parity_log(f"lpips_tap C={C} F={Fr} HW={P}: max|gpu - f64| = {err:.3e}, f32 cpu deviation = {bound / 4:.3e}, "
                        f"bound = {bound:.3e}, max ref = {ref.max().item():.3e}")
        assert bound > 0 and err <= bound, (C, P, err, bound)


def test_tap_same_bits_every_run_and_for_every_batch(dev):
    from flair_amd import ops
    for C, P in ((64, 323), (192, 77), (512, 40)):
        fa, fb, w = lr.random_tap_case(C, P, 3, seed=1)
        a, b, w = fa.view(3, 1, P, C).to(dev), fb.view(3, 1, P, C).to(dev), w.to(dev)
        first = ops.lpips_tap(a, b, w, torch.zeros(3, dtype=torch.float64, device=dev)).clone()
        again = ops.lpips_tap(a, b, w, torch.zeros(3, dtype=torch.float64, device=dev))
        assert torch.equal(util.bits(first), util.bits(again))
        for n in range(3):
            one = ops.lpips_tap(a[n:n + 1], b[n:n + 1], w, torch.zeros(1, dtype=torch.float64, device=dev))
            assert torch.equal(util.bits(one[0]), util.bits(first[n])), (C, n)


# ------------------------------------------------------------------------------------------- preparation
@pytest.mark.parametrize("W", [5, 17, 64])
def test_prepare_every_byte_value_at_every_alignment(dev, W):
    from flair_amd import ops
    N, H = 2, -(-256 // W)
    i = torch.arange(N * H * W)
    a = torch.stack([i % 256, (7 * i + 3) % 256, 255 - i % 256], dim=1).to(torch.uint8).view(N, H, W, 3)
    b = torch.stack([(5 * i + 1) % 256, 255 - i % 256, (3 * i + 2) % 256], dim=1).to(torch.uint8).view(N, H, W, 3)
    for t in (a, b):
        assert all(len(set(t[..., c].flatten().tolist())) == 256 for c in range(3))
    want = torch.cat([lr.prepare(a, torch.float64), lr.prepare(b, torch.float64)]).permute(0, 2, 3, 1)
    for off in range(4):
        hold_a = torch.full((a.numel() + 16,), 0x5A, dtype=torch.uint8, device=dev)
        hold_b = torch.full((b.numel() + 16,), 0xA5, dtype=torch.uint8, device=dev)
        va, vb = hold_a[off:off + a.numel()].view(a.shape), hold_b[(off + 3) % 4:(off + 3) % 4 + b.numel()].view(b.shape)
        assert va.data_ptr() % 4 == off and vb.data_ptr() % 4 == (off + 3) % 4
        va.copy_(a)
        vb.copy_(b)
        buf, out = util.guarded(2 * N, H, W, 16, torch.float32, dev, coff=4, ld=24)
        before = buf.clone()
        ops.lpips_prepare(va, vb, out=out)
        torch.cuda.synchronize()
        util.assert_untouched(buf, before, view=out, what=f"prepare W={W} off={off}")
        worst = util.assert_within_ulps(out[..., :3], want.contiguous(), 1, what=f"prepare W={W} off={off}")
        assert torch.equal(util.bits(out[..., 3:]), torch.zeros_like(util.bits(out[..., 3:]))), "pad channels"
        print(f"lpips_prepare W={W} alignment a={off} b={(off + 3) % 4}: worst distance {worst} ulp")


# ------------------------------------------------------------------------------------------- pool and stem
@pytest.mark.parametrize("k", [3, 2])
@pytest.mark.parametrize("H, W", [(7, 7), (8, 9), (15, 31)])
def test_valid_pool_bit_for_bit(dev, H, W, k):
    from flair_amd import ops
    g = torch.Generator().manual_seed(H * W + k)
    x = torch.randn(2, H, W, 8, generator=g) - 0.5
    want = F.max_pool2d(x.permute(0, 3, 1, 2), k, 2).permute(0, 2, 3, 1).contiguous()
    xbuf, xv = util.guarded(2, H, W, 8, torch.float32, dev, coff=4, ld=16, fill=util.IN_FILL)
    xv.copy_(x)
    x0 = xbuf.clone()
    ybuf, yv = util.guarded(2, want.shape[1], want.shape[2], 8, torch.float32, dev, coff=8, ld=20)
    y0 = ybuf.clone()
    ops.maxpool_valid(xv, k, out=yv)
    torch.cuda.synchronize()
    util.assert_untouched(xbuf, x0, what="x")
    util.assert_untouched(ybuf, y0, view=yv, what="y")
    util.assert_bits_equal(yv.cpu().contiguous(), want, what=f"maxpool_valid {H}x{W} k={k}")
    assert want.min() < 0


@pytest.mark.parametrize("H, W", [(31, 31), (37, 50), (7, 71)])
def test_alexnet_stem_within_4x_the_f32_restatement(dev, H, W):
    from flair_amd import ops
    trunk, _ = lr.state_dicts("alex")
    w, b = trunk["features.0.weight"], trunk["features.0.bias"]
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(2, 3, H, W, generator=g)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=4, padding=2)).permute(0, 2, 3, 1)
    bound = lr.bound_4x(ref, F.relu(F.conv2d(x, w, b, stride=4, padding=2)).permute(0, 2, 3, 1))
    xbuf, xv = util.guarded(2, H, W, 3, torch.float32, dev, coff=0, ld=16, fill=util.IN_FILL)
    xv.copy_(x.permute(0, 2, 3, 1))
    ybuf, yv = util.guarded(2, ref.shape[1], ref.shape[2], 64, torch.float32, dev, coff=4, ld=72)
    y0 = ybuf.clone()
    ops.alexnet_stem(xv, w.permute(2, 3, 1, 0).reshape(363, 64).contiguous().to(dev), b.to(dev), out=yv)
    torch.cuda.synchronize()
    util.assert_untouched(ybuf, y0, view=yv, what="y")
    err = (yv.cpu().double() - ref).abs().max().item()
    util.parity_log(f"alexnet_stem {H}x{W}: max|gpu - f64| = {err:.3e}, f32 cpu deviation = {bound / 4:.3e}, bound = {bound:.3e}")
    assert tuple(yv.shape[1:3]) == ((H - 7) // 4 + 1, (W - 7) // 4 + 1) and bound > 0 and err <= bound


# ------------------------------------------------------------------------------------------- the whole metric
SHAPES = {"vgg": [(16, 16), (37, 50), (64, 48)], "alex": [(31, 31), (37, 50), (64, 48)]}
AMPLITUDES = (8, 64)


def frames(net, shape, amp):
    """Three random frames and the same frames plus noise of amplitude `amp`, (3, H, W, 3) uint8 each."""
    H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + amp + len(net))
    a = torch.randint(0, 256, (3, H, W, 3), generator=g)
    b = (a + torch.randint(-amp, amp + 1, a.shape, generator=g)).clamp(0, 255)
    return a.to(torch.uint8), b.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def references(net):
    """{(shape, amp): float64 reference (3,)} of every case of a trunk and the trunk's bound: 4 x the largest deviation of the
    float32 CPU restatement over those cases.  Computed once and shared."""
    refs, dev32 = {}, 0.0
    for shape in SHAPES[net]:
        for amp in AMPLITUDES:
            a, b = frames(net, shape, amp)
            refs[(shape, amp)] = lr.lpips(net, a, b)
            dev32 = max(dev32, (lr.lpips(net, a, b, torch.float32).double() - refs[(shape, amp)]).abs().max().item())
    return refs, 4.0 * dev32


@functools.lru_cache(maxsize=None)
def model(net):
    from flair_amd import lpips as flp
    m = flp.LPIPS(net)
    m.load_state_dict(flp.lpips_state_dict(net, *lr.state_dicts(net)))
    return m.to("cuda:0")


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_whole_metric_within_4x_the_f32_restatement(dev, net):
    refs, bound = references(net)
    m = model(net)
    worst = 0.0
    for (shape, amp), ref in refs.items():
        a, b = (t.to(dev) for t in frames(net, shape, amp))
        got3 = torch.tensor(m(a, b), dtype=torch.float64)
        got1 = torch.tensor(m(a[:1], b[:1]), dtype=torch.float64)
        err = max((got3 - ref).abs().max().item(), (got1 - ref[:1]).abs().max().item())
        worst = max(worst, err)
        util.parity_log(f"lpips {net} {shape[0]}x{shape[1]} noise {amp}: ref {ref.tolist()}, max|gpu - f64| = {err:.3e} "
                        f"(N = 3 and N = 1), f32 cpu bound of the trunk = {bound:.3e}")
        assert ref.min() > 0 and err <= bound, (net, shape, amp, err, bound)
        assert m(a, a.clone()) == [0.0, 0.0, 0.0] and m(b[:1], b[:1].clone()) == [0.0]
    util.parity_log(f"lpips {net}: worst |gpu - f64| = {worst:.3e}, f32 cpu deviation = {bound / 4:.3e}, bound = {bound:.3e}")


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_whole_metric_same_bits_for_every_batch(dev, net):
    m = model(net)
    a, b = (t.to(dev) for t in frames(net, (37, 50), 64))
    first = m(a, b)
    assert m(a, b) == first
    for n in range(3):
        assert m(a[n:n + 1], b[n:n + 1]) == [first[n]], (net, n)


def test_evaluate_dirs_reports_forward_on_the_same_bytes(dev, tmp_path):
    from PIL import Image
    from flair_amd import metrics
    m = model("vgg")
    a, b = frames("vgg", (32, 32), 8)
    for d, t in (("out", a), ("truth", b)):
        (tmp_path / d).mkdir()
        for n in range(3):
            Image.fromarray(t[n].numpy(), mode="RGB").save(tmp_path / d / f"{n:04d}.png", format="PNG")
    want = m(a.to(dev), b.to(dev))
    for batch in (8, 2):
        res = metrics.evaluate_dirs(str(tmp_path / "out"), str(tmp_path / "truth"), dev, batch=batch, lpips=m)
        assert [f["lpips"] for f in res["frames"]] == want and res["mean"]["lpips"] == sum(want) / 3
        assert set(res["frames"][0]) == {"name", "psnr", "ssim", "lpips"}
    assert metrics.format_report(res)[-1].endswith(f"  lpips {sum(want) / 3:.4f}")
    plain = metrics.evaluate_dirs(str(tmp_path / "out"), str(tmp_path / "truth"), dev)
    assert set(plain["frames"][0]) == {"name", "psnr", "ssim"} and set(plain["mean"]) == {"psnr", "ssim"}


# ------------------------------------------------------------------------------------------- refusals
def test_wrapper_refusals_reach_the_entries(dev):
    from flair_amd import _lib, ops
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)                                              # noqa: E731
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_tap: C = 96 is not a tap width"):
        ops.lpips_tap(z(1, 1, 4, 96), z(1, 1, 4, 96), z(96), acc)
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_tap: fa stride/alignment: fa_ld = 66"):
        ops.lpips_tap(z(1, 1, 4, 66)[..., :64], z(1, 1, 4, 64), z(64), acc)
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_tap: fb stride/alignment: fb_ld = 68 .* 16-byte aligned"):
        ops.lpips_tap(z(1, 1, 4, 64), z(1, 1, 4, 68)[..., 1:65], z(64), acc)
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_tap: w = .* must be 16-byte aligned"):
        ops.lpips_tap(z(1, 1, 4, 64), z(1, 1, 4, 64), z(65)[1:], acc)
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_tap: fa must be float32, got float64"):
        ops.lpips_tap(z(1, 1, 4, 64).double(), z(1, 1, 4, 64), z(64), acc)
    u8 = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_prepare: y stride/alignment: y_ld = 18"):
        ops.lpips_prepare(u8, u8, out=z(2, 4, 4, 18)[..., :16])
    with pytest.raises(_lib.FlairHipError, match="flair_lpips_prepare: y stride/alignment: y_ld = 12 must be >= C = 16"):
        ops.lpips_prepare(u8, u8, out=z(2, 4, 4, 12))
    with pytest.raises(_lib.FlairHipError, match="flair_maxpool_valid_s2_nhwc: k = 4"):
        ops.maxpool_valid(z(1, 8, 8, 8), 4)
    with pytest.raises(_lib.FlairHipError, match="flair_maxpool_valid_s2_nhwc: C = 6 is not a positive multiple of 4"):
        ops.maxpool_valid(z(1, 8, 8, 6), 3)
    with pytest.raises(_lib.FlairHipError, match="flair_maxpool_valid_s2_nhwc: y stride/alignment: y_ld = 10"):
        ops.maxpool_valid(z(1, 8, 8, 8), 3, out=z(1, 3, 3, 10)[..., :8])
    # (a frame without a window has an empty output, whose null pointer is refused first: tests/test_lpips_cpu.py covers those)
    with pytest.raises(_lib.FlairHipError, match="flair_alexnet_stem: y stride/alignment: y_ld = 66"):
        ops.alexnet_stem(z(1, 31, 31, 16), z(363, 64), z(64), out=z(1, 7, 7, 66)[..., :64])
    with pytest.raises(_lib.FlairHipError, match="flair_alexnet_stem: w = .* must be 16-byte aligned"):
        ops.alexnet_stem(z(1, 31, 31, 16), z(363, 64), z(65)[1:])
