"""GPU: the ArcFace identity kernels (csrc/ident.hip, include/flair_ident.h) and flair_amd.identity against tests/ident_ref.py.

The preparation is compared per element with the float64 definition within one f32 rounding; the embedding kernel bit for bit on
integer data, whose every partial sum is exact, and per element on random data within the rounding of its float64 sums; the
whole network and the command on the calibrated case.  Where a comparison of the network is not exact its bound is 4 x the
deviation of the float32 CPU restatement from float64 on the same inputs, computed here and logged."""
import functools
import json
import re

import numpy as np
import pytest
import torch

from tests import ident_ref as R
from tests import util

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- preparation
@functools.lru_cache(maxsize=None)
def prepare_case(H, W):
    """Two sets of three random frames and the float64 definition of all six, (6, 128, 128)."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    a = torch.randint(0, 256, (3, H, W, 3), generator=g).to(torch.uint8)
    b = torch.randint(0, 256, (3, H, W, 3), generator=g).to(torch.uint8)
    return a, b, torch.cat([R.prepare(a), R.prepare(b)])[:, 0]


def test_the_reference_of_the_exact_ratio_is_the_mean_of_the_two_middle_taps():
    """512 -> 128 is 4:1: src = 4 d + 1.5, so both weights are 1/2 on both axes and pixels 4 d + 1, 4 d + 2 are read."""
    a, _, want = prepare_case(512, 512)
    x = 2.0 * a.double() / 255.0 - 1.0
    gray = 0.2989 * x[..., 0] + 0.5870 * x[..., 1] + 0.1140 * x[..., 2]
    mid = (gray[:, 1::4, 1::4] + gray[:, 1::4, 2::4] + gray[:, 2::4, 1::4] + gray[:, 2::4, 2::4]) / 4
    assert (want[:3] - mid).abs().max().item() < 1e-15


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H, W", [(512, 512), (96, 80), (50, 37)])
def test_prepare_per_element(dev, H, W, N):
    """Exact 4:1 (both weights 1/2), a fractional ratio, and an enlargement with edge clamps whose odd row length starts rows
    at every byte alignment; one set (b null) and two; the frames at odd addresses; y_ld = 24 between guard frames.  The bound
    is one f32 rounding of a value of magnitude <= 1: 2^-24."""
    from flair_amd import ops
    a3, b3, want3 = prepare_case(H, W)
    a, b = a3[:N], b3[:N]
    want = torch.cat([want3[:N], want3[3:3 + N]])
    assert want.abs().max().item() <= 1.0
    for off, with_b in ((1, True), (0, False), (3, False), (2, True)):
        hold_a = torch.full((a.numel() + 16,), 0x5A, dtype=torch.uint8, device=dev)
        hold_b = torch.full((b.numel() + 16,), 0xA5, dtype=torch.uint8, device=dev)
        va, vb = hold_a[off:off + a.numel()].view(a.shape), hold_b[(off + 1) % 4:(off + 1) % 4 + b.numel()].view(b.shape)
        assert va.data_ptr() % 4 == off and vb.data_ptr() % 4 == (off + 1) % 4
        va.copy_(a)
        vb.copy_(b)
        Fr = 2 * N if with_b else N
        buf, out = util.guarded(Fr, 128, 128, 16, torch.float32, dev, coff=0, ld=24)
        before = buf.clone()
        ops.ident_prepare(va, vb if with_b else None, out=out)
        torch.cuda.synchronize()
        util.assert_untouched(buf, before, view=out, what=f"ident_prepare {H}x{W} N={N} off={off}")    # channels 16 .. 23 and the guard frames
        err = (out[..., 0].cpu().double() - want[:Fr]).abs().max().item()
        print(f"ident_prepare {H}x{W} N={N} alignment {off} b={with_b}: max|gpu - f64| = {err:.3e} (bound {2.0 ** -24:.3e})")
        assert err <= 2.0 ** -24, (H, W, N, off, err)
        assert torch.equal(util.bits(out[..., 1:]), torch.zeros_like(util.bits(out[..., 1:]))), "channels 1 .. 15"


# ------------------------------------------------------------------------------------------- the embedding kernel
O = 512


def rows(Fr, n, ld, off, fill, dev):
    """-> (buf, view): buf (Fr + 2, ld) filled with `fill`, view = buf[1:Fr + 1, off:off + n]: guard rows and guard columns."""
    buf = torch.full((Fr + 2, ld), fill, dtype=torch.float32, device=dev)
    return buf, buf[1:Fr + 1, off:off + n]


def assert_rows_untouched(buf, before, view, off, what):
    changed = util.bits(buf) != util.bits(before)
    if view is not None:
        changed[1:1 + view.shape[0], off:off + view.shape[1]] = False
    assert not bool(changed.any()), f"{what}: {int(changed.sum())} element(s) changed outside the view, first at {changed.nonzero()[0].tolist()}"


def run_embed(x, w, bias, dev):
    """One flair_ident_embed call through the typed binding: x (F, K) cpu f32 placed between NaN guard rows and columns
    (x_ld = K + 8), the output between guards (out_ld = O + 5), the workspace inside a guarded allocation -> (F, O) cpu f32."""
    from flair_amd import _lib, ops
    Fr, K = x.shape
    xbuf, xv = rows(Fr, K, K + 8, 4, util.IN_FILL, dev)
    xv.copy_(x)
    x0 = xbuf.clone()
    obuf, ov = rows(Fr, w.shape[0], w.shape[0] + 5, 3, util.OUT_FILL, dev)
    o0 = obuf.clone()
    n = -(-K // ops.IDENT_EMBED_KCHUNK) * Fr * w.shape[0]
    wbuf, wv, w0 = util.flat_guarded((n,), torch.float64, dev, util.OUT_FILL)
    _lib.call.flair_ident_embed(xv, K + 8, Fr, K, w, bias, w.shape[0], ov, w.shape[0] + 5, wv, 8 * n)
    torch.cuda.synchronize()
    assert_rows_untouched(xbuf, x0, None, 0, "x")
    assert_rows_untouched(obuf, o0, ov, 3, "out")
    util.assert_flat_untouched(wbuf, w0, view=wv, what="workspace")
    return ov.cpu().contiguous()


@functools.lru_cache(maxsize=None)
def integer_case(K):
    """Integers in -3 .. 3 (x, w) and -8 .. 8 (bias): |every partial sum| <= 9 K + 8 < 2^24, exact in float64 and in the f32 result."""
    g = torch.Generator().manual_seed(K)
    x = util.int_tensor((16, K), -3, 3, g)
    w = util.int_tensor((O, K), -3, 3, g)
    bias = util.int_tensor((O,), -8, 8, g)
    want = x.double() @ w.double().t() + bias.double()
    assert 9 * K + 8 < 2 ** 24 and torch.equal(want, want.round()) and want.abs().max() > 100
    return x, w, bias, want.float()


@pytest.mark.parametrize("Fr", [1, 3, 16])
@pytest.mark.parametrize("K", [2048, 32768])
def test_embed_exact_on_integers(dev, K, Fr):
    x, w, bias, want = integer_case(K)
    got = run_embed(x[:Fr], w.to(dev), bias.to(dev), dev)
    util.assert_bits_equal(got, want[:Fr].contiguous(), what=f"ident_embed K={K} F={Fr}")


@functools.lru_cache(maxsize=None)
def random_case(K):
    g = torch.Generator().manual_seed(K + 1)
    x = torch.randn(16, K, generator=g).clamp_min(-0.3)             # a PReLU output: mostly positive
    w = torch.randn(O, K, generator=g) * (2.0 / K) ** 0.5
    bias = torch.randn(O, generator=g)
    ref = x.double() @ w.double().t() + bias.double()
    mag = x.double().abs() @ w.double().abs().t() + bias.double().abs()
    return x, w, bias, ref, mag


@pytest.mark.parametrize("Fr", [1, 3, 16])
@pytest.mark.parametrize("K", [2048, 32768])
def test_embed_random_within_the_rounding_of_float64_sums(dev, K, Fr):
    """Per element within 2^-24 |e| (the one rounding to f32) + K 2^-52 sum |w x| (float64 sums of K exact products in any order)."""
    x, w, bias, ref, mag = random_case(K)
    got = run_embed(x[:Fr], w.to(dev), bias.to(dev), dev).double()
    bound = 2.0 ** -24 * ref[:Fr].abs() + K * 2.0 ** -52 * mag[:Fr]
    err = (got - ref[:Fr]).abs()
    util.parity_log(f"ident_embed K={K} F={Fr}: max|gpu - f64| = {err.max().item():.3e}, max of err / bound = {(err / bound).max().item():.3f}, "
                    f"max |e| = {ref[:Fr].abs().max().item():.3f}")
    assert bool((err <= bound).all()), (K, Fr, (err / bound).max().item())


@pytest.mark.parametrize("K", [2048, 32768])
def test_embed_same_bits_every_run_and_for_every_batch(dev, K):
    from flair_amd import ops
    x, w, bias, _, _ = random_case(K)
    x, w, bias = x.to(dev), w.to(dev), bias.to(dev)
    first = ops.ident_embed(x, w, bias).clone()
    again = ops.ident_embed(x, w, bias)
    assert torch.equal(util.bits(first), util.bits(again))
    for f in (0, 7, 15):
        one = ops.ident_embed(x[f:f + 1], w, bias)
        assert torch.equal(util.bits(one[0]), util.bits(first[f])), (K, f)
    three = ops.ident_embed(x[5:8], w, bias)
    assert torch.equal(util.bits(three), util.bits(first[5:8]))


def test_embed_more_frames_than_one_tile_and_odd_sizes(dev):
    """17 frames (two frame tiles), O = 6 (a partial row tile), K = 8196 (nine chunks, the last of one float4 in one partial step)."""
    from flair_amd import ops
    g = torch.Generator().manual_seed(5)
    x, w, bias = util.int_tensor((17, 8196), -3, 3, g), util.int_tensor((6, 8196), -3, 3, g), util.int_tensor((6,), -8, 8, g)
    want = (x.double() @ w.double().t() + bias.double()).float()
    got = run_embed(x, w.to(dev), bias.to(dev), dev)
    util.assert_bits_equal(got, want, what="ident_embed 17 x 8196 -> 6")
    assert torch.equal(ops.ident_embed(x.to(dev), w.to(dev), bias.to(dev)).cpu(), want)


# ------------------------------------------------------------------------------------------- the network
@functools.lru_cache(maxsize=None)
def model():
    from flair_amd import identity as fid
    m = fid.ArcFace()
    m.load_state_dict(fid.identity_state_dict(R.case()["sd"]))
    return m.to("cuda:0")


def cosine_pairs(e):
    """The 16 cosines a report of the case is made of: frame k with its truth, and both sets' consecutive frames."""
    return np.concatenate([R.cosines(e[:6], e[6:]), R.cosines(e[1:6], e[:5]), R.cosines(e[7:], e[6:11])])


def test_network_within_4x_the_f32_restatement(dev):
    c = R.case()
    m = model()
    got = m.embed(c["a"].to(dev), c["b"].to(dev))
    assert got.shape == (12, 512) and got.dtype == np.float64
    bound_e = 4.0 * np.abs(c["e32"] - c["e64"]).max()
    bound_c = 4.0 * np.abs(cosine_pairs(c["e32"]) - cosine_pairs(c["e64"])).max()
    err_e = np.abs(got - c["e64"]).max()
    err_c = np.abs(cosine_pairs(got) - cosine_pairs(c["e64"])).max()
    util.parity_log(f"identity network N=6: max|gpu - f64| on embeddings = {err_e:.3e} (f32 cpu deviation {bound_e / 4:.3e}, bound {bound_e:.3e}, "
                    f"max |e| = {np.abs(c['e64']).max():.3f}); on the 16 cosines = {err_c:.3e} (f32 cpu deviation {bound_c / 4:.3e}, "
                    f"bound {bound_c:.3e}); ids = {R.cosines(got[:6], got[6:]).tolist()}")
    assert bound_e > 0 and err_e <= bound_e, (err_e, bound_e)
    assert bound_c > 0 and err_c <= bound_c, (err_c, bound_c)


def test_network_same_bits_alone_and_in_a_batch(dev):
    """Frame k's embedding in a batch of 6 is its embedding alone, and a second run gives the same bits.  (Across ALL batch sizes
    only the two kernels of ident.hip promise equal bits: flair_conv_nhwc picks its split of K by the size of the launch, and
    the 12-frame batch of the test above differs from this one by 1e-5 on embeddings of magnitude 3, the f32 restatement's own
    deviation.  Within one batch equal frames do get equal embeddings: the command's test finds an exact 1.)"""
    m = model()
    a = R.case()["a"].to(dev)
    six = m.embed(a)
    assert six.shape == (6, 512) and np.array_equal(six, m.embed(a))
    for k in (0, 3, 5):
        assert np.array_equal(m.embed(a[k:k + 1])[0], six[k]), k


# ------------------------------------------------------------------------------------------- the command
def test_evaluate_with_identity_end_to_end(dev, tmp_path, capsys):
    from PIL import Image
    from flair_amd.__main__ import main
    c = R.case()
    for d, t in (("out", c["a"]), ("truth", c["b"])):
        (tmp_path / d).mkdir()
        for n in range(6):
            Image.fromarray(t[n].numpy(), mode="RGB").save(tmp_path / d / f"{n:04d}.png", format="PNG")
    torch.save({"module." + k: v for k, v in c["sd"].items()}, tmp_path / "arcface_resnet18.pth")
    rc = main(["evaluate", str(tmp_path / "out"), str(tmp_path / "truth"), "--identity", str(tmp_path / "arcface_resnet18.pth"),
               "--json", str(tmp_path / "m.json"), "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert rc == 0 and len(lines) == 7
    e = c["e64"]
    ids = R.cosines(e[:6], e[6:])
    for n in range(6):
        assert re.fullmatch(rf"{n:04d}\.png  psnr \S+  ssim \S+  ids {ids[n]:.4f}", lines[n]), (lines[n], ids[n])
    want = dict(ids=float(ids.mean()), id_drift=R.drift(e[:6]), id_drift_truth=R.drift(e[6:]))
    assert lines[6].endswith(f"  ids {want['ids']:.4f}  id-drift {want['id_drift']:.4f} (truth {want['id_drift_truth']:.4f})"), lines[6]
    got = json.load(open(tmp_path / "m.json"))
    # every figure is a cosine of the case or a mean of some: 4 x the f32 restatement's largest deviation on those cosines
    bound = 4.0 * np.abs(cosine_pairs(c["e32"]) - cosine_pairs(e)).max()
    assert set(got["mean"]) == {"psnr", "ssim", "ids", "id_drift", "id_drift_truth"} and set(got["frames"][0]) == {"name", "psnr", "ssim", "ids"}
    for n in range(6):
        assert abs(got["frames"][n]["ids"] - ids[n]) <= bound, (n, got["frames"][n]["ids"], ids[n])
    for k, v in want.items():
        assert abs(got["mean"][k] - v) <= bound, (k, got["mean"][k], v, bound)
    assert got["frames"][0]["ids"] == 1.0
    # without the option: the lines and the keys of before
    main(["evaluate", str(tmp_path / "out"), str(tmp_path / "truth"), "--json", str(tmp_path / "plain.json"), "--device", "cuda:0"])
    plain = capsys.readouterr().out.strip().splitlines()
    assert plain == [re.sub(r"  ids .*", "", line) for line in lines]
    assert set(json.load(open(tmp_path / "plain.json"))["mean"]) == {"psnr", "ssim"}
    # rectangular frames are refused by name
    for d in ("r_out", "r_truth"):
        (tmp_path / d).mkdir()
        Image.fromarray(np.zeros((64, 96, 3), dtype=np.uint8), mode="RGB").save(tmp_path / d / "0000.png", format="PNG")
    with pytest.raises(SystemExit, match=r"identity: evaluate: .*r_out.0000\.png is 64x96; the score takes aligned face crops"):
        main(["evaluate", str(tmp_path / "r_out"), str(tmp_path / "r_truth"), "--identity", str(tmp_path / "arcface_resnet18.pth"),
              "--device", "cuda:0"])


# ------------------------------------------------------------------------------------------- refusals
def test_every_refusal_of_the_header_comes_before_any_launch(dev):
    from flair_amd import _lib, ops
    lib = _lib.lib()
    for name, args, what in R.entry_refusals():
        R.assert_refused(lib, name, args, what)
    torch.cuda.synchronize()                       # nothing was enqueued: the device is as it was
    z = lambda *s: torch.zeros(*s, device=dev)     # noqa: E731
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FlairHipError, match="flair_ident_prepare: y stride/alignment: y_ld = 18"):
        ops.ident_prepare(u8, out=z(1, 128, 128, 18)[..., :16])
    with pytest.raises(_lib.FlairHipError, match="flair_ident_prepare: y stride/alignment: y_ld = 12 must be >= C = 16"):
        ops.ident_prepare(u8, u8, out=z(2, 128, 128, 12))
    with pytest.raises(_lib.FlairHipError, match="flair_ident_embed: K = 6 is not a multiple of 4"):
        ops.ident_embed(z(2, 6), z(8, 6), z(8))
    with pytest.raises(_lib.FlairHipError, match="flair_ident_embed: x stride/alignment: x_ld = 10"):
        ops.ident_embed(z(2, 10)[:, :8], z(8, 8), z(8))
    with pytest.raises(_lib.FlairHipError, match="flair_ident_embed: w = .* must be 16-byte aligned"):
        ops.ident_embed(z(2, 8), z(65)[1:].view(8, 8), z(8))
    with pytest.raises(_lib.FlairHipError, match="flair_ident_embed: x must be float32, got float64"):
        ops.ident_embed(z(2, 8).double(), z(8, 8), z(8))
