"""The tail of AMT-G and the split instance norm (csrc/amt.hip) against the float64 closed forms of tests/amt_tail_ref.py,
per element: flair_amt_multiflow_combine, flair_amt_multiflow_prepare, flair_axpby_nhwc, flair_corr_scale and
flair_instnorm_nhwc on planes of more than 512 pixels, where it sums a plane in chunks.

Bit for bit: the combine kernel on integer images, quarter-pixel flows (with pinned landings far outside the frame, on its
last column and row, on 0 and between -1 and 0), masks in eighths, img_res in quarters and integer means, where every value
it forms is an f32 number; the flow and img_res channels of the prepare kernel on quarter-grid data; axpby against f32
arithmetic with both products rounded (a fused multiply-add changes more than a quarter of the elements); corr_scale against
f32 division; the instance norm on +-1 planes whose chunk sums are nonzero integers that cancel.

Bounded, at 4 x the deviation of the reference's own f32 ATen arithmetic from the closed form on the same inputs: the
combine kernel on seeded data, the sigmoid of the prepare kernel, the instance norm on seeded planes whose mean is 1, 30 and
300 standard deviations.  tests/test_amt_tail_cpu.py shows that an f32 emulation of each kernel meets these bounds with a
factor of 2.5 or more to spare, and that no mutant of a closed form passes.

Every input lies in a NaN-guarded channel view and every output in a sentinel-guarded one (run_both runs the dense call
as well and compares the two bit for bit); neg_mean is column 0 of a (B, 8) tensor of NaN.  The worst err / bound per kernel
goes to parity_log (profiles/amt_tail_parity.txt is the record).
"""
import ctypes

import pytest
import torch

from tests import amt_tail_ref as R
from tests.test_gpu_strides import run_both
from tests.util import (OUT_FILL, assert_bits_equal, assert_flat_untouched, assert_untouched, bits, flat_guarded, guarded,
                        parity_log)

pytestmark = pytest.mark.gpu
FP = torch.float32
N = R.N
ids = R.ids


def _ops():
    from flair_amd import ops
    return ops


def log(kernel, case, ratio, extra=""):
    parity_log(f"amt_tail {kernel} {case}: worst err/bound {ratio:.3f}{extra}")


# ------------------------------------------------------------------------------------------------ combine
def run_combine(dev, d, what):
    """-> x (B, H, W, 16), avg (B, H, W, 4) float64 on the CPU.  pair is handed over 8 channels wide (the entry takes no
    pixel stride of 6 floats), the two past the images NaN."""
    ops = _ops()
    B, H, W, _ = d["pair"].shape
    pair = torch.cat([d["pair"], torch.full((B, H, W, 2), float("nan"))], dim=-1)
    nm = d["neg_mean"].to(dev)
    assert nm.stride(0) > 1
    out = run_both(dev, {"pair": (pair, FP, 4, 16), "prep": (d["prep"], FP, 8, 52)},
                   {"x": ((B, H, W, 16), FP, 4, 24), "avg": ((B, H, W, 4), FP, 8, 16)},
                   lambda pair, prep, x, avg: ops.amt_multiflow_combine(pair, prep, nm[:, :1], x=x, avg=avg), what)
    assert_bits_equal(nm.cpu(), d["neg_mean"], f"{what}: neg_mean")
    return out["x"], out["avg"]


@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_combine_exact_bit_for_bit(dev, shape):
    B, H, W = shape
    d = R.combine_exact_case(*shape)
    assert all(R.landing_classes(d["prep"], H, W).values())                     # every pinned class is there
    assert not torch.equal(d["pair"][..., 0:3], d["pair"][..., 3:6])            # a swap of the images shows
    if B > 1:
        assert d["neg_mean"][0, 0] != d["neg_mean"][1, 0]                       # and so does the other frame's mean
    want_x, want_avg, _ = R.combine_exact_reference(*shape)
    x, avg = run_combine(dev, d, f"combine exact {shape}")
    assert_bits_equal(x.float(), want_x.float(), f"combine exact {shape}: x")
    assert_bits_equal(avg.float(), want_avg.float(), f"combine exact {shape}: avg")


@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_combine_seeded_against_float64(dev, shape):
    """Per element within 4 x the deviation of tests/amt_cpu.multi_flow_combine's own f32 arithmetic (img_warps and their
    mean) from the closed form."""
    want_x, want_avg, dev_x, dev_avg = R.combine_seeded_reference(*shape)
    assert 0 < dev_x < 1e-4 and 0 < dev_avg < 1e-4
    x, avg = run_combine(dev, R.combine_seeded_case(*shape), f"combine seeded {shape}")
    ex, ea = R.max_err(x, want_x), R.max_err(avg, want_avg)
    log("combine", ids(shape), max(ex / (4 * dev_x), ea / (4 * dev_avg)),
        f" (x: f32 ATen deviation {dev_x:.2e}, max err {ex:.2e}; avg: {dev_avg:.2e}, {ea:.2e})")
    assert ex <= 4 * dev_x, (ex, dev_x)
    assert ea <= 4 * dev_avg, (ea, dev_avg)
    assert (x[..., 15] == 0).all() and (avg[..., 3] == 0).all()


# ------------------------------------------------------------------------------------------------ prepare
def run_prepare(dev, d, what):
    ops = _ops()
    return run_both(dev, {"dec": (d["dec"], FP, 4, 52), "up": (d["up"], FP, 4, 12)},
                    {"out": (tuple(d["dec"].shape), FP, 8, 52)},
                    lambda dec, up, out: ops.amt_multiflow_prepare(dec, up, out=out), what)["out"]


@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_prepare_flows_bit_for_bit_and_sigmoid_against_float64(dev, shape):
    """dec + 2 up on a quarter grid is exact: the flow and img_res channels bit for bit.  The mask channels (normal values
    of sigma 4) per element within 4 x the deviation of torch.sigmoid in f32 from float64 on the same values."""
    want, dev32 = R.prepare_reference(*shape)
    got = run_prepare(dev, R.prepare_case(*shape), f"prepare {shape}")
    assert_bits_equal(R.not_mask(got).float(), R.not_mask(want).float(), f"prepare {shape}: flows and img_res")
    err = R.max_err(got[..., 4 * N:5 * N], want[..., 4 * N:5 * N])
    log("prepare sigmoid", ids(shape), err / (4 * dev32), f" (f32 sigmoid deviation {dev32:.2e}, max err {err:.2e})")
    assert err <= 4 * dev32, (err, dev32)


def test_prepare_sigmoid_saturates_in_order(dev):
    y = run_prepare(dev, R.saturation_case(), "prepare saturation")[0, 0, :, 4 * N:5 * N]
    assert R.SATURATION == sorted(R.SATURATION) and R.SATURATION[3] == 0.0
    assert not torch.isnan(y).any() and (y >= 0).all() and (y <= 1).all()
    assert (y[3] == 0.5).all() and (y[1:] >= y[:-1]).all() and (y[2] < 0.5).all() and (y[4] > 0.5).all()
    assert (y == y[:, :1]).all()


# ------------------------------------------------------------------------------------------------ axpby
def axpby_in_place(dev, x0, a, x1, b, target, what):
    """out is x0 (target 0) or x1 (target 1): dense, then on views between sentinel channels and frames -> the result."""
    ops = _ops()
    T, H, W, C = x0.shape
    srcs = [x0] if x1 is None else [x0, x1]
    dense = [t.to(dev) for t in srcs]
    ops.axpby_nhwc(dense[0], a, dense[1] if x1 is not None else None, b, out=dense[target])
    held = []
    for t, coff in zip(srcs, (4, 8)):
        buf, v = guarded(T, H, W, C, FP, dev, coff=coff, ld=C + 12)
        v.copy_(t.to(dev))
        held.append((buf, v, buf.clone()))
    ops.axpby_nhwc(held[0][1], a, held[1][1] if x1 is not None else None, b, out=held[target][1])
    torch.cuda.synchronize()
    for j, (buf, v, before) in enumerate(held):
        assert_untouched(buf, before, v if j == target else None, f"{what}: operand {j}")
    assert not (bits(held[target][1]) != bits(dense[target])).any(), f"{what}: the view and the dense call differ"
    return dense[target].cpu()


@pytest.mark.parametrize("shape", R.AXPBY_P, ids=ids)
@pytest.mark.parametrize("C", R.AXPBY_C)
def test_axpby_bit_for_bit(dev, C, shape):
    """f32 torch on the CPU with each product rounded before the sum is the one answer of the entry's documented order;
    with (1/3, 1.7) a fused multiply-add would change more than a quarter of the elements (tests/test_amt_tail_cpu.py)."""
    ops = _ops()
    x0, x1 = R.axpby_case(shape, C)
    third = 1.0 / 3.0
    for a, b, second in [(third, 0.0, None)] + [(a, b, x1) for a, b in R.AXPBY_COEFS]:
        what = f"axpby C = {C} {shape} a = {a:.3g} b = {b:.3g}"
        want = R.axpby_emul32(x0, a, second, b)
        if second is not None and (a, b) == R.AXPBY_COEFS[1]:
            assert (want != R.axpby_emul32(x0, a, second, b, fault="fma")).float().mean().item() >= 0.05
        ins = {"x0": (x0, FP, 4, C + 12)}
        if second is not None:
            ins["x1"] = (x1, FP, 8, C + 8)
        got = run_both(dev, ins, {"y": (tuple(x0.shape), FP, 4, C + 8)},
                       lambda x0, y, x1=None: ops.axpby_nhwc(x0, a, x1, b, out=y), what)["y"]
        assert_bits_equal(got.float(), want, what + ", out a third tensor")
        for target in (0, 1) if second is not None else (0,):
            assert_bits_equal(axpby_in_place(dev, x0, a, second, b, target, what), want, what + f", out is x{target}")


# ------------------------------------------------------------------------------------------------ corr_scale
@pytest.mark.parametrize("n", R.CORR_SCALE_N)
def test_corr_scale_bit_for_bit(dev, n):
    """flair_corr_scale as ops.corr_volume calls it: a true f32 division by the f32 sqrt(128), in place; n = 1, 3 and 5
    leave one to three elements to the scalar tail, 1027 takes more than one workgroup."""
    ops = _ops()
    x = R.corr_scale_case(n)
    div = float(torch.sqrt(torch.tensor(128).float()))
    buf, v, before = flat_guarded((n,), FP, dev, OUT_FILL, src=x)
    ops.check(ops.lib().flair_corr_scale(ops.ptr(v), ctypes.c_long(n), ctypes.c_float(div), ops.stream()), "flair_corr_scale")
    torch.cuda.synchronize()
    want = x / torch.tensor(div, dtype=FP)
    assert (want != x * torch.tensor(1.0 / div, dtype=FP)).any() or n < 1000      # a reciprocal multiply is another answer
    assert_bits_equal(v.cpu(), want, f"corr_scale n = {n}")
    assert_flat_untouched(buf, before, v, f"corr_scale n = {n}")


# ------------------------------------------------------------------------------------------------ instance norm
# (F, H, W, C)         what it reaches (in_split(HW) = HW / 512 chunks of ceil(HW / S) pixels, at most 64)
#   (2, 32, 32, 64)    HW = 1024: S = 2, equal chunks
#   (2, 33, 36, 112)   S = 2, chunks of 594; the second channel block has 48 live lanes
#   (1, 40, 41, 4)     S = 3, chunks of 547, 547, 546; the smallest C
#   (1, 182, 182, 64)  HW = 33124: S capped at 64, chunks of 518 and a last one of 490
#   (2, 33, 35, 64)    odd HW, S = 2, chunks of 578 and 577 (no balanced planes: the float64 test only)
def run_instnorm(dev, x, relu, what):
    ops = _ops()
    C = x.shape[3]
    return run_both(dev, {"x": (x, FP, 4, C + 12)}, {"y": (tuple(x.shape), FP, 8, C + 16)},
                    lambda x, y: ops.instance_norm(x, ops.ACT_RELU if relu else ops.ACT_NONE, 1e-5, out=y), what)["y"]


@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("shape", R.INSTNORM_SHAPES[:4], ids=ids)
def test_instance_norm_split_balanced_planes_bit_for_bit(dev, shape, relu):
    """As many +1 as -1 in every plane, at seeded places: each chunk's sum is a nonzero integer and the total is 0, so a
    chunk dropped, cut short or counted twice moves the mean and the variance; the answer is +-f32(1 / sqrt(1 + eps))."""
    x = R.instnorm_balanced_case(shape)
    assert (x.sum((1, 2)) == 0).all() and R.in_split(shape[1] * shape[2]) > 1
    got = run_instnorm(dev, x, relu, f"instance norm balanced {shape}")
    assert_bits_equal(got.float(), R.instnorm64(x, relu=relu).float(), f"instance norm balanced {shape} relu={relu}")


@pytest.mark.parametrize("offset", R.INSTNORM_OFFSETS)
@pytest.mark.parametrize("shape", R.INSTNORM_SHAPES, ids=ids)
def test_instance_norm_split_against_float64(dev, shape, offset):
    """Seeded planes whose mean is `offset` standard deviations, every channel with a scale and a mean of its own and the
    second frame three times the size of the first: per element within 4 x the deviation of F.instance_norm (+ ReLU) in
    f32 ATen from its float64 evaluation on the same data."""
    x = R.instnorm_seeded_case(shape, offset)
    for relu in (False, True):
        want, dev32 = R.instnorm_seeded_reference(shape, offset, relu)
        assert dev32 > 0
        got = run_instnorm(dev, x, relu, f"instance norm {shape} offset {offset}")
        err = R.max_err(got, want)
        log("instance_norm", f"{ids(shape)} offset {offset} {'relu' if relu else 'none'}", err / (4 * dev32),
            f" (f32 ATen deviation {dev32:.2e}, max err {err:.2e})")
        assert err <= 4 * dev32, (err, dev32)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    """Each is refused before anything is launched."""
    ops = _ops()
    from flair_amd._lib import FlairHipError
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(FlairHipError, match="flair_axpby_nhwc: C = 6 must be a multiple of 4"):
        ops.axpby_nhwc(z(1, 2, 2, 6), 1.0)
    good = dict(pair=z(1, 2, 2, 8), prep=z(1, 2, 2, 40), x=z(1, 2, 2, 16), avg=z(1, 2, 2, 4))
    nm = z(1, 8)
    ops.amt_multiflow_combine(good["pair"], good["prep"], nm, x=good["x"], avg=good["avg"])        # the good set is accepted
    odd_ld = dict(pair=z(1, 2, 2, 7)[..., :6], prep=z(1, 2, 2, 42)[..., :40], x=z(1, 2, 2, 18)[..., :16], avg=z(1, 2, 2, 6)[..., :4])
    off_4 = dict(pair=z(1, 2, 2, 12)[..., 1:7], prep=z(1, 2, 2, 44)[..., 1:41], x=z(1, 2, 2, 20)[..., 2:18], avg=z(1, 2, 2, 8)[..., 3:7])
    for bad in (odd_ld, off_4):
        for name, view in bad.items():
            args = dict(good, **{name: view})
            with pytest.raises(FlairHipError, match=f"flair_amt_multiflow_combine: {name} stride/alignment"):
                ops.amt_multiflow_combine(args["pair"], args["prep"], nm, x=args["x"], avg=args["avg"])
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in good.values())
    with pytest.raises(FlairHipError, match="flair_instnorm_nhwc: activation"):
        ops.instance_norm(z(1, 4, 4, 8), ops.ACT_SILU)
    with pytest.raises(FlairHipError, match="flair_instnorm_nhwc: C = 6 must be a multiple of 4"):
        ops.instance_norm(z(1, 4, 4, 6))
