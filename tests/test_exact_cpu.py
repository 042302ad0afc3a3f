"""The exact-arithmetic harness of tests/test_gpu_exact.py, checked without a GPU: its helpers, its float64 deformable
gather against the two DCN oracles, and the written record of the gap it closes -- a reference with ONE weight off by one
unit fails assert_bits_equal, while the same fault on the randn data of test_gpu_kernels.test_conv passes assert_close."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_exact import (BF, FP, LRELU01, NONE, RELU, act_f32, conv64, dcn_gather_ref, epilogue_f32,
                                  unrepresentable_share)
from tests.util import assert_bits_equal, assert_close, assert_exact_headroom, bits, int_tensor, rb


def test_int_tensor_is_integer_valued_in_range_and_exact_in_bf16():
    g = torch.Generator().manual_seed(1)
    t = int_tensor((4, 1000), -256, 256, g)
    assert t.dtype == FP and torch.equal(t, t.round()) and t.min().item() == -256 and t.max().item() == 256
    assert torch.equal(t.to(BF).float(), t)
    assert set(int_tensor((1000,), 0, 2, g).tolist()) == {0.0, 1.0, 2.0}


def test_exact_headroom_bound():
    assert assert_exact_headroom(torch.tensor([2.0 ** 24 - 1], dtype=torch.float64)) == 2.0 ** 24 - 1
    with pytest.raises(AssertionError, match="2\\^24"):
        assert_exact_headroom(torch.tensor([1.0, 2.0 ** 24], dtype=torch.float64))
    with pytest.raises(AssertionError):
        assert_exact_headroom(torch.tensor([1.0]))             # not float64


def test_bits_equal_reports_count_first_index_largest_difference_and_tile_histogram():
    ref = torch.arange(2 * 16 * 64 * 8, dtype=FP).view(2, 16, 64, 8)
    assert_bits_equal(ref.clone(), ref, "same")
    got = ref.clone()
    got[:, 7::8, :, 5] += 512.0                                 # the last row of every 8-row tile, cout 5
    with pytest.raises(AssertionError) as e:
        assert_bits_equal(got, ref, "rows", tile=(8, 32, 8))
    msg = str(e.value)
    assert "256 of 16384 element(s) differ" in msg and "first at [0, 7, 0, 5]" in msg and "largest |difference| 512" in msg
    assert "by h % 8: [0, 0, 0, 0, 0, 0, 0, 256]" in msg and "by c % 8: [0, 0, 0, 0, 0, 256, 0, 0]" in msg
    assert "by w % 32: [" + ", ".join(["8"] * 32) + "]" in msg
    with pytest.raises(AssertionError, match="1 of 16384"):     # one last-place bit of one element
        one = bits(ref.to(BF))
        one[1, 3, 9, 2] ^= 1
        assert_bits_equal(one.view(BF), ref.to(BF), "one ulp")


def test_bits_equal_leaves_the_sign_of_zero_open_and_nothing_else():
    a = torch.tensor([0.0, -0.0, 1.0, float("nan")])
    b = torch.tensor([-0.0, 0.0, 1.0, float("nan")])
    assert_bits_equal(a, b, "zeros")
    with pytest.raises(AssertionError):
        assert_bits_equal(torch.tensor([1e-45]), torch.tensor([0.0]), "denormal")
    with pytest.raises(AssertionError):
        assert_bits_equal(torch.tensor([float("nan")]), torch.tensor([1.0]), "nan")
    with pytest.raises(AssertionError):
        assert_bits_equal(torch.tensor([-1.0]), torch.tensor([1.0]), "sign")


def test_leaky_relu_is_one_f32_product():
    """act_f32, F.leaky_relu and max(v, v * slope) (the kernels' fmaxf form) give the same bits on integers."""
    v = torch.arange(-5000, 5000, dtype=FP)
    slope = torch.tensor(0.1, dtype=FP)
    a = act_f32(v, LRELU01)
    assert torch.equal(bits(a), bits(F.leaky_relu(v, 0.1))) and torch.equal(bits(a), bits(torch.maximum(v, v * slope)))


def _sharp_case(integer):
    """(2, 16, 16, [32, 32], 64, (1, 3, 3)) in bf16, res0 and out_scale 0.5: the f32 value before the cast for the right
    weights and for weights with ONE (cout, tap, channel) entry off by 1 on the integer data (weights in [-3, 3]: half
    their standard deviation), by the same half standard deviation, 0.5 / sqrt(fan), on the randn data of
    test_gpu_kernels.test_conv, and with one product dropped (on the randn data one whose weight is 0.4 .. 0.5 standard
    deviations: the tolerance test does catch a fault of a whole standard deviation where |x| reaches 3)."""
    T, H, W, cin, cout, k = 2, 16, 16, 64, 64, (1, 3, 3)
    g = torch.Generator().manual_seed(2 * 1000 + 16 * 10 + 64)
    fan = cin * 9
    if integer:
        x, w, b = int_tensor((T, cin, H, W), -8, 8, g), int_tensor((cout, cin, *k), -3, 3, g), int_tensor((cout,), -8, 8, g)
        res, unit = int_tensor((T, cout, H, W), -64, 64, g), 1.0
    else:
        x = rb(torch.randn(T, cin, H, W, generator=g), BF)
        w = rb(torch.randn(cout, cin, *k, generator=g) / math.sqrt(fan), BF)
        b = torch.randn(cout, generator=g) * 0.1
        res, unit = rb(torch.randn(T, cout, H, W, generator=g), BF), 0.5 / math.sqrt(fan)
    at = (37, 11, 0, 2, 1)
    if not integer:
        small = ((w[37].abs() * math.sqrt(fan) - 0.45).abs() <= 0.05).nonzero()[0].tolist()
    outs = []
    for fault in (None, "off by one", "dropped"):
        w2 = w.clone()
        if fault == "off by one":
            w2[at] += unit
        elif fault == "dropped":
            w2[at if integer else (37, *small)] = 0.0
        conv = conv64(x.double(), w2.double(), k)
        outs.append(epilogue_f32(conv.float(), b, None, NONE, [res], 0.5))
    if integer:
        assert_exact_headroom(conv64(x.double().abs(), w.double().abs() + 1, k) + 8 + 64)
    return outs


def test_one_wrong_product_fails_bit_equality_and_passes_the_bf16_tolerance():
    """The gap this file's GPU sibling closes.  One weight off by half its standard deviation moves the 2 * 16 * 16 outputs
    of one cout by |x| * 0.5 sigma * out_scale: on integer data every one of them with x != 0 changes bits; on randn data
    the same fault is at most 0.035 (|x| <= 3.3) on top of the bf16 rounding, against a bound of 1.6e-2 * max|ref| + 1e-3 =
    0.051."""
    good, off, dropped = _sharp_case(integer=True)
    assert unrepresentable_share(good, BF) >= 0.05
    for bad in (off, dropped):
        with pytest.raises(AssertionError, match="differ in bits"):
            assert_bits_equal(bad.to(BF), good.to(BF), "integer data")
        with pytest.raises(AssertionError, match="differ in bits"):
            assert_bits_equal(bad, good, "integer data, f32")
    good, off, dropped = _sharp_case(integer=False)
    for bad in (off, dropped):
        assert (bad != good).sum().item() > 400
        assert_close(bad.to(BF).float(), good, BF, "randn data: the fault passes")


def test_truncation_instead_of_rne_fails_bit_equality_and_passes_the_bf16_tolerance():
    good = _sharp_case(integer=True)[0]
    trunc = (bits(good) & ~0xFFFF).view(FP)                     # f32 -> bf16 by dropping the low 16 bits
    assert torch.equal(trunc.to(BF).float(), trunc)
    with pytest.raises(AssertionError, match="differ in bits"):
        assert_bits_equal(trunc.to(BF), good.to(BF), "truncated")
    assert_close(trunc, good, BF, "truncation passes the tolerance")


def _dcn_case():
    H, W, G, cin, cout = 9, 11, 8, 32, 12
    g = torch.Generator().manual_seed(9 * 11 + G)
    x = int_tensor((2, cin, H, W), -3, 3, g)
    w = int_tensor((cout, cin, 3, 3), -3, 3, g)
    b = int_tensor((cout,), -8, 8, g)
    offset = int_tensor((2, 18 * G, H, W), -7, 7, g)
    mask = int_tensor((2, 9 * G, H, W), 0, 2, g) * 0.5
    return x, w, b, offset, mask, G


def test_dcn_gather_equals_the_reference_source_bit_for_bit():
    """dcn_gather_ref against oracle/dcn_ref.py (the literal restatement of the DCNv2 source) in float64: integer
    positions, masks in {0, 0.5, 1}; every sum is a multiple of 0.5 far below 2^53, so the two agree in every bit."""
    from oracle import dcn_ref
    x, w, b, offset, mask, G = _dcn_case()
    got, inside, edge = dcn_gather_ref(x, offset, mask, w, b, G)
    share = inside.float().mean().item()
    assert 0.10 <= share <= 0.90 and min(edge) > 0, (share, edge)
    ref = dcn_ref.modulated_deform_conv_forward(x.double().numpy(), w.double().numpy(), b.double().numpy(),
                                                offset.double().numpy(), mask.double().numpy(), deformable_group=G)
    assert got.dtype == torch.float64 and ref.dtype == np.float64
    assert np.array_equal(got.numpy().view(np.int64), ref.view(np.int64))
    assert torch.equal(got * 2, (got * 2).round())


def test_dcn_gather_equals_deform_conv2d():
    """... and oracle.thirdparty.deform_conv2d (grid_sample based: its position normalisation is inexact) to 1e-11."""
    from oracle.thirdparty import deform_conv2d
    x, w, b, offset, mask, G = _dcn_case()
    got, _, _ = dcn_gather_ref(x, offset, mask, w, b, G)
    ref = deform_conv2d(x.double(), offset.double(), w.double(), b.double(), (1, 1), (1, 1), (1, 1), mask.double())
    assert (got - ref).abs().max().item() <= 1e-11 * max(1.0, ref.abs().max().item())


def test_dcn_gather_refuses_fractional_positions():
    x, w, b, offset, mask, G = _dcn_case()
    offset[0, 3, 2, 2] += 0.5
    with pytest.raises(AssertionError, match="integer"):
        dcn_gather_ref(x, offset, mask, w, b, G)


def test_relu_and_scale_keep_integers_exact():
    """The epilogue of the reference on integers is exact: equal to the float64 evaluation."""
    g = torch.Generator().manual_seed(3)
    conv = int_tensor((2, 8, 5, 7), -40000, 40000, g)
    bias, fb = int_tensor((8,), -8, 8, g), int_tensor((2, 12), -8, 8, g)
    res = [int_tensor(conv.shape, -64, 64, g) for _ in range(2)]
    got = epilogue_f32(conv, bias, fb, RELU, res, 0.5)
    ref = (torch.relu(conv.double() + bias.double().view(1, -1, 1, 1) + fb[:, :8, None, None].double())
           + res[0].double() + res[1].double()) * 0.5
    assert torch.equal(got.double(), ref)
