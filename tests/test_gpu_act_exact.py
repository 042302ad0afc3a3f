"""SiLU, GELU and DCN-offset epilogues of the convolution kernels (conv.hip, chain.hip, dwconv.hip), judged per element
against float64 on an EXACT pre-activation.

tests/test_gpu_exact.py pins these kernels bit for bit, but only with the activations that are exact on integers.  The
transcendental ones exist in about a dozen separately written epilogue copies and met only assert_close, a bound on
max|ref| of the whole tensor: with the DCN residues (max|ref| = 10) a bf16 mask in [0, 1] could be off by 0.32.

Method.  The data of test_gpu_exact (integers), with weights, bias and frame bias multiplied by 2^-s: every partial sum
is a multiple of 2^-s that f32 holds exactly in any order (assert_exact_headroom on the unscaled integers), so the
pre-activation v = conv + bias (+ frame_bias) is known exactly and the activation arithmetic is all that is left to
judge.  s is chosen per geometry so that v has a standard deviation of about 3 (asserted: at least half of |v| in
[0.25, 4], both signs >= 20 %, both DCN classes present).  A few couts per 64-cout block and class carry a bias of
+-128: there SiLU and GELU must return v and 0, the residues +-mag and the masks 1 and 0, exactly (a zero of either
sign, or below 2^-120), with __expf overflowing to inf on the way.  Residuals are integers / 8, out_scale is a power of
two.  The reference is float64 throughout: act64 / dcn_act64 of the exact v, + residuals, * out_scale.

Bound, per element:  |got - ref| <= k 2^-24 S + sum over the residual adds of 2^-24 |partial sum| + 2^-120
                                    (+ half a bf16 ulp of ref for a bf16 output: util.out_rounding),
S = util.act_sens64: |a| + |v a'(v)| plus the cancellation term of the formula (0.5 |v| (1 + |erf|) for GELU, mag (1 -
tanh) for mag (1 - 2 r)).

k, per form, from the accuracy of the instructions (u = 2^-24; one rounding of an f32 operation is <= u relative; a
1-ulp instruction -- v_exp_f32, v_rcp_f32 as the ISA guide gives them -- is <= 2 u relative; __expf(x) is
v_exp_f32(x * log2 e): the product and the constant put 2 u on the argument, i.e. 2 u |x| on the result; with
s = sigmoid(v), t = tanh(v)):
  SiLU, IEEE divide   v / (1 + __expf(-v)): e^-v carries (2 |v| + 2) u, of which 1 - s reaches the sum; the sum and the
                      correctly rounded divide one u each:  |a| ((1 - s)(2 |v| + 2) + 2) u  <= 5.6 u S (worst at
                      v = -1.28, the minimum of SiLU, where v a'(v) = 0)                               -> k = 6
  SiLU, v_rcp_f32     v * rcp(1 + exp(-v)) (variant 8, and conv_resident_kernel's exp2 form with out_scale folded in):
                      2 u for the reciprocal and u for the product in place of the divide's u: <= 7.6 u S -> k = 8
  GELU                0.5 v (1 + erff(v / sqrt 2)): the argument carries 2 u (2 v^2 phi(v) u on the result), erff E ulp
                      (E |v| |erf| u), the sum and the product one u each (2 |a| u): sup over v of the total / S is
                      max(E, 2.6) -- E = 4 ulp is what the HIP math reference lists for erff                -> k = 4
  mag tanh            mag (1 - 2 rcp(1 + __expf(2 v))): ((1 - t^2)(2 |v| + 1) + 3 (1 - t) + 2 |t|) mag u <= 4 u S (at
                      v = 0); the fma form with per-lane constants has one rounding less
  sigmoid             rcp(1 + __expf(-v)): s ((1 - s)(2 |v| + 2) + 3) u <= 4 u S (at v = 0); the fma form
                      fma(rcp(1 + 2^(k v)), A, B) rounds once more: <= 5 u S              -> k = 5 for FLAIR_ACT_DCN_OFFSETS
tests/test_act_exact_cpu.py evaluates these error models against S on a dense grid, holds f32 restatements of every form
to k / 2, and shows that the comparison rejects a sigmoid of 2 v, a class boundary off by 8 channels, a tanh GELU, a bias
added after the activation, a pre-activation rounded to bf16, out_scale on the wrong side of the residual and more.  A
measured ratio above k is a finding about that kernel, never a reason to raise k.  The largest err / (2^-24 S) of every
case goes to parity_log; profiles/act_exact_parity.txt is the record.

Coverage (test_act_cases_reach_every_variant): flair_conv_variant 0..9 in bf16 and 0..7 in f32 under SiLU and under DCN
offsets, 0..7 under GELU (the host keeps GELU off the LDS-DMA kernels: the two DMA geometries are run with GELU and land
on variants 3 and 6), store_quad (bf16 Cout = 4 mod 8, and the split-K reduce), act_period 24, 48 and 72.
flair_conv_chain: conv_resident_kernel (SiLU and DCN, out_scale folded, a partial last block), the general kernel at
c = 64 and 128 with and without stage A, stage A's act_vec through a selector stage B (wB[j, j, centre] = 1: the output IS
the stored intermediate).  conv_pair_kernel and conv_frame_kernel take only the leaky class (flair_conv_chain's `lin`,
frame_kernel_ok): their geometries are run with SiLU / DCN and must be right on the kernel they fall to.
flair_dwconv_nhwc: apply_act in both stages (the fused 1x1 applies the activation a second time: a(a(v)), bounded by
k u (S(a(v)) + Lip(a) S(v))).
"""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_exact import chain_data, conv_data, nhwc
from tests.util import (ACT_DCN_OFFSETS, ACT_FLOOR, ACT_GELU, ACT_LIPSCHITZ, ACT_NONE, ACT_RELU, ACT_SILU, OUT_FILL, U24, act64,
                        act_sens64, assert_act_close, assert_exact_headroom, dcn_act64, dcn_is_residue, int_tensor, parity_log,
                        round_to)

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float32
NAME = {BF: "bf16", FP: "f32"}
SILU, GELU, DCN = ACT_SILU, ACT_GELU, ACT_DCN_OFFSETS
ACT_NAME = {SILU: "silu", GELU: "gelu", DCN: "dcn"}
MAG = 10.0
K_SILU_DIV, K_SILU_RCP, K_GELU, K_DCN = 6, 8, 4, 5


def _ops():
    from flair_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ the exact pre-activation
def shift_for(conv):
    """s with std(conv) * 2^-s about 3 (between 2.1 and 4.3)."""
    return max(0, round(math.log2(conv.double().std().item() / 3.0)))


def planted(cout, act, period):
    """-> (plus, minus): the couts that get a bias of +128 and of -128 -- in every 64-cout block the second and the last
    but one cout of each class that has four or more couts there."""
    co = torch.arange(cout)
    residue = dcn_is_residue(co, period) if act == DCN else torch.ones(cout, dtype=torch.bool)
    plus, minus = [], []
    for b0 in range(0, cout, 64):
        for cls in (True, False):
            idx = [c for c in range(b0, min(b0 + 64, cout)) if bool(residue[c]) == cls]
            if len(idx) >= 4:
                plus.append(idx[1])
                minus.append(idx[-2])
    return plus, minus


def plant(bias_int, s, act, period):
    """-> (integer bias with +-128 * 2^s on the planted couts, bool (C,) of the planted couts)."""
    plus, minus = planted(bias_int.numel(), act, period)
    b = bias_int.clone()
    b[plus] = 128.0 * 2 ** s
    b[minus] = -128.0 * 2 ** s
    sat = torch.zeros(b.numel(), dtype=torch.bool)
    sat[plus + minus] = True
    return b, sat


def assert_spread(v, sat, act, period, what):
    """v (T, H, W, C) float64: the couts that are not planted cover the range where the activations bend."""
    free = v[..., ~sat]
    inner = ((free.abs() >= 0.25) & (free.abs() <= 4.0)).double().mean().item()
    pos, neg = (free > 0).double().mean().item(), (free < 0).double().mean().item()
    assert inner >= 0.5 and pos >= 0.2 and neg >= 0.2, f"{what}: {inner:.2f} of |v| in [0.25, 4], {pos:.2f} > 0, {neg:.2f} < 0"
    assert free.abs().max().item() < 64.0 and v[..., sat].abs().min().item() > 100.0, what
    if act == DCN:
        cls = dcn_is_residue(torch.arange(v.shape[-1]), period)
        assert bool((cls & ~sat).any()) and bool((~cls & ~sat).any()), f"{what}: one DCN class only"
        assert bool((cls & sat).any()) and bool((~cls & sat).any()), f"{what}: one DCN class only among the planted couts"


def expectations(v, act, period, res, scale):
    """v (T, H, W, C) float64, res: list of (T, H, W, C) float64 -> ref, S, extra (the residual adds' roundings) and `sat`,
    the exact result where the activation is saturated; all float64, out_scale applied."""
    co = torch.arange(v.shape[-1])
    if act == DCN:
        a, cls = dcn_act64(v, co, MAG, period), dcn_is_residue(co, period)
        ideal = torch.where(cls, MAG * torch.sign(v), (v > 0).double())
    else:
        a, ideal = act64(v, act), v.clamp_min(0.0)
    S = act_sens64(v, act, co=co, mag=MAG, period=period)
    extra = torch.zeros_like(v)
    for r in res:
        a, ideal = a + r, ideal + r
        extra = extra + U24 * a.abs()
    return dict(ref=a * scale, S=S * abs(scale), extra=extra * abs(scale), sat=ideal * scale)


def judge(got, e, sat, k, dtype, what, tile):
    """The per-element bound everywhere, no NaN / Inf, and the exact expectation on the planted couts."""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got.float()).all()), f"{what}: NaN or Inf in the output"
    ratio = assert_act_close(got, e["ref"], e["S"], k, dtype, what, tile=tile, extra=e["extra"])
    want = round_to(e["sat"][..., sat].contiguous(), dtype)
    bad = ~((got[..., sat].double() - want).abs() <= ACT_FLOOR)
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} saturated element(s) are not exact; first at {list(first)} "
                             f"(planted cout {sat.nonzero().flatten()[first[-1]].item()}): got {got[..., sat][first].item()!r}, "
                             f"expected {want[first].item()!r}")
    parity_log(f"act_exact {what}: max err / (2^-24 S) = {ratio:.3f} (k = {k})")
    return ratio


# ------------------------------------------------------------------------------------------------ flair_conv_nhwc
Conv = collections.namedtuple("Conv", "T H W segs cout k R act nres scale bf fp period fb splitk")


def A(T, H, W, segs, cout, k, R, act, nres, scale, bf, fp, period=48, fb=False, splitk=False):
    return Conv(T, H, W, tuple(segs), cout, k, R, act, nres, scale, bf, fp, period, fb, splitk)


def three(T, H, W, segs, cout, k, R, bf, fp, nres=(1, 0, 1), scales=(0.5, 1.0, 2.0), **kw):
    return [A(T, H, W, segs, cout, k, R, act, n, sc, bf, fp, **kw) for act, n, sc in zip((SILU, GELU, DCN), nres, scales)]


K11, K33, K333 = (1, 1, 1), (1, 3, 3), (3, 3, 3)
# T, H, W, segs, cout, kernel, R, act, residuals, out_scale, variant in bf16, in f32 (None: not run)
CONV_ACT = (
    # ---- im2col variants 0, 1, 2: igemm_epilogue<ACT = 2, 3, 1>
    three(1, 256, 256, [96, 32], 72, K11, 16, 0, 0)
    + three(1, 256, 256, [32, 32], 64, K11, 16, 1, 1, nres=(0, 1, 0))
    + three(2, 16, 16, [32, 32], 64, K33, 8, 2, 2)
    + [A(5, 16, 16, [64], 64, K33, 8, SILU, 0, 1.0, 2, 2, fb=True), A(5, 16, 16, [64], 64, K33, 8, DCN, 1, 0.5, 2, 2, fb=True)]
    # bf16 Cout = 4 (mod 8): store_quad
    + three(2, 16, 16, [32], 36, K33, 16, 2, None)
    # split-K: the reduce kernel's store_quad
    + [A(16, 4, 4, [512], 512, K333, 3, SILU, 1, 2.0, 2, 2, splitk=True), A(16, 4, 4, [512], 512, K333, 3, GELU, 0, 1.0, 2, 2, splitk=True)]
    # act_period 24 and 72 (8 consecutive couts in one class is tightest at 24)
    + [A(2, 16, 16, [32], 216, K33, 16, DCN, 0, 1.0, 2, 2, period=24), A(2, 16, 16, [32], 648, K33, 16, DCN, 1, 0.5, 2, 2, period=72)]
    # ---- halo variants 3, 4, 5 and K-split halo variants 6, 7
    + three(4, 136, 128, [32], 48, K33, 16, 3, 3)
    + three(2, 136, 128, [32], 48, K33, 16, 4, 4, nres=(0, 1, 0))
    + three(2, 16, 32, [32, 32], 64, K33, 8, 5, 5)
    + three(2, 16, 32, [32], 36, K33, 16, 5, None)               # bf16 Cout = 4 (mod 8): the halo kernel's store_quad calls
    + [A(2, 16, 32, [32], 216, K33, 16, DCN, 1, 2.0, 5, 5, period=24), A(2, 16, 32, [32], 648, K33, 16, DCN, 0, 1.0, 5, 5, period=72)]
    + three(1, 250, 256, [32], 48, K33, 16, 6, 6, nres=(2, 0, 1))
    + three(1, 125, 128, [32], 72, K33, 16, 7, 7, nres=(0, 1, 2), fb=True)
    # ---- variant 8 (bf16), epilogue_as: SiLU without and with res0 + res1, DCN with out_scale != 1, DCN at Cout = 432; GELU
    # at this geometry falls to the halo kernel
    + [A(4, 128, 128, [64], 128, K33, 8, SILU, 0, 1.0, 8, None), A(4, 128, 128, [64], 128, K33, 8, SILU, 2, 0.5, 8, None),
       A(4, 128, 128, [64], 128, K33, 8, DCN, 1, 0.5, 8, None), A(4, 128, 128, [64], 128, K33, 8, GELU, 1, 2.0, 3, None),
       A(1, 128, 128, [128], 432, K33, 8, DCN, 0, 1.0, 8, None)]
    # ---- variant 9 (bf16), epilogue_plain_as of the one-tile LDS-DMA kernel; conv_frame_kernel takes the leaky class only, so
    # SiLU at its geometry lands on the one-tile kernel as well; GELU falls to the K-split halo kernel
    + [A(1, 128, 256, [32], 128, K33, 16, SILU, 1, 2.0, 9, None), A(1, 128, 256, [32], 128, K33, 16, DCN, 2, 0.5, 9, None),
       A(1, 128, 256, [32], 128, K33, 16, GELU, 0, 1.0, 6, None), A(1, 256, 256, [32], 64, K33, 16, SILU, 0, 0.5, 9, None)]
)
CONV_RUNS = [(c, dt) for c in CONV_ACT for dt in (BF, FP) if (c.bf if dt == BF else c.fp) is not None]


def _conv_id(v):
    if isinstance(v, torch.dtype):
        return NAME[v]
    return (f"v{v.bf}-{v.T}x{v.H}x{v.W}-{'+'.join(map(str, v.segs))}-o{v.cout}-k{''.join(map(str, v.k))}-{ACT_NAME[v.act]}"
            f"-r{v.nres}-s{v.scale}-p{v.period}" + ("-fb" if v.fb else "") + ("-splitk" if v.splitk else ""))


def conv_k(case, dtype):
    """The k of the epilogue copy the case lands on: only variant 8 spells SiLU with v_rcp_f32."""
    if case.act == SILU:
        return K_SILU_RCP if (case.bf if dtype == BF else case.fp) == 8 else K_SILU_DIV
    return K_GELU if case.act == GELU else K_DCN


@functools.lru_cache(maxsize=1)
def conv_preact(case):
    """-> the integer data of the geometry, s, the scaled bias / frame bias the kernel gets, the exact v (T, H, W, C) float64,
    its parts (conv, bias, frame bias: for the CPU mutants) and the planted couts.  Shared by the dtypes; read only."""
    c = case
    d = conv_data(c.T, c.H, c.W, c.segs, c.cout, c.k, c.R)
    s = shift_for(d["conv"])
    bias, sat = plant(d["bias"], s, c.act, c.period)
    add = bias.view(1, -1, 1, 1).double()
    fb = d["fb"] if c.fb else None
    assert_exact_headroom(d["mag"] + add.abs() + (fb[:, :c.cout, None, None].abs().double() if c.fb else 0.0))
    step = 2.0 ** -s
    parts = dict(conv=(d["conv"].double() * step).permute(0, 2, 3, 1), bias=(bias.double() * step).view(1, 1, 1, -1),
                 fb=(fb[:, None, None, :c.cout].double() * step) if c.fb else None)
    v = (parts["conv"] + parts["bias"] + (parts["fb"] if c.fb else 0.0)).contiguous()
    assert_spread(v, sat, c.act, c.period, _conv_id(c))
    res = [(r.double() / 8).permute(0, 2, 3, 1).contiguous() for r in d["res"][:c.nres]]
    return dict(d=d, s=s, bias=bias * step, fb=fb * step if c.fb else None, v=v, sat=sat, res=res, parts=parts)


@functools.lru_cache(maxsize=1)
def conv_expect(case):
    p = conv_preact(case)
    return expectations(p["v"], case.act, case.period, p["res"], case.scale)


def test_act_cases_reach_every_variant():
    """Every case is listed under the variant flair_conv_variant gives it (the activation is part of the choice); SiLU and
    DCN reach 0..9 in bf16 and 0..7 in f32, GELU 0..7 in both; periods 24, 48 and 72 occur."""
    ops = _ops()
    seen = collections.defaultdict(set)
    for c, dt in CONV_RUNS:
        v = ops.conv_variant(c.T, c.H, c.W, list(c.segs), c.cout, c.k, dtype=dt, act=c.act)
        assert v == (c.bf if dt == BF else c.fp), (_conv_id(c), NAME[dt], v)
        seen[c.act, dt].add(v)
    for act in (SILU, DCN):
        assert seen[act, BF] == set(range(10)) and seen[act, FP] == set(range(8)), (ACT_NAME[act], dict(seen))
    assert seen[GELU, BF] == set(range(8)) and seen[GELU, FP] == set(range(8)), dict(seen)
    assert {c.period for c in CONV_ACT if c.act == DCN} == {24, 48, 72}
    assert any(c.cout % 8 == 4 for c in CONV_ACT) and any(c.splitk for c in CONV_ACT) and any(c.fb for c in CONV_ACT)


@pytest.mark.parametrize("case,dtype", CONV_RUNS, ids=_conv_id)
def test_conv_act_exact(dev, case, dtype):
    ops = _ops()
    c = case
    variant = c.bf if dtype == BF else c.fp
    assert ops.conv_variant(c.T, c.H, c.W, list(c.segs), c.cout, c.k, dtype=dtype, act=c.act) == variant
    p, e = conv_preact(c), conv_expect(c)
    d, step = p["d"], 2.0 ** -p["s"]
    xs, o = [], 0
    for n in c.segs:
        xs.append(nhwc(d["x"][:, o:o + n], dtype, dev))
        o += n
    wp = ops.pack_conv_weight(d["w"] * step, [(n, n) for n in c.segs], dtype).to(dev)
    rs = [r.to(dev, dtype) for r in p["res"]] + [None, None]
    if c.splitk:
        q = ops.ConvParams()
        q.dtype = 1 if dtype == BF else 0
        q.T, q.H, q.W = c.T, c.H, c.W
        q.KT, q.KH, q.KW = c.k
        q.Cout, q.nseg, q.stride, q.y_ld, q.act = c.cout, len(c.segs), 1, c.cout + 8, c.act
        for i, n in enumerate(c.segs):
            q.seg_c[i] = q.seg_ld[i] = n
        assert ops._conv_ws_bytes(q) > 0, "the deep-K geometry no longer splits K"
    out = torch.full((c.T, c.H, c.W, c.cout + 8), OUT_FILL, dtype=dtype, device=dev)
    ops.conv(xs, wp, p["bias"].to(dev), c.cout, c.k, out=out, act=c.act, res0=rs[0], res1=rs[1], out_scale=c.scale,
             frame_bias=p["fb"].to(dev) if c.fb else None, act_param=MAG if c.act == DCN else 0.0,
             act_period=c.period if c.act == DCN else 0)
    torch.cuda.synchronize()
    what = f"conv {_conv_id(c)} {NAME[dtype]}"
    assert bool((out[..., c.cout:] == OUT_FILL).all()), f"{what}: pad channels of the output buffer were written"
    rows = {3: 8, 4: 4, 5: 2, 6: 8, 7: 4, 8: 16, 9: 8}.get(variant, 8)
    judge(out[..., :c.cout], e, p["sat"], conv_k(c, dtype), dtype, what, (rows, 32, min(64, c.cout)))


# ------------------------------------------------------------------------------------------------ flair_conv_chain
# T, H, W, segs (None: no stage A), c_mid, coutB, act, residuals, out_scale, act_period, dtypes.  stage = "B": stage A is an
# exact ReLU convolution and `act` is stage B's; stage = "A": `act` is stage A's and stage B is the selector.
Chain = collections.namedtuple("Chain", "stage T H W segs cm coutB act nres scale period dtypes")
BOTH = (BF, FP)
CHAIN_ACT = [
    # conv_resident_kernel in bf16 (C = 64, no stage A, W % 32 == 0, H % 8 == 0, no residuals), the general kernel in f32
    Chain("B", 1, 64, 64, None, 64, 432, SILU, 0, 0.5, 48, BOTH), Chain("B", 1, 64, 64, None, 64, 432, DCN, 0, 0.5, 48, BOTH),
    Chain("B", 1, 64, 64, None, 64, 72, SILU, 0, 2.0, 24, (BF,)), Chain("B", 1, 64, 64, None, 64, 72, DCN, 0, 2.0, 24, (BF,)),
    # conv_pair_kernel's geometry with both residuals: SiLU and DCN are outside its `lin` class -> the general kernel
    Chain("B", 1, 64, 64, (64,), 64, 64, SILU, 2, 0.5, 48, (BF,)), Chain("B", 1, 64, 64, (64,), 64, 64, DCN, 2, 0.5, 48, (BF,)),
    # the general kernel at c = 64 and c = 128, and without stage A at c = 128 (tiles hang over the image bottom)
    Chain("B", 2, 32, 32, (64, 32), 64, 64, SILU, 1, 2.0, 48, BOTH), Chain("B", 2, 32, 32, (64, 32), 64, 64, DCN, 1, 2.0, 48, BOTH),
    Chain("B", 1, 32, 64, (128,), 128, 128, SILU, 2, 1.0, 48, BOTH), Chain("B", 1, 32, 64, (128,), 128, 128, DCN, 2, 1.0, 48, BOTH),
    Chain("B", 1, 20, 32, None, 128, 72, SILU, 1, 0.5, 48, BOTH), Chain("B", 1, 20, 32, None, 128, 72, DCN, 1, 0.5, 24, BOTH),
    # stage A's act_vec, read through the selector
    Chain("A", 2, 32, 32, (64, 32), 64, 64, SILU, 0, 1.0, 48, BOTH), Chain("A", 1, 32, 64, (128,), 128, 128, SILU, 0, 1.0, 48, BOTH),
]
CHAIN_RUNS = [(c, dt) for c in CHAIN_ACT for dt in c.dtypes]


def _chain_id(v):
    if isinstance(v, torch.dtype):
        return NAME[v]
    return (f"{v.stage}-{v.T}x{v.H}x{v.W}-{'+'.join(map(str, v.segs)) if v.segs else 'noA'}-c{v.cm}-o{v.coutB}-{ACT_NAME[v.act]}"
            f"-r{v.nres}-s{v.scale}-p{v.period}")


def chain_resident(c, dtype):
    """flair_conv_chain's host rule for conv_resident_kernel (the output buffer's stride is a multiple of 8 channels here)."""
    return c.segs is None and dtype == BF and c.cm == 64 and c.W % 32 == 0 and c.H % 8 == 0 and c.nres == 0 and c.coutB % 8 == 0


def chain_k(c, dtype):
    if c.act == SILU:
        return K_SILU_RCP if chain_resident(c, dtype) else K_SILU_DIV
    return K_DCN


@functools.lru_cache(maxsize=1)
def chain_preact(case, dtype):
    """Stage "B": the intermediate is relu(conv_A + bias_A) on integers, cast with .to(dtype) (integers again), and stage B's
    weights and bias carry 2^-s.  Stage "A": stage A's do."""
    c = case
    d = chain_data(c.T, c.H, c.W, c.segs, c.cm, c.coutB)
    if c.stage == "A":
        conv, mag, bias_int = d["convA"].double(), d["magA"], d["bA"]
    else:
        mid = torch.relu(d["convA"] + d["bA"].view(1, -1, 1, 1)).to(dtype).float() if c.segs else d["x"]
        conv = F.conv2d(mid.double(), d["wB"].double(), padding=1)
        mag = F.conv2d(mid.double().abs(), d["wB"].double().abs(), padding=1)
        bias_int = d["bB"]
    s = shift_for(conv)
    bias, sat = plant(bias_int, s, c.act, c.period)
    assert_exact_headroom(mag + bias.abs().double().view(1, -1, 1, 1))
    step = 2.0 ** -s
    v = ((conv + bias.double().view(1, -1, 1, 1)) * step).permute(0, 2, 3, 1).contiguous()
    assert_spread(v, sat, c.act, c.period, _chain_id(c))
    res = [(r.double() / 8).permute(0, 2, 3, 1).contiguous() for r in d["res"][:c.nres]]
    return dict(d=d, s=s, bias=bias * step, v=v, sat=sat, res=res, e=expectations(v, c.act, c.period, res, c.scale))


def test_chain_cases_reach_every_kernel():
    """conv_resident_kernel under SiLU and DCN with a full and a partial last block, the general kernel with and without
    stage A at both widths and in both types, stage A's activation at both widths."""
    res = [c for c in CHAIN_ACT if chain_resident(c, BF)]
    assert {(c.act, c.coutB % 64 == 0) for c in res} >= {(SILU, False), (DCN, False)} and {c.period for c in res} == {24, 48}
    assert all(c.scale != 1.0 for c in res)
    gen = {(c.act, c.cm, c.segs is not None, dt) for c, dt in CHAIN_RUNS if c.stage == "B" and not chain_resident(c, dt)}
    assert gen >= {(a, cm, hasA, dt) for a in (SILU, DCN) for cm in (64, 128) for hasA in (True, False) for dt in BOTH
                   if (cm, hasA, dt) != (64, False, BF)}, gen
    assert {(c.cm, dt) for c, dt in CHAIN_RUNS if c.stage == "A"} == {(64, BF), (64, FP), (128, BF), (128, FP)}


@pytest.mark.parametrize("case,dtype", CHAIN_RUNS, ids=_chain_id)
def test_conv_chain_act_exact(dev, case, dtype):
    ops = _ops()
    c = case
    p = chain_preact(c, dtype)
    d, step = p["d"], 2.0 ** -p["s"]
    xs, o = [], 0
    for n in (c.segs or (c.cm,)):
        xs.append(nhwc(d["x"][:, o:o + n], dtype, dev))
        o += n
    if c.stage == "A":
        wA, bA, actA = d["wA"] * step, p["bias"], c.act
        wB = torch.zeros(c.coutB, c.cm, 3, 3)
        wB[torch.arange(c.cm), torch.arange(c.cm), 1, 1] = 1.0
        bB, actB = torch.zeros(c.coutB), ACT_NONE
    else:
        wA, bA, actA = (d["wA"], d["bA"], ACT_RELU) if c.segs else (None, None, ACT_NONE)
        wB, bB, actB = d["wB"] * step, p["bias"], c.act
    wAp = ops.pack_conv_weight(wA[:, :, None], [(n, n) for n in c.segs], dtype).to(dev) if c.segs else None
    wBp = ops.pack_conv_weight(wB[:, :, None], [(c.cm, c.cm)], dtype).to(dev)
    rs = [r.to(dev, dtype) for r in p["res"]] + [None, None]
    out = torch.full((c.T, c.H, c.W, c.coutB + 8), OUT_FILL, dtype=dtype, device=dev)
    ops.conv_chain(xs, wAp, bA.to(dev) if c.segs else None, actA, wBp, bB.to(dev), actB, c.cm, c.coutB, res0=rs[0], res1=rs[1],
                   out_scale=c.scale, out=out, act_param=MAG if c.act == DCN else 0.0, act_period=c.period if c.act == DCN else 0)
    torch.cuda.synchronize()
    what = f"conv_chain {_chain_id(c)} {NAME[dtype]}"
    assert bool((out[..., c.coutB:] == OUT_FILL).all()), f"{what}: pad channels of the output buffer were written"
    judge(out[..., :c.coutB], p["e"], p["sat"], chain_k(c, dtype), dtype, what, (8, 32, 64))


# ------------------------------------------------------------------------------------------------ flair_dwconv_nhwc
DW_SHAPES = [(2, 9, 11, 16), (1, 16, 16, 32)]


@functools.lru_cache(maxsize=2)
def dw_preact(shape, stride):
    """test_dwconv_exact's data; depthwise taps and bias times 2^-s -> x, taps, bias, v (T, Ho, Wo, C) float64, planted couts."""
    T, H, W, Cc = shape
    g = torch.Generator().manual_seed(10 + stride + Cc)
    x = int_tensor((T, Cc, H, W), -8, 8, g)
    w_dw = int_tensor((9, Cc), -3, 3, g)
    b_dw = int_tensor((Cc,), -8, 8, g)
    wd = w_dw.double().t().reshape(Cc, 1, 3, 3)
    conv = F.conv2d(x.double(), wd, stride=stride, padding=1, groups=Cc)
    s = shift_for(conv)
    bias, sat = plant(b_dw, s, SILU, 48)
    assert_exact_headroom(F.conv2d(x.double().abs(), wd.abs(), stride=stride, padding=1, groups=Cc) + bias.abs().double().view(1, -1, 1, 1))
    step = 2.0 ** -s
    v = ((conv + bias.double().view(1, -1, 1, 1)) * step).permute(0, 2, 3, 1).contiguous()
    assert_spread(v, sat, SILU, 48, f"dwconv {shape} s{stride}")
    return dict(x=x, w=w_dw * step, bias=bias * step, v=v, sat=sat)


def dw_expect(v, act, pw):
    """Without the 1x1 stage a(v).  With the selector 1x1 the kernel applies the activation again: a(a(v)), where the
    first stage's error k u S(v) passes through a slope of at most Lip(a)."""
    e = expectations(v, act, 48, [], 1.0)
    if pw:
        e2 = expectations(e["ref"], act, 48, [], 1.0)
        e2["S"] = e2["S"] + ACT_LIPSCHITZ[act] * e["S"]
        e2["sat"] = e["sat"]                                      # a(a(v)) = v and a(0) = 0 at +-128
        return e2
    return e


@pytest.mark.parametrize("act", [SILU, GELU], ids=lambda a: ACT_NAME[a])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pw", [False, True], ids=["dw", "dw+selector"])
@pytest.mark.parametrize("shape", DW_SHAPES)
def test_dwconv_act_exact(dev, shape, pw, stride, act):
    ops = _ops()
    p = dw_preact(shape, stride)
    Cc = shape[3]
    v = p["v"]
    out = torch.full((v.shape[0], v.shape[1], v.shape[2], Cc + 8), OUT_FILL, dtype=FP, device=dev)
    ops.dwconv(nhwc(p["x"], FP, dev), p["w"].to(dev), p["bias"].to(dev), stride=stride,
               pw=(torch.eye(Cc).to(dev), None) if pw else None, act=act, out=out[..., :Cc])
    torch.cuda.synchronize()
    what = f"dwconv {shape} s{stride} {'dw+selector' if pw else 'dw'} {ACT_NAME[act]}"
    assert bool((out[..., Cc:] == OUT_FILL).all()), f"{what}: pad channels of the output buffer were written"
    judge(out[..., :Cc], dw_expect(v, act, pw), p["sat"], K_SILU_DIV if act == SILU else K_GELU, FP, what, (1, 4, 4))
