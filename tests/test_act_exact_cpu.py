"""The method of tests/test_gpu_act_exact.py, proved without a GPU: the derived k of every epilogue form covers its error
model, f32 restatements of the kernels' formulas stay within k / 2 on the test's own data (planted +-128 couts included),
the same comparison rejects every mutant listed below in f32 and in bf16, the pre-activations of every GPU case are spread
as the method needs, and dcn_act64's class map is the reference's chunk(3) order."""
import math

import pytest
import torch

from tests.test_gpu_act_exact import (BF, CHAIN_RUNS, CONV_ACT, DCN, DW_SHAPES, FP, GELU, K_DCN, K_GELU, K_SILU_DIV, K_SILU_RCP, MAG,
                                      SILU, A, K33, chain_preact, conv_expect, conv_preact, dw_preact, expectations, planted)
from tests.util import ACT_FLOOR, U24, act64, act_sens64, assert_act_close, bits, dcn_act64, dcn_is_residue, round_to

LOG2E = 1.4426950408889634


# ------------------------------------------------------------------------------------------------ k against the error model
def test_k_covers_the_error_model_of_every_form():
    """The docstring's error models, in units of 2^-24, against S on a grid of 2 * 10^5 points in [-40, 40]."""
    v = torch.linspace(-40, 40, 200001, dtype=torch.float64)
    s, t = torch.sigmoid(v), torch.tanh(v)
    sup = lambda num, S: (num / S.clamp_min(1e-300)).max().item()
    S = act_sens64(v, SILU)
    a = (v * s).abs()
    assert 5.0 < sup(a * ((1 - s) * (2 * v.abs() + 2) + 2), S) <= K_SILU_DIV
    assert 7.0 < sup(a * ((1 - s) * (2 * v.abs() + 2) + 4), S) <= K_SILU_RCP
    erf, phi = torch.erf(v * math.sqrt(0.5)), torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    assert sup(2 * v * v * phi + 4 * v.abs() * erf.abs() + 2 * (0.5 * v * (1 + erf)).abs(), act_sens64(v, GELU)) <= K_GELU
    res, msk = torch.zeros(1, dtype=torch.long), torch.full((1,), 40)
    S = act_sens64(v[:, None], DCN, co=res, mag=MAG, period=48)[:, 0]
    assert sup(MAG * ((1 - t * t) * (2 * v.abs() + 1) + 3 * (1 - t) + 2 * t.abs()), S) <= 4.0 + 1e-9 <= K_DCN
    S = act_sens64(v[:, None], DCN, co=msk, mag=MAG, period=48)[:, 0]
    assert 4.9 < sup(s * ((1 - s) * (2 * v.abs() + 2) + 4), S) <= K_DCN


# ------------------------------------------------------------------------------------------------ restatements
SILU_CASE = A(5, 16, 16, [64], 64, K33, 8, SILU, 1, 0.5, 2, 2, fb=True)
GELU_CASE = A(2, 16, 16, [32, 32], 64, K33, 8, GELU, 1, 0.5, 2, 2)
DCN_CASE = A(2, 16, 16, [32], 216, K33, 16, DCN, 1, 0.5, 2, 2, period=24)


def _finish(a32, case, dtype):
    """The epilogue after the activation in f32, as the kernels run it: + residuals, * out_scale, the cast."""
    for r in conv_preact(case)["res"]:
        a32 = a32 + r.float()
    return (a32 * torch.tensor(case.scale, dtype=FP)).to(dtype)


def _rcp(x):
    return torch.ones_like(x) / x


def restatements(case):
    """name -> (f32 activation of the exact v, k of that form)."""
    v = conv_preact(case)["v"].float()
    assert torch.equal(v.double(), conv_preact(case)["v"])
    if case.act == SILU:
        return {"divide SiLU": (v / (1 + torch.exp(-v)), K_SILU_DIV), "reciprocal SiLU": (v * _rcp(1 + torch.exp(-v)), K_SILU_RCP),
                "exp2 SiLU": (v * _rcp(1 + torch.exp2(torch.tensor(-LOG2E, dtype=FP) * v)), K_SILU_RCP)}
    if case.act == GELU:
        return {"erf GELU": (0.5 * v * (1 + torch.erf(v * torch.tensor(math.sqrt(0.5), dtype=FP))), K_GELU)}
    cls = dcn_is_residue(torch.arange(v.shape[-1]), case.period)
    mag = torch.tensor(MAG, dtype=FP)
    slow = torch.where(cls, mag * (1 - 2 * _rcp(1 + torch.exp(2 * v))), _rcp(1 + torch.exp(-v)))
    kk = torch.where(cls, torch.tensor(2 * LOG2E, dtype=FP), torch.tensor(-LOG2E, dtype=FP))
    r = _rcp(1 + torch.exp2(kk * v))
    fast = (r.double() * torch.where(cls, -2 * MAG, 1.0) + torch.where(cls, MAG, 0.0)).float()         # one fma
    return {"mag (1 - 2 r) | sigmoid": (slow, K_DCN), "fma(rcp(1 + 2^(k v)), A, B)": (fast, K_DCN)}


@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [SILU_CASE, GELU_CASE, DCN_CASE], ids=["silu", "gelu", "dcn"])
def test_f32_restatements_stay_within_half_the_bound(case, dtype):
    e, sat = conv_expect(case), conv_preact(case)["sat"]
    for name, (a32, k) in restatements(case).items():
        got = _finish(a32, case, dtype)
        assert bool(torch.isfinite(got.float()).all()), name
        assert_act_close(got, e["ref"], e["S"], k / 2, dtype, name, extra=e["extra"])
        want = round_to(e["sat"][..., sat].contiguous(), dtype)
        assert bool(((got[..., sat].double() - want).abs() <= ACT_FLOOR).all()), f"{name}: saturated couts"


def test_fma_form_with_out_scale_folded_in():
    """conv_resident_kernel's fold: A and B carry out_scale (a power of two), no residual."""
    case = DCN_CASE._replace(nres=0, scale=0.5)
    v = conv_preact(case)["v"].float()
    cls = dcn_is_residue(torch.arange(v.shape[-1]), case.period)
    kk = torch.where(cls, torch.tensor(2 * LOG2E, dtype=FP), torch.tensor(-LOG2E, dtype=FP))
    r = _rcp(1 + torch.exp2(kk * v))
    got = (r.double() * torch.where(cls, -2 * MAG * 0.5, 0.5) + torch.where(cls, MAG * 0.5, 0.0)).float()
    e = conv_expect(case)
    for dtype in (FP, BF):
        assert_act_close(got.to(dtype), e["ref"], e["S"], K_DCN / 2, dtype, "folded fma form")


# ------------------------------------------------------------------------------------------------ mutants
def _mutants(case):
    """name -> float64 output of an epilogue with one fault, on the case's exact data."""
    p = conv_preact(case)
    v, parts, res, sc = p["v"], p["parts"], p["res"], case.scale
    co = torch.arange(v.shape[-1])
    act = (lambda x, shift=0, mag=MAG: dcn_act64(x, co + shift, mag, case.period)) if case.act == DCN else (lambda x: act64(x, case.act))
    rsum = sum(res) if res else 0.0
    out = {}
    if case.act == GELU:
        out["tanh-approximated GELU"] = (0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3))) + rsum) * sc
        out["v * sigmoid(1.702 v) as GELU"] = (v * torch.sigmoid(1.702 * v) + rsum) * sc
    if case.act == SILU:
        out["pre-activation rounded to bf16"] = (act(v.float().to(BF).double()) + rsum) * sc
    if case.act == DCN:
        cls = dcn_is_residue(co, case.period)
        out["sigmoid of 2 v on the masks"] = (torch.where(cls, MAG * torch.tanh(v), torch.sigmoid(2 * v)) + rsum) * sc
        out["classes swapped"] = (torch.where(cls, torch.sigmoid(v), MAG * torch.tanh(v)) + rsum) * sc
        out["class boundary shifted by 8 channels"] = (act(v, shift=8) + rsum) * sc
        out["mag of 1"] = (act(v, mag=1.0) + rsum) * sc
    out["bias added after the activation"] = (act(v - parts["bias"]) + parts["bias"] + rsum) * sc
    if case.fb:
        out["frame bias added after the activation"] = (act(v - parts["fb"]) + parts["fb"] + rsum) * sc
    assert res and sc != 1.0
    out["out_scale applied before the residual add"] = act(v) * sc + rsum
    out["residual added before the activation"] = act(v + rsum) * sc
    return out


@pytest.mark.parametrize("dtype", [FP, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [SILU_CASE, GELU_CASE, DCN_CASE], ids=["silu", "gelu", "dcn"])
def test_every_mutant_fails_the_comparison(case, dtype):
    e = conv_expect(case)
    k = {SILU: K_SILU_RCP, GELU: K_GELU, DCN: K_DCN}[case.act]           # the widest k of the class
    assert_act_close(e["ref"].float().to(dtype), e["ref"], e["S"], k, dtype, "the reference itself", extra=e["extra"])
    muts = _mutants(case)
    assert len(muts) >= 4
    for name, m in muts.items():
        with pytest.raises(AssertionError, match="beyond"):
            assert_act_close(m.float().to(dtype), e["ref"], e["S"], k, dtype, name, extra=e["extra"], tile=(8, 32, 24))


def test_a_shifted_class_boundary_is_named_by_the_histogram():
    """Period 24, boundary off by 8: the couts 8..15 of every period become masks, 16..23 residues -- and nothing else."""
    e = conv_expect(DCN_CASE)
    m = _mutants(DCN_CASE)["class boundary shifted by 8 channels"]
    with pytest.raises(AssertionError) as err:
        assert_act_close(m.float(), e["ref"], e["S"], K_DCN, FP, "shifted", extra=e["extra"], tile=(8, 32, 24))
    hist = [int(x) for x in str(err.value).split("by c % 24: [")[1].split("]")[0].split(",")]
    assert all(h == 0 for h in hist[:8]) and all(h > 0 for h in hist[8:]), hist


@pytest.mark.parametrize("case", [SILU_CASE, GELU_CASE, DCN_CASE], ids=["silu", "gelu", "dcn"])
def test_truncation_instead_of_rne_fails_in_bf16(case):
    e = conv_expect(case)
    trunc = (bits(e["ref"].float()) & ~0xFFFF).view(FP).to(BF)
    with pytest.raises(AssertionError, match="beyond"):
        assert_act_close(trunc, e["ref"], e["S"], K_SILU_RCP, BF, "truncated", extra=e["extra"])


def test_nan_and_inf_fail():
    e = conv_expect(SILU_CASE)
    for bad in (float("nan"), float("inf")):
        got = e["ref"].float()
        got[1, 2, 3, 4] = bad
        with pytest.raises(AssertionError):
            assert_act_close(got, e["ref"], e["S"], K_SILU_DIV, FP, "nan", extra=e["extra"])


# ------------------------------------------------------------------------------------------------ spread, class map
def test_planted_couts_cover_every_block_and_class():
    assert planted(8, SILU, 48) == ([1], [6])
    assert planted(36, DCN, 48) == ([1, 33], [30, 34])
    plus, minus = planted(216, DCN, 24)
    cls = dcn_is_residue(torch.arange(216), 24)
    for b0 in range(0, 216, 64):
        for c in (True, False):
            assert any(b0 <= i < b0 + 64 and bool(cls[i]) == c for i in plus) and any(b0 <= i < b0 + 64 and bool(cls[i]) == c for i in minus)


def test_pre_activations_of_every_gpu_case_are_spread():
    """conv_preact / chain_preact / dw_preact assert the spread (assert_spread) and the exact headroom of their case."""
    seen = set()
    for c in CONV_ACT:
        key = c._replace(nres=0, scale=1.0, bf=0, fp=0, act=DCN if c.act == DCN else SILU, period=c.period if c.act == DCN else 48)
        if key not in seen:
            seen.add(key)
            s = conv_preact(c)["s"]
            assert 0 <= s <= 12
    for c, dt in CHAIN_RUNS:
        chain_preact(c, dt)
    for shape in DW_SHAPES:
        for stride in (1, 2):
            dw_preact(shape, stride)


@pytest.mark.parametrize("G", [8, 16, 24])
def test_dcn_class_map_is_the_reference_order(G):
    """The reference activates conv_offset's output as chunk(3): o1 | o2 (tanh) | mask (sigmoid); ops.dcn_raw_permutation
    takes that order to the tap-major one the kernels write, where the class is 3 * (co % period) < 2 * period."""
    from flair_amd import ops
    period = 3 * G
    perm = ops.dcn_raw_permutation(G)
    co = torch.arange(27 * G)
    assert torch.equal(dcn_is_residue(co, period), perm < 18 * G)
    raw = torch.linspace(-3, 3, 27 * G, dtype=torch.float64)[torch.randperm(27 * G, generator=torch.Generator().manual_seed(G))]
    o1, o2, mask = raw.chunk(3)
    ref = torch.cat([MAG * torch.tanh(torch.cat((o1, o2))), torch.sigmoid(mask)])
    assert torch.equal(dcn_act64(raw[perm][None], co, MAG, period)[0], ref[perm])


def test_expectations_count_every_residual_add():
    v = torch.tensor([[[[1.0, -2.0]]]], dtype=torch.float64)
    r = torch.tensor([[[[4.0, 8.0]]]], dtype=torch.float64)
    e = expectations(v, SILU, 48, [r, r], 0.5)
    a = act64(v, SILU)
    assert torch.equal(e["ref"], (a + r + r) * 0.5) and torch.equal(e["extra"], U24 * ((a + r).abs() + (a + r + r).abs()) * 0.5)
    assert torch.equal(e["sat"], (v.clamp_min(0) + r + r) * 0.5)
