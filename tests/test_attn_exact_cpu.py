"""The exact-softmax harness of tests/test_gpu_attn_exact.py, checked without a GPU: the preconditions of its input
builders for every GPU case, its float64 references against the project's oracles, its two assertion helpers, and the
written record of the gap it closes -- a phantom key beyond L with score 0 and a softmax scale off by 1 %, emulated in
float64, pass test_gpu_kernels.test_qkv_attention's assert_close on that test's randn data, while the tie test fails on
the first and the staircase test on the second."""
import math

import pytest
import torch

from tests.test_gpu_attn_exact import (BF, BF16_REL, FP, P_, SPATIAL, TEMPORAL_D, TEMPORAL_D_MORE, TEMPORAL_HEADS, _id, _tseed, f32_rel,
                                       selection_case, staircase_case, temporal_selection_case, temporal_shapes, tie_case)
from tests.test_gpu_attn_exact import test_cases_reach_every_attention_build as _cases_reach_every_build
from tests.util import (MARGIN, QKV_LAYOUTS, STAIRS, assert_attn_close, assert_close, assert_exact_headroom, assert_within_ulps,
                        attn_ref64, bits, heads_to_clip, ordered_bits, pack_qkv, rb, round_to, sign_code, stair_levels,
                        temporal_ref64, temporal_staircase, temporal_tie, temporal_windows, window_frames)

HALF = torch.float16


def _exact_in(t, *dtypes):
    return all(torch.equal(rb(t, dt), t) for dt in dtypes)


def test_case_table_reaches_every_attention_build():
    _cases_reach_every_build()


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("case", [c for c in SPATIAL if c[4] == BF], ids=_id)
def test_spatial_preconditions(case):
    """Every query of every selection case leads by >= 110 nats; every selection and tie value is exact in bf16; the tie
    sums stay below 2^24 and the tie levels include -64, 0 and +64 (as far as L allows)."""
    fam, d, shapes, L, _ = case
    for frames, heads in shapes:
        for last in (False, True):
            q, k, v, want, margin = selection_case(fam, d, frames, heads, L, last)
            assert margin >= MARGIN, (case, margin)
            assert _exact_in(q, BF) and _exact_in(k, BF) and _exact_in(v, BF) and q.abs().max().item() <= 256
            assert want.shape == v.shape
        q, k, v, want, a = tie_case(fam, d, frames, heads, L)
        assert _exact_in(q, BF) and _exact_in(k, BF) and _exact_in(v, BF)
        assert_exact_headroom(v.double().abs().sum(2))
        assert a[0, 0, :3].tolist() == [-64.0, 0.0, 64.0][:L] and a.abs().max().item() <= 64
        s = q.double() @ k.double().transpose(-1, -2)
        assert torch.equal(s, s[..., :1].expand_as(s))                   # all keys of a query tie exactly
        assert torch.equal(s[..., 0], a.double() * d)
        for variant in STAIRS:
            q, k, v = staircase_case(fam, d, frames, heads, L, variant, BF)[:3]
            assert _exact_in(q, BF) and _exact_in(k, BF) and _exact_in(v, BF)


def test_selection_strength_of_the_issue():
    """A = 64 gives a lead of 112 at (d, L) = (64, 400); at (128, 97) A = 32 falls short (102) and the builder takes 64."""
    q, k, v, want, margin = selection_case("native", 64, 1, 2, 400, False)
    assert q.abs().max().item() == 64 and margin == 112.0
    q, k, v, want, margin = selection_case("native", 128, 1, 2, 97, False)
    assert q.abs().max().item() == 64 and margin >= MARGIN > margin / 2
    with pytest.raises(AssertionError, match="shorten L"):
        from tests.util import selection_strength
        selection_strength(1 << 20, 32)


def test_staircase_levels():
    """About 3 nats per 32-key tile at a = 1; up rises in every tile, down never after tile 0, alt on alternate tiles."""
    for d in (32, 40, 64, 96, 128, 192, 1024):
        z = torch.zeros(130, dtype=torch.long)
        up, down, alt = (stair_levels(130, d, v, z) * math.sqrt(d) for v in STAIRS)
        assert 2.5 <= (up[32] - up[0]).item() <= 4.0, d
        assert torch.equal(up[::32], up[::32].sort().values) and torch.equal(down[::32], down[::32].sort(descending=True).values)
        assert torch.equal(alt[::64], up[::64]) and torch.equal(alt[32::64], down[32::64])


@pytest.mark.parametrize("d", TEMPORAL_D + TEMPORAL_D_MORE)
def test_temporal_preconditions(d):
    for T, window in temporal_shapes(d):
        for kind in ("slot", "frame"):
            q, k, v, kpos, hit, want, margin = temporal_selection_case(kind, d, T, window)
            assert margin >= MARGIN, (kind, d, T, window, margin)
            for z in (q, k, v, kpos):
                assert _exact_in(z, BF, HALF)
            n = hit.sum(-1)
            assert bool((n == 1).all()) if kind == "slot" else bool((n >= 1).all())
            if kind == "frame" and T < window - 1:
                assert bool((n > 1).any())                               # the clamp sends several slots to one frame
        q, k, v, kpos, want = temporal_tie(T, P_, TEMPORAL_HEADS, d, window, torch.Generator().manual_seed(_tseed(d, T, window, 3)))
        for z in (q, k, v):
            assert _exact_in(z, BF, HALF)
        assert v.min().item() >= 0 and v.max().item() <= 256 and not kpos.any()


def test_window_frames_clamp():
    assert window_frames(3, 5).tolist() == [[0, 0, 1, 2], [0, 0, 2, 2], [0, 1, 2, 2]]
    assert window_frames(1, 7).tolist() == [[0] * 6]


# ------------------------------------------------------------------------------------------------ references vs oracles
# The oracles compute in f32 with more roundings than the kernels' bound f32_rel counts: q and k are scaled separately
# (two more per product), the softmax is normalised before P.V (one per term) and the scores, up to X = max|score| nats,
# carry X * 2^-24 of their own.  Hence (2L + 4d + 4R + 4X) * 2^-24 * S, about twice the kernels' bound.
def _oracle_rel(L, d, R, X):
    return (2 * L + 4 * d + 4 * R + 4 * X) * 2.0 ** -24


ORACLE_CASES = [("native", 32, 1, 2, 33), ("native", 64, 1, 2, 130), ("wide", 192, 1, 2, 100), ("prior", 40, 2, 3, 35)]


@pytest.mark.parametrize("layout", QKV_LAYOUTS[:2])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=[f"{c[0]}-d{c[1]}-L{c[4]}" for c in ORACLE_CASES])
def test_float64_reference_agrees_with_the_qkv_oracles(case, layout):
    from oracle.unet import qkv_attention_legacy, qkv_attention_new
    fam, d, frames, heads, L = case
    run = qkv_attention_new if layout == "new" else qkv_attention_legacy

    def oracle(q, k, v):
        x, _ = pack_qkv(q, k, v, layout)
        return run(x[:, 0].permute(0, 2, 1).contiguous(), heads).permute(0, 2, 1).reshape(frames, 1, L, heads * d)
    inputs = [tie_case(fam, d, frames, heads, L)[:3]] + [staircase_case(fam, d, frames, heads, L, v, FP)[:3] for v in STAIRS]
    for q, k, v in inputs:
        ref, S, R = attn_ref64(q, k, v)
        X = (q.double() @ k.double().transpose(-1, -2)).abs().max().item() / math.sqrt(d)
        assert_attn_close(oracle(q, k, v), heads_to_clip(ref), heads_to_clip(S), _oracle_rel(L, d, R, X), f"oracle {case} {layout}")
    q, k, v, want, _ = selection_case(fam, d, frames, heads, L, False)
    assert torch.equal(oracle(q, k, v), heads_to_clip(want))             # one-hot in the oracle's f32 softmax too
    q, k, v, want, _ = selection_case(fam, d, frames, heads, L, False)
    assert torch.equal(attn_ref64(q, k, v)[0].float(), want)             # the float64 reference rounds to exactly the V row
    q, k, v, want, _ = tie_case(fam, d, frames, heads, L)
    assert (attn_ref64(q, k, v)[0] - want).abs().max().item() <= 1e-12 * 256


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("d,T,window", [(8, 3, 5), (24, 2, 7), (64, 6, 5), (96, 1, 3)])
def test_float64_reference_agrees_with_flash_attn_func(d, T, window, fp16):
    """The temporal reference against oracle.thirdparty.flash_attn_func on unfolded windows, as
    test_gpu_kernels.test_temporal_attention builds them."""
    from oracle.thirdparty import flash_attn_func
    heads, n = TEMPORAL_HEADS, window - 1
    g = torch.Generator().manual_seed(d + T)
    cases = [temporal_staircase(T, P_, heads, d, window, g, FP) + (None,), temporal_tie(T, P_, heads, d, window, g)[:4] + (None,)]
    cases += [(lambda c: c[:4] + (c[5],))(temporal_selection_case(kind, d, T, window)) for kind in ("slot", "frame")]
    for q, k, v, kpos, want in cases:
        ref, S, R = temporal_ref64(q, k, v, kpos, window, round_fp16=fp16)
        idx = window_frames(T, window)
        kw, vw = k[idx] + kpos[None, :, None], v[idx]                    # T, n, P, heads, d

        def tok(z):
            return z.permute(0, 2, 1, 3, 4).reshape(T * P_, z.shape[1], heads, d)
        qq = tok(q[:, None])
        if fp16:
            o = flash_attn_func(qq.half(), tok(kw).half(), tok(vw).half()).float()
        else:
            o = flash_attn_func(qq, tok(kw), tok(vw))
        if want is not None:      # selection: one-hot (or an exact tie of clamped slots) in the oracle too
            assert_within_ulps(o.reshape(T, P_, heads, d), want.double(), 1, f"flash_attn_func selection d={d}")
            assert torch.equal(ref.float(), want)
            continue
        X = temporal_windows(q, k, v, kpos, window, fp16)
        X = torch.einsum("tphd,tnphd->tphn", X[0].double(), X[1].double()).abs().max().item() / math.sqrt(d)
        rel = _oracle_rel(n, d, R, X) + (2.0 ** -11 if fp16 else 0.0)
        assert_attn_close(o.reshape(T, P_, heads, d), ref, S, rel, f"flash_attn_func d={d} T={T} window={window}",
                          ab=2.0 ** -25 if fp16 else 0.0)


# ------------------------------------------------------------------------------------------------ the helpers
def test_round_to_rounds_once_to_nearest_even():
    x = torch.tensor([1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -3.0, 0.0, 300.7], dtype=torch.float64)
    assert round_to(x, BF).tolist() == [1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -3.0, 0.0, 300.0]
    # a cast through float32 rounds twice: 1 + 2^-8 + 2^-40 -> 1 + 2^-8 (f32) -> 1 (bf16, tie to even)
    assert x[3].float().to(BF).item() == 1.0 and round_to(x[3:4], BF).item() == 1 + 2.0 ** -7
    y = torch.rand(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 200 - 100
    assert torch.equal(round_to(y, FP), y.float().double()) and torch.equal(round_to(y, HALF), y.half().double())
    with pytest.raises(AssertionError, match="normal range"):
        round_to(torch.tensor([1e-40], dtype=torch.float64), FP)


def test_ordered_bits_orders_across_zero():
    for dt in (FP, BF, HALF):
        tiny = torch.finfo(dt).smallest_normal
        t = torch.tensor([-1.0, -tiny, -0.0, 0.0, tiny, 1.0]).to(dt)
        o = ordered_bits(t)
        assert o[2].item() == o[3].item() == 0 and torch.equal(o, o.sort().values) and o[0].item() == -o[5].item()


def _step(t, n):
    """t moved by n units in the last place (away from zero for n > 0)."""
    return (bits(t) + n).view(t.dtype)


@pytest.mark.parametrize("dt", [FP, BF], ids=["float32", "bfloat16"])
def test_within_ulps_counts_units_in_the_last_place(dt):
    ref64 = torch.tensor([[127.3, 128.0, 0.75, -5.5]], dtype=torch.float64)
    exact = round_to(ref64, dt).to(dt)
    assert assert_within_ulps(exact, ref64, 0) == 0
    assert assert_within_ulps(_step(exact, 1), ref64, 1) == 1
    assert assert_within_ulps(_step(exact, -1), ref64, 1) == 1            # 128 -> the value below it, half as far away
    with pytest.raises(AssertionError, match="4 of 4 element"):
        assert_within_ulps(_step(exact, 1), ref64, 0)
    with pytest.raises(AssertionError, match="largest distance 2 ulp"):
        assert_within_ulps(_step(exact, 2), ref64, 1)
    assert assert_within_ulps(_step(exact, 2), ref64, 2) == 2


@pytest.mark.parametrize("dt", [FP, BF], ids=["float32", "bfloat16"])
def test_within_ulps_sign_change_and_nan(dt):
    tiny = torch.finfo(dt).smallest_normal
    ref64 = torch.tensor([tiny, 1.0], dtype=torch.float64)
    with pytest.raises(AssertionError, match="1 of 2 element"):           # -tiny is 2 * (tiny's ordinal) steps from +tiny
        assert_within_ulps(torch.tensor([-tiny, 1.0]).to(dt), ref64, 1)
    with pytest.raises(AssertionError, match="1 of 2 element"):
        assert_within_ulps(torch.tensor([tiny, -1.0]).to(dt), ref64, 1)
    with pytest.raises(AssertionError, match=r"\(1 NaN\)"):
        assert_within_ulps(torch.tensor([tiny, float("nan")]).to(dt), ref64, 1 << 30)
    with pytest.raises(AssertionError, match=r"\(1 NaN\)"):
        assert_within_ulps(torch.tensor([tiny, 1.0]).to(dt), torch.tensor([tiny, float("nan")], dtype=torch.float64), 1 << 30)
    z = torch.zeros(2, dtype=torch.float64)
    assert assert_within_ulps(torch.tensor([0.0, -0.0]).to(dt), z, 0) == 0


@pytest.mark.parametrize("dt", [FP, BF], ids=["float32", "bfloat16"])
def test_attn_close_is_per_element(dt):
    ref = torch.tensor([[[[1.0, 2.0 ** -7, -2.0]]]], dtype=torch.float64)
    S = torch.tensor([[[[1.0, 1.0, 4.0]]]], dtype=torch.float64)
    rel = 2.0 ** -6
    ok = (ref + torch.tensor([0.5, -0.5, 0.5]) * rel * S).to(dt)          # exact in both types
    assert abs(assert_attn_close(ok, ref, S, rel) - 0.5) < 1e-12
    bad = (ref + torch.tensor([0.0, 1.5, 0.0]) * rel * S).to(dt)          # far inside rel * max|ref|, beyond rel * S
    with pytest.raises(AssertionError, match="1 of 3 element"):
        assert_attn_close(bad, ref, S, rel)
    with pytest.raises(AssertionError, match="1 of 3 element"):           # a sign change
        assert_attn_close(torch.tensor([[[[1.0, -2.0 ** -7, -2.0]]]]).to(dt), ref, S, 2.0 ** -9)
    with pytest.raises(AssertionError, match="1 of 3 element"):
        assert_attn_close(torch.tensor([[[[1.0, float("nan"), -2.0]]]]).to(dt), ref, S, 1e9)
    assert assert_attn_close(bad, ref, S, rel, ab=1.5 * rel) == 0.0


# ------------------------------------------------------------------------------------------------ the written record
# test_gpu_kernels.test_qkv_attention's data (d = 64, seed 11, * 1.5, bf16-rounded) at its cases L = 400, 256 and 1024; the
# first two frames and four heads of each keep the float64 score matrices small
OLD_CASES = [(5, 20, 20, 13), (16, 16, 16, 4), (16, 32, 32, 4)]


def _old_data(case):
    Fr, H, W, heads = case
    C, L = heads * 64, H * W
    qkv = rb(torch.randn(Fr, 3 * C, L, generator=torch.Generator().manual_seed(11)) * 1.5, BF)
    x = qkv[:2].reshape(2, heads, 3, 64, L)[:, :4]                       # the legacy order: heads, then q | k | v
    return tuple(x[:, :, i].transpose(-1, -2).contiguous() for i in range(3))


@pytest.mark.parametrize("case", OLD_CASES, ids=["L400", "L256", "L1024"])
def test_phantom_key_and_scale_error_pass_the_max_norm_bound(case):
    """Both faults, emulated in float64 and rounded to bf16, pass assert_close(scale=2.0) on the old test's data: the phantom
    key by a factor above 100, the 1 % scale error by a factor near 2, with a typical |output| several times below max|ref|."""
    q, k, v = _old_data(case)
    ref, S, _ = attn_ref64(q, k, v)
    bound = 2.0 * 1.6e-2 * ref.abs().max().item() + 1e-3
    phantom = attn_ref64(q, k, v, extra_key_score=0.0)[0]
    scaled = attn_ref64(q, k, v, scale_error=0.01)[0]
    for bad, lo, hi in ((phantom, 1e-4, bound / 100), (scaled, 5e-2, bound / 1.5)):
        err = assert_close(bad, ref, BF, "the fault itself", scale=2.0)
        assert lo <= err <= hi, (err, bound)
        assert_close(rb(bad.float(), BF).double(), ref, BF, "the fault after bf16 rounding of the output passes", scale=2.0)
    assert ref.abs().median().item() * 5 <= ref.abs().max().item()
    # per element the scale error reaches 1.7e-2 ... 2.3e-2 of S: three times the staircase test's bf16 bound
    assert ((scaled - ref).abs() / S).max().item() >= 2.5 * BF16_REL


@pytest.mark.parametrize("L", [33, 130])
def test_tie_at_a_negative_level_fails_on_a_phantom_key(L):
    q, k, v, want, a = tie_case("native", 64, 1, 2, L)
    good = attn_ref64(q, k, v)[0]
    for dt in (FP, BF):
        assert_within_ulps(heads_to_clip(good).to(dt), heads_to_clip(want), 1, "the right answer passes")
    phantom = attn_ref64(q, k, v, extra_key_score=0.0)[0]
    neg, zero = a <= -32, a == 0                                         # the phantom key leads by >= 256 nats
    assert bool(neg.any()) and bool(zero.any())
    assert phantom[neg].abs().max().item() < 1e-100 and good[neg].min().item() > 64       # about 128 collapses to 0
    assert ((good - phantom)[zero] - good[zero] / (L + 1)).abs().max().item() < 1e-9       # level 0: one share of L + 1
    for dt in (FP, BF):
        with pytest.raises(AssertionError, match="more than 1 ulp"):
            assert_within_ulps(heads_to_clip(phantom).to(dt), heads_to_clip(want), 1, "phantom key")
        with pytest.raises(AssertionError, match="more than 1 ulp"):    # ... on the negative levels alone
            assert_within_ulps(torch.where(neg[..., None], phantom, good).to(dt), want, 1, "phantom key, negative levels")
    with pytest.raises(AssertionError, match="more than 1 ulp"):        # level 0: f32 at any L, bf16 while 128 / (L + 1) shows
        assert_within_ulps(torch.where(zero[..., None], phantom, good).float(), want, 1, "phantom key, level 0")


@pytest.mark.parametrize("variant", STAIRS)
def test_staircase_fails_on_a_scale_error(variant):
    q, k, v, ref, S, R = staircase_case("native", 64, 1, 2, 130, variant, BF)
    scaled = attn_ref64(q, k, v, scale_error=0.01)[0]
    for dt, rel in ((BF, BF16_REL), (FP, f32_rel(130, 64, R))):
        assert assert_attn_close(ref.to(dt), ref, S, rel, "the right answer passes") <= (0.7 if dt == BF else 0.1)
        if dt == BF and variant == "down":
            # the 32 keys of the leading tile lie within 3 nats (a = 1) of each other, and 1 % of that moves the output by
            # 0.4 % of S, under the bf16 bound of 0.59 %: this variant is there for the skipped rescale, and sees a scale
            # error in f32 only
            assert 0.5 <= assert_attn_close(scaled.to(dt), ref, S, rel, "1 % scale error, down, bf16") <= 1.0
            continue
        with pytest.raises(AssertionError, match="beyond"):
            assert_attn_close(scaled.to(dt), ref, S, rel, "1 % scale error")
    # ... and the selection test cannot see it (one-hot either way): that is what the staircase is for
    q, k, v, want, _ = selection_case("native", 64, 1, 2, 130, False)
    assert torch.equal(attn_ref64(q, k, v, scale_error=0.01)[0].float(), want)
