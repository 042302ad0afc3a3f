"""What tests/test_gpu_ew_exact.py relies on, shown without a GPU (tests/ew_ref.py holds the references):
  (i)   an f32 emulation of every per-element kernel, unfused and fully contracted, stays within 0.8 of its bound, and the
        bit-for-bit references equal a second, independent formulation;
  (ii)  every mutant of a kernel fails a named comparison on the GPU tests' own data;
  (iii) the conditions that the GPU tests assert on their data hold (rounding exercised, exact headroom, both sides of
        each clamp, values one grid apart distinct);
  and the constants that rest on a library function are 4 x the measured deviation of the reference's f32 formulation.
Invisible by construction, and said here: at rho = 0.5 the swap of sqrt_rho and sqrt_one_minus_rho changes nothing (the two
are equal); rho = 0 and 0.25 catch it."""
import itertools

import numpy as np
import pytest
import torch

from tests import ew_ref as R
from tests.ew_ref import BF, FP, NAME, U
from tests.util import (ACT_GELU, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, assert_act_close, assert_exact_headroom,
                        round_to)

DTYPES = [FP, BF]
SHARP = 0.8
BRANCHES = list(itertools.product([0, 1], repeat=5))        # restored, aux, nonzero, clip, prev


def both(emul, ref64, bound, what, dtype=FP):
    """emul(fused) for fused in (False, True) within SHARP of the bound -> the two ratios.  With a bf16 output the bound is
    mostly the half unit in the last place of the store, which a correctly rounded result uses up to 1.0: there the
    emulation is only held to the bound, and the f32 case shows the margin of the arithmetic part."""
    out = []
    sharp = SHARP if dtype == FP else 1.0
    for fused in (False, True):
        r = R.within(emul(fused), ref64, bound, f"{what} {'contracted' if fused else 'unfused'}")
        assert r <= sharp, f"{what} {'contracted' if fused else 'unfused'}: err / bound = {r:.3f} > {sharp}"
        out.append(r)
    print(f"{what}: f32 emulation err / bound = {out[0]:.3f} unfused, {out[1]:.3f} contracted")
    return out


# ------------------------------------------------------------------------------------------------ (i) A references
def test_rne_cast_three_ways():
    """torch's cast, the integer formula and util.round_to agree on all rounding cases: ties to even, the largest f32
    values to inf, denormals kept, -0.0 kept, NaN to NaN."""
    v, want, wide = R.bf16_case()
    u = R.bf16_case_bits()
    assert v.numel() % 72 == 0 and v.numel() >= 4 * 65536 - 3 * 256
    assert R.same_bits(want, R.bf16_from_bits(R.rne_bf16_bits(u)))
    normal = (v.abs() <= torch.finfo(BF).max) & (v.abs() >= 2.0 ** -126)
    assert normal.float().mean() > 0.98
    assert bool((round_to(v[normal].double(), BF) == wide[normal].double()).all())
    assert bool(torch.isinf(want[torch.from_numpy((u == 0x7F7F8000))]).all())                      # the tie below inf rounds up
    den = (v != 0) & (v.abs() < 2.0 ** -126)
    assert int(den.sum()) > 500 and bool((want[den & (v.abs() > 2.0 ** -133)] != 0).all())        # no denormal is flushed
    assert R.same_bits(want[torch.from_numpy(u == 0x80000000)], torch.tensor([-0.0], dtype=BF))
    assert bool(torch.isnan(want[torch.isnan(v)]).all()) and int(torch.isnan(v).sum()) == 254
    x0, half, s = R.tie_case()
    assert x0.numel() % 8 == 0 and x0.numel() > 58000
    assert R.same_bits(s, R.bf16_from_bits(R.rne_bf16_bits((x0.float() + half.float()).numpy().view(np.uint32))))


def test_store_mutants_are_caught():
    """Truncation and round-half-away each change outputs of the scalar-store case (bf16_case) and of the vector-store
    case (tie_case), so test_bf16_store_all_rounding_cases and test_bf16_vector_store_ties reject them."""
    u = R.bf16_case_bits()
    want = R.bf16_case()[1]
    x0, half, s = R.tie_case()
    tie_bits = (x0.float() + half.float()).numpy().view(np.uint32)
    for fault in ("truncate", "half_away"):
        assert not R.same_bits(want, R.bf16_from_bits(R.rne_bf16_bits(u, fault))), fault
        assert not R.same_bits(s, R.bf16_from_bits(R.rne_bf16_bits(tie_bits, fault))), fault
    # and the one-operation data: a truncating store changes a good part of every bf16 output
    d = R.pixel_case(BF)
    v = R.frame_bias_f32(d["x"], d["fb"])
    trunc = R.bf16_from_bits(R.rne_bf16_bits(v.numpy().view(np.uint32), "truncate"))
    assert (trunc.float() != v.to(BF).float()).float().mean() > 0.2


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_one_operation_references_and_mutants(dtype):
    d = R.pixel_case(dtype)
    x, x1 = d["x"], d["x1"]
    # the f32 operation, then torch's cast == float64 operation rounded once (no double rounding: an f32 sum or product of
    # two numbers of at most 24 bits rounds a value that float64 holds exactly)
    for name, v32, v64 in (("add_frame_bias", R.frame_bias_f32(x, d["fb"]), x.double() + d["fb"][:, :48].double().view(3, 1, 1, 48)),
                           ("scale_pixels", R.scale_pixels_f32(x, d["wmap"]), x.double() * d["wmap"].double().view(3, 5, 7, 1)),
                           ("add", R.add_act_f32(x, x1, ACT_NONE), x.double() + x1.double())):
        assert bool((v32.double() == v64.float().double()).all()), name
        R.assert_rounding_exercised(v32, dtype, name)
    want = R.frame_bias_f32(x, d["fb"]).to(dtype)
    for fault in ("next_frame", "next_channel"):
        assert not R.same_bits(want, R.frame_bias_f32(x, d["fb"], fault).to(dtype)), f"add_frame_bias {fault}: test_add_frame_bias_bits"
    assert not R.same_bits(R.scale_pixels_f32(x, d["wmap"]).to(dtype), R.scale_pixels_f32(x, d["wmap"], "next_pixel").to(dtype)), \
        "scale_pixels next_pixel: test_scale_pixels_bits"
    for act in (ACT_RELU, ACT_LRELU01, ACT_LRELU02):
        v = R.add_act_f32(x, x1, act)
        slope = {ACT_RELU: 0.0, ACT_LRELU01: 0.1, ACT_LRELU02: 0.2}[act]
        assert bool((v == torch.nn.functional.leaky_relu(x.float() + x1.float(), slope)).all())
        R.assert_rounding_exercised(v, dtype, f"add_act {act}")


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_maxpool_reference_and_mutant(dtype, shape):
    x = R.pool_case(dtype, shape)
    want = R.maxpool_ref(x)
    assert R.same_bits(want, R.maxpool_loop(x))
    zero = R.maxpool_ref(x, "pad_zero")
    T, Ho, Wo, C = want.shape
    border = torch.zeros(Ho, Wo, dtype=torch.bool)
    border[0, :] = border[:, 0] = True
    if shape[1] % 2:
        border[-1, :] = True
    if shape[2] % 2:
        border[:, -1] = True
    assert bool((zero[:, border] == 0).all()) and bool((want < 0).all()), "padding counted as 0: test_maxpool_bits"


# ------------------------------------------------------------------------------------------------ (i) + (ii) linear
@pytest.mark.parametrize("M,K,N", R.LINEAR_SHAPES)
def test_linear_int_is_exact_in_the_kernel_order(M, K, N):
    x, w, b, ref, mag = R.linear_int_case(M, K, N)
    assert_exact_headroom(mag)
    for fused in (False, True):
        assert bool((R.linear_emul(x, w, b, ACT_NONE, ACT_NONE, fused).double() == ref).all())
    caught = {"bias_next": True, "k_tail": K % 512 != 0, "act_in_rows": False}       # integers: no act_in in this family
    for fault, expect in caught.items():
        differs = not bool((R.linear_emul(x, w, b, ACT_NONE, ACT_NONE, True, fault).double() == ref).all())
        assert differs == expect, f"linear {fault} M={M} K={K} N={N}: test_linear_int_bits"


@pytest.mark.parametrize("M,K,N", [s for s in R.LINEAR_SHAPES if s[2] < 1000] + [R.LINEAR_SHAPES[-1]])
def test_linear_randn_emulation_and_mutants(M, K, N):
    x, w, b = R.linear_case(M, K, N)
    for act_in, act_out in itertools.product((ACT_NONE, ACT_SILU), repeat=2):
        ref, bound = R.linear64(x, w, b, act_in, act_out)
        both(lambda fused: R.linear_emul(x, w, b, act_in, act_out, fused), ref, bound, f"linear {M}x{K}x{N} in={act_in} out={act_out}")
        assert R.beyond(R.linear_emul(x, w, b, act_in, act_out, True, "bias_next"), ref, bound), "bias_next: test_linear_randn"
        if K % 512:
            assert R.beyond(R.linear_emul(x, w, b, act_in, act_out, True, "k_tail"), ref, bound), "k_tail: test_linear_randn"
        if act_in == ACT_SILU and M > 8:
            assert R.beyond(R.linear_emul(x, w, b, act_in, act_out, True, "act_in_rows"), ref, bound), "act_in_rows: test_linear_randn"
    assert any(m > 8 for m, _, _ in R.LINEAR_SHAPES) and any(k % 512 for _, k, _ in R.LINEAR_SHAPES)


def test_linear_shapes_cover_the_paths():
    ms = {m for m, _, _ in R.LINEAR_SHAPES}
    assert {8, 9, 16, 17, 32} <= ms and all(m * k * 4 <= 64 * 1024 for m, k, _ in R.LINEAR_SHAPES)
    assert any(n >= 8192 and n % 32 for _, _, n in R.LINEAR_SHAPES)
    ks = {k for _, k, _ in R.LINEAR_SHAPES}
    assert any(k < 512 for k in ks) and 512 in ks and any(k > 512 and k % 64 for k in ks)
    m, k, _ = R.LINEAR_REFUSED
    assert m * k * 4 > 64 * 1024


# ------------------------------------------------------------------------------------------------ (i) + (ii) sampler
@pytest.mark.parametrize("i", R.TIMESTEPS)
@pytest.mark.parametrize("Cm", [3, 6])
def test_predict_xstart_emulation_and_mutants(Cm, i):
    x, mo, a, b = R.xstart_case(Cm, i)
    for clip in (0, 1):
        ref, bound = R.xstart64(x, mo, a, b, clip)
        both(lambda fused: R.xstart_emul(x, mo, a, b, clip, fused), ref, bound, f"predict_xstart Cm={Cm} i={i} clip={clip}")
        if Cm == 6:
            assert R.beyond(R.xstart_emul(x, mo, a, b, clip, False, "image_stride"), ref, bound), "C HW image stride: test_predict_xstart"
    if Cm == 3:     # the stride mutant is the correct kernel when Cm = C: why the cases have Cm = 6
        assert R.same_bits(R.xstart_emul(x, mo, a, b, 0, False, "image_stride"), R.xstart_emul(x, mo, a, b, 0))
    raw = R.xstart64(x, mo, a, b, 0)[0]
    assert bool((raw > 1).any()) and bool((raw < -1).any()) and bool((raw.abs() < 1).any())


SAMPLER_FAULTS = ("prev_index", "clamp_after_blend", "w_for_1mw", "swap_rho", "div_recip")


@pytest.mark.parametrize("i", R.TIMESTEPS)
def test_sampler_emulation_and_mutants(i):
    d = R.sampler_case(i)
    worst = [0.0, 0.0]
    caught = {(f, rho, w): False for f in SAMPLER_FAULTS for rho in R.RHOS for w in R.WS}
    for rho, w in itertools.product(R.RHOS, R.WS):
        for has_r, has_a, nonzero, clip, has_p in BRANCHES:
            c = R.sampler_coefs(i, rho, w, clip, nonzero)
            e = R.sampler_x0_64(c, d, has_r, has_a, has_p)
            for fused in (False, True):
                x0, xp = R.sampler_emul(c, d, has_r, has_a, has_p, fused)
                what = f"sampler i={i} rho={rho} w={w} branch={(has_r, has_a, nonzero, clip, has_p)} fused={fused}"
                r0 = R.within(x0, e["ref"], e["bound"], what + " x0")
                ref, bound = R.sampler_xprev_64(c, d, x0)
                r1 = R.within(xp, ref, bound, what + " x_prev")
                worst = [max(worst[0], r0), max(worst[1], r1)]
                assert R.same_bits(x0[e["pinned"]], _pinned(d)[e["pinned"]])
                assert bool((x0[e["sat"] != 0].double() == e["sat"][e["sat"] != 0]).all())
                if not nonzero:
                    assert R.same_bits(xp, R.t32(c["prev"]) * x0)
            for fault in SAMPLER_FAULTS:
                x0, xp = R.sampler_emul(c, d, has_r, has_a, has_p, False, fault)
                bad = R.beyond(x0, e["ref"], e["bound"])
                if not bad:
                    ref, bound = R.sampler_xprev_64(c, d, x0)
                    bad = R.beyond(xp, ref, bound)
                caught[fault, rho, w] |= bad
    print(f"sampler_update i={i}: f32 emulation err / bound = {worst[0]:.3f} (x0), {worst[1]:.3f} (x_prev)")
    assert worst[0] <= SHARP and worst[1] <= SHARP, worst
    noise = R.sampler_coefs(i, 0.25, 0.5, 1, 1)["co"] != 0       # at the last timestep the noise coefficient is 0
    for (fault, rho, w), hit in caught.items():
        if fault == "swap_rho":
            assert hit == (noise and rho != 0.5), (fault, rho, w, "test_sampler_update: rho = 0.5 hides the swap")
        elif fault == "w_for_1mw":
            assert hit == (w != 0.5), (fault, rho, w, "test_sampler_update: w = 0.5 hides it, w = 0.75 does not")
        elif fault == "div_recip":
            assert hit == noise, (fault, rho, w, "test_sampler_update x_prev")
        else:
            assert hit, (fault, rho, w, "test_sampler_update x0")


def _pinned(d):
    return R._pin(torch.zeros_like(d["x0"]), d["prev"], d["T"], d["Tp"])


def test_sampler_data_reaches_both_sides_of_the_clamps():
    for i in R.TIMESTEPS:
        d = R.sampler_case(i)
        c = R.sampler_coefs(i, 0.25, 0.75, 1, 1)
        e = R.sampler_x0_64(c, d, 1, 0, 0)
        assert bool((e["sat"] == 1).any()) and bool((e["sat"] == -1).any()) and bool((e["sat"] == 0).any()), i
        assert bool((d["aux"] > 1).any()) and bool((d["aux"] < -1).any())


# ------------------------------------------------------------------------------------------------ (i) the small f32 entries
def test_axpby_emulation():
    x, y = R.axpby_case(4099)
    for (a, b), (lo, hi), with_y in itertools.product(R.AXPBY_COEFS, R.AXPBY_CLAMPS, (False, True)):
        ref, bound = R.axpby64(x, y if with_y else None, a, b, lo, hi)
        both(lambda fused: R.axpby_emul(x, y if with_y else None, a, b, lo, hi, fused), ref, bound, f"axpby a={a:.3g} b={b:.3g} [{lo}, {hi}] y={with_y}")
    raw = R.axpby64(x, y, 1.7, -0.6, float("-inf"), float("inf"))[0]
    assert bool((raw > 1).any()) and bool((raw < -1).any()) and bool((raw < -0.25).any())


def test_affine_emulation_and_clamp_sides():
    x, sub, mul = R.affine_case()
    ref, bound, pre = R.affine64(x, sub, mul)
    both(lambda fused: R.affine_emul(x, sub, mul, fused), ref, bound, "affine_channels")
    assert bool((pre > 0.8).any()) and bool((pre < -0.8).any()) and bool((pre.abs() < 0.8).any())
    assert R.beyond(R.affine_emul(x, sub.roll(1), mul), ref, bound) and R.beyond(R.affine_emul(x, sub, mul.roll(1)), ref, bound)


def test_learned_range_emulation_and_mutants():
    mo, C, lo, hi = R.learned_range_case()
    lv, b_lv, var, b_var = R.learned_range64(mo, C, lo, hi)
    both(lambda fused: R.learned_range_emul(mo, C, lo, hi, fused)[0], lv, b_lv, "learned_range log variance")
    both(lambda fused: R.learned_range_emul(mo, C, lo, hi, fused)[1], var, b_var, "learned_range variance")
    for fault in ("first_channels", "image_stride"):
        assert R.beyond(R.learned_range_emul(mo, C, lo, hi, False, fault)[0], lv, b_lv), f"{fault}: test_learned_range_variance"


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("C", [40, 128])
def test_gated_blend_emulation_and_mutant(dtype, C):
    x, m, gate = R.blend_case(dtype, C)
    ref, bound = R.blend64(x, m, gate, dtype)
    both(lambda fused: R.blend_emul(x, m, gate, dtype, fused), ref, bound, f"gated_blend C={C} {NAME[dtype]}", dtype)
    assert R.beyond(R.blend_emul(x, m, gate, dtype, False, "swap_s"), ref, bound), "s and 1 - s swapped: test_gated_blend"
    got = R.blend_emul(x, m, gate, dtype).float()
    assert R.same_bits(got[..., 3], m[..., 3]) and R.same_bits(got[..., 4], x[..., 4]) and R.same_bits(got[..., 1], m[..., 1])


@pytest.mark.parametrize("sin_first", [False, True])
@pytest.mark.parametrize("dim", R.EMB_DIMS)
def test_embedding_emulation_and_mutants(dim, sin_first):
    t = torch.tensor(R.EMB_T)
    ref, bound = R.embedding64(t, dim, sin_first)
    r = R.within(R.embedding_emul(t, dim, sin_first), ref, bound, f"embedding dim={dim}")
    print(f"timestep_embedding dim={dim} sin_first={sin_first}: f32 reference err / bound = {r:.3f}")
    assert r <= 0.26                                                          # the constants are 4 x this formulation's own error
    assert R.beyond(R.embedding_emul(t, dim, sin_first, "swap"), ref, bound), "sin and cos swapped: test_timestep_embedding"
    assert R.beyond(R.embedding_emul(t, dim, sin_first, "half_minus_1"), ref, bound), "k / (half - 1): test_timestep_embedding"
    if dim % 2:
        assert R.beyond(R.embedding_emul(t, dim, sin_first, "odd_unwritten", fill=-1232.0), ref, bound), "last column: test_timestep_embedding"


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_add_act_silu_gelu_emulation(dtype):
    x0, x1 = R.add_act_case(dtype)
    for act, two in itertools.product((ACT_SILU, ACT_GELU), (False, True)):
        ref, S, extra = R.add_act64(x0, x1 if two else None, act)
        r = assert_act_close(R.add_act_emul(x0, x1 if two else None, act, dtype), ref, S, R.K_ACT[act], dtype, f"add_act {act}", extra=extra)
        print(f"add_act act={act} two={two} {NAME[dtype]}: f32 emulation err / (u S) = {r:.3f} of k = {R.K_ACT[act]}")
        assert r <= SHARP * R.K_ACT[act]


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_sft_and_gate_emulation(dtype):
    dec, sc, sh = R.sft_case(dtype)
    ref, bound = R.sft64(dec, sc, sh, dtype)
    both(lambda fused: R.sft_emul(dec, sc, sh, dtype, fused), ref, bound, f"sft_fuse {NAME[dtype]}", dtype)
    x, a, gate, bias = R.gate_case(dtype)
    for use, kw in R.GATE_USES.items():
        ref, bound = R.gate64(x, a, gate, bias, kw, dtype)
        both(lambda fused: R.gate_emul(x, a, gate, bias, kw, dtype, fused), ref, bound, f"channel_gate {use} {NAME[dtype]}", dtype)


# ------------------------------------------------------------------------------------------------ the library constants
def test_library_constants():
    """Each constant is at least 4 x (and at most 8 x) the deviation of the reference's f32 formulation from float64 on the
    inputs the GPU tests use."""
    def rel(f32v, f64v):
        return ((f32v.double() - f64v).abs() / f64v.abs().clamp_min(1e-300)).max().item() / U
    mo, C, lo, hi = R.learned_range_case()
    lv32 = R.learned_range_emul(mo, C, lo, hi)[0]
    gates = torch.cat([R.blend_case(FP, c)[2].flatten() for c in (40, 128)])
    gates = gates[gates.abs() < 80]
    m_exp = max(rel(torch.exp(lv32), torch.exp(lv32.double())), rel(torch.exp(-gates), torch.exp(-gates.double())))
    g = R.gate_case(FP)[2]
    m_sig = rel(torch.sigmoid(g), torch.sigmoid(g.double()))
    devs = [R.embedding_deviation(torch.tensor(R.EMB_T), dim) for dim in R.EMB_DIMS]
    m_arg, m_out = max(d[0] for d in devs), max(d[1] for d in devs)
    print(f"measured: exp {m_exp:.2f} u, sigmoid {m_sig:.2f} u, embedding argument {m_arg:.2f} u, cos / sin {m_out:.2f} u")
    for name, measured, const in (("C_EXP", m_exp, R.C_EXP), ("C_SIG", m_sig, R.C_SIG), ("C_ARG", m_arg, R.C_ARG), ("C_OUT", m_out, R.C_OUT)):
        assert 4 * measured <= const <= 8 * measured, (name, measured, const)


# ------------------------------------------------------------------------------------------------ (iii) the trip data
def test_trip_cases_take_a_third_trip_on_distinct_values():
    for dtype in DTYPES:
        v = R.VEC[dtype]
        d = R.pixel_case(dtype, trip=True)
        assert R.trips_distinct(d["x"].reshape(-1, v).float()), "pixel_case"
        assert d["x"].numel() // v == 2 * R.GRID + 269
        x0, _ = R.add_act_case(dtype, trip=True)
        assert R.trips_distinct(x0.reshape(-1, v).float())
        x, m, _ = R.blend_case(dtype, v, trip=True)
        assert R.trips_distinct(x.reshape(-1, v).float())
        p = R.pool_case(dtype, None, trip=True)
        assert (p.shape[1] + 1) // 2 * ((p.shape[2] + 1) // 2) * p.shape[0] > 2 * R.GRID
    lay = R.layout_trip_case()
    assert R.trips_distinct(lay.permute(0, 2, 3, 1).reshape(-1, 3)) and R.rounding_share(lay, BF) > 0.9
    x, y = R.axpby_case(R.TRIP_N)
    assert R.trips_distinct(x.view(-1, 1)) and R.trips_distinct(y.view(-1, 1))
    x, mo, _, _ = R.xstart_case(6, 25, trip=True)
    assert R.trips_distinct(x.reshape(-1, 1))
    assert R.trips_distinct(R.sampler_case(25, trip=True)["x"].reshape(-1, 1))
    assert R.trips_distinct(R.affine_case(trip=True)[0].reshape(-1, 1))
    mo, C, _, _ = R.learned_range_case(trip=True)
    assert R.trips_distinct(mo[:, C:].reshape(-1, 1))
