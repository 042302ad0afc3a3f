"""The streaming kernels of csrc/ew.hip, flair_sft_fuse and flair_channel_gate_nhwc, judged bit for bit where the answer is
unique and per element against float64 where the arithmetic is rounded.  tests/ew_ref.py holds the references, the data,
the bounds (n u S per element, n counted from the kernel source) and the constants that rest on a library function;
tests/test_ew_exact_cpu.py proves them sound and sharp and shows which comparison rejects which mutant.

  A  bit for bit   every bf16 rounding case through the scalar and the vector stores and back; add_frame_bias, scale_pixels,
                   add_act (none / ReLU / both leaky slopes) and maxpool3x3s2 as RNE(dtype, one f32 operation);
                   flair_linear_f32 on integers at both sides of every MMAX boundary and in the eight-features-per-wave
                   form; the pinned frames, the saturated clamps and the noise-free x_prev of flair_sampler_update
  B  per element   predict_xstart, sampler_update (32 branches x 3 timesteps x rho x w), axpby_f32, affine_channels_f32,
                   learned_range_variance, gated_blend, timestep_embedding, linear_f32 on randn, add_act with SiLU / GELU,
                   sft_fuse, channel_gate
  C  a case of more than two grids (2048 x 256 threads) of work items per looping entry, under the same criterion

Every call keeps the guard discipline of the older direct tests: inputs between NaNs, outputs between sentinels, and where
an entry takes strides the dense and the strided call equal bit for bit (tests/test_gpu_strides.py run_both).  The worst
err / bound of every case goes to parity_log; profiles/ew_exact_parity.txt is the record.  A ratio above 1 is a finding
about the kernel, never a reason to widen a bound."""
import itertools

import pytest
import torch

from tests import ew_ref as R
from tests.ew_ref import BF, FP, NAME
from tests.test_gpu_strides import run_both
from tests.util import (ACT_FLOOR, ACT_GELU, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, IN_FILL, OUT_FILL,
                        assert_act_close, assert_exact_headroom, assert_flat_untouched, bits, flat_guarded, parity_log)

pytestmark = pytest.mark.gpu
DTYPES = [FP, BF]
TRIPS = [False, True]
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LRELU01: "lrelu01", ACT_LRELU02: "lrelu02", ACT_SILU: "silu", ACT_GELU: "gelu"}


def _ops():
    from flair_amd import ops
    return ops


def _tid(v):
    if isinstance(v, torch.dtype):
        return NAME[v]
    if isinstance(v, bool):
        return "trip" if v else "small"
    return str(v)


def _in(dev, t):
    """A cpu f32 tensor as a dense device tensor between NaNs."""
    return flat_guarded(tuple(t.shape), FP, dev, IN_FILL, t)


def _out(dev, shape, dtype=FP):
    return flat_guarded(tuple(shape), dtype, dev, OUT_FILL)


def _check_guards(ins, outs, what):
    torch.cuda.synchronize()
    for i, (buf, _, before) in enumerate(ins):
        assert_flat_untouched(buf, before, None, f"{what}: input {i}")
    for i, (buf, v, before) in enumerate(outs):
        assert_flat_untouched(buf, before, v, f"{what}: output {i}")


def log_bits(what):
    parity_log(f"ew_exact {what}: bit for bit")


def log_ratio(what, r):
    parity_log(f"ew_exact {what}: worst err / bound = {r:.3f}")


def gran(dtype):
    return R.VEC[dtype]


# ================================================================================================ A1: the bf16 store
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_bf16_store_all_rounding_cases(dev, dtype):
    """All 2^16 bf16 patterns with 0, 0x7FFF, 0x8000 and 0x8001 below them, through the two scalar stores; in f32 the same
    calls return their input."""
    ops = _ops()
    v, want, wide = R.bf16_case()
    expect = want if dtype == BF else v
    P = v.numel() // 3
    shape = (1, 24, P // 24, 3)
    # cast_channels: a 4-wide view at channel 4 of 12, written at dst_coff = 1 (an odd element offset)
    got = run_both(dev, {"s": (v.view(shape), FP, 1, 7)}, {"d": (shape[:3] + (4,), dtype, 4, 12)},
                   lambda s, d: ops.cast_channels(s, d, coff=1), "cast_channels")["d"].to(dtype)
    R.assert_same_bits(got[..., 1:], expect.view(shape), f"cast_channels {NAME[dtype]}")
    assert bool((got[..., 0] == OUT_FILL).all())
    # nchw -> clip
    src = _in(dev, v.view(1, 3, 24, P // 24))
    got = run_both(dev, {}, {"d": ((1, 24, P // 24, 8), dtype, 4, 24)}, lambda d: ops.nchw_to_clip(src[1], d, coff=3),
                   "nchw_to_clip")["d"].to(dtype)
    _check_guards([src], [], "nchw_to_clip")
    R.assert_same_bits(got[..., 3:6], expect.view(1, 3, 24, P // 24).permute(0, 2, 3, 1), f"nchw_to_clip {NAME[dtype]}")
    assert bool((got[..., :3] == OUT_FILL).all()) and bool((got[..., 6:] == OUT_FILL).all())
    # and back: the bf16 result widens to p << 16 exactly
    x = expect.view(shape)
    box = []
    run_both(dev, {"x": (x, dtype, 5, 12)}, {}, lambda x: box.append(ops.clip_to_nchw(x, 3)), "clip_to_nchw")
    assert torch.equal(bits(box[0]), bits(box[1]))
    R.assert_same_bits(box[0], (wide if dtype == BF else v).view(shape).permute(0, 3, 1, 2), f"clip_to_nchw {NAME[dtype]}")
    log_bits(f"bf16 store, scalar paths (cast_channels, nchw_to_clip, clip_to_nchw) {NAME[dtype]} n={v.numel()}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_bf16_store_vector_paths_pass_every_pattern(dev, dtype):
    """The vector entries take their input in the output's type, so the rounded patterns go in: every bf16 number (zeros of
    both signs, denormals, infinities, NaNs) comes back bit for bit through add_act (x1 = None, ACT_NONE) and through
    scale_pixels with a map of ones (in place), equal to the scalar stores' result; in f32 the f32 cases do."""
    ops = _ops()
    v, want, _ = R.bf16_case()
    expect = want if dtype == BF else v
    shape = (1, 3, v.numel() // 24, 8)
    g = gran(dtype)
    got = run_both(dev, {"a": (expect.view(shape), dtype, g, 8 + 2 * g)}, {"y": (shape, dtype, g, 8 + g)},
                   lambda a, y: ops.add_act(a, None, ACT_NONE, out=y), "add_act copy")["y"].to(dtype)
    R.assert_same_bits(got, expect.view(shape), f"add_act copy {NAME[dtype]}")
    ones = torch.ones(v.numel() // 8, device=dev)
    got = run_both(dev, {}, {"x": (shape, dtype, g, 8 + 2 * g, expect.view(shape))}, lambda x: ops.scale_pixels(x, ones),
                   "scale_pixels by one")["x"].to(dtype)
    R.assert_same_bits(got, expect.view(shape), f"scale_pixels by one {NAME[dtype]}")
    log_bits(f"bf16 store, vector paths pass every pattern (add_act, scale_pixels) {NAME[dtype]}")


def test_bf16_vector_store_ties(dev):
    """x0 + x1 is exactly the tie above every finite bf16 number, formed in f32 inside add_act: the vector store must round
    it to even."""
    ops = _ops()
    x0, x1, want = R.tie_case()
    shape = (1, 1, x0.numel() // 8, 8)
    got = run_both(dev, {"a": (x0.view(shape), BF, 8, 24), "b": (x1.view(shape), BF, 16, 32)}, {"y": (shape, BF, 8, 16)},
                   lambda a, b, y: ops.add_act(a, b, ACT_NONE, out=y), "add_act ties")["y"].to(BF)
    R.assert_same_bits(got, want.view(shape), "add_act ties")
    log_bits(f"bf16 store, vector path, {x0.numel()} ties")


@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_layout_and_cast_beyond_two_grids(dev, dtype):
    """More than two grids of work items through nchw_to_clip and back (one per pixel) and through cast_channels (one per
    element): the RNE cast of randn, the f32 input itself in f32."""
    ops = _ops()
    x = R.layout_trip_case()
    N, C, H, W = x.shape
    src = _in(dev, x)
    got = run_both(dev, {}, {"d": ((N, H, W, 8), dtype, 4, 24)}, lambda d: ops.nchw_to_clip(src[1], d, coff=3), "nchw_to_clip")["d"].to(dtype)
    _check_guards([src], [], "nchw_to_clip")
    clip = x.permute(0, 2, 3, 1).contiguous().to(dtype)
    R.assert_same_bits(got[..., 3:6], clip, f"nchw_to_clip {NAME[dtype]} {tuple(x.shape)}")
    box = []
    run_both(dev, {"x": (clip, dtype, 5, 12)}, {}, lambda x: box.append(ops.clip_to_nchw(x, 3)), "clip_to_nchw")
    assert torch.equal(bits(box[0]), bits(box[1]))
    R.assert_same_bits(box[0], clip.float().permute(0, 3, 1, 2), f"clip_to_nchw {NAME[dtype]}")
    xs = R.affine_case(True)[0]
    got = run_both(dev, {"s": (xs, FP, 1, 7)}, {"d": (tuple(xs.shape[:3]) + (4,), dtype, 4, 12)},
                   lambda s, d: ops.cast_channels(s, d, coff=1), "cast_channels")["d"].to(dtype)
    R.assert_same_bits(got[..., 1:], xs.to(dtype), f"cast_channels {NAME[dtype]} {tuple(xs.shape)}")
    log_bits(f"nchw_to_clip, clip_to_nchw {tuple(x.shape)} and cast_channels {tuple(xs.shape)} {NAME[dtype]}, beyond two grids")


# ================================================================================================ A2: one f32 operation
@pytest.mark.parametrize("trip", TRIPS, ids=_tid)
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_add_frame_bias_bits(dev, dtype, trip):
    ops = _ops()
    d = R.pixel_case(dtype, trip)
    x, fb = d["x"], d["fb"]
    C, g = x.shape[3], gran(dtype)
    v32 = R.frame_bias_f32(x, fb)
    R.assert_rounding_exercised(v32, dtype, "add_frame_bias")
    fbd = fb.to(dev)
    got = run_both(dev, {}, {"x": (tuple(x.shape), dtype, g, C + 2 * g, x)}, lambda x: ops.add_frame_bias(x, fbd), "add_frame_bias")["x"]
    R.assert_same_bits(got.to(dtype), v32.to(dtype), f"add_frame_bias {NAME[dtype]} {_tid(trip)}")
    log_bits(f"add_frame_bias {NAME[dtype]} {tuple(x.shape)}")


@pytest.mark.parametrize("trip", TRIPS, ids=_tid)
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_scale_pixels_bits(dev, dtype, trip):
    ops = _ops()
    d = R.pixel_case(dtype, trip)
    x, wmap = d["x"], d["wmap"]
    C, g = x.shape[3], gran(dtype)
    v32 = R.scale_pixels_f32(x, wmap)
    R.assert_rounding_exercised(v32, dtype, "scale_pixels")
    wd = _in(dev, wmap)
    got = run_both(dev, {}, {"x": (tuple(x.shape), dtype, g, C + 2 * g, x)}, lambda x: ops.scale_pixels(x, wd[1]), "scale_pixels")["x"]
    _check_guards([wd], [], "scale_pixels")
    R.assert_same_bits(got.to(dtype), v32.to(dtype), f"scale_pixels {NAME[dtype]} {_tid(trip)}")
    log_bits(f"scale_pixels {NAME[dtype]} {tuple(x.shape)}")


@pytest.mark.parametrize("two", [False, True], ids=["x0", "x0+x1"])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_LRELU01, ACT_LRELU02], ids=ACT_NAMES.get)
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_add_act_bits(dev, dtype, act, two):
    _add_act_bits(dev, dtype, act, two, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_add_act_bits_beyond_two_grids(dev, dtype):
    _add_act_bits(dev, dtype, ACT_LRELU01, True, True)


def _add_act_bits(dev, dtype, act, two, trip):
    ops = _ops()
    d = R.pixel_case(dtype, trip)
    x0, x1 = d["x"], d["x1"] if two else None
    C, g = x0.shape[3], gran(dtype)
    v32 = R.add_act_f32(x0, x1, act)
    if two:
        R.assert_rounding_exercised(v32, dtype, "add_act")
    ins = {"a": (x0, dtype, g, C + 2 * g)}
    if two:
        ins["b"] = (x1, dtype, 2 * g, C + 3 * g)
    got = run_both(dev, ins, {"y": (tuple(x0.shape), dtype, g, C + g)}, lambda a, y, b=None: ops.add_act(a, b, act, out=y), "add_act")["y"]
    want = v32.to(dtype)
    # the sign of a zero is open: ReLU's `v > 0 ? v : 0` gives +0 for every v <= 0
    got = got.to(dtype)
    zero = (got == 0) & (want == 0)
    R.assert_same_bits(torch.where(zero, torch.zeros_like(got), got), torch.where(zero, torch.zeros_like(want), want),
                       f"add_act {ACT_NAMES[act]} two={two} {NAME[dtype]}")
    log_bits(f"add_act {ACT_NAMES[act]} two={two} {NAME[dtype]} {tuple(x0.shape)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_bits(dev, dtype, shape):
    """All-negative data, H and W odd and even."""
    _maxpool_bits(dev, dtype, R.pool_case(dtype, shape))


def test_maxpool_bits_beyond_two_grids(dev):
    """f32, the smaller of the two types at one vector per pixel."""
    _maxpool_bits(dev, FP, R.pool_case(FP, None, trip=True))


def _maxpool_bits(dev, dtype, x):
    ops = _ops()
    T, H, W, C = x.shape
    g = gran(dtype)
    want = R.maxpool_ref(x.to(dtype))
    got = run_both(dev, {"x": (x, dtype, g, C + 2 * g)}, {"y": (tuple(want.shape), dtype, 2 * g, C + 3 * g)},
                   lambda x, y: ops.maxpool3x3s2(x, out=y), "maxpool")["y"]
    R.assert_same_bits(got.to(dtype), want, f"maxpool {NAME[dtype]} {tuple(x.shape)}")
    log_bits(f"maxpool3x3s2 {NAME[dtype]} {tuple(x.shape)}")


# ================================================================================================ flair_linear_f32
def _linear(dev, x, w, b, act_in, act_out, what):
    """x between NaN rows, y rows y_ld = N + 5 apart inside a sentinel buffer -> y (cpu)."""
    ops = _ops()
    M, K = x.shape
    N = w.shape[0]
    xbuf = torch.full((M + 2, K), IN_FILL, device=dev)
    xv = xbuf[1:M + 1]
    xv.copy_(x.to(dev))
    xbefore = xbuf.clone()
    ybuf = torch.full((M + 2, N + 5), OUT_FILL, device=dev)
    yv = ybuf[1:M + 1, 2:2 + N]
    ybefore = ybuf.clone()
    ops.linear(xv, w.to(dev), b.to(dev), act_in=act_in, act_out=act_out, out=yv)
    torch.cuda.synchronize()
    changed = bits(ybuf) != bits(ybefore)
    changed[1:M + 1, 2:2 + N] = False
    assert not changed.any(), f"{what}: {int(changed.sum())} element(s) changed outside y, first {changed.nonzero()[0].tolist()}"
    assert torch.equal(bits(xbuf), bits(xbefore)), what
    return yv.cpu()


@pytest.mark.parametrize("M,K,N", R.LINEAR_SHAPES)
def test_linear_int_bits(dev, M, K, N):
    """Integers: every partial sum is exact, so lane order, the shuffle tree and contraction cannot change the result."""
    x, w, b, ref, mag = R.linear_int_case(M, K, N)
    assert_exact_headroom(mag)
    got = _linear(dev, x, w, b, ACT_NONE, ACT_NONE, f"linear int {M}x{K}x{N}")
    R.assert_same_bits(got, ref.float(), f"linear int {M}x{K}x{N}")
    log_bits(f"linear_f32 integers M={M} K={K} N={N}")


@pytest.mark.parametrize("act_out", [ACT_NONE, ACT_SILU], ids=["out_none", "out_silu"])
@pytest.mark.parametrize("act_in", [ACT_NONE, ACT_SILU], ids=["in_none", "in_silu"])
@pytest.mark.parametrize("M,K,N", R.LINEAR_SHAPES)
def test_linear_randn(dev, M, K, N, act_in, act_out):
    x, w, b = R.linear_case(M, K, N)
    ref, bound = R.linear64(x, w, b, act_in, act_out)
    what = f"linear_f32 randn M={M} K={K} N={N} in={ACT_NAMES[act_in]} out={ACT_NAMES[act_out]}"
    log_ratio(what, R.within(_linear(dev, x, w, b, act_in, act_out, what), ref, bound, what))


def test_linear_refuses_rows_beyond_the_lds_staging(dev):
    from flair_amd._lib import FlairHipError
    M, K, N = R.LINEAR_REFUSED
    with pytest.raises(FlairHipError, match="M\\*K too large for LDS staging"):
        _ops().linear(torch.zeros(M, K, device=dev), torch.zeros(N, K, device=dev), None)


# ================================================================================================ predict_xstart / sampler
@pytest.mark.parametrize("clip", [0, 1], ids=["raw", "clipped"])
@pytest.mark.parametrize("i", R.TIMESTEPS)
@pytest.mark.parametrize("Cm", [3, 6])
def test_predict_xstart(dev, Cm, i, clip):
    _predict_xstart(dev, Cm, i, clip, False)


def test_predict_xstart_beyond_two_grids(dev):
    _predict_xstart(dev, 6, 25, 1, True)


def _predict_xstart(dev, Cm, i, clip, trip):
    ops = _ops()
    x, mo, a, b = R.xstart_case(Cm, i, trip)
    ref, bound = R.xstart64(x, mo, a, b, clip)
    ins = [_in(dev, x), _in(dev, mo)]
    out = _out(dev, x.shape)
    ops.predict_xstart(ins[0][1], ins[1][1], a, b, clip, out=out[1])
    what = f"predict_xstart Cm={Cm} i={i} clip={clip} {tuple(x.shape)}"
    _check_guards(ins, [out], what)
    log_ratio(what, R.within(out[1], ref, bound, what))


def _coefs(ops, c, d):
    k = ops.SamplerCoefs()
    k.gamma, k.w_aux = c["gamma"], c["w"]
    k.sqrt_recip_alphas_cumprod, k.sqrt_recipm1_alphas_cumprod = c["recip"], c["recipm1"]
    k.sqrt_alphas_cumprod_prev, k.sqrt_one_minus_alphas_cumprod_prev = c["prev"], c["co"]
    k.sqrt_one_minus_rho, k.sqrt_rho = c["sq1mrho"], c["sqrho"]
    k.clip_denoised, k.nonzero = c["clip"], c["nonzero"]
    k.frame_elems, k.frames, k.prev_frames = d["frame_elems"], d["T"], d["Tp"]
    return k


def _sampler_update(dev, d, placed, c, branch, what):
    """One launch of a branch -> the worst err / bound of x0 and of x_prev, after the exact checks: the pinned frames equal
    prev_recon, a value beyond +-1 by more than its bound is exactly +-1, and without noise x_prev = f32(c_prev * x0)."""
    ops = _ops()
    has_r, has_a, nonzero, clip, has_p = branch
    r_d, a_d, z_d, p_d = (placed[k][1] if on else None for k, on in (("restored", has_r), ("aux", has_a), ("z", nonzero), ("prev", has_p)))
    x0g = flat_guarded(tuple(d["x0"].shape), FP, dev, OUT_FILL, d["x0"])          # read and written in place
    out = _out(dev, d["x"].shape)
    ops.sampler_update(_coefs(ops, c, d), placed["x"][1], x0g[1], r_d, a_d, z_d, p_d, out=out[1])
    _check_guards(list(placed.values()), [x0g, out], what)
    x0, xp = x0g[1].cpu(), out[1].cpu()
    e = R.sampler_x0_64(c, d, has_r, has_a, has_p)
    r0 = R.within(x0, e["ref"], e["bound"], what + " x0")
    if has_p:
        pin = R._pin(torch.zeros_like(d["x0"]), d["prev"], d["T"], d["Tp"])
        R.assert_same_bits(x0[e["pinned"]], pin[e["pinned"]], what + " pinned frames")
    sat = e["sat"] != 0
    assert bool((x0[sat].double() == e["sat"][sat]).all()), what + ": a clamped value is not exactly +-1"
    if not nonzero:
        R.assert_same_bits(xp, R.t32(c["prev"]) * x0, what + " x_prev without noise")
    ref, bound = R.sampler_xprev_64(c, d, x0)
    return r0, R.within(xp, ref, bound, what + " x_prev")


@pytest.mark.parametrize("i", R.TIMESTEPS)
def test_sampler_update(dev, i):
    """restored x aux x nonzero x clip x prev_recon at timestep i of 50, with rho in {0, 0.25, 0.5} wherever there is noise
    and w in {0.75, 0.5} wherever there is an aux blend (elsewhere the two do not enter)."""
    d = R.sampler_case(i)
    placed = {k: _in(dev, d[k]) for k in ("x", "restored", "aux", "z", "prev")}
    worst = {}
    for branch in itertools.product([0, 1], repeat=5):
        has_r, has_a, nonzero, clip, has_p = branch
        for rho, w in itertools.product(R.RHOS if nonzero else (0.25,), R.WS if has_a else (0.75,)):
            c = R.sampler_coefs(i, rho, w, clip, nonzero)
            what = f"sampler_update i={i} rho={rho} w={w} restored={has_r} aux={has_a} nonzero={nonzero} clip={clip} prev={has_p}"
            r0, r1 = _sampler_update(dev, d, placed, c, branch, what)
            key = f"restored={has_r} aux={has_a} nonzero={nonzero}"
            worst[key] = tuple(max(p, q) for p, q in zip(worst.get(key, (0.0, 0.0)), (r0, r1)))
    for key, (r0, r1) in worst.items():
        parity_log(f"ew_exact sampler_update i={i} {key} (clip, prev, rho, w: all): worst err / bound = {r0:.3f} (x0), {r1:.3f} (x_prev); "
                   "pinned frames, saturated clamps and the noise-free x_prev bit for bit")


def test_sampler_update_beyond_two_grids(dev):
    d = R.sampler_case(25, trip=True)
    placed = {k: _in(dev, d[k]) for k in ("x", "restored", "aux", "z", "prev")}
    c = R.sampler_coefs(25, 0.25, 0.75, 1, 1)
    what = f"sampler_update i=25 all branches on, n={d['x'].numel()}"
    r0, r1 = _sampler_update(dev, d, placed, c, (1, 1, 1, 1, 1), what)
    parity_log(f"ew_exact {what}: worst err / bound = {r0:.3f} (x0), {r1:.3f} (x_prev)")


# ================================================================================================ axpby / affine / variance
@pytest.mark.parametrize("with_y", [False, True], ids=["x_only", "x_and_y"])
@pytest.mark.parametrize("clamp", R.AXPBY_CLAMPS, ids=["unclamped", "clamped", "floor_only"])
@pytest.mark.parametrize("coefs", R.AXPBY_COEFS, ids=["third_1.7", "1.7_-0.6"])
def test_axpby(dev, coefs, clamp, with_y):
    _axpby(dev, 4099, coefs, clamp, with_y)


def test_axpby_beyond_two_grids(dev):
    _axpby(dev, R.TRIP_N, R.AXPBY_COEFS[0], R.AXPBY_CLAMPS[1], True)


def _axpby(dev, n, coefs, clamp, with_y):
    ops = _ops()
    x, y = R.axpby_case(n)
    (a, b), (lo, hi) = coefs, clamp
    ref, bound = R.axpby64(x, y if with_y else None, a, b, lo, hi)
    ins = [_in(dev, x)] + ([_in(dev, y)] if with_y else [])
    out = _out(dev, (n,))
    ops.axpby(ins[0][1], ins[1][1] if with_y else None, R.f32(a), R.f32(b), out=out[1], lo=lo, hi=hi)
    what = f"axpby_f32 n={n} a={a:.3g} b={b:.3g} [{lo}, {hi}] y={with_y}"
    _check_guards(ins, [out], what)
    log_ratio(what, R.within(out[1], ref, bound, what))


@pytest.mark.parametrize("trip", TRIPS, ids=_tid)
def test_affine_channels(dev, trip):
    ops = _ops()
    x, sub, mul = R.affine_case(trip)
    ref, bound, pre = R.affine64(x, sub, mul)
    assert bool((pre > 0.8).any()) and bool((pre < -0.8).any()) and bool((pre.abs() < 0.8).any())
    sd, md = _in(dev, sub), _in(dev, mul)
    A = R.AFFINE
    got = run_both(dev, {"s": (x, FP, 1, 7)}, {"y": (tuple(x.shape), FP, 2, 6)},
                   lambda s, y: ops.affine_channels(s, 3, A["a"], A["b"], A["lo"], A["hi"], sd[1], md[1], y), "affine_channels")["y"]
    _check_guards([sd, md], [], "affine_channels")
    what = f"affine_channels_f32 {tuple(x.shape)}"
    log_ratio(what, R.within(got, ref, bound, what))


@pytest.mark.parametrize("trip", TRIPS, ids=_tid)
def test_learned_range_variance(dev, trip):
    ops = _ops()
    mo, C, lo, hi = R.learned_range_case(trip)
    lv, b_lv, var, b_var = R.learned_range64(mo, C, lo, hi)
    ins = [_in(dev, mo)]
    shape = (mo.shape[0], C) + tuple(mo.shape[2:])
    vo, lo_ = _out(dev, shape), _out(dev, shape)
    ops.learned_range_variance(ins[0][1], C, lo, hi, out=(vo[1], lo_[1]))
    what = f"learned_range_variance {tuple(mo.shape)}"
    _check_guards(ins, [vo, lo_], what)
    r0 = R.within(lo_[1], lv, b_lv, what + " log variance")
    r1 = R.within(vo[1], var, b_var, what + " variance")
    parity_log(f"ew_exact {what}: worst err / bound = {r0:.3f} (log variance), {r1:.3f} (variance)")


# ================================================================================================ gated blend
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
@pytest.mark.parametrize("C", [40, 128, None], ids=["C40", "C128", "trip"])
def test_gated_blend(dev, dtype, C):
    ops = _ops()
    trip = C is None
    C = gran(dtype) if trip else C
    x, m, gate = R.blend_case(dtype, C, trip)
    ref, bound = R.blend64(x, m, gate, dtype)
    Fr, g = gate.shape[0], gran(dtype)
    gbuf = torch.full((Fr + 2, C + 24), IN_FILL, device=dev)
    gv = gbuf[1:Fr + 1, 8:8 + C]
    gv.copy_(gate.to(dev))
    gbefore = gbuf.clone()
    got = run_both(dev, {"x": (x, dtype, g, C + 2 * g), "m": (m, dtype, 2 * g, C + 3 * g)}, {"y": (tuple(x.shape), dtype, g, C + g)},
                   lambda x, m, y: ops.gated_blend(x, m, gv, out=y), "gated_blend")["y"]
    assert torch.equal(bits(gbuf), bits(gbefore))
    what = f"gated_blend {NAME[dtype]} {tuple(x.shape)}"
    r = R.within(got, ref, bound, what)
    if not trip:    # saturation: s = 1 exactly at g = 20 and 90 (the output is m), s = 0 exactly at g = -90 (the output is x)
        got = got.float()
        R.assert_same_bits(got[..., 1], m[..., 1], what + " g = 20")
        R.assert_same_bits(got[..., 3], m[..., 3], what + " g = 90")
        R.assert_same_bits(got[..., 4], x[..., 4], what + " g = -90")
    log_ratio(what, r)


# ================================================================================================ timestep embedding
@pytest.mark.parametrize("sin_first", [False, True], ids=["cos_sin", "sin_cos"])
@pytest.mark.parametrize("dim", R.EMB_DIMS)
def test_timestep_embedding(dev, dim, sin_first):
    ops = _ops()
    t = torch.tensor(R.EMB_T)
    ref, bound = R.embedding64(t, dim, sin_first)
    tin = _in(dev, t)
    out = _out(dev, (t.numel(), dim))
    ops.timestep_embedding(tin[1], dim, R.MAX_PERIOD, out=out[1], sin_first=sin_first)
    what = f"timestep_embedding dim={dim} sin_first={sin_first}"
    _check_guards([tin], [out], what)
    log_ratio(what, R.within(out[1], ref, bound, what))


# ================================================================================================ add_act with SiLU / GELU
@pytest.mark.parametrize("two", [False, True], ids=["x0", "x0+x1"])
@pytest.mark.parametrize("act", [ACT_SILU, ACT_GELU], ids=ACT_NAMES.get)
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_add_act_silu_gelu(dev, dtype, act, two):
    _add_act_close(dev, dtype, act, two, False)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_add_act_silu_beyond_two_grids(dev, dtype):
    _add_act_close(dev, dtype, ACT_SILU, True, True)


def _add_act_close(dev, dtype, act, two, trip):
    ops = _ops()
    x0, x1 = R.add_act_case(dtype, trip)
    x1 = x1 if two else None
    C, g = x0.shape[3], gran(dtype)
    ref, S, extra = R.add_act64(x0, x1, act)
    ins = {"a": (x0, dtype, g, C + 2 * g)}
    if two:
        ins["b"] = (x1, dtype, 2 * g, C + 3 * g)
    got = run_both(dev, ins, {"y": (tuple(x0.shape), dtype, g, C + g)}, lambda a, y, b=None: ops.add_act(a, b, act, out=y), "add_act")["y"]
    what = f"add_act {ACT_NAMES[act]} two={two} {NAME[dtype]} {tuple(x0.shape)}"
    assert bool(torch.isfinite(got).all()), what
    r = assert_act_close(got.to(dtype), ref, S, R.K_ACT[act], dtype, what, extra=extra)
    if not trip:
        assert bool((got[..., 1] == 128.0).all()) and bool((got[..., 2].abs() <= ACT_FLOOR).all()), what + ": saturated ends"
    parity_log(f"ew_exact {what}: max err / (2^-24 S) = {r:.3f} (k = {R.K_ACT[act]})")


# ================================================================================================ sft_fuse / channel_gate
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_sft_fuse(dev, dtype):
    """Per element on the small case; tests/test_gpu_prior_strides.py already runs one beyond two grids."""
    ops = _ops()
    dec, sc, sh = R.sft_case(dtype)
    ref, bound = R.sft64(dec, sc, sh, dtype)
    shape = (1, 1, dec.numel() // gran(dtype), gran(dtype))
    placed = [flat_guarded(shape, dtype, dev, IN_FILL, t) for t in (dec, sc, sh)]
    out = _out(dev, shape, dtype)
    ops.sft_fuse(placed[0][1], placed[1][1], placed[2][1], R.SFT_W, out=out[1])
    what = f"sft_fuse {NAME[dtype]} n={dec.numel()}"
    _check_guards(placed, [out], what)
    log_ratio(what, R.within(out[1].reshape(-1), ref, bound, what))


@pytest.mark.parametrize("use", list(R.GATE_USES))
@pytest.mark.parametrize("dtype", DTYPES, ids=_tid)
def test_channel_gate(dev, dtype, use):
    ops = _ops()
    kw = R.GATE_USES[use]
    x, a, gate, bias = R.gate_case(dtype)
    T, H, W, C = x.shape
    g = gran(dtype)
    ref, bound = R.gate64(x, a, gate, bias, kw, dtype)
    gd, bd = _in(dev, gate), _in(dev, bias)
    ins = {"x": (x, dtype, g, C + 2 * g)}
    if kw.get("add"):
        ins["a"] = (a, dtype, 2 * g, C + 2 * g)

    def call(x, y, a=None):
        ops.channel_gate(x, gd[1], logit=kw["logit"], add_x=kw.get("add_x", False), bias=bd[1] if kw.get("bias") else None, add=a, out=y)
    got = run_both(dev, ins, {"y": ((T, H, W, C), dtype, g, C + 3 * g)}, call, f"channel_gate {use}")["y"]
    what = f"channel_gate {use} {NAME[dtype]} {tuple(x.shape)}"
    r0 = R.within(got, ref, bound, what)
    xd = x.to(dev, dtype).contiguous()
    call(xd, xd, a.to(dev, dtype) if kw.get("add") else None)           # in place, as the model calls it
    _check_guards([gd, bd], [], what)
    r1 = R.within(xd, ref, bound, what + " in place")
    assert torch.equal(xd.double().cpu(), got), what + ": in place differs from out of place"
    log_ratio(what, max(r0, r1))
