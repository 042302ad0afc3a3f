"""The image-space f32 entries of the sampler and of the degradation operators, called directly.

flair_predict_xstart, flair_sampler_update, flair_axpby_f32, flair_learned_range_variance, flair_depthwise_filter,
flair_matmul_f32 and flair_gather_mac_f32 are otherwise reached only through p_sample_loop, pseudoSR, SRConv and Resizer
at one or two square sizes and with tolerances sized for a whole trajectory.  Here each runs alone against float64 torch
at small non-square shapes that pin its branches, with tests/util.py:TOL[f32] relative to max|ref| (the filters: the
2e-5 * max(1, |ref|) of test_blur_operator_vs_oracle).  These entries take no strides: every output is a dense slice of a
longer allocation of sentinels (tests/util.py:flat_guarded) that must come back unchanged around the slice, every input
a slice of an allocation of NaNs that must come back unchanged altogether."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import IN_FILL, OUT_FILL, TOL, assert_flat_untouched, bits, flat_guarded

pytestmark = pytest.mark.gpu
FP = torch.float32


def _ops():
    from flair_amd import ops
    return ops


def _in(dev, t, dtype=FP):
    """A cpu tensor as a dense device tensor between NaNs (an int32 one between zeros)."""
    return flat_guarded(tuple(t.shape), dtype, dev, IN_FILL if dtype == FP else 0, t)


def _out(dev, shape):
    return flat_guarded(tuple(shape), FP, dev, OUT_FILL)


def _check_guards(ins, outs, what):
    torch.cuda.synchronize()
    for i, (buf, _, before) in enumerate(ins):
        assert_flat_untouched(buf, before, None, f"{what}: input {i}")
    for i, (buf, v, before) in enumerate(outs):
        assert_flat_untouched(buf, before, v, f"{what}: output {i}")


def close(got, ref, what, scale=1.0):
    """TOL[f32] relative to max|ref|."""
    rel, ab = TOL[FP]
    err = (got.double().cpu() - ref).abs().max().item()
    bound = scale * rel * ref.abs().max().item() + ab
    print(f"{what}: max|err| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e}"


def _tables(steps=50):
    from oracle import diffusion as odiff
    return odiff.Spaced(odiff.spaced_steps(1000, str(steps)), odiff.named_betas("face_blur", 1000))


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ predict_xstart
@pytest.mark.parametrize("clip", [0, 1], ids=["raw", "clipped"])
@pytest.mark.parametrize("Cm", [3, 6])
def test_predict_xstart(dev, clip, Cm):
    """Three images, so that a model output of Cm = 6 channels (eps | variance) is strided differently from x."""
    ops = _ops()
    tab = _tables()
    N, C, H, W = 3, 3, 10, 14
    g = torch.Generator().manual_seed(Cm)
    x, mo = torch.randn(N, C, H, W, generator=g), torch.randn(N, Cm, H, W, generator=g)
    a, b = f32(tab.sqrt_recip_alphas_cumprod[25]), f32(tab.sqrt_recipm1_alphas_cumprod[25])
    ref = a * x.double() - b * mo[:, :C].double()
    if clip:
        ref = ref.clamp(-1, 1)
    ins = [_in(dev, x), _in(dev, mo)]
    out = _out(dev, x.shape)
    ops.predict_xstart(ins[0][1], ins[1][1], a, b, clip, out=out[1])
    _check_guards(ins, [out], "predict_xstart")
    close(out[1], ref, f"predict_xstart Cm={Cm} clip={clip}")


# ------------------------------------------------------------------------------------------------ sampler_update
def _update_ref(dt, c, x, x0, restored, aux, z, prev, T, Tp):
    """gaussian_diffusion.py:465-515 in dtype dt; c: dict of python floats (already rounded to f32)."""
    x, x0 = x.to(dt), x0.to(dt)
    v = x0
    if restored is not None:
        v = v - c["gamma"] * restored.to(dt)
        if c["clip"]:
            v = v.clamp(-1, 1)
    if aux is not None:
        f = aux.to(dt)
        if c["clip"]:
            f = f.clamp(-1, 1)
        v = c["w"] * v + (1 - c["w"]) * f
    if prev is not None:
        v = v.reshape(-1, T, *v.shape[1:]).clone()
        v[:, :Tp] = prev.to(dt)
        v = v.reshape(-1, *v.shape[2:])
    eps = (c["recip"] * x - v) / c["recipm1"]
    out = c["prev"] * v
    if c["nonzero"]:
        out = out + c["sq1mrho"] * c["co"] * eps + c["sqrho"] * c["co"] * z.to(dt)
    return v, out


@pytest.mark.parametrize("i", [49, 25, 0], ids=["early", "middle", "last"])
def test_sampler_update_branches(dev, i):
    """The whole cross-product restored x aux x nonzero x clip x prev_recon (32 tiny launches) with the oracle's
    coefficients at timestep i of 50.  Two clips of T = 4 frames, the first Tp = 2 of each pinned to prev_recon (the
    b * Tp + t indexing needs more than one clip to show).  x0 is made the way the sampler makes it (predict_xstart of
    x and a model eps, then perturbed), so that eps' = (c_recip * x - x0) / c_recipm1 is the cancellation it is in use.
    Both x0 (updated in place) and x_prev take TOL[f32] as it stands.  The division by c_recipm1 = 0.01 at the last
    timestep does not need more: there the noise coefficient is 0, and the same formula in f32 torch on the CPU errs
    against the float64 reference by at most 4.9e-7 (i = 49), 4.6e-7 (i = 25) and 8.7e-8 (i = 0) over the 32 cases, under
    1 % of the bounds 6.3e-5, 7.7e-5 and 2.1e-5."""
    ops = _ops()
    tab = _tables()
    B, T, Tp, C, H, W = 2, 4, 2, 3, 6, 10
    g = torch.Generator().manual_seed(100 + i)
    shape = (B * T, C, H, W)
    x = torch.randn(shape, generator=g)
    recip, recipm1 = f32(tab.sqrt_recip_alphas_cumprod[i]), f32(tab.sqrt_recipm1_alphas_cumprod[i])
    x0 = (recip * x - recipm1 * torch.randn(shape, generator=g) + 0.3 * torch.randn(shape, generator=g)).clamp(-1.3, 1.3)
    restored = torch.randn(shape, generator=g) * 0.5
    aux = torch.randn(shape, generator=g) * 0.9
    z = torch.randn(shape, generator=g)
    prev = torch.rand(B, Tp, C, H, W, generator=g) * 2 - 1
    rho = 0.25
    for has_r, has_a, nonzero, clip, has_p in itertools.product([0, 1], repeat=5):
        c = dict(gamma=f32(0.7), w=f32(0.75), recip=recip, recipm1=recipm1, prev=f32(tab.sqrt_alphas_cumprod_prev[i]),
                 co=f32(tab.sqrt_one_minus_alphas_cumprod_prev[i]), sq1mrho=f32(np.sqrt(1 - rho)), sqrho=f32(np.sqrt(rho)),
                 clip=clip, nonzero=nonzero)
        args = (x, x0, restored if has_r else None, aux if has_a else None, z, prev if has_p else None, T, Tp)
        ref_x0, ref_prev = _update_ref(torch.float64, c, *args)
        k = ops.SamplerCoefs()
        k.gamma, k.w_aux = c["gamma"], c["w"]
        k.sqrt_recip_alphas_cumprod, k.sqrt_recipm1_alphas_cumprod = recip, recipm1
        k.sqrt_alphas_cumprod_prev, k.sqrt_one_minus_alphas_cumprod_prev = c["prev"], c["co"]
        k.sqrt_one_minus_rho, k.sqrt_rho = c["sq1mrho"], c["sqrho"]
        k.clip_denoised, k.nonzero = clip, nonzero
        k.frame_elems, k.frames, k.prev_frames = C * H * W, T, Tp
        ins = [_in(dev, x)] + [_in(dev, t) for t, on in ((restored, has_r), (aux, has_a), (z, nonzero), (prev, has_p)) if on]
        it = iter(ins[1:])
        r_d, a_d, z_d, p_d = (next(it)[1] if on else None for on in (has_r, has_a, nonzero, has_p))
        x0g = flat_guarded(shape, FP, dev, OUT_FILL, x0)          # read and written in place
        out = _out(dev, shape)
        ops.sampler_update(k, ins[0][1], x0g[1], r_d, a_d, z_d, p_d, out=out[1])
        what = f"sampler_update i={i} restored={has_r} aux={has_a} nonzero={nonzero} clip={clip} prev={has_p}"
        _check_guards(ins, [x0g, out], what)
        close(x0g[1], ref_x0, what + " x0")
        close(out[1], ref_prev, what + " x_prev")


# ------------------------------------------------------------------------------------------------ axpby / variance
@pytest.mark.parametrize("lo,hi", [(float("-inf"), float("inf")), (-1.0, 1.0), (-0.25, float("inf"))],
                         ids=["unclamped", "clamped", "floor_only"])
@pytest.mark.parametrize("with_y", [False, True], ids=["x_only", "x_and_y"])
def test_axpby(dev, lo, hi, with_y):
    ops = _ops()
    n = 4099                                            # 16 workgroups and three threads
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = f32(1.7), f32(-0.6)
    ref = (a * x.double() + (b * y.double() if with_y else 0)).clamp(lo, hi)
    ins = [_in(dev, x)] + ([_in(dev, y)] if with_y else [])
    out = _out(dev, (n,))
    ops.axpby(ins[0][1], ins[1][1] if with_y else None, a, b, out=out[1], lo=lo, hi=hi)
    _check_guards(ins, [out], "axpby")
    close(out[1], ref, "axpby")


def test_learned_range_variance(dev):
    """Channels [C, 2C) of three images at a non-square size, with the oracle's clipped posterior log variance and
    log beta at timestep 25 of 50 as the range."""
    ops = _ops()
    tab = _tables()
    N, C, H, W = 3, 3, 6, 10
    lo, hi = f32(tab.posterior_log_variance_clipped[25]), f32(np.log(tab.betas[25]))
    mo = torch.randn(N, 2 * C, H, W, generator=torch.Generator().manual_seed(9))
    frac = (mo[:, C:].double() + 1) / 2
    ref_log = frac * hi + (1 - frac) * lo
    ins = [_in(dev, mo)]
    var, logvar = _out(dev, (N, C, H, W)), _out(dev, (N, C, H, W))
    ops.learned_range_variance(ins[0][1], C, lo, hi, out=(var[1], logvar[1]))
    _check_guards(ins, [var, logvar], "learned_range_variance")
    close(logvar[1], ref_log, "learned_range log variance")
    close(var[1], ref_log.exp(), "learned_range variance")


# ------------------------------------------------------------------------------------------------ depthwise filter
def _pad_index(a, n, reflect):
    if reflect:
        a = a.abs()
        a = torch.where(a > n - 1, 2 * (n - 1) - a, a)
        return a.clamp(min=0)
    return a.clamp(0, n - 1)


def _filter_ref(x, K, pad, stride, off, stuff, stuff_off, Ho, Wo, reflect):
    """The definition in include/flair_hip.h, float64: zero-stuff, pad by index (replicate or reflect), cross-correlate."""
    N, C, H, W = x.shape
    v = torch.zeros(N, C, H * stuff, W * stuff, dtype=torch.float64)
    v[:, :, stuff_off::stuff, stuff_off::stuff] = x.double()
    kh, kw = K.shape
    ri = _pad_index(torch.arange((Ho - 1) * stride + kh) + off - pad, H * stuff, reflect)
    ci = _pad_index(torch.arange((Wo - 1) * stride + kw) + off - pad, W * stuff, reflect)
    vp = v[:, :, ri][:, :, :, ci].reshape(N * C, 1, len(ri), len(ci))
    return F.conv2d(vp, K.double()[None, None], stride=stride).reshape(N, C, Ho, Wo)


def _operator():
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(sigma=1.8),
                     kernel_indx=10).WrapArchitecture_PyTorch()
    return {k: torch.from_numpy(v) for k, v in A._host.items()}, int(A.pre_stride[0]), A.ds_factor


def _run_filter(dev, x, K, out_hw, **kw):
    ops = _ops()
    ins = [_in(dev, x), _in(dev, K)]
    out = _out(dev, (*x.shape[:2], *out_hw))
    ops.depthwise_filter(ins[0][1], ins[1][1], out_hw=out_hw, out=out[1], **kw)
    _check_guards(ins, [out], f"depthwise_filter {kw}")
    return out[1]


def _close_filter(got, ref, what):
    err = (got.double().cpu() - ref).abs().max().item()
    bound = 2e-5 * max(1.0, ref.abs().max().item())
    print(f"{what}: max|err| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("which", ["down", "inv", "up", "reflect"])
def test_depthwise_filter_parameter_sets(dev, which):
    """pseudoSR's three Filter_Layers (Down: 9 x 9, stride 4 from the pre-stride offset; InvHtH: 39 x 39; Up: 9 x 9 on
    the zero-stuffed grid) and imresize_efficient's reflect-padded blur, on a 40 x 56 low-resolution / 160 x 224
    high-resolution pair (neither a multiple of 32: the generic kernel)."""
    Ks, pre, f = _operator()
    h, w = 40, 56
    g = torch.Generator().manual_seed(3)
    lr, hr = torch.rand(2, 3, h, w, generator=g) * 2 - 1, torch.rand(2, 3, h * f, w * f, generator=g) * 2 - 1
    if which == "down":
        K = Ks["down"]
        got = _run_filter(dev, hr, K, (h, w), pad=K.shape[0] // 2, out_stride=f, out_offset=pre)
        ref = _filter_ref(hr, K, K.shape[0] // 2, f, pre, 1, 0, h, w, False)
    elif which == "inv":
        K = Ks["inv"]
        assert tuple(K.shape) == (39, 39)
        got = _run_filter(dev, lr, K, (h, w), pad=19)
        ref = _filter_ref(lr, K, 19, 1, 0, 1, 0, h, w, False)
    elif which == "up":
        K = Ks["up"]
        got = _run_filter(dev, lr, K, (h * f, w * f), pad=K.shape[0] // 2, stuff=f, stuff_offset=pre)
        ref = _filter_ref(lr, K, K.shape[0] // 2, 1, 0, f, pre, h * f, w * f, False)
    else:
        K = Ks["down"]
        got = _run_filter(dev, lr, K, (h, w), pad=K.shape[0] // 2, out_stride=1, out_offset=0, reflect=True)
        ref = _filter_ref(lr, K, K.shape[0] // 2, 1, 0, 1, 0, h, w, True)
    _close_filter(got, ref, f"depthwise_filter {which}")


@pytest.mark.parametrize("reflect", [False, True], ids=["replicate", "reflect"])
def test_depthwise_filter_tiled_equals_generic(dev, reflect):
    """39 x 39 taps, stride 1, a 64 x 96 output: the tiled kernel.  The same planes with one more output row (65 is no
    multiple of 32) go through the generic kernel; csrc/degrade.hip promises the same tap order and fused multiply-adds,
    so the 64 shared rows are bit-equal.  Both against float64."""
    Ks, _, _ = _operator()
    K = Ks["inv"]
    H, W = 64, 96
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(39)) * 2 - 1
    tiled = _run_filter(dev, x, K, (H, W), pad=19, reflect=reflect)
    generic = _run_filter(dev, x, K, (H + 1, W), pad=19, reflect=reflect)
    _close_filter(tiled, _filter_ref(x, K, 19, 1, 0, 1, 0, H, W, reflect), "depthwise_filter tiled")
    _close_filter(generic, _filter_ref(x, K, 19, 1, 0, 1, 0, H + 1, W, reflect), "depthwise_filter generic 39 x 39")
    ne = bits(tiled) != bits(generic[:, :, :H])
    assert not ne.any(), f"tiled and generic kernels differ at {int(ne.sum())} element(s), first {ne.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ matmul / gather
@pytest.mark.parametrize("shared", ["none", "A", "B"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (17, 33, 50), (64, 48, 256)])
def test_matmul(dev, shared, M, N, K):
    """Batch 3; sizes on and off the 16 x 16 tile; either operand shared across the batch (batch stride 0)."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(*(() if shared == "A" else (3,)), M, K, generator=g)
    b = torch.randn(*(() if shared == "B" else (3,)), K, N, generator=g)
    ref = a.double() @ b.double()
    ins = [_in(dev, a), _in(dev, b)]
    out = _out(dev, (3, M, N))
    ops.matmul(ins[0][1], ins[1][1], out=out[1])
    _check_guards(ins, [out], "matmul")
    close(out[1], ref, f"matmul {M}x{N}x{K} shared={shared}")


@pytest.mark.parametrize("axis", ["middle", "last"])
@pytest.mark.parametrize("taps", [1, 8])
@pytest.mark.parametrize("Lin,Lout", [(24, 7), (9, 31)], ids=["shrink", "grow"])
def test_gather_mac(dev, axis, taps, Lin, Lout):
    """y[o][i][n] = sum_k w[k][i] * x[o][fov[k][i]][n] along a middle axis (inner = 5) and along the last (inner = 1);
    the field of view holds every index of [0, Lin), the first and the last among them."""
    ops = _ops()
    outer, inner = 6, (5 if axis == "middle" else 1)
    g = torch.Generator().manual_seed(taps * 100 + Lin)
    x = torch.randn(outer, Lin, inner, generator=g)
    fov = torch.randint(0, Lin, (taps, Lout), generator=g).int()
    fov[0, 0], fov[-1, -1] = 0, Lin - 1
    w = torch.randn(taps, Lout, generator=g)
    ref = torch.einsum("ki,okin->oin", w.double(), x.double()[:, fov.long()])
    ins = [_in(dev, x), _in(dev, fov, torch.int32), _in(dev, w)]
    out = _out(dev, (outer, Lout, inner))
    ops.gather_mac(ins[0][1], outer, Lin, inner, ins[1][1], ins[2][1], out=out[1])
    _check_guards(ins, [out], "gather_mac")
    close(out[1], ref, f"gather_mac {axis} taps={taps} {Lin}->{Lout}")
