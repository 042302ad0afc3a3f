"""References, data, bounds, f32 emulations and mutants for the streaming kernels of csrc/ew.hip, and for their look-alikes
flair_sft_fuse (prior.hip) and flair_channel_gate_nhwc (parse.hip).  Plain torch / numpy on the CPU; used by
tests/test_ew_exact_cpu.py (which proves what is claimed here) and tests/test_gpu_ew_exact.py (which runs the entries).

Two criteria.
  A, bit for bit: an output that is RNE(dtype, one f32 operation), a copy, a selection, or a sum of integers below 2^24 has
     exactly one correct value.
  B, per element: ew.hip is built with -ffp-contract=fast, so an expression of products and sums has several legitimate f32
     results.  |got - ref64| <= n u S + out_rounding, u = 2^-24, S = the sum of the magnitudes of the terms that the kernel
     rounds (float64, per element), n = the longest chain of f32 roundings that any term of S passes through in the
     kernel's unfused form, counted from the source beside each N_* below (a contraction only removes roundings).
Where a bound rests on a library function (expf, logf, sinf, cosf, __expf, the sigmoid), its constant is 4 times the
deviation of the reference's own float32 formulation on the CPU from float64 on the same inputs: the margin the project
uses against f32 ATen for its warp, AMT and SuperSloMo kernels.  The measurements are beside the constants; the CPU test
repeats them.  No bound comes from a kernel's output.

Outside the entries' contract and not tested: NaN in the pools (fmaxf drops a NaN where torch propagates it).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.util import (ACT_GELU, ACT_LIPSCHITZ, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, U24, act64, act_sens64,
                        int_tensor, out_rounding, rb)

BF, FP = torch.bfloat16, torch.float32
NAME = {BF: "bf16", FP: "f32"}
U = U24
GRID = 2048 * 256           # threads of a capped launch: grid_for(n, 256, 2048) (common.h:46), every looping entry of ew.hip
VEC = {BF: 8, FP: 4}        # elements per 16-byte access (common.h ET<E>::VEC)
TRIP_SHAPE = (7, 105, 1427)  # 1,048,845 pixels = 2 * GRID + 269: every thread runs twice, 269 of them a third time
TRIP_SHAPE3 = (7, 35, 1427)  # the same count as pixels x 3 channels, for the entries whose work item is one element

# ---- constants that rest on a library function: 4 x the measured deviation of the f32 CPU formulation, rounded up by less
# than a tenth so that another build of ATen's vector math does not trip the check (measured with torch 2.10 on the
# inputs of the cases below; tests/test_ew_exact_cpu.py::test_library_constants measures again and holds 4 x measured <= C)
C_EXP = 4.0     # relative error of expf in units of u.  torch.exp(f32) against exp(float64): 0.92 u at most on the log
#                 variances of learned_range_case and on -g of the gates of blend_case
C_SIG = 6.8     # relative error of the f32 sigmoid 1 / (1 + expf(-g)) in units of u.  torch.sigmoid(f32): 1.59 u on gate_case
C_ARG = 44.0    # relative error of the embedding's argument t * exp(-log(P) k / half) formed in f32 as the reference
#                 (oracle.unet.timestep_embedding) forms it, against t * P^(-k / half) in float64: 10.47 u (dim 1280)
C_OUT = 2.6     # absolute error of cosf / sinf at that f32 argument, in units of u: 0.60 u
LOG2E = 1.4426950408889634


def f32(v):
    return float(np.float32(v))


def t32(v):
    return torch.tensor(v, dtype=FP)


def fma32(a, b, c):
    """a * b + c rounded once to f32 (the product of two f32 numbers is exact in float64; the float64 sum rounds before the
    f32 rounding does, which moves a result only at a 2^-29 near-tie: good enough for an emulation)."""
    a, b, c = (v if torch.is_tensor(v) else t32(v) for v in (a, b, c))
    return (a.double() * b.double() + c.double()).float()


def within(got, ref64, bound, what):
    """|got - ref64| <= bound for every element, NaN fails -> the worst err / bound (0 / 0 counts as 0).  The message names
    the worst ratio and the first offending index; `what` carries the branch."""
    assert ref64.dtype == torch.float64 and bound.dtype == torch.float64 and got.shape == ref64.shape, (what, got.shape, ref64.shape)
    err = (got.detach().cpu().double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    bad = err > bound
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} element(s) beyond the bound, worst err / bound "
                             f"{ratio.max().item():.3f}; first at {list(first)}: got {got[first].item()!r}, expected "
                             f"{ref64[first].item()!r}, err {err[first].item():.3e} > {bound[first].item():.3e}")
    return ratio.max().item()


def beyond(got, ref64, bound):
    """Whether the comparison of `within` rejects got (for the mutants)."""
    err = (got.detach().cpu().double() - ref64).abs()
    return bool((torch.isnan(err) | (err > bound.expand_as(err))).any())


def same_bits(a, b):
    """Strict equality of the bits where neither is NaN, NaN exactly where the other is NaN (a NaN's payload is no part of
    any contract); the sign of a zero counts."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all()) and bool(((a.view(it) == b.view(it)) | na).all())


def assert_same_bits(got, want, what):
    if same_bits(got, want):
        return
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    ne = (torch.isnan(got) != torch.isnan(want)) | ((got.view(it) != want.view(it)) & ~torch.isnan(got))
    first = tuple(ne.nonzero()[0].tolist())
    raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} element(s) differ in bits; first at {list(first)}: got "
                         f"{got[first].item()!r} ({got.view(it)[first].item() & 0xFFFFFFFF:#x}), expected {want[first].item()!r} "
                         f"({want.view(it)[first].item() & 0xFFFFFFFF:#x})")


def rounding_share(v32, dtype):
    """The share of the f32 values that are no numbers of `dtype`: there the store has to round."""
    return (v32.to(dtype).float() != v32).float().mean().item()


def assert_rounding_exercised(v32, dtype, what, least=0.25):
    if dtype == BF:
        share = rounding_share(v32, dtype)
        assert share >= least, f"{what}: only {share:.1%} of the outputs need rounding to bf16"


def trips_distinct(items):
    """items: (work items, values per item).  No two work items GRID apart hold equal values, and there is a third trip."""
    n = items.shape[0]
    return n > 2 * GRID and bool((items[:-GRID] != items[GRID:]).any(1).all())


# ================================================================================================ A1: the bf16 store
RNE_DELTAS = (0, 0x7FFF, 0x8000, 0x8001)    # on the bf16 number, just below a tie, the tie, just above it


def u32_to_f32(u):
    return torch.from_numpy(np.asarray(u, dtype=np.uint32).view(np.float32).copy())


def bf16_case_bits():
    """(p << 16) + d for all 2^16 bf16 patterns p and the four d; where p is inf or NaN only d = 0 is kept (the other sums
    are NaNs that no finite value leads to): 261,376 values, padded with 1.0 to a multiple of 72 -> uint32 numpy array."""
    p = np.arange(1 << 16, dtype=np.uint32)
    special = (p & 0x7F80) == 0x7F80
    u = np.concatenate([((p << 16) + np.uint32(d))[~special if d else np.ones_like(special)] for d in RNE_DELTAS])
    return np.concatenate([u, np.full((-u.size) % 72, 0x3F800000, dtype=np.uint32)])


def rne_bf16_bits(u, fault=None):
    """Round-to-nearest-even of f32 bit patterns to bf16 bit patterns by integer arithmetic (NaN -> a quiet NaN).
    fault: 'truncate' drops the low half, 'half_away' adds 0x8000 before dropping it."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    if fault == "truncate":
        r = u >> 16
    elif fault == "half_away":
        r = (u + 0x8000) >> 16
    else:
        r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_from_bits(b):
    return torch.from_numpy(np.asarray(b, dtype=np.uint16).view(np.int16).copy()).view(BF)


@functools.lru_cache(maxsize=1)
def bf16_case():
    """-> (f32 values (261,432,), their RNE cast by torch, widened back to f32 = p' << 16)."""
    v = u32_to_f32(bf16_case_bits())
    want = v.to(BF)
    return v, want, want.float()


@functools.lru_cache(maxsize=1)
def tie_case():
    """For the vector stores, whose input is bf16 already: x0 = every finite bf16 number with an exponent of at least -100,
    x1 = half a bf16 unit in the last place of x0 with x0's sign (a power of two: a bf16 number).  The f32 sum x0 + x1 is
    exact and is the tie above x0, for even and for odd significands -> (x0, x1, RNE(x0 + x1)), length a multiple of 8."""
    p = np.arange(1 << 16, dtype=np.uint32)
    e = (p >> 7) & 0xFF
    p = p[(e >= 27) & (e <= 254)]
    p = p[:p.size // 8 * 8]
    x0 = u32_to_f32(p << 16)
    half = u32_to_f32(((p & 0x8000) | ((((p >> 7) & 0xFF) - 8) << 7)) << 16)
    s = x0 + half
    assert bool((s.double() == x0.double() + half.double()).all())
    assert bool((torch.from_numpy(s.numpy().view(np.uint32).astype(np.int64)) & 0xFFFF == 0x8000).all())
    return x0.to(BF), half.to(BF), s.to(BF)


@functools.lru_cache(maxsize=1)
def layout_trip_case():
    """(N, 3, H, W) f32 with N H W = 2 * GRID + 269 pixels, the work items of both layout conversions."""
    T, H, W = TRIP_SHAPE
    return torch.randn(T, 3, H, W, generator=torch.Generator().manual_seed(77))


# ================================================================================================ A2: one f32 operation
def act_f32(v, act):
    """apply_act (common.h:118) for the activations that are one f32 operation: the leaky slopes are one product."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    slope = t32({ACT_LRELU01: 0.1, ACT_LRELU02: 0.2}[act])
    return torch.where(v > 0, v, slope * v)


@functools.lru_cache(maxsize=None)
def pixel_case(dtype, trip=False):
    """x (T, H, W, C) rounded to dtype, a second operand of the same kind, a weight per pixel with no two neighbours equal,
    bias rows (T, C + 6) that differ between the frames.  trip: C = one vector, more than two grids of pixels."""
    g = torch.Generator().manual_seed(41 + trip)
    shape = TRIP_SHAPE + (VEC[dtype],) if trip else (3, 5, 7, 48)
    T, H, W, C = shape
    x, x1 = rb(torch.randn(shape, generator=g), dtype), rb(torch.randn(shape, generator=g), dtype)
    wmap = torch.rand(T * H * W, generator=g) + 0.5
    fb = torch.randn(T, C + 6, generator=g)
    assert bool((wmap[1:] != wmap[:-1]).all()) and bool((fb[1:, :C] != fb[:-1, :C]).all())
    return dict(x=x, x1=x1, wmap=wmap, fb=fb)


def frame_bias_f32(x, fb, fault=None):
    """add_frame_bias_kernel (ew.hip:181): x + bias[f][c] in f32 (before the store's cast)."""
    T, H, W, C = x.shape
    b = fb[:, :C]
    if fault == "next_frame":
        b = fb.roll(-1, 0)[:, :C]
    elif fault == "next_channel":
        b = fb[:, 1:C + 1]
    return x.float() + b.view(T, 1, 1, C)


def scale_pixels_f32(x, wmap, fault=None):
    """scale_pixels_kernel (ew.hip:153): x * wmap[p] in f32."""
    T, H, W, C = x.shape
    w = wmap.roll(-1) if fault == "next_pixel" else wmap
    return x.float() * w.view(T, H, W, 1)


def add_act_f32(x0, x1, act):
    """add_act_kernel (ew.hip:234-237): the f32 sum, then the one-operation activation."""
    return act_f32(x0.float() + x1.float() if x1 is not None else x0.float(), act)


POOL_SHAPES = ((2, 9, 11), (2, 8, 10), (2, 9, 10))


@functools.lru_cache(maxsize=None)
def pool_case(dtype, shape, trip=False):
    """All negative data: a padded position counted as 0 wins in every border window."""
    T, H, W = (TRIP_SHAPE[0], 2 * TRIP_SHAPE[1] - 1, 2 * TRIP_SHAPE[2] - 1) if trip else shape
    C = VEC[dtype] if trip else 24
    g = torch.Generator().manual_seed(H * W + C)
    x = rb(-(torch.randn(T, H, W, C, generator=g).abs() + 0.01), dtype)
    assert bool((x < 0).all())
    return x


def maxpool_ref(x, fault=None):
    """nn.MaxPool2d(3, 2, 1) of a (T, H, W, C) tensor by F.max_pool2d in f32 (a selection: exact in any type)."""
    xn = x.float().permute(0, 3, 1, 2)
    if fault == "pad_zero":
        y = F.max_pool2d(F.pad(xn, (1, 1, 1, 1), value=0.0), 3, 2, 0)
    else:
        y = F.max_pool2d(xn, 3, 2, 1)
    return y.permute(0, 2, 3, 1).contiguous().to(x.dtype)


def maxpool_loop(x):
    """The same by an explicit loop over the windows (maxpool3s2_kernel, ew.hip:258-269)."""
    T, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y = torch.full((T, Ho, Wo, C), float("-inf"))
    for ho in range(Ho):
        for wo in range(Wo):
            for dh in (-1, 0, 1):
                for dw in (-1, 0, 1):
                    h, w = 2 * ho + dh, 2 * wo + dw
                    if 0 <= h < H and 0 <= w < W:
                        y[:, ho, wo] = torch.maximum(y[:, ho, wo], x[:, h, w].float())
    return y.to(x.dtype)


# ================================================================================================ flair_linear_f32
# (M, K, N): both sides of each MMAX boundary (8 | 9, 16 | 17), K below, at and above one 512-wide round of the k loop with
# a ragged tail, N = 8205 >= 8192: eight features per wave, N % 32 = 13 (idle waves and a partly used one in the last
# workgroup).  The entry stages M * K floats in 64 KiB of LDS, so M = 32 goes with K <= 512 and K = 1031 with M <= 15.
LINEAR_SHAPES = ((8, 64, 36), (9, 77, 36), (16, 511, 36), (17, 513, 36), (32, 512, 131), (15, 1031, 131), (3, 96, 8205))
LINEAR_REFUSED = (32, 1031, 131)        # 131,968 bytes of staging: refused by the entry (ew.hip:318)


@functools.lru_cache(maxsize=None)
def linear_int_case(M, K, N):
    """Integers: x in [-8, 8], w in [-3, 3], bias in [-8, 8] -> x, w, b, the float64 product, sum |x| |w| + |b|."""
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b = int_tensor((M, K), -8, 8, g), int_tensor((N, K), -3, 3, g), int_tensor((N,), -8, 8, g)
    return x, w, b, x.double() @ w.double().t() + b.double(), x.double().abs() @ w.double().abs().t() + b.double().abs()


@functools.lru_cache(maxsize=None)
def linear_case(M, K, N):
    g = torch.Generator().manual_seed(7 * M + K + N)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)


K_SILU = 6      # v / (1 + __expf(-v)) with the IEEE divide: tests/test_gpu_act_exact.py derives k = 6


def linear64(x, w, b, act_in, act_out):
    """-> ref64, bound.  linear_f32_kernel (ew.hip:55-81): a lane adds ceil(K / 64) products with fmaf (one rounding each,
    :73), the shuffle tree adds six times (:80), the bias once (:81): n = ceil(K / 64) + 7 on S = sum_k |act(x) w| + |b|.
    act_in (:55) puts K_SILU u act_sens64(x) on every input, act_out (:81) K_SILU u act_sens64(v) on the result and
    passes the error of v through a slope of at most ACT_LIPSCHITZ."""
    K = x.shape[1]
    xa, w64, b64 = act64(x.double(), act_in), w.double(), b.double()
    v = xa @ w64.t() + b64
    bound = (math.ceil(K / 64) + 7) * U * (xa.abs() @ w64.abs().t() + b64.abs())
    if act_in != ACT_NONE:
        bound = bound + K_SILU * U * (act_sens64(x.double(), act_in) @ w64.abs().t())
    if act_out != ACT_NONE:
        bound = ACT_LIPSCHITZ[act_out] * bound + K_SILU * U * act_sens64(v, act_out)
    return act64(v, act_out), bound


def silu32(v):
    return v / (1.0 + torch.exp(-v))


def linear_emul(x, w, b, act_in, act_out, fused=True, fault=None):
    """The kernel's order in f32: lane l adds k = l, l + 64, ... (fmaf, or a product and a sum), then the xor tree.
    fault: 'k_tail' drops the k beyond the last full 512, 'bias_next' takes the bias of feature n + 1, 'act_in_rows'
    skips act_in for the rows m >= 8."""
    M, K = x.shape
    xs = silu32(x) if act_in == ACT_SILU else x.clone()
    if fault == "act_in_rows":
        xs[8:] = x[8:]
    Ke = K // 512 * 512 if fault == "k_tail" else K
    acc = torch.zeros(M, w.shape[0], 64)
    for k0 in range(0, Ke, 64):
        n = min(64, Ke - k0)
        xv, wv = xs[:, None, k0:k0 + n], w[None, :, k0:k0 + n]
        acc[..., :n] = fma32(xv, wv, acc[..., :n]) if fused else acc[..., :n] + xv * wv
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ off]
    bb = b.roll(-1) if fault == "bias_next" else b
    v = acc[..., 0] + bb
    return silu32(v) if act_out == ACT_SILU else v


# ================================================================================================ predict_xstart / sampler
@functools.lru_cache(maxsize=1)
def tables(steps=50):
    from oracle import diffusion as odiff
    return odiff.Spaced(odiff.spaced_steps(1000, str(steps)), odiff.named_betas("face_blur", 1000))


TIMESTEPS = (49, 25, 0)
XSTART_TRIP = (3, 3, 342, 341)      # 1,049,598 elements


@functools.lru_cache(maxsize=None)
def xstart_case(Cm, i, trip=False):
    """Three images, so that a C-for-Cm image stride of the model output shows -> x, model output, c_recip, c_recipm1."""
    N, C, H, W = XSTART_TRIP if trip else (3, 3, 10, 14)
    g = torch.Generator().manual_seed(10 * Cm + i)
    tab = tables()
    return (torch.randn(N, C, H, W, generator=g), torch.randn(N, Cm, H, W, generator=g),
            f32(tab.sqrt_recip_alphas_cumprod[i]), f32(tab.sqrt_recipm1_alphas_cumprod[i]))


N_XSTART = 3    # ew.hip:96: two products and their difference


def xstart64(x, mo, a, b, clip):
    """-> ref64, bound = N_XSTART u (|a x| + |b eps|).  The clamp (ew.hip:97) rounds nothing and has slope <= 1."""
    e = mo[:, :x.shape[1]].double()
    ref = a * x.double() - b * e
    return (ref.clamp(-1, 1) if clip else ref), N_XSTART * U * ((a * x.double()).abs() + (b * e).abs())


def xstart_emul(x, mo, a, b, clip, fused=False, fault=None):
    N, C, H, W = x.shape
    e = mo.reshape(-1)[:x.numel()].view(x.shape) if fault == "image_stride" else mo[:, :C]
    v = fma32(a, x, -(t32(b) * e)) if fused else t32(a) * x - t32(b) * e
    return v.clamp(-1, 1) if clip else v


RHOS, WS = (0.0, 0.25, 0.5), (0.75, 0.5)
SAMPLER_GEOM = dict(B=2, T=4, Tp=2, C=3, H=6, W=10)


@functools.lru_cache(maxsize=None)
def sampler_case(i, trip=False):
    """The data of test_sampler_update_branches: two clips of T = 4 frames, the first Tp = 2 of each pinned to prev (which
    differs between the clips); x0 made the way the sampler makes it.  trip: frames of 3 x 209 x 210 (1,053,360 elements)."""
    geo = dict(SAMPLER_GEOM, H=209, W=210) if trip else SAMPLER_GEOM
    B, T, Tp, C, H, W = (geo[k] for k in ("B", "T", "Tp", "C", "H", "W"))
    tab = tables()
    g = torch.Generator().manual_seed(100 + i)
    shape = (B * T, C, H, W)
    x = torch.randn(shape, generator=g)
    recip, recipm1 = f32(tab.sqrt_recip_alphas_cumprod[i]), f32(tab.sqrt_recipm1_alphas_cumprod[i])
    x0 = (recip * x - recipm1 * torch.randn(shape, generator=g) + 0.3 * torch.randn(shape, generator=g)).clamp(-1.3, 1.3)
    restored = torch.randn(shape, generator=g) * 0.5
    aux = torch.randn(shape, generator=g) * 0.9
    z = torch.randn(shape, generator=g)
    prev = torch.rand(B, Tp, C, H, W, generator=g) * 2 - 1
    assert bool((prev[0] != prev[1]).any())
    return dict(x=x, x0=x0, restored=restored, aux=aux, z=z, prev=prev, T=T, Tp=Tp, frame_elems=C * H * W)


def sampler_coefs(i, rho, w, clip, nonzero):
    """The f32 coefficients of flair_sampler_coefs at timestep i of 50, as python floats."""
    tab = tables()
    return dict(gamma=f32(0.7), w=f32(w), recip=f32(tab.sqrt_recip_alphas_cumprod[i]), recipm1=f32(tab.sqrt_recipm1_alphas_cumprod[i]),
                prev=f32(tab.sqrt_alphas_cumprod_prev[i]), co=f32(tab.sqrt_one_minus_alphas_cumprod_prev[i]),
                sq1mrho=f32(np.sqrt(1 - rho)), sqrho=f32(np.sqrt(rho)), clip=clip, nonzero=nonzero)


def _pin(v, prev, T, Tp):
    v = v.reshape(-1, T, *v.shape[1:]).clone()
    v[:, :Tp] = prev.to(v.dtype)
    return v.reshape(-1, *v.shape[2:])


N_X0_RESTORED = 2   # ew.hip:110: gamma * restored, the difference
N_X0_BLEND = 4      # ew.hip:116: 1 - w, two products, the sum
N_XPREV = 7         # ew.hip:126-128: the eps term passes c_recip * x, the difference, the division, sq1mRho * coNoise, the
#                     product with eps and two sums; c_prev * v one product and a sum; the z term two products and two sums


def sampler_x0_64(c, d, has_r, has_a, has_p):
    """x0 after sampler_update_kernel (ew.hip:108-124) in float64 -> dict(ref, bound, pinned (bool), and, where a clamp of
    x0 itself is the last operation, sat = +-1 where the value before the clamp is beyond +-1 by more than its bound, 0
    elsewhere)."""
    v = d["x0"].double()
    bound = torch.zeros_like(v)
    sat = torch.zeros_like(v)
    if has_r:
        t = c["gamma"] * d["restored"].double()
        bound = N_X0_RESTORED * U * (v.abs() + t.abs())
        v = v - t
        if c["clip"]:
            sat = torch.where(v.abs() - 1 > bound, torch.sign(v), sat)
            v = v.clamp(-1, 1)
    if has_a:
        f = d["aux"].double()
        if c["clip"]:
            f = f.clamp(-1, 1)
        w = c["w"]
        bound = N_X0_BLEND * U * ((w * v).abs() + ((1 - w) * f).abs()) + abs(w) * bound     # the blend passes v's error on
        v = w * v + (1 - w) * f
        sat = torch.zeros_like(v)
    pinned = torch.zeros_like(v, dtype=torch.bool)
    if has_p:
        v = _pin(v, d["prev"], d["T"], d["Tp"])
        pinned = _pin(pinned, torch.ones_like(d["prev"], dtype=torch.bool), d["T"], d["Tp"])
        bound = torch.where(pinned, torch.zeros_like(bound), bound)
        sat = torch.where(pinned, torch.zeros_like(sat), sat)
    return dict(ref=v, bound=bound, pinned=pinned, sat=sat)


def sampler_xprev_64(c, d, x0_out):
    """x_prev (ew.hip:125-129) in float64 from the kernel's own x0 output, so that x0's error is not charged twice (the rule
    of tests/test_gpu_norm_exact.py for the norm-then-affine case) -> ref, bound = N_XPREV u S,
    S = |c_prev v| + (c1 / c_recipm1)(|c_recip x| + |v|) + |c2 z|, c1 = sqrt(1 - rho) co, c2 = sqrt(rho) co."""
    v = x0_out.detach().cpu().double()
    cx = c["recip"] * d["x"].double()
    ref, S = c["prev"] * v, (c["prev"] * v).abs()
    if c["nonzero"]:
        c1, c2 = c["sq1mrho"] * c["co"], c["sqrho"] * c["co"]
        ref = ref + c1 * (cx - v) / c["recipm1"] + c2 * d["z"].double()
        S = S + abs(c1 / c["recipm1"]) * (cx.abs() + v.abs()) + (c2 * d["z"].double()).abs()
    return ref, N_XPREV * U * S


def sampler_emul(c, d, has_r, has_a, has_p, fused=False, fault=None):
    """sampler_update_kernel step by step in f32 -> (x0, x_prev).  fused: every product that feeds a sum is contracted.
    fault: 'prev_index' (prev_recon indexed b * T + t: frames beyond the tensor read NaN guards), 'clamp_after_blend',
    'w_for_1mw', 'swap_rho', 'div_recip'."""
    x, v = d["x"], d["x0"].clone()
    clip = c["clip"]
    if has_r:
        v = fma32(-c["gamma"], d["restored"], v) if fused else v - t32(c["gamma"]) * d["restored"]
        if clip and fault != "clamp_after_blend":
            v = v.clamp(-1, 1)
    if has_a:
        f = d["aux"].clamp(-1, 1) if clip else d["aux"]
        w = t32(c["w"])
        omw = w if fault == "w_for_1mw" else t32(1.0) - w
        v = fma32(w, v, omw * f) if fused else w * v + omw * f
        if clip and has_r and fault == "clamp_after_blend":
            v = v.clamp(-1, 1)
    if has_p:
        T, Tp = d["T"], d["Tp"]
        if fault == "prev_index":
            flat = d["prev"].reshape(-1, *v.shape[1:])
            n = torch.arange(v.shape[0])
            idx = (n // T) * T + n % T
            src = torch.where((idx < flat.shape[0]).view(-1, 1, 1, 1), flat[idx.clamp_max(flat.shape[0] - 1)],
                              torch.full_like(v, float("nan")))
            v = torch.where((n % T < Tp).view(-1, 1, 1, 1), src, v)
        else:
            v = _pin(v, d["prev"], T, Tp)
    sq1, sq = (c["sqrho"], c["sq1mrho"]) if fault == "swap_rho" else (c["sq1mrho"], c["sqrho"])
    den = t32(c["recip"] if fault == "div_recip" else c["recipm1"])
    eps = (fma32(c["recip"], x, -v) if fused else t32(c["recip"]) * x - v) / den
    a1, a2 = t32(sq1) * t32(c["co"]), t32(sq) * t32(c["co"])
    if not c["nonzero"]:
        return v, t32(c["prev"]) * v
    if fused:
        return v, fma32(c["prev"], v, fma32(a1, eps, a2 * d["z"]))
    return v, t32(c["prev"]) * v + (a1 * eps + a2 * d["z"])


# ================================================================================================ axpby / affine / variance
AXPBY_COEFS = ((1.0 / 3.0, 1.7), (1.7, -0.6))
AXPBY_CLAMPS = ((float("-inf"), float("inf")), (-1.0, 1.0), (-0.25, float("inf")))
N_AXPBY = 3     # ew.hip:137: two products and their sum; the clamp rounds nothing
TRIP_N = 2 * GRID + 259


@functools.lru_cache(maxsize=None)
def axpby_case(n):
    g = torch.Generator().manual_seed(n % 9973)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def axpby64(x, y, a, b, lo, hi):
    a, b = f32(a), f32(b)
    t = b * y.double() if y is not None else torch.zeros_like(x, dtype=torch.float64)
    return (a * x.double() + t).clamp(lo, hi), N_AXPBY * U * ((a * x.double()).abs() + t.abs())


def axpby_emul(x, y, a, b, lo, hi, fused=False):
    t = t32(b) * y if y is not None else torch.zeros_like(x)
    return (fma32(a, x, t) if fused else t32(a) * x + t).clamp(lo, hi)


AFFINE = dict(a=0.5, b=0.1, lo=-0.8, hi=0.8)
N_AFFINE = 4    # ew.hip:167-168: x * a, + b, - sub[c], * mul[c], on S = (|x a| + |b| + |sub|) |mul| (the clamp only shrinks)


@functools.lru_cache(maxsize=None)
def affine_case(trip=False):
    """C = 3, sub and mul differ per channel, x = 2 randn: values on both sides of both clamp ends."""
    g = torch.Generator().manual_seed(5 + trip)
    shape = TRIP_SHAPE3 + (3,) if trip else (2, 5, 7, 3)
    x = torch.randn(shape, generator=g) * 2
    sub, mul = torch.randn(3, generator=g), torch.rand(3, generator=g) + 0.5
    assert len(set(sub.tolist())) == 3 and len(set(mul.tolist())) == 3
    return x, sub, mul


def affine64(x, sub, mul):
    a, b, lo, hi = (f32(AFFINE[k]) for k in ("a", "b", "lo", "hi"))
    pre = x.double() * a + b
    ref = (pre.clamp(lo, hi) - sub.double()) * mul.double()
    return ref, N_AFFINE * U * ((x.double() * a).abs() + abs(b) + sub.double().abs()) * mul.double().abs(), pre


def affine_emul(x, sub, mul, fused=False):
    a, b, lo, hi = (f32(AFFINE[k]) for k in ("a", "b", "lo", "hi"))
    v = (fma32(x, a, b) if fused else x * t32(a) + t32(b)).clamp(lo, hi)
    return (v - sub) * mul


N_LOGVAR = 5    # ew.hip:428-430: v + 1 (the halving is exact), 1 - frac, two products, the sum


@functools.lru_cache(maxsize=None)
def learned_range_case(trip=False):
    """The model's variance channels [C, 2C) of N = 3 images; the range of timestep 25 of 50."""
    tab = tables()
    N, C, H, W = XSTART_TRIP if trip else (3, 3, 6, 10)
    lo, hi = f32(tab.posterior_log_variance_clipped[25]), f32(np.log(tab.betas[25]))
    return torch.randn(N, 2 * C, H, W, generator=torch.Generator().manual_seed(9 + trip)), C, lo, hi


def learned_range64(mo, C, lo, hi):
    """-> log variance, its bound, variance, its bound.  S of the log variance: |frac max| + |(1 - frac) min| and, for the
    error that frac's own rounding carries into 1 - frac, |frac min|.  The variance is expf of the f32 log variance
    (ew.hip:431): var64 (bound on logvar + C_EXP u)."""
    frac = (mo[:, C:].double() + 1) / 2
    lv = frac * hi + (1 - frac) * lo
    b_lv = N_LOGVAR * U * ((frac * hi).abs() + ((1 - frac) * lo).abs() + (frac * lo).abs())
    var = lv.exp()
    return lv, b_lv, var, var * (b_lv + C_EXP * U)


def learned_range_emul(mo, C, lo, hi, fused=False, fault=None):
    N, C2, H, W = mo.shape
    v = mo[:, :C] if fault == "first_channels" else (mo.reshape(-1)[C * H * W:][:N * C * H * W].view(N, C, H, W)
                                                    if fault == "image_stride" else mo[:, C:])
    frac = (v + 1.0) / 2.0
    lv = fma32(frac, hi, (1.0 - frac) * t32(lo)) if fused else frac * t32(hi) + (1.0 - frac) * t32(lo)
    return lv, torch.exp(lv)


# ================================================================================================ gated blend
PLANTED_GATES = {1: 20.0, 2: -20.0, 3: 90.0, 4: -90.0}      # channel -> logit
N_BLEND = 4     # ew.hip:202: 1 - s, two products, the sum


@functools.lru_cache(maxsize=None)
def blend_case(dtype, C, trip=False):
    """x, m (Fr, H, W, C) rounded to dtype, gate logits (Fr, C) = 3 randn; without trip the channels of PLANTED_GATES hold
    +-20 and +-90 in every frame."""
    g = torch.Generator().manual_seed(C + trip)
    shape = TRIP_SHAPE + (C,) if trip else (3, 5, 7, C)
    x, m = (rb(torch.randn(shape, generator=g), dtype) for _ in range(2))
    gate = torch.randn(shape[0], C, generator=g) * 3
    if not trip:
        for ch, v in PLANTED_GATES.items():
            gate[:, ch] = v
    return x, m, gate


def sigmoid_err(g64, c_exp_arg):
    """The error of 1 / (1 + e), e = exp(-g) carrying (C_EXP + c_exp_arg) u relative: of that 1 - s reaches s, the sum and
    the divide add one u each."""
    s = torch.sigmoid(g64)
    return s * ((1 - s) * (C_EXP + c_exp_arg) + 2) * U


def blend64(x, m, gate, dtype):
    """y = (1 - s) x + s m, s = 1 / (1 + __expf(-g)) (ew.hip:201-202) -> ref64, bound = N_BLEND u (|(1 - s) x| + |s m|) +
    err(s) |m - x| + out_rounding.  __expf(x) is exp2 of the f32 product x log2(e), worth |g| log2(e) u relative."""
    Fr, C = gate.shape
    g64 = gate.double().view(Fr, 1, 1, C)
    s = torch.sigmoid(g64)
    xd, md = x.double(), m.double()
    ref = (1 - s) * xd + s * md
    bound = N_BLEND * U * (((1 - s) * xd).abs() + (s * md).abs()) + sigmoid_err(g64, g64.abs() * LOG2E) * (md - xd).abs()
    return ref, bound + out_rounding(ref, dtype)


def blend_emul(x, m, gate, dtype, fused=False, fault=None):
    Fr, C = gate.shape
    s = (1.0 / (1.0 + torch.exp(-gate))).view(Fr, 1, 1, C)
    a, b = (1.0 - s, s) if fault != "swap_s" else (s, 1.0 - s)
    xf, mf = x.float(), m.float()
    return (fma32(a, xf, b * mf) if fused else a * xf + b * mf).to(dtype)


# ================================================================================================ timestep embedding
EMB_T = (0.0, 1.0, 37.0, 500.5, 999.0)
EMB_DIMS = (6, 33, 1280)
MAX_PERIOD = 10000.0


def embedding64(t, dim, sin_first):
    """From the definition: freq_k = P^(-k / half), out = [cos | sin](t freq) (or [sin | cos]), a zero in the last column of
    an odd dim -> ref64, bound = u (C_ARG |t freq| + C_OUT) (sin and cos have slope <= 1)."""
    half = dim // 2
    arg = t.double()[:, None] * MAX_PERIOD ** (-torch.arange(half, dtype=torch.float64) / half)[None]
    ref = torch.zeros(t.numel(), dim, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    c, s = (half, 0) if sin_first else (0, half)
    ref[:, c:c + half], ref[:, s:s + half] = torch.cos(arg), torch.sin(arg)
    bound[:, :2 * half] = U * (C_ARG * torch.cat([arg, arg], 1).abs() + C_OUT)
    return ref, bound


def embedding_emul(t, dim, sin_first, fault=None, fill=float("nan")):
    """oracle.unet.timestep_embedding (f32), reordered for sin_first.  fault: 'swap' (sin and cos exchanged), 'half_minus_1'
    (exponent k / (half - 1)), 'odd_unwritten' (the last column of an odd dim keeps the buffer's fill)."""
    from oracle.unet import timestep_embedding
    half = dim // 2
    if fault == "half_minus_1":
        freqs = torch.exp(-math.log(MAX_PERIOD) * torch.arange(half, dtype=FP) / max(half - 1, 1))
        args = t[:, None].float() * freqs[None]
        emb = torch.cat([torch.cos(args), torch.sin(args)], -1)
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], -1) if dim % 2 else emb
    else:
        emb = timestep_embedding(t, dim, MAX_PERIOD)
    if sin_first != (fault == "swap"):
        emb = torch.cat([emb[:, half:2 * half], emb[:, :half], emb[:, 2 * half:]], -1)
    if fault == "odd_unwritten" and dim % 2:
        emb[:, -1] = fill
    return emb


def embedding_deviation(t, dim):
    """The reference's f32 formulation against float64 -> (relative error of the argument, absolute error of cos / sin at
    the f32 argument), both in units of u."""
    from oracle.unet import timestep_embedding
    half = dim // 2
    arg64 = t.double()[:, None] * MAX_PERIOD ** (-torch.arange(half, dtype=torch.float64) / half)[None]
    arg32 = (t[:, None].float() * torch.exp(-math.log(MAX_PERIOD) * torch.arange(half, dtype=FP) / half)[None]).double()
    r_arg = torch.where(arg64 == 0, torch.zeros_like(arg64), (arg32 - arg64).abs() / arg64.abs().clamp_min(1e-300)).max().item() / U
    emb = timestep_embedding(t, dim, MAX_PERIOD).double()
    r_out = max((emb[:, :half] - torch.cos(arg32)).abs().max().item(), (emb[:, half:2 * half] - torch.sin(arg32)).abs().max().item()) / U
    return r_arg, r_out


# ================================================================================================ add_act with SiLU / GELU
K_ACT = {ACT_SILU: 6, ACT_GELU: 4}      # tests/test_gpu_act_exact.py: the divide SiLU and GELU of apply_act


@functools.lru_cache(maxsize=None)
def add_act_case(dtype, trip=False):
    """x0, x1 = 2 randn rounded to dtype; without trip channel 1 of x0 holds +128 and channel 2 -128 (x1 = 0 there): SiLU and
    GELU must return 128 and 0 exactly."""
    g = torch.Generator().manual_seed(3 + trip)
    shape = TRIP_SHAPE + (VEC[dtype],) if trip else (3, 7, 9, 40)
    x0, x1 = (rb(torch.randn(shape, generator=g) * 2, dtype) for _ in range(2))
    if not trip:
        x0[..., 1], x0[..., 2] = 128.0, -128.0
        x1[..., 1:3] = 0.0
    return x0, x1


def add_act64(x0, x1, act):
    """-> ref64, S = act_sens64(v), extra = Lipschitz u |v| for the f32 sum that feeds the activation (ew.hip:234)."""
    v = x0.double() + (x1.double() if x1 is not None else 0.0)
    extra = ACT_LIPSCHITZ[act] * U * v.abs() if x1 is not None else torch.zeros_like(v)
    return act64(v, act), act_sens64(v, act), extra


def add_act_emul(x0, x1, act, dtype):
    v = x0.float() + x1.float() if x1 is not None else x0.float()
    return (silu32(v) if act == ACT_SILU else t32(0.5) * v * (1.0 + torch.erf(v * t32(0.70710678118654752)))).to(dtype)


# ================================================================================================ sft_fuse / channel_gate
SFT_W = 0.7
N_SFT = 3       # prior.hip:249: fmaf(d, sc, sh), the product with w, the sum with d


@functools.lru_cache(maxsize=None)
def sft_case(dtype, nvec=15):
    g = torch.Generator().manual_seed(nvec)
    return tuple(rb(torch.randn(nvec * VEC[dtype], generator=g), dtype) for _ in range(3))


def sft64(dec, sc, sh, dtype):
    w = f32(SFT_W)
    d, s, h = dec.double(), sc.double(), sh.double()
    ref = d + w * (d * s + h)
    return ref, N_SFT * U * (d.abs() + abs(w) * ((d * s).abs() + h.abs())) + out_rounding(ref, dtype)


def sft_emul(dec, sc, sh, dtype, fused=False):
    d, t = dec.float(), fma32(dec.float(), sc.float(), sh.float())
    return (fma32(SFT_W, t, d) if fused else d + t32(SFT_W) * t).to(dtype)


GATE_USES = {"arm32": dict(logit=True, bias=True), "arm16": dict(logit=True, add=True), "ffm": dict(logit=True, add_x=True),
             "plain": dict(logit=False, bias=True, add=True, add_x=True)}       # tests/test_gpu_bisenet.py
GATE_SHAPE = (2, 9, 11, 40)
N_GATE = 4      # parse.hip:81-89: x g, + x, + bias, + add


@functools.lru_cache(maxsize=None)
def gate_case(dtype):
    T, H, W, C = GATE_SHAPE
    g = torch.Generator().manual_seed(C)
    x, a = (rb(torch.randn(T, H, W, C, generator=g), dtype) for _ in range(2))
    return x, a, torch.randn(T, C, generator=g) * 2, torch.randn(T, C, generator=g)


def gate64(x, a, gate, bias, kw, dtype):
    """-> ref64, bound = N_GATE u (|x g| + |x| + |bias| + |add|, the parts in use) + C_SIG u s |x| for the f32 sigmoid
    1 / (1 + expf(-v)) (parse.hip:73) + out_rounding."""
    T, C = gate.shape
    g64 = gate.double().view(T, 1, 1, C)
    gg = torch.sigmoid(g64) if kw["logit"] else g64
    xd = x.double()
    ref, S = xd * gg, (xd * gg).abs()
    if kw.get("add_x"):
        ref, S = ref + xd, S + xd.abs()
    if kw.get("bias"):
        ref, S = ref + bias.double().view(T, 1, 1, C), S + bias.double().abs().view(T, 1, 1, C)
    if kw.get("add"):
        ref, S = ref + a.double(), S + a.double().abs()
    bound = N_GATE * U * S + (C_SIG * U * gg * xd.abs() if kw["logit"] else 0.0)
    return ref, bound + out_rounding(ref, dtype)


def gate_emul(x, a, gate, bias, kw, dtype, fused=False):
    T, C = gate.shape
    gg = (torch.sigmoid(gate) if kw["logit"] else gate).view(T, 1, 1, C)
    xf = x.float()
    if kw.get("add_x"):
        r = fma32(xf, gg, xf) if fused else xf * gg + xf
    else:
        r = xf * gg
    if kw.get("bias"):
        r = r + bias.view(T, 1, 1, C)
    if kw.get("add"):
        r = r + a.float()
    return r.to(dtype)
