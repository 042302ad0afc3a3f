"""flair_groupnorm_nhwc (both code paths), flair_layernorm_nhwc and flair_adain_nhwc on inputs whose statistics are known.

The tolerance tests of this family (test_gpu_kernels.test_group_norm, test_gpu_strides, test_codeformer,
test_gpu_fullsize) bound max|err| by a multiple of max|ref| on randn data with SiLU only; a statistic that loses or
repeats one element, or mixes in a frame of its neighbour, stays below those bounds (tests/test_norm_exact_cpu.py keeps
the figures).  Here:
  1 balanced: every (statistic, group) holds as many +1 as -1 in a seeded random order and eps = 0, so mean = 0 and
    rstd = 1 in any summation order; gamma = +-2^k, beta = -+gamma and FiLM from {0, 1, -0.5, 3} / integers make every
    output a small integer, 0 on about half of the elements: assert_bits_equal in f32 and bf16, act NONE and RELU, with
    the resampled raw copy.  One element too few or too many at count <= 2^21 changes the f32 A and B and leaves about
    gamma / count where 0 belongs;
  2 spike: integers in [-3, 3] and one 64 per (statistic, group), eps = 1e-5, random gamma / beta / FiLM, all six
    activations.  Every sum is an integer below 2^24, so the statistics carry only their final roundings:
      |err| <= Lip(act) * 8 * 2^-24 * S  (+ half a bf16 ulp of ref for a bf16 output, + 4 * 2^-24 |ref| for an f32 SiLU /
      GELU; half an ulp is 2^-9 |ref| only at the top of a binade and 2^-8 |ref| at its bottom: util.out_rounding),
      S = ((|x| + |mean|) rstd |gamma| + |beta|) |1 + scale| + |shift|
    (rstd and mean cast to f32, the A / B fold with its FiLM step, one fma); a pooled y is held to the mean of its four
    bounds, with the output rounding taken once, on the pooled value.  The SiLU tail scales gamma until the normalised values span +-120: finite, within the bound + 2^-126;
  3 offsets: x = mu + z, z an integer in [-2, 2] (halves at bf16 mu = 64).  GroupNorm forms var = E[x^2] - mean^2 from f32
    sums; the sums of x are exact here (integers, or halves, below 2^24: asserted on the CPU), every fma of the sum of
    squares rounds the running sum by <= 2^-24 relative, so after a chain of K additions E[x^2] is off by <= K 2^-24
    relative, var by K 2^-24 E[x^2] absolute, rstd by half of that over var:
      |err| <= bound of 2 + 1/2 K 2^-24 (E[x^2] / var) |(x - mean) rstd gamma (1 + scale)|.
    K is the longest f32 chain of the path (gn_chain): three launches -- ceil(per / rows) fmas of a thread's own channel,
    rows additions of the row fold and C / groups of the channel fold in LDS, per = ceil(pixels / workgroups); one launch --
    ceil(pixels / (1024 / pp)) * VEC fmas into the thread's single accumulator; everything after that is f64.
    LayerNorm and AdaIN centre the data before squaring: (chain + 8) 2^-24 S with no such term, at every mu;
  4 LayerNorm on balanced rows at the widths around its 64-lane pieces (bf16 bit for bit, f32 within 2 ulp: rsqrtf is a
    1-ulp instruction), with the positional output; AdaIN with style = content, with a constant content (every pixel is
    the style mean, correctly rounded) and on integers against float64.
Shapes are the smallest that reach each path; test_cases_reach_every_groupnorm_path recomputes the host's selection rule
(gn_path) and checks the table.  Largest err / bound per path go to parity_log (profiles/norm_parity.txt is the record)."""
import collections
import functools

import pytest
import torch

from tests.util import (ACT_GELU, ACT_LIPSCHITZ, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, U24, act64,
                        adain_ref64, assert_bits_equal, assert_elem_close, assert_within_ulps, balanced_signs, exact_film,
                        gn_ref64, int_tensor, layernorm_ref64, out_rounding, parity_log, pool2, pow2_affine, resample_ref, spiked_ints)

pytestmark = pytest.mark.gpu
FP, BF = torch.float32, torch.bfloat16
BOTH = (FP, BF)
VEC = {FP: 4, BF: 8}
ESZ = {FP: 4, BF: 2}
NAME = {FP: "f32", BF: "bf16"}
ACTS = (ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU01, ACT_LRELU02, ACT_GELU)
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_RELU: "relu", ACT_LRELU01: "lrelu01", ACT_LRELU02: "lrelu02",
            ACT_GELU: "gelu"}
MAX_COUNT = 1 << 21


def _ops():
    from flair_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ case table
# fps: frames per statistic (None = all T); film: None, "aligned" (rows of 2C + 8 floats) or "unaligned" (2C + 5).
class Gn(collections.namedtuple("Gn", "T H W c0 c1 fps groups resample film dtypes")):
    @property
    def C(self):
        return self.c0 + self.c1

    @property
    def frames(self):
        return self.fps or self.T

    def __str__(self):
        return (f"{self.T}x{self.H}x{self.W}x{self.c0}+{self.c1}-fps{self.frames}-g{self.groups}-r{self.resample}"
                + (f"-{self.film}" if self.film else ""))


def G(T, H, W, c0, c1=0, fps=None, groups=32, resample=0, film=None, dtypes=BOTH):
    return Gn(T, H, W, c0, c1, fps, groups, resample, film, dtypes)


EXACT = [
    # ---- three launches
    G(2, 7, 9, 96),                                   # cpg = 3: a 16-byte piece straddles groups
    G(3, 5, 6, 64, 32, fps=1, film="unaligned"),      # two segments, per-frame statistics, 30 pixels
    G(4, 6, 10, 768, fps=2, film="aligned"),          # cpg / vec = 3 or 6: does not divide 1024
    G(3, 4, 4, 1024, 1024, resample=2),               # 2048 channels: one pixel row per workgroup in f32; raw
    G(2, 8, 8, 128, resample=1, film="aligned"),      # pooling with the raw output
    G(2, 224, 224, 64),                               # 196 / 392 workgroups per statistic: finalize's unrolled loop, ragged
    G(4, 256, 256, 64),                               # the cap of 512 workgroups per statistic
    G(1, 8, 8, 64, fps=1, groups=1), G(1, 8, 8, 64, fps=1, groups=2), G(1, 8, 8, 64, fps=1, groups=8),
    G(8, 32, 33, 256, dtypes=(BF,)),                  # one pixel row past the LDS limit of the one-launch kernel
    # ---- one launch, a workgroup per (statistic, group)
    G(8, 32, 32, 256, dtypes=(BF,)), G(4, 32, 32, 256, dtypes=(FP,)),        # exactly 128 KiB per group
    G(4, 1, 1, 256, fps=1),                           # one pixel per statistic
    # 4 rows - 1, 4 rows, 4 rows + 1 pixels (rows = 1024 in bf16): the U = 4 tail and both tails of the pairwise apply loop
    G(1, 63, 65, 256, dtypes=(BF,)), G(1, 64, 64, 256, dtypes=(BF,)), G(1, 17, 241, 256, dtypes=(BF,)),
    G(1, 23, 89, 256, dtypes=(FP,)), G(1, 3, 683, 256, dtypes=(FP,)),        # the same with rows = 512 in f32
    G(16, 4, 4, 1024, fps=4, film="aligned"),         # pp = 4 / 8, 1 < frames_per_stat < T
    G(3, 4, 4, 1024, 1024, film="unaligned"),         # pp = 8 / 16, two segments
    G(5, 3, 5, 256, 256, fps=1),                      # the second segment, 15 pixels
    G(2, 8, 8, 256, film="aligned"), G(2, 8, 8, 256, film="unaligned"),      # filmVec on and off, two frames
    G(2, 8, 8, 128, fps=1),                           # cpg = 4: pp = 1 in f32 (three launches in bf16)
]
SPIKE = [EXACT[1], EXACT[2], EXACT[4], EXACT[19], EXACT[21]]
TAIL = [EXACT[1], EXACT[21]]
OFFSET = [G(2, 24, 24, 64, film="aligned"), G(8, 32, 32, 256, dtypes=(BF,)), G(4, 32, 32, 256, dtypes=(FP,))]
MUS = {BF: (0, 16, 64), FP: (0, 16, 64, 256, 1024)}


def _pairs(cases):
    return [pytest.param(c, dt, id=f"{c}-{NAME[dt]}") for c in cases for dt in c.dtypes]


def gn_path(c, dtype, with_raw=None):
    """The selection rule of flair_groupnorm_nhwc and its launch geometry -> dict(kernel, rows, wgs, pp)."""
    vec, C = VEC[dtype], c.C
    cpg = C // c.groups
    pix = c.frames * c.H * c.W
    nstat = c.T // c.frames
    raw = bool(c.resample) if with_raw is None else with_raw
    assert C % vec == 0 and c.c0 % vec == 0 and C // vec <= 512
    if (c.resample == 0 and not raw and cpg % vec == 0 and 1024 % (cpg // vec) == 0 and c.c0 % cpg == 0
            and pix * cpg * ESZ[dtype] <= 128 << 10 and nstat * c.groups >= 16):
        pp = cpg // vec
        return dict(kernel="group", rows=1024 // pp, wgs=1, pp=pp)
    cv = C // vec
    rows = 256 // cv if cv <= 256 else 1
    return dict(kernel="three", rows=rows, wgs=max(1, min(512, -(-pix // (rows * 16)))), pp=0)


def gn_chain(c, dtype):
    """K: the number of f32 additions on the longest way of one x^2 into a partial sum (module docstring, 3)."""
    p = gn_path(c, dtype)
    pix = c.frames * c.H * c.W
    if p["kernel"] == "group":
        return -(-pix // p["rows"]) * VEC[dtype]
    per = -(-pix // p["wgs"])
    return -(-per // p["rows"]) + p["rows"] + c.C // c.groups


def test_cases_reach_every_groupnorm_path():
    seen = collections.defaultdict(set)
    for c in EXACT:
        for dt in c.dtypes:
            p = gn_path(c, dt)
            k = p["kernel"]
            seen[k, "any"].add(dt)
            seen[k, "frames", "one" if c.frames == 1 else ("two" if c.frames == 2 else "many")].add(dt)
            if c.film:
                seen[k, "film", c.film].add(dt)
            if c.c1:
                seen[k, "two segments"].add(dt)
            if 1 < c.frames < c.T:
                seen[k, "1 < fps < T"].add(dt)
            if k == "three":
                seen["resample", c.resample].add(dt)
                w = p["wgs"]
                seen["wgs", "<= 64" if w <= 64 else ("193..511" if 193 <= w <= 511 else ("512" if w == 512 else "other"))].add(dt)
                if p["rows"] == 1:
                    seen["one pixel row"].add(dt)
            else:
                seen["pp", min(p["pp"], 8)].add(dt)
                pix = c.frames * c.H * c.W
                r = pix % (4 * p["rows"])
                if pix > 4 * p["rows"] - 2:
                    seen["U tail", "before" if r == 4 * p["rows"] - 1 else ("at" if r == 0 else ("after" if r == 1 else "other"))].add(dt)
                if pix * (c.C // c.groups) * ESZ[dt] == 128 << 10:
                    seen["128 KiB"].add(dt)
    need = [("group", "any"), ("three", "any"), ("wgs", "<= 64"), ("wgs", "193..511"), ("wgs", "512"), ("resample", 0),
            ("resample", 1), ("resample", 2), "one pixel row", "128 KiB", ("U tail", "before"), ("U tail", "at"),
            ("U tail", "after"), ("pp", 1), ("pp", 2), ("pp", 4), ("pp", 8), ("group", "two segments"),
            ("three", "two segments"), ("group", "1 < fps < T"), ("three", "1 < fps < T")]
    need += [(k, "film", f) for k in ("group", "three") for f in ("aligned", "unaligned")]
    need += [(k, "frames", n) for k in ("group", "three") for n in ("one", "two", "many")]
    missing = [(n, sorted(NAME[d] for d in set(BOTH) - seen[n])) for n in need if seen[n] != set(BOTH)]
    assert not missing, missing
    # the bf16 case one pixel row past 128 KiB falls back to three launches; the part-2 and part-3 subsets hold both paths
    assert gn_path(EXACT[10], BF)["kernel"] == "three" and gn_path(EXACT[11], BF)["kernel"] == "group"
    for cases in (SPIKE, OFFSET, TAIL):
        for dt in BOTH:
            assert {gn_path(c, dt)["kernel"] for c in cases if dt in c.dtypes} == {"group", "three"}
    assert any(c.c1 for c in SPIKE) and any(1 < c.frames < c.T for c in SPIKE)


# ------------------------------------------------------------------------------------------------ builders
def _film(c, g):
    return exact_film(c.T, c.C, 2 * c.C + (8 if c.film == "aligned" else 5), g) if c.film else None


def _seed(c):
    return 1000 + 7 * c.T + 13 * c.H + 17 * c.W + c.C + 3 * c.frames + c.groups + c.resample


@functools.lru_cache(maxsize=1)
def balanced_case(c):
    """-> x, gamma, beta, film, pre: the exact output before the activation and the resampling (float64)."""
    g = torch.Generator().manual_seed(_seed(c))
    x = balanced_signs(c.T, c.H, c.W, c.C, c.frames, c.groups, g)
    gamma, beta = pow2_affine(c.C, g)
    film = _film(c, g)
    pre = x.double() * gamma.double() + beta.double()
    if film is not None:
        pre = pre * (1.0 + film[:, None, None, :c.C].double()) + film[:, None, None, c.C:2 * c.C].double()
    return x, gamma, beta, film, pre


@functools.lru_cache(maxsize=2)
def spike_case(c, tail=False):
    """-> x, gamma, beta, film.  tail: beta = 0, no FiLM and gamma = +-120 / (the largest normalised value of the
    channel's group over all statistics)."""
    g = torch.Generator().manual_seed(_seed(c) + 1)
    x, _ = spiked_ints(c.T, c.H, c.W, c.C, c.frames, c.groups, g)
    if not tail:
        film = None
        if c.film:
            film = _film(c, g)
            film[:, :2 * c.C] = torch.randn(c.T, 2 * c.C, generator=g) * 0.5
        return x, torch.randn(c.C, generator=g), torch.randn(c.C, generator=g), film
    one = gn_ref64(x, torch.ones(c.C), torch.zeros(c.C), c.frames, c.groups, 1e-5)["pre"]
    top = one.abs().amax((0, 1, 2)).view(c.groups, -1).amax(1, keepdim=True).expand(c.groups, c.C // c.groups).reshape(c.C)
    sign = torch.randint(0, 2, (c.C,), generator=g).double() * 2 - 1
    return x, (sign * 120.0 / top).float(), torch.zeros(c.C), None


def offset_input(shape, mu, dtype, g):
    """mu + z, z an integer in [-2, 2], in halves at bf16 mu = 64: every value is exact in `dtype`."""
    z = int_tensor(shape, -2, 2, g) * (0.5 if dtype == BF and mu >= 64 else 1.0)
    x = mu + z
    assert torch.equal(x.to(dtype).float(), x)
    return x


@functools.lru_cache(maxsize=2)
def offset_case(c, mu, dtype):
    g = torch.Generator().manual_seed(_seed(c) + 2 + mu)
    x = offset_input((c.T, c.H, c.W, c.C), mu, dtype, g)
    film = None
    if c.film:
        film = _film(c, g)
        film[:, :2 * c.C] = torch.randn(c.T, 2 * c.C, generator=g) * 0.5
    return x, torch.randn(c.C, generator=g), torch.randn(c.C, generator=g), film


def run_gn(dev, c, dtype, x, gamma, beta, film, act, eps):
    ops = _ops()
    xa = x[..., :c.c0].to(device=dev, dtype=dtype).contiguous()
    xb = x[..., c.c0:].to(device=dev, dtype=dtype).contiguous() if c.c1 else None
    res = ops.group_norm(xa, gamma.to(dev), beta.to(dev), x1=xb, groups=c.groups, eps=eps, act=act,
                         film=film.to(dev) if film is not None else None, frames_per_stat=c.frames,
                         resample=c.resample, want_raw=bool(c.resample))
    torch.cuda.synchronize()
    y, raw = res if c.resample else (res, None)
    return y.cpu(), (raw.cpu() if raw is not None else None)


def gn_bound(ref, r, act, dtype, K=0, out=True):
    """The per-element bound of parts 2 and 3 on the activated output `ref` (before the resampling); out = False leaves
    out the rounding to the output type."""
    b = 8 * U24 * r["S"]
    if K:
        b = b + 0.5 * K * U24 * (r["ex2"] / r["var"]) * r["slope"].abs()
    b = ACT_LIPSCHITZ[act] * b
    if dtype == FP and act in (ACT_SILU, ACT_GELU):
        b = b + 4 * U24 * ref.abs()
    return b + out_rounding(ref, dtype) if out else b


# ------------------------------------------------------------------------------------------------ 1 balanced
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("c,dtype", _pairs(EXACT))
def test_groupnorm_balanced_bits(dev, c, dtype, act):
    x, gamma, beta, film, pre = balanced_case(c)
    y, raw = run_gn(dev, c, dtype, x, gamma, beta, film, act, 0.0)
    want = resample_ref(act64(pre, act), c.resample)
    assert_bits_equal(y, want.to(dtype), f"gn balanced {c} {NAME[dtype]} act {ACT_NAME[act]} ({gn_path(c, dtype)})")
    if c.resample:
        assert_bits_equal(raw, resample_ref(x.double(), c.resample).to(dtype), f"gn balanced raw {c} {NAME[dtype]}")


# ------------------------------------------------------------------------------------------------ 2 spike
@pytest.mark.parametrize("act", ACTS, ids=[ACT_NAME[a] for a in ACTS])
@pytest.mark.parametrize("c,dtype", _pairs(SPIKE))
def test_groupnorm_spike(dev, c, dtype, act):
    x, gamma, beta, film = spike_case(c)
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 1e-5, film)
    ref = act64(r["pre"], act)
    bound = gn_bound(ref, r, act, dtype)
    y, raw = run_gn(dev, c, dtype, x, gamma, beta, film, act, 1e-5)
    if c.resample == 1:     # the four activated values are averaged in f32 and rounded once
        ref, bound = pool2(ref), pool2(gn_bound(ref, r, act, dtype, out=False))
        bound = bound + out_rounding(ref, dtype)
        assert_bits_equal(raw, pool2(x.double()).to(dtype), f"gn spike raw {c}")
    ratio = assert_elem_close(y, ref, bound, 1.0, f"gn spike {c} {NAME[dtype]} act {ACT_NAME[act]}")
    parity_log(f"norm spike      {gn_path(c, dtype)['kernel']:5s} {NAME[dtype]:4s} {ACT_NAME[act]:7s} {str(c):44s} "
               f"err/bound {ratio:.3f}")


@pytest.mark.parametrize("c,dtype", _pairs(TAIL))
def test_groupnorm_silu_tail(dev, c, dtype):
    x, gamma, beta, film = spike_case(c, True)
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 1e-5)
    pre = r["pre"]
    assert 119.9 <= pre.max().item() <= 120.1 and -120.1 <= pre.min().item() <= -119.9
    ref = act64(pre, ACT_SILU)
    y, _ = run_gn(dev, c, dtype, x, gamma, beta, None, ACT_SILU, 1e-5)
    assert bool(torch.isfinite(y).all()), f"{int((~torch.isfinite(y)).sum())} non-finite outputs"
    ratio = assert_elem_close(y, ref, gn_bound(ref, r, ACT_SILU, dtype), 1.0, f"gn silu tail {c} {NAME[dtype]}", ab=2.0 ** -126)
    gone = pre < -110.0                                  # |silu| < 2^-149: nothing in f32 or bf16
    assert bool(gone.any()) and bool((y[gone] == 0).all())
    parity_log(f"norm silu tail  {gn_path(c, dtype)['kernel']:5s} {NAME[dtype]:4s} {str(c):44s} err/bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------ 3 offsets
def _offset_params(cases):
    return [pytest.param(c, dt, mu, id=f"{c}-{NAME[dt]}-mu{mu}") for c in cases for dt in c.dtypes for mu in MUS[dt]]


@pytest.mark.parametrize("c,dtype,mu", _offset_params(OFFSET))
def test_groupnorm_offset(dev, c, dtype, mu):
    x, gamma, beta, film = offset_case(c, mu, dtype)
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 1e-5, film)
    K = gn_chain(c, dtype)
    y, _ = run_gn(dev, c, dtype, x, gamma, beta, film, ACT_NONE, 1e-5)
    kappa = (r["ex2"] / r["var"]).max().item()
    ratio = assert_elem_close(y, r["pre"], gn_bound(r["pre"], r, ACT_NONE, dtype, K=K), 1.0,
                              f"gn offset {c} {NAME[dtype]} mu {mu} (K = {K}, E[x^2] / var = {kappa:.3g})")
    plain = ((y.double() - r["pre"]).abs() / gn_bound(r["pre"], r, ACT_NONE, dtype)).max().item()
    parity_log(f"norm offset     {gn_path(c, dtype)['kernel']:5s} {NAME[dtype]:4s} mu {mu:4d} K {K:3d} E[x^2]/var {kappa:9.3g} "
               f"err/bound {ratio:.4f} (err / the bound without the variance term {plain:.3f})")


@functools.lru_cache(maxsize=2)
def _ln_ad_case(mu, dtype):
    """The input of the one-launch GroupNorm case of this dtype and offset, a style tensor of the same family, gamma, beta."""
    c = next(c for c in OFFSET[1:] if dtype in c.dtypes)
    x = offset_case(c, mu, dtype)[0]
    g = torch.Generator().manual_seed(77 + mu)
    return x, offset_input(x.shape, mu, dtype, g), torch.randn(c.C, generator=g), torch.randn(c.C, generator=g)


def adain_chain(HW):
    """A pixel lane adds ceil(HW / 4) values, then the four lanes are added."""
    return -(-HW // 4) + 4


@pytest.mark.parametrize("dtype,mu", [pytest.param(dt, mu, id=f"{NAME[dt]}-mu{mu}") for dt in BOTH for mu in MUS[dt]])
def test_layernorm_adain_offset(dev, dtype, mu):
    """Two passes, centred squares: the bound has no E[x^2] / var term and holds unchanged at every offset."""
    ops = _ops()
    x, style, gamma, beta = _ln_ad_case(mu, dtype)
    ref, S = layernorm_ref64(x, gamma, beta, 1e-5)
    y = ops.layer_norm(x.to(dev, dtype), gamma.to(dev), beta.to(dev), eps=1e-5)
    C = x.shape[3]
    r1 = assert_elem_close(y.cpu(), ref, (C + 8) * U24 * S + out_rounding(ref, dtype), 1.0, f"layer_norm {NAME[dtype]} mu {mu}")
    ref, S = adain_ref64(x, style, 1e-5)
    y = ops.adain(x.to(dev, dtype), style.to(dev, dtype), eps=1e-5)
    hw = x.shape[1] * x.shape[2]
    r2 = assert_elem_close(y.cpu(), ref, (adain_chain(hw) + 8) * U24 * S + out_rounding(ref, dtype), 1.0, f"adain {NAME[dtype]} mu {mu}")
    parity_log(f"norm offset     layernorm {NAME[dtype]:4s} mu {mu:4d} err/bound {r1:.4f}   adain err/bound {r2:.4f}")


# ------------------------------------------------------------------------------------------------ 4 LayerNorm, AdaIN
LN_SHAPES = ((3, 1, 3), (2, 2, 3))          # rows % 4 = 1 and 0; the positional table has H * W < rows rows


def ln_widths(dtype):
    v = VEC[dtype]
    return (v, 63 * v, 64 * v, 65 * v, 256 * v)


def layernorm_balanced_case(dtype, k, shape):
    C = ln_widths(dtype)[k]
    g = torch.Generator().manual_seed(300 + C + shape[0])
    F_, H, W = shape
    x = balanced_signs(F_ * H * W, 1, 1, C, 1, 1, g).view(F_, H, W, C)
    gamma, beta = pow2_affine(C, g)
    return x, gamma, beta, int_tensor((H * W, C), -8, 8, g)


@pytest.mark.parametrize("with_pos", [False, True], ids=["", "pos"])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", range(5), ids=["vec", "63vec", "64vec", "65vec", "256vec"])
@pytest.mark.parametrize("dtype", BOTH, ids=lambda d: NAME[d])
def test_layernorm_balanced(dev, dtype, k, shape, with_pos):
    ops = _ops()
    x, gamma, beta, pos = layernorm_balanced_case(dtype, k, shape)
    want = x.double() * gamma.double() + beta.double()
    res = ops.layer_norm(x.to(dev, dtype), gamma.to(dev), beta.to(dev), eps=0.0, pos=pos.to(dev) if with_pos else None)
    torch.cuda.synchronize()
    y, y2 = res if with_pos else (res, None)
    what = f"layer_norm balanced C = {x.shape[3]} {shape} {NAME[dtype]}"
    wpos = want + pos.double().view(1, shape[1], shape[2], -1)
    if dtype == BF:
        assert_bits_equal(y.cpu(), want.to(BF), what)
        if with_pos:
            assert_bits_equal(y2.cpu(), wpos.to(BF), what + " + pos")
    else:
        assert_within_ulps(y, want, 2, what)
        if with_pos:
            assert_within_ulps(y2, wpos, 2, what + " + pos")
    if with_pos:        # the wrap of the positional table: row r of any frame gets pos[r % (H * W)]
        assert_bits_equal((y2.cpu().double() - y.cpu().double()).float(), pos.view(1, shape[1], shape[2], -1).expand_as(x).contiguous(),
                          what + ": y2 - y")


ADAIN_SHAPES = [(hw, C) for hw in ((1, 2), (1, 5), (16, 16)) for C in (8, 64, 72)]


def _adain_id(s):
    return f"hw{s[0][0] * s[0][1]}-c{s[1]}"


def adain_ints(hw, C, g):
    return int_tensor((2, hw[0], hw[1], C), -8, 8, g), int_tensor((2, hw[0], hw[1], C), -8, 8, g)


@pytest.mark.parametrize("shape", ADAIN_SHAPES, ids=_adain_id)
@pytest.mark.parametrize("dtype", BOTH, ids=lambda d: NAME[d])
def test_adain_exact(dev, dtype, shape):
    ops = _ops()
    hw, C = shape
    g = torch.Generator().manual_seed(500 + hw[1] + C)
    content, style = adain_ints(hw, C, g)
    run = lambda a, b: ops.adain(a.to(dev, dtype), b.to(dev, dtype), eps=1e-5).cpu()
    # style = content: the statistics cancel
    mean = content.double().mean((1, 2), keepdim=True)
    y = run(content, content)
    assert_elem_close(y, content.double(), 4 * U24 * (content.double().abs() + mean.abs()) + out_rounding(content.double(), dtype), 1.0,
                      f"adain style = content {shape} {NAME[dtype]}")
    # constant content: every pixel is the style mean (an integer sum over HW, rounded once to f32, then to the output type)
    const = content[:, :1, :1, :].expand_as(content).contiguous()
    want = (style.double().sum((1, 2), keepdim=True) / (hw[0] * hw[1])).float().to(dtype).expand_as(content).contiguous()
    assert_bits_equal(run(const, style), want, f"adain constant content {shape} {NAME[dtype]}")
    # integers against float64 (unbiased variance)
    ref, S = adain_ref64(content, style, 1e-5)
    ratio = assert_elem_close(run(content, style), ref, (adain_chain(hw[0] * hw[1]) + 8) * U24 * S + out_rounding(ref, dtype), 1.0,
                              f"adain integers {shape} {NAME[dtype]}")
    parity_log(f"norm adain ints {NAME[dtype]:4s} {_adain_id(shape):12s} err/bound {ratio:.3f}")
