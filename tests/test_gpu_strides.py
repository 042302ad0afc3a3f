"""Kernel entries on strided channel views with guarded neighbours.

The models read and write channel slices and frame slices of shared buffers (codeformer.py's qkv halves, SPyNet's
b[..., 4:8] / b[..., 8:12], the recurrence's dest[idx:idx + 1]).  Every case here runs one entry twice: once on dense
tensors, once on views [1:T + 1, :, :, coff:coff + C] of wider guarded buffers (tests/util.py:guarded; NaN around the
inputs, a finite sentinel around the outputs), and checks
  a. the output against a float64 CPU reference computed from the same dtype-rounded inputs (per-kernel tolerances as in
     the kernel's own test),
  b. the strided output bitwise equal to the dense one (the kernels are deterministic: a stride must not change the
     arithmetic),
  c. every byte of every output buffer outside its view unchanged (pad channels, the frames before and after, the rows
     under a tile that hangs over the image),
  d. every input buffer unchanged.
The NaN frame before each input also checks the temporal clip edge: a 3x3x3 tap that read frame -1 instead of padding it
with zeros would turn its output into NaN."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import IN_FILL, OUT_FILL, TOL, assert_untouched, bits, guarded, rb

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float32
DTYPES = [FP, BF]
ACTS = {0: lambda v: v, 1: torch.relu, 2: lambda v: F.leaky_relu(v, 0.1), 3: F.silu}


def _ops():
    from flair_amd import ops
    return ops


def _g(dtype):
    """Elements per 16 bytes."""
    return 16 // torch.tensor([], dtype=dtype).element_size()


def run_both(dev, ins, outs, call, what):
    """ins: {name: (cpu (T,H,W,C) tensor, dtype, coff, ld)}; outs: {name: ((T,H,W,C), dtype, coff, ld[, cpu init])}.
    call(**views) issues the launch.  Runs dense, then on guarded views; checks b, c, d; -> dense outputs (f64, cpu)."""
    dense = {k: d.to(dev, dt).contiguous() for k, (d, dt, *_) in ins.items()}
    dout = {}
    for k, (s, dt, _, _, *init) in outs.items():
        dout[k] = init[0].to(dev, dt).contiguous() if init else torch.full(s, OUT_FILL, dtype=dt, device=dev)
    call(**dense, **dout)
    gin, gout = {}, {}
    for k, (d, dt, coff, ld) in ins.items():
        buf, v = guarded(*d.shape, dt, dev, coff=coff, ld=ld, fill=IN_FILL)
        v.copy_(d.to(dev, dt))
        gin[k] = (buf, v, buf.clone())
    for k, (s, dt, coff, ld, *init) in outs.items():
        buf, v = guarded(*s, dt, dev, coff=coff, ld=ld, fill=OUT_FILL)
        if init:
            v.copy_(init[0].to(dev, dt))
        gout[k] = (buf, v, buf.clone())
    call(**{k: t[1] for k, t in gin.items()}, **{k: t[1] for k, t in gout.items()})
    torch.cuda.synchronize()
    for k, (buf, v, before) in gout.items():
        ne = bits(v) != bits(dout[k])
        assert not ne.any(), f"{what}: output {k} differs from the dense call at {int(ne.sum())} element(s), " \
                             f"first {ne.nonzero()[0].tolist()}"
        assert_untouched(buf, before, v, f"{what}: output {k}")
    for k, (buf, v, before) in gin.items():
        assert_untouched(buf, before, None, f"{what}: input {k}")
    return {k: t.double().cpu() for k, t in dout.items()}


def close(got, ref, dtype, what, scale=1.0):
    rel, ab = TOL[dtype]
    err = (got - ref).abs().max().item()
    bound = scale * rel * ref.abs().max().item() + ab
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e}"


def nchw(t):
    return t.permute(0, 3, 1, 2)


def clip(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ conv
# T, H, W, segs, cout, kernel, act, nres, extra; expected bf16 / f32 variant (flair_conv_variant)
CONV_CASES = [
    ((1, 256, 256, [32, 32], 72, (1, 1, 1), 1, 2, {}), 0, 0),
    ((1, 256, 256, [32, 32], 64, (1, 1, 1), 3, 1, {}), 1, 1),
    ((2, 16, 16, [32, 32], 64, (1, 3, 3), 2, 2, {}), 2, 2),
    ((4, 136, 128, [32, 32], 8, (1, 3, 3), 0, 1, {}), 3, 3),
    ((2, 136, 128, [32, 32], 8, (1, 3, 3), 2, 2, {}), 4, 4),
    ((3, 30, 32, [32, 32, 32], 64, (3, 3, 3), 1, 2, {}), 5, 5),
    ((1, 250, 256, [32, 32], 8, (1, 3, 3), 3, 1, {}), 6, 6),       # last row of tiles hangs over the image
    ((1, 125, 128, [32, 32], 72, (1, 3, 3), 2, 2, {}), 7, 7),
    ((2, 256, 256, [32, 32], 8, (1, 3, 3), 1, 2, {}), 8, 3),
    ((1, 256, 256, [32, 32], 24, (1, 3, 3), 0, 1, {}), 9, 6),
    # stride 2, F.pad(0, 1, 0, 1) + stride 2, reflection padding, per-frame bias rows wider than Cout
    ((2, 32, 64, [32, 32], 64, (1, 3, 3), 2, 1, {"stride": 2}), 2, 2),
    ((2, 32, 32, [32, 32], 64, (1, 3, 3), 0, 1, {"stride": 2, "asym_pad": True}), 2, 2),
    ((2, 20, 24, [32, 32], 64, (1, 3, 3), 1, 1, {"reflect_pad": True}), 2, 2),
    ((2, 16, 16, [32, 32], 64, (1, 3, 3), 3, 1, {"frame_bias": 12}), 2, 2),
    ((1, 256, 256, [32, 32], 24, (1, 3, 3), 1, 1, {"frame_bias": 4}), 9, 6),
    # bf16 Cout = 4 (mod 8): 8-byte quads (dense y_ld = Cout is 8-byte granular; the strided y_ld is too)
    ((1, 256, 256, [32], 68, (1, 1, 1), 0, 1, {}), 0, 0),
    ((1, 256, 256, [32], 36, (1, 1, 1), 2, 2, {}), 1, 1),
    ((2, 16, 16, [32], 36, (1, 3, 3), 1, 2, {}), 2, 2),
    ((1, 256, 256, [32], 36, (1, 3, 3), 3, 1, {}), 3, 3),
    ((1, 256, 128, [32], 36, (1, 3, 3), 0, 2, {}), 4, 4),
    ((2, 16, 32, [32], 36, (1, 3, 3), 2, 1, {}), 5, 5),
]


def _conv_layout(dtype, segs, cout):
    """Strided placement: each segment, residual and y at its own offset and stride (16-byte granular), except that
    Cout % 8 == 4 outputs / residuals take an 8-byte granular stride."""
    g = _g(dtype)
    seg = [((i + 1) * g, (i + 1) * g + c + 2 * g) for i, c in enumerate(segs)]
    if cout % 8:
        return seg, [(g // 2, cout + g), (g, cout + 2 * g)], (g, cout + 2 * g)     # strides = 4 (mod 8) elements
    return seg, [(g, cout + 3 * g), (2 * g, cout + 2 * g + g)], (g, cout + 2 * g)


def test_conv_cases_cover_every_variant_on_strided_views():
    """Every variant 0-9 of flair_conv_variant runs strided in bf16; f32 reaches 0-7."""
    ops = _ops()
    for dtype, col in ((BF, 1), (FP, 2)):
        seen = set()
        for case in CONV_CASES:
            T, H, W, segs, cout, k, _, _, ex = case[0]
            v = ops.conv_variant(T, H, W, segs, cout, k, dtype=dtype, stride=ex.get("stride", 1))
            assert v == case[col], (case, dtype, v)
            seen.add(v)
        assert seen == set(range(10) if dtype == BF else range(8)), seen


@pytest.mark.parametrize("dtype,case", [(dt, c[0]) for dt in DTYPES for c in CONV_CASES if dt == BF or c[0][4] % 8 == 0],
                         ids=lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else
                         f"{v[:6]}{sorted(v[8])}".replace(" ", ""))
def test_conv_strided(dev, dtype, case):
    """(Cout = 4 (mod 8) cases are bf16 only: f32 stores 16-byte quads.)"""
    ops = _ops()
    T, H, W, segs, cout, k, act, nres, ex = case
    stride = ex.get("stride", 1)
    g = torch.Generator().manual_seed(T * 1000 + H * 10 + cout + len(ex))
    cin = sum(segs)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    x = rb(torch.randn(T, cin, H, W, generator=g), dtype)
    w = rb(torch.randn(cout, cin, *k, generator=g) / math.sqrt(cin * k[0] * k[1] * k[2]), dtype)
    b = torch.randn(cout, generator=g) * 0.1
    res = [rb(torch.randn(T, cout, Ho, Wo, generator=g), dtype) for _ in range(nres)]
    fb = torch.randn(T, cout + ex["frame_bias"], generator=g) if "frame_bias" in ex else None
    # float64 reference
    xd, wd = x.double(), w.double()
    if ex.get("reflect_pad"):
        ref = F.conv2d(F.pad(xd, (1, 1, 1, 1), mode="reflect"), wd[:, :, 0], b.double())
    elif ex.get("asym_pad"):
        ref = F.conv2d(F.pad(xd, (0, 1, 0, 1)), wd[:, :, 0], b.double(), stride=2)
    elif k[0] == 1:
        ref = F.conv2d(xd, wd[:, :, 0], b.double(), padding=(k[1] // 2, k[2] // 2), stride=stride)
    else:
        ref = F.conv3d(xd.permute(1, 0, 2, 3)[None], wd, b.double(), padding=tuple(v // 2 for v in k))[0].permute(1, 0, 2, 3)
    if fb is not None:
        ref = ref + fb[:, :cout, None, None].double()
    ref = ACTS[act](ref)
    for r in res:
        ref = ref + r.double()
    ref = ref * 0.5
    seg_l, res_l, y_l = _conv_layout(dtype, segs, cout)
    ins, o = {}, 0
    for i, c in enumerate(segs):
        ins[f"x{i}"] = (clip(x[:, o:o + c]), dtype, *seg_l[i])
        o += c
    for i, r in enumerate(res):
        ins[f"r{i}"] = (clip(r), dtype, *res_l[i])
    outs = {"y": ((T, Ho, Wo, cout), dtype, *y_l)}
    wp = ops.pack_conv_weight(w, [(c, c) for c in segs], dtype).to(dev)
    bd = b.to(dev)
    fbd = fb.to(dev)[:, :] if fb is not None else None

    def call(y, **t):
        ops.conv([t[f"x{i}"] for i in range(len(segs))], wp, bd, cout, k, act=act, out=y, res0=t.get("r0"),
                 res1=t.get("r1"), out_scale=0.5, stride=stride, frame_bias=fbd, asym_pad=ex.get("asym_pad", False),
                 reflect_pad=ex.get("reflect_pad", False))
    got = run_both(dev, ins, outs, call, f"conv {case} {dtype}")["y"]
    close(nchw(got), ref, dtype, f"conv {case}")


# ------------------------------------------------------------------------------------------------ conv chain
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [
    # T, H, W, segs (None: no stage A), c_mid, coutB, actA, actB, nres -- bf16 kernel
    (1, 64, 64, None, 64, 72, 0, 2, 0),        # conv_resident_kernel (no residuals by its rule)
    (1, 64, 64, [64], 64, 64, 1, 0, 2),        # conv_pair_kernel, both residuals
    (2, 32, 32, [64, 32], 64, 64, 2, 1, 1),    # general chain, c = 64
    (1, 32, 64, [128], 128, 128, 1, 0, 2),     # general chain, c = 128
    (1, 20, 32, None, 128, 72, 0, 2, 1),       # no stage A at c = 128; tiles hang over the image bottom
])
def test_conv_chain_strided(dev, dtype, case):
    ops = _ops()
    T, H, W, segs, cm, coutB, actA, actB, nres = case
    g = torch.Generator().manual_seed(T * 977 + H * 13 + coutB)
    cin = sum(segs) if segs else cm
    x = rb(torch.randn(T, cin, H, W, generator=g), dtype)
    wB = rb(torch.randn(coutB, cm, 3, 3, generator=g) / math.sqrt(9 * cm), dtype)
    bB = torch.randn(coutB, generator=g) * 0.1
    res = [rb(torch.randn(T, coutB, H, W, generator=g), dtype) for _ in range(nres)]
    if segs:
        wA = rb(torch.randn(cm, cin, 3, 3, generator=g) / math.sqrt(9 * cin), dtype)
        bA = torch.randn(cm, generator=g) * 0.1
        mid = rb(ACTS[actA](F.conv2d(x.double(), wA.double(), bA.double(), padding=1)).float(), dtype).double()
    else:
        wA = bA = None
        mid = x.double()
    ref = ACTS[actB](F.conv2d(mid, wB.double(), bB.double(), padding=1))
    for r in res:
        ref = ref + r.double()
    ref = ref * 0.5
    gr = _g(dtype)
    ins, o = {}, 0
    for i, c in enumerate(segs or [cm]):
        ins[f"x{i}"] = (clip(x[:, o:o + c]), dtype, (i + 1) * gr, (i + 1) * gr + c + gr)
        o += c
    for i, r in enumerate(res):
        ins[f"r{i}"] = (clip(r), dtype, (i + 1) * gr, coutB + (3 - i) * gr)
    outs = {"y": ((T, H, W, coutB), dtype, gr, coutB + 2 * gr)}
    wAp = ops.pack_conv_weight(wA[:, :, None], [(c, c) for c in segs], dtype).to(dev) if segs else None
    wBp = ops.pack_conv_weight(wB[:, :, None], [(cm, cm)], dtype).to(dev)
    bAd = bA.to(dev) if segs else None
    bBd = bB.to(dev)

    def call(y, **t):
        ops.conv_chain([t[f"x{i}"] for i in range(len(segs or [cm]))], wAp, bAd, actA, wBp, bBd, actB, cm, coutB,
                       res0=t.get("r0"), res1=t.get("r1"), out_scale=0.5, out=y)
    got = run_both(dev, ins, outs, call, f"conv_chain {case} {dtype}")["y"]
    # the intermediate is rounded to the element type: one bf16 ulp of it moves the result by more than TOL's share
    close(nchw(got), ref, dtype, f"conv_chain {case}", scale=1.0 if dtype == FP else 2.0)


# ------------------------------------------------------------------------------------------------ group norm
def _gn_call(x, x1, gamma, beta, film, y, raw, *, groups=32, resample=0, act=3):
    import ctypes
    from flair_amd import _lib, ops
    T, H, W, c0 = x.shape
    C = c0 + (x1.shape[3] if x1 is not None else 0)
    p = ops.GnParams()
    p.dtype, p.C, p.c0 = _lib.dtype_code(x), C, c0
    p.ld0, p.ld1 = ops._ld(x), ops._ld(x1) if x1 is not None else 0
    p.groups, p.F, p.H, p.W, p.frames_per_stat, p.eps, p.act, p.resample = groups, T, H, W, T, 1e-5, act, resample
    p.y_ld, p.raw_ld = ops._ld(y), ops._ld(raw) if raw is not None else 0
    p.film_ld = film.stride(0) if film is not None else 0
    ws = ops._workspace(ops.lib_ws_bytes(p), x.device)
    _lib.check(_lib.lib().flair_groupnorm_nhwc(ctypes.byref(p), _lib.ptr(x), _lib.ptr(x1), _lib.ptr(gamma), _lib.ptr(beta),
                                               _lib.ptr(film), _lib.ptr(y), _lib.ptr(raw), _lib.ptr(ws), _lib.stream()),
               "flair_groupnorm_nhwc")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("film_pad", [8, 5], ids=["film_aligned", "film_unaligned"])
@pytest.mark.parametrize("case", [
    # T, H, W, c0, c1, resample
    (4, 8, 8, 128, 128, 0),       # one-launch small-tensor kernel (a workgroup per group)
    (3, 12, 20, 128, 64, 0),      # two-pass kernel
    (2, 16, 14, 64, 64, 1),       # two-pass, 2x2 average pooling, raw
    (2, 7, 9, 128, 0, 2),         # two-pass, nearest 2x, raw; pixel counts off every vector / block multiple
])
def test_group_norm_strided(dev, dtype, film_pad, case):
    T, H, W, c0, c1, resample = case
    C = c0 + c1
    g = torch.Generator().manual_seed(7 + C + H)
    x = rb(torch.randn(T, C, H, W, generator=g) * 1.7 + 0.3, dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    emb = torch.randn(T, 2 * C + film_pad, generator=g) * 0.5
    xd = x.double()
    n = F.group_norm(xd.permute(1, 0, 2, 3)[None], 32, gamma.double(), beta.double(), 1e-5)[0].permute(1, 0, 2, 3)
    ref = F.silu(n * (1 + emb[:, :C, None, None].double()) + emb[:, C:2 * C, None, None].double())
    raw_ref = xd
    if resample == 1:
        ref, raw_ref = F.avg_pool2d(ref, 2), F.avg_pool2d(xd, 2)
    elif resample == 2:
        ref, raw_ref = F.interpolate(ref, scale_factor=2, mode="nearest"), F.interpolate(xd, scale_factor=2, mode="nearest")
    Ho, Wo = ref.shape[2:]
    gr = _g(dtype)
    ins = {"x": (clip(x[:, :c0]), dtype, gr, c0 + 3 * gr)}
    if c1:
        ins["x1"] = (clip(x[:, c0:]), dtype, 2 * gr, c1 + 3 * gr)
    outs = {"y": ((T, Ho, Wo, C), dtype, gr, C + 2 * gr)}
    if resample:
        outs["raw"] = ((T, Ho, Wo, C), dtype, 2 * gr, C + 3 * gr)
    # film rows: with film_pad = 5 the row stride is not a multiple of 4 floats (the scalar path of gn.hip's filmVec)
    film = emb.to(dev)
    gd, bd = gamma.to(dev), beta.to(dev)

    def call(x, y, x1=None, raw=None):
        _gn_call(x, x1, gd, bd, film, y, raw, resample=resample)
    got = run_both(dev, ins, outs, call, f"gn {case} {dtype}")
    close(nchw(got["y"]), ref, dtype, f"gn {case}", scale=4.0)
    if resample:
        close(nchw(got["raw"]), raw_ref, dtype, f"gn raw {case}")


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(qkv, heads, d, new_order):
    """qkv (F, L, 3C) f64 -> (F, L, C)."""
    Fr, L, _ = qkv.shape
    C = heads * d
    outs = []
    for h in range(heads):
        if new_order:
            q, k, v = qkv[..., h * d:(h + 1) * d], qkv[..., C + h * d:C + (h + 1) * d], qkv[..., 2 * C + h * d:2 * C + (h + 1) * d]
        else:
            base = 3 * d * h
            q, k, v = qkv[..., base:base + d], qkv[..., base + d:base + 2 * d], qkv[..., base + 2 * d:base + 3 * d]
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(d), dim=-1)
        outs.append(p @ v)
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("new_order", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_qkv_attention_strided(dev, dtype, new_order, d):
    """L = 10 * 13 = 130: not a multiple of any KV tile."""
    ops = _ops()
    Fr, H, W, heads = 2, 10, 13, 2
    C = heads * d
    g = torch.Generator().manual_seed(11 + d)
    qkv = rb(torch.randn(Fr, H, W, 3 * C, generator=g) * 1.5, dtype)
    ref = _attn_ref(qkv.double().reshape(Fr, H * W, 3 * C), heads, d, new_order).reshape(Fr, H, W, C)
    ins = {"qkv": (qkv, dtype, 8, 3 * C + 24)}
    outs = {"y": ((Fr, H, W, C), dtype, 16, C + 24)}

    def call(qkv, y):
        ops.qkv_attention(qkv, heads, new_order=new_order, out=y)
    got = run_both(dev, ins, outs, call, f"attn d={d} {dtype}")["y"]
    close(got, ref, dtype, f"attn d={d}", scale=2.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_dim", [64, 32])
def test_temporal_attention_strided(dev, dtype, head_dim):
    ops = _ops()
    T, H, W, C, window = 5, 3, 5, 128, 5
    heads = C // head_dim
    g = torch.Generator().manual_seed(5 + head_dim)
    qkv = rb(torch.randn(T, H, W, 3 * C, generator=g), dtype)
    kpos = torch.randn(window - 1, C, generator=g) * 0.3
    qd = qkv.double()
    q, k, v = qd[..., :C], qd[..., C:2 * C], qd[..., 2 * C:]
    idx = (torch.arange(T).view(T, 1) + torch.tensor([-2, -1, 1, 2]).view(1, 4)).clamp(0, T - 1)
    kw = k[idx] + kpos.double().view(1, 4, 1, 1, C)                 # T,4,H,W,C
    vw = v[idx]
    qh = q.reshape(T, H, W, heads, head_dim)
    kh = kw.reshape(T, 4, H, W, heads, head_dim)
    vh = vw.reshape(T, 4, H, W, heads, head_dim)
    s = torch.einsum("thwnd,tjhwnd->thwnj", qh, kh) / math.sqrt(head_dim)
    ref = torch.einsum("thwnj,tjhwnd->thwnd", torch.softmax(s, dim=-1), vh).reshape(T, H, W, C)
    ins = {"qkv": (qkv, dtype, 8, 3 * C + 16)}
    outs = {"y": ((T, H, W, C), dtype, 8, C + 16)}
    kd = kpos.to(dev)

    def call(qkv, y):
        ops.temporal_attention(qkv, kd, window, round_fp16=False, head_dim=head_dim, out=y)
    got = run_both(dev, ins, outs, call, f"tattn d={head_dim} {dtype}")["y"]
    close(got, ref, dtype, f"tattn d={head_dim}", scale=4.0)


# ------------------------------------------------------------------------------------------------ DCN
DCN_CASES = [
    # dtype, F, H, W, half (= Cin / 2), Cout, G, activated   -> instantiation <NCF, NPF, TPP, ACTIVATED, ONEFRAME>
    (BF, 2, 64, 128, 128, 128, 16, True),     # <4,2,16,A,1F>  (P >= 16384, half % 128 == 0)
    (BF, 2, 65, 127, 128, 128, 16, True),     # <4,2,16,A,->
    (BF, 2, 64, 128, 128, 128, 16, False),    # <4,2,16,-,->  the general kernel at large P
    (BF, 2, 64, 128, 64, 128, 8, True),       # <4,2,8,A,1F>   (P >= 16384, half 64 < Cout)
    (BF, 2, 65, 127, 64, 128, 8, True),       # <4,2,8,A,->
    (BF, 2, 64, 128, 64, 128, 16, False),     # <4,2,8,-,->
    (BF, 1, 12, 16, 128, 128, 16, True),      # <4,1,8,A,1F>   (P < 16384)
    (BF, 2, 9, 23, 64, 96, 8, True),          # <4,1,8,A,->
    (BF, 2, 9, 23, 128, 128, 16, False),      # <4,1,8,-,->
    (BF, 4, 128, 128, 64, 64, 16, True),      # <2,4,8,A,1F>   (Cout <= 64, P >= 65536)
    (BF, 5, 121, 109, 64, 64, 8, True),       # <2,4,8,A,->
    (BF, 4, 128, 128, 64, 64, 16, False),     # <2,4,8,-,->
    (BF, 1, 16, 32, 64, 64, 16, True),        # <2,2,8,A,1F>   (P < 65536)
    (BF, 2, 11, 13, 64, 32, 8, True),         # <2,2,8,A,->
    (BF, 2, 11, 13, 64, 64, 16, False),       # <2,2,8,-,->
    (FP, 1, 16, 32, 64, 64, 16, True),        # <2,2,4,A,1F>   (f32, Cout <= 64)
    (FP, 2, 11, 13, 32, 48, 8, True),         # <2,2,4,A,->
    (FP, 2, 11, 13, 64, 64, 16, False),       # <2,2,4,-,->
    (FP, 1, 8, 16, 128, 128, 16, True),       # <4,1,8,A,1F>   (f32, Cout > 64)
    (FP, 2, 9, 23, 64, 128, 8, True),         # <4,1,8,A,->
    (FP, 2, 9, 23, 128, 128, 16, False),      # <4,1,8,-,->
]
__doc__ += """
DCN (flair_dcn_align) cases and the instantiation each selects.  launch_dcn picks ACTIVATED = raw_activated and ONEFRAME = activated and H*W a multiple of the pixel tile 32 * NPF:
    case (dtype, F, H, W, Cin/2, Cout, G, act)   instantiation <E, NCF, NPF, TPP, ACTIVATED, ONEFRAME>   branch condition
    bf16 2 64x128  128 128 G16 act              <bf16, 4, 2, 16, 1, 1>   (Cout > 64, P >= 16384, Cin/2 % 128 == 0)
    bf16 2 65x127  128 128 G16 act              <bf16, 4, 2, 16, 1, 0>
    bf16 2 64x128  128 128 G16 pre              <bf16, 4, 2, 16, 0, 0>
    bf16 2 64x128   64 128 G8  act              <bf16, 4, 2, 8, 1, 1>    (Cout > 64, P >= 16384, Cin/2 = 64)
    bf16 2 65x127   64 128 G8  act              <bf16, 4, 2, 8, 1, 0>
    bf16 2 64x128   64 128 G16 pre              <bf16, 4, 2, 8, 0, 0>
    bf16 1 12x16   128 128 G16 act              <bf16, 4, 1, 8, 1, 1>    (Cout > 64, P < 16384)
    bf16 2 9x23     64  96 G8  act              <bf16, 4, 1, 8, 1, 0>
    bf16 2 9x23    128 128 G16 pre              <bf16, 4, 1, 8, 0, 0>
    bf16 4 128x128  64  64 G16 act              <bf16, 2, 4, 8, 1, 1>    (Cout <= 64, P >= 65536)
    bf16 5 121x109  64  64 G8  act              <bf16, 2, 4, 8, 1, 0>
    bf16 4 128x128  64  64 G16 pre              <bf16, 2, 4, 8, 0, 0>
    bf16 1 16x32    64  64 G16 act              <bf16, 2, 2, 8, 1, 1>    (Cout <= 64, P < 65536)
    bf16 2 11x13    64  32 G8  act              <bf16, 2, 2, 8, 1, 0>
    bf16 2 11x13    64  64 G16 pre              <bf16, 2, 2, 8, 0, 0>
    f32  1 16x32    64  64 G16 act              <f32, 2, 2, 4, 1, 1>     (Cout <= 64)
    f32  2 11x13    32  48 G8  act              <f32, 2, 2, 4, 1, 0>
    f32  2 11x13    64  64 G16 pre              <f32, 2, 2, 4, 0, 0>
    f32  1 8x16    128 128 G16 act              <f32, 4, 1, 8, 1, 1>     (Cout > 64)
    f32  2 9x23     64 128 G8  act              <f32, 4, 1, 8, 1, 0>
    f32  2 9x23    128 128 G16 pre              <f32, 4, 1, 8, 0, 0>
The float64 reference runs on the last frame of multi-frame cases (frames are independent); (b) covers every frame."""


@pytest.mark.parametrize("case", DCN_CASES, ids=lambda c: f"{'bf16' if c[0] == BF else 'f32'}-{c[1]}x{c[2]}x{c[3]}-"
                         f"h{c[4]}-o{c[5]}-G{c[6]}-{'act' if c[7] else 'pre'}")
def test_dcn_strided(dev, case):
    from oracle.thirdparty import deform_conv2d
    ops = _ops()
    dtype, Fr, H, W, half, cout, G, activated = case
    g = torch.Generator().manual_seed(21 + half + cout + H)
    x = rb(torch.randn(Fr, 2 * half, H, W, generator=g), dtype)
    raw = torch.randn(Fr, 27 * G, H, W, generator=g)
    f1 = torch.randn(Fr, H, W, 2, generator=g) * 2
    f2 = torch.randn(Fr, H, W, 2, generator=g) * 2
    w = rb(torch.randn(cout, 2 * half, 3, 3, generator=g) / math.sqrt(18 * half), dtype)
    b = torch.randn(cout, generator=g) * 0.1
    if activated:
        o1, o2, mask = raw.chunk(3, dim=1)
        raw = torch.cat([rb(10 * torch.tanh(torch.cat((o1, o2), dim=1)), dtype), rb(torch.sigmoid(mask), dtype)], dim=1)
    else:
        raw = rb(raw, dtype)
    # reference (float64) on the last frame
    f = Fr - 1
    rd = raw[f:f + 1].double()
    if activated:
        off, msk = rd[:, :18 * G], rd[:, 18 * G:]
    else:
        o1, o2, m = rd.chunk(3, dim=1)
        off, msk = 10 * torch.tanh(torch.cat((o1, o2), dim=1)), torch.sigmoid(m)
    off1, off2 = off.chunk(2, dim=1)
    off1 = off1 + f1[f:f + 1].double().permute(0, 3, 1, 2).flip(1).repeat(1, off1.shape[1] // 2, 1, 1)
    off2 = off2 + f2[f:f + 1].double().permute(0, 3, 1, 2).flip(1).repeat(1, off2.shape[1] // 2, 1, 1)
    ref = deform_conv2d(x[f:f + 1].double(), torch.cat([off1, off2], 1), w.double(), b.double(), (1, 1), (1, 1), (1, 1), msk)
    gr = _g(dtype)
    ins = {"x0": (clip(x[:, :half]), dtype, gr, half + 3 * gr), "x1": (clip(x[:, half:]), dtype, 2 * gr, half + 2 * gr),
           "raw": (clip(raw[:, ops.dcn_raw_permutation(G)]), dtype, gr, 27 * G + 2 * gr),
           "f1": (f1, FP, 0, 2), "f2": (f2, FP, 0, 2)}
    outs = {"y": ((Fr, H, W, cout), dtype, gr, cout + 2 * gr)}
    wp = ops.pack_conv_weight(w, [(2 * half, 2 * half)], dtype).to(dev)
    bd = b.to(dev)

    def call(x0, x1, raw, f1, f2, y):
        ops.dcn_align(x0, x1, raw, f1, f2, wp, bd, cout, groups=G, out=y, raw_activated=activated)
    got = run_both(dev, ins, outs, call, f"dcn {case}")["y"]
    close(nchw(got[f:f + 1]), ref, dtype, f"dcn {case}", scale=2.0)


# ------------------------------------------------------------------------------------------------ element-wise / warps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("two", [False, True])
def test_add_act_strided(dev, dtype, two):
    ops = _ops()
    T, H, W, C = 3, 7, 9, 40                   # 189 pixels a frame: off every block multiple
    g = torch.Generator().manual_seed(3)
    x0 = rb(torch.randn(T, H, W, C, generator=g), dtype)
    x1 = rb(torch.randn(T, H, W, C, generator=g), dtype)
    ref = torch.relu(x0.double() + (x1.double() if two else 0))
    gr = _g(dtype)
    ins = {"a": (x0, dtype, gr, C + 2 * gr)}
    if two:
        ins["b"] = (x1, dtype, 2 * gr, C + 3 * gr)
    outs = {"y": ((T, H, W, C), dtype, gr, C + gr)}

    def call(a, y, b=None):
        ops.add_act(a, b, ops.ACT_RELU, out=y)
    close(run_both(dev, ins, outs, call, "add_act")["y"], ref, dtype, "add_act")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_pixels_and_add_frame_bias_strided(dev, dtype):
    """In-place entries: the view is both read and written."""
    ops = _ops()
    T, H, W, C = 3, 5, 7, 48
    g = torch.Generator().manual_seed(4)
    x = rb(torch.randn(T, H, W, C, generator=g), dtype)
    wmap = torch.rand(T * H * W, generator=g) + 0.5
    fb = torch.randn(T, C + 6, generator=g)                     # bias rows wider than C (bias_ld = C + 6)
    gr = _g(dtype)
    outs = {"x": ((T, H, W, C), dtype, gr, C + 2 * gr, x)}
    wd, fbd = wmap.to(dev), fb.to(dev)
    got = run_both(dev, {}, outs, lambda x: ops.scale_pixels(x, wd), "scale_pixels")["x"]
    close(got, x.double() * wmap.double().view(T, H, W, 1), dtype, "scale_pixels")
    got = run_both(dev, {}, outs, lambda x: ops.add_frame_bias(x, fbd), "add_frame_bias")["x"]
    close(got, x.double() + fb[:, :C].double().view(T, 1, 1, C), dtype, "add_frame_bias")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_and_affine_channels_strided(dev, dtype):
    ops = _ops()
    T, H, W, C = 2, 5, 7, 3
    g = torch.Generator().manual_seed(5)
    src = torch.randn(T, H, W, C, generator=g)
    ins = {"s": (src, FP, 1, 7)}
    outs = {"d": ((T, H, W, C), dtype, 4, 12)}
    got = run_both(dev, ins, outs, lambda s, d: ops.cast_channels(s, d), "cast_channels")["d"]
    close(got, rb(src, dtype).double(), dtype, "cast_channels")
    if dtype == FP:
        sub, mul = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        sd, md = sub.to(dev), mul.to(dev)
        outs = {"y": ((T, H, W, C), FP, 2, 6)}
        got = run_both(dev, ins, outs, lambda s, y: ops.affine_channels(s, C, 0.5, 0.1, -0.8, 0.8, sd, md, y),
                       "affine_channels")["y"]
        ref = ((src.double() * 0.5 + 0.1).clamp(-0.8, 0.8) - sub.double()) * mul.double()
        close(got, ref, FP, "affine_channels")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,size,C,vec", [
    (0, (13, 11), 3, False), (1, (14, 18), 2, False), (2, (9, 13), 3, False), (3, (3, 4), 3, False),
    (4, (14, 18), 3, False),     # nearest 2x, C off the vector width: the generic kernel
    (4, (14, 18), 16, True),     # nearest 2x, C and strides on the vector width: nearest2x_kernel (warp.hip:369)
    (4, (10, 13), 16, False),    # nearest, not 2x: the generic kernel
])
def test_resize_strided(dev, dtype, mode, size, C, vec):
    ops = _ops()
    T, Hi, Wi = 2, 7, 9
    g = torch.Generator().manual_seed(9 + mode)
    x = rb(torch.randn(T, Hi, Wi, C, generator=g), dtype)
    if mode == 3:
        x = rb(torch.randn(T, 2 * size[0], 2 * size[1], C, generator=g), dtype)
    xd = nchw(x.double())
    ref = {0: lambda: F.interpolate(xd, size=size, mode="bilinear", align_corners=False),
           1: lambda: F.interpolate(xd, size=size, mode="bilinear", align_corners=True),
           2: lambda: F.interpolate(xd, size=size, mode="bicubic"),
           3: lambda: F.avg_pool2d(xd, 2, 2),
           4: lambda: F.interpolate(xd, size=size, mode="nearest")}[mode]()
    sc = 1.0 if mode == 4 else 2.0
    ref[:, 0] *= sc
    gr = _g(dtype)
    ins = {"x": (x, dtype, gr if vec else 1, C + 2 * gr if vec else C + 3)}
    outs = {"y": ((T, *size, C), dtype, gr if vec else 2, C + gr if vec else C + 5)}

    def call(x, y):
        ops.resize(x, size, mode, channels=C, out=y, scale_c0=sc)
    got = run_both(dev, ins, outs, call, f"resize {mode}")["y"]
    close(nchw(got), ref, dtype, f"resize {mode}", scale=8.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("border", [False, True])
def test_flow_warp_strided(dev, dtype, border):
    from oracle.thirdparty import flow_warp
    ops = _ops()
    T, H, W, C = 2, 11, 10, 32
    g = torch.Generator().manual_seed(3)
    x = rb(torch.randn(T, H, W, C, generator=g), dtype)
    flow = torch.randn(T, H, W, 2, generator=g) * 3.0
    ref = flow_warp(nchw(x.double()), flow.double(), padding_mode="border" if border else "zeros")
    gr = _g(dtype)
    ins = {"x": (x, dtype, gr, C + 2 * gr), "f": (flow, FP, 4, 12)}          # flow_ld = 12 (SPyNet: b[..., 8:10])
    outs = {"y": ((T, H, W, C), dtype, 2 * gr, C + 3 * gr)}

    def call(x, f, y):
        ops.flow_warp(x, f, border=border, out=y)
    close(nchw(run_both(dev, ins, outs, call, "flow_warp")["y"]), ref, dtype, "flow_warp", scale=4.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_edges_with_channel_offset(dev, dtype):
    ops = _ops()
    N, C, H, W = 2, 6, 5, 7
    g = torch.Generator().manual_seed(6)
    src = torch.randn(N, C, H, W, generator=g)
    srcd = src.to(dev)
    # nchw -> channels [coff, coff + C) of a clip tensor whose view starts at channel 4 of a 24-wide buffer
    outs = {"d": ((N, H, W, 16), dtype, 4, 24)}
    got = run_both(dev, {}, outs, lambda d: ops.nchw_to_clip(srcd, d, coff=3), "nchw_to_clip")["d"]
    close(got[..., 3:3 + C], clip(rb(src, dtype)).double(), dtype, "nchw_to_clip")
    assert torch.all(got[..., :3] == OUT_FILL) and torch.all(got[..., 3 + C:] == OUT_FILL)
    # clip channels [coff, coff + C) -> nchw
    x = rb(torch.randn(N, H, W, 16, generator=g), dtype)
    ins = {"x": (x, dtype, 4, 24)}
    box = {}

    def back(x):
        box.setdefault("n", []).append(ops.clip_to_nchw(x, C, coff=5))
    run_both(dev, ins, {}, back, "clip_to_nchw")
    dense, strided = box["n"]
    assert torch.equal(bits(dense), bits(strided))
    close(dense.double().cpu(), nchw(x[..., 5:5 + C].double()), FP, "clip_to_nchw")


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool_strided(dev, dtype):
    ops = _ops()
    T, H, W, C = 2, 9, 11, 24
    g = torch.Generator().manual_seed(8)
    x = rb(torch.randn(T, H, W, C, generator=g), dtype)
    ref = clip(F.max_pool2d(nchw(x.double()), 3, 2, 1))
    gr = _g(dtype)
    ins = {"x": (x, dtype, gr, C + 2 * gr)}
    outs = {"y": ((T, 5, 6, C), dtype, 2 * gr, C + 3 * gr)}
    close(run_both(dev, ins, outs, lambda x, y: ops.maxpool3x3s2(x, out=y), "maxpool")["y"], ref, dtype, "maxpool")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pw", [False, True])
def test_dwconv_strided(dev, stride, pw):
    ops = _ops()
    T, H, W, C, cout = 2, 9, 11, 16, 24
    g = torch.Generator().manual_seed(10 + stride)
    x = torch.randn(T, H, W, C, generator=g)
    w_dw = torch.randn(9, C, generator=g) * 0.3
    b_dw = torch.randn(C, generator=g) * 0.1
    w_pw = torch.randn(cout, C, generator=g) / 4
    b_pw = torch.randn(cout, generator=g) * 0.1
    d = F.conv2d(nchw(x.double()), w_dw.double().t().reshape(C, 1, 3, 3), b_dw.double(), stride=stride, padding=1, groups=C)
    d = F.leaky_relu(d, 0.1)
    if pw:
        d = F.leaky_relu(F.conv2d(d, w_pw.double()[:, :, None, None], b_pw.double()), 0.1)
    Ho, Wo = d.shape[2:]
    co = cout if pw else C
    ins = {"x": (x, FP, 4, C + 8)}
    outs = {"y": ((T, Ho, Wo, co), FP, 4, co + 12)}
    args = [t.to(dev) for t in (w_dw, b_dw, w_pw, b_pw)]

    def call(x, y):
        ops.dwconv(x, args[0], args[1], stride=stride, pw=(args[2], args[3]) if pw else None, out=y)
    close(nchw(run_both(dev, ins, outs, call, "dwconv")["y"]), d, FP, "dwconv", scale=2.0)
