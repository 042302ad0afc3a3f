"""The prior, warp and embedding entries on strided channel views with guarded neighbours.

The regime of tests/test_gpu_strides.py (its run_both: a float64 reference from the dtype-rounded inputs, dense and strided
outputs bit-equal, everything around the outputs and every input unchanged) for the entries that suite stops short of:
flair_layernorm_nhwc, flair_attention_wide, flair_argmax_codebook, flair_vq_nearest_nhwc, flair_adain_nhwc,
flair_gated_blend, flair_sft_fuse, flair_vsrpp_warp2 / flair_vsrpp_prep, flair_flow_compose, flair_linear_f32 and
flair_timestep_embedding.  Every view handed to an entry is inside its contract (the refusals are tests/test_strides_cpu.py's).
Entries with scalar accesses take odd offsets and strides; the 16-byte ones take 16-byte granular ones.  Tensors an entry
takes without a stride (flows, the embedding rows, sft_fuse's operands) are dense slices of a longer guarded allocation."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_strides import DTYPES, FP, _g, clip, close, nchw, run_both
from tests.util import (ARGMAX_FILL, IN_FILL, OUT_FILL, assert_flat_untouched, assert_untouched, bits, flat_guarded, guarded,
                        rb)

pytestmark = pytest.mark.gpu


def _ops():
    from flair_amd import ops
    return ops


def _placed(dev, t, dtype, coff, ld, fill):
    """A cpu (T,H,W,C) tensor as a guarded view -> (buf, view, copy of buf before the launch)."""
    buf, v = guarded(*t.shape, dtype, dev, coff=coff, ld=ld, fill=fill)
    v.copy_(t.to(dev, dtype))
    return buf, v, buf.clone()


# ------------------------------------------------------------------------------------------------ layer norm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_pos", [False, True], ids=["plain", "pos"])
@pytest.mark.parametrize("C", [40, 512, "max"])
def test_layer_norm_strided(dev, dtype, with_pos, C):
    """3 x 5 x 7 = 105 rows: the last workgroup has one row of four.  "max": 1024 (f32) / 2048 (bf16), every lane holding
    four 16-byte pieces.  out and out_pos at their own offsets and strides."""
    ops = _ops()
    gr = _g(dtype)
    C = 64 * 4 * gr if C == "max" else C
    T, H, W = 3, 5, 7
    g = torch.Generator().manual_seed(C + 1)
    x = rb(torch.randn(T, H, W, C, generator=g) * 2 + 0.5, dtype)
    gamma, beta, pos = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(H * W, C, generator=g)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    ins = {"x": (x, dtype, gr, C + 2 * gr)}
    outs = {"y": ((T, H, W, C), dtype, gr, C + 3 * gr)}
    if with_pos:
        outs["y2"] = ((T, H, W, C), dtype, 3 * gr, C + 4 * gr)
    gd, bd, pd = gamma.to(dev), beta.to(dev), pos.to(dev)

    def call(x, y, y2=None):
        ops.layer_norm(x, gd, bd, pos=pd if with_pos else None, out=y, out_pos=y2)
    got = run_both(dev, ins, outs, call, f"layer_norm C={C} {dtype}")
    close(got["y"], ref, dtype, f"layer_norm C={C}", scale=4.0)
    if with_pos:
        close(got["y2"], ref + pos.double().view(1, H, W, C), dtype, f"layer_norm + pos C={C}", scale=4.0)


# ------------------------------------------------------------------------------------------------ attention, wide heads
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(5, 7), (16, 16)], ids=["L35", "L256"])
@pytest.mark.parametrize("heads,d,interleaved", [(3, 40, False), (1, 512, False), (2, 96, True)])
def test_attention_wide_strided(dev, dtype, hw, heads, d, interleaved):
    """q, k and v at non-adjacent channel offsets of one guarded buffer, the channels between them NaN (the dense call
    sees the same layout): planar q | k | v blocks with gaps, or per-head v | q | k triples with gaps.  L = 35 leaves
    the last 16-query tile ragged and has fewer keys than threads."""
    ops = _ops()
    gr = _g(dtype)
    Fr, (H, W), C = 2, hw, heads * d
    if interleaved:
        hs, (qo, ko, vo) = 3 * d + 3 * gr, (d + gr, 2 * d + 2 * gr, 0)
        width = heads * hs
    else:
        hs, (qo, ko, vo) = d, (0, C + gr, 2 * C + 3 * gr)
        width = 3 * C + 4 * gr
    g = torch.Generator().manual_seed(heads * 1000 + d + H)
    qkv = torch.full((Fr, H, W, width), IN_FILL)
    parts = {}
    for h in range(heads):
        for name, o in (("q", qo), ("k", ko), ("v", vo)):
            parts[name, h] = rb(torch.randn(Fr, H, W, d, generator=g) * 0.8, dtype)
            qkv[..., o + h * hs:o + h * hs + d] = parts[name, h]
    ref = []
    for h in range(heads):
        q, k, v = (parts[n, h].double().reshape(Fr, H * W, d) for n in "qkv")
        ref.append(torch.softmax(q @ k.transpose(1, 2) / math.sqrt(d), dim=-1) @ v)
    ref = torch.cat(ref, dim=-1).reshape(Fr, H, W, C)
    ins = {"qkv": (qkv, dtype, gr, width + 2 * gr)}
    outs = {"y": ((Fr, H, W, C), dtype, 2 * gr, C + 3 * gr)}

    def call(qkv, y):
        ops.attention_wide(qkv, heads, d, q_off=qo, k_off=ko, v_off=vo, head_stride=hs, out=y)
    got = run_both(dev, ins, outs, call, f"attention_wide {heads}x{d} L={H * W} {dtype}")["y"]
    close(got, ref, dtype, f"attention_wide {heads}x{d} L={H * W}", scale=4.0)


# ------------------------------------------------------------------------------------------------ arg-max + codebook row
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("forced", [False, True], ids=["argmax", "forced"])
@pytest.mark.parametrize("N,D", [(37, 24), (1024, 256)])
def test_argmax_codebook_strided(dev, dtype, forced, N, D):
    """The logits sit in a guard of ARGMAX_FILL (finite, above every logit: tests/test_strides_cpu.py shows that an arg-max
    reading one class too many, or one too early, picks it), at an odd offset and stride (scalar loads).  Ties: the
    first index wins; the last class wins one row; forced indices out of range are clamped.  Indices and codes exact."""
    ops = _ops()
    T, H, W = 2, 3, 5
    rows = T * H * W                                   # 30: the last workgroup has two rows of four
    g = torch.Generator().manual_seed(N + D)
    logits = rb(torch.randn(T, H, W, N, generator=g) * 3, dtype)
    logits[0, 0, 0, 5] = logits[0, 0, 0, N - 1] = 50.0     # a tie with the last class: index 5
    logits[0, 0, 1, 0] = logits[0, 0, 1, 1] = 50.0         # a tie of neighbours: index 0
    logits[1, 2, 4, N - 1] = 60.0                          # the last class of the last row wins
    book = torch.randn(N, D, generator=g) * 0.1
    want = logits.reshape(rows, N).argmax(1)
    want[0], want[1] = 5, 0
    assert want[rows - 1] == N - 1
    fidx = None
    if forced:
        fidx = torch.randint(0, N, (rows,), generator=g).int()
        fidx[:5] = torch.tensor([-3, N, N + 1000, N - 1, 0], dtype=torch.int32)
        want = fidx.clamp(0, N - 1).long()
    bookd, fd = book.to(dev), fidx.to(dev) if forced else None
    # dense
    ld_, yd = logits.to(dev, dtype), torch.full((T, H, W, D), OUT_FILL, dtype=dtype, device=dev)
    _, idx_d = ops.argmax_codebook(ld_, N, bookd, forced_idx=fd, out=yd)
    # strided
    lbuf, lv, lbefore = _placed(dev, logits, dtype, 3, N + 7, ARGMAX_FILL)
    ybuf, yv = guarded(T, H, W, D, dtype, dev, coff=1, ld=D + 3, fill=OUT_FILL)
    ybefore = ybuf.clone()
    _, idx_s = ops.argmax_codebook(lv, N, bookd, forced_idx=fd, out=yv)
    torch.cuda.synchronize()
    what = f"argmax_codebook N={N} D={D} {dtype}"
    assert torch.equal(idx_d.cpu().long(), want), what
    assert torch.equal(idx_s, idx_d), f"{what}: strided indices differ at rows {(idx_s != idx_d).nonzero().flatten().tolist()}"
    assert torch.equal(bits(yv), bits(yd)), what
    assert torch.equal(yd.cpu().reshape(rows, D), book[want].to(dtype)), what
    assert_untouched(ybuf, ybefore, yv, what + ": codes")
    assert_untouched(lbuf, lbefore, None, what + ": logits")


# ------------------------------------------------------------------------------------------------ nearest codebook row
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [37, 512])
@pytest.mark.parametrize("N,D", [(300, 12), (1024, 256)])
def test_vq_nearest_strided(dev, dtype, rows, N, D):
    """z and y as views at odd offsets and strides (scalar accesses).  Indices by the rule of test_vq_nearest_random
    (tests/test_gpu_restoreformer.py): exact where the float64 top-2 margin is clear of f32 rounding, within that rounding
    of the minimum elsewhere; the codes bit-equal to the chosen rows rounded to the dtype."""
    ops = _ops()
    g = torch.Generator().manual_seed(rows * 7 + N + D)
    e = torch.randn(N, D, generator=g) / D ** 0.5
    z = rb(torch.randn(1, rows, 1, D, generator=g), dtype)
    ins = {"z": (z, dtype, 3, D + 5)}
    outs = {"y": ((1, rows, 1, D), dtype, 1, D + 3)}
    ed, box = e.to(dev), []

    def call(z, y):
        box.append(ops.vq_nearest(z, ed, out=y)[1])
    codes = run_both(dev, ins, outs, call, f"vq_nearest rows={rows} N={N} D={D} {dtype}")["y"]
    idx_d, idx_s = box
    assert torch.equal(idx_d, idx_s)
    got = idx_d.cpu().long()
    z64, e64 = z.double().reshape(rows, D), e.double()
    dist = (z64 ** 2).sum(1, keepdim=True) + (e64 ** 2).sum(1)[None] - 2 * z64 @ e64.t()
    top2 = dist.sort(dim=1).values[:, :2]
    tol = 1e-5 * (dist.abs().max().item() + 1.0)
    clear = (top2[:, 1] - top2[:, 0]) > tol
    assert clear.float().mean().item() > 0.9
    assert torch.equal(got[clear], dist.argmin(1)[clear])
    assert bool((dist[torch.arange(rows), got] - dist.min(1).values <= tol).all())
    assert torch.equal(codes.reshape(rows, D), e[got].to(dtype).double())


# ------------------------------------------------------------------------------------------------ AdaIN
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(3, 5), (16, 16)], ids=["HW15", "HW256"])
@pytest.mark.parametrize("C", [72, 256])
def test_adain_strided(dev, dtype, hw, C):
    """Two frames (statistics per frame and channel), content, style and y each at their own odd offset and stride;
    C = 72 leaves the second 64-channel block partly idle, HW = 15 is not a multiple of the four pixel lanes."""
    ops = _ops()
    Fr, (H, W) = 2, hw
    g = torch.Generator().manual_seed(C + H)
    content = rb(torch.randn(Fr, H, W, C, generator=g) * 2, dtype)
    style = rb(torch.randn(Fr, H, W, C, generator=g) * 1.5 + 0.3, dtype)
    c64, s64 = content.double(), style.double()
    mc, ms = c64.mean((1, 2), keepdim=True), s64.mean((1, 2), keepdim=True)
    sc = (c64.var((1, 2), unbiased=True, keepdim=True) + 1e-5).sqrt()
    ss = (s64.var((1, 2), unbiased=True, keepdim=True) + 1e-5).sqrt()
    ref = (c64 - mc) / sc * ss + ms
    ins = {"content": (content, dtype, 3, C + 5), "style": (style, dtype, 1, C + 2)}
    outs = {"y": ((Fr, H, W, C), dtype, 2, C + 7)}
    got = run_both(dev, ins, outs, lambda content, style, y: ops.adain(content, style, out=y), f"adain C={C} {dtype}")["y"]
    close(got, ref, dtype, f"adain C={C} HW={H * W}", scale=4.0)


# ------------------------------------------------------------------------------------------------ gated blend
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [40, 128])
def test_gated_blend_strided(dev, dtype, C):
    """x, m and y at different strides; the gate a column slice [8, 8 + C) of wider f32 rows, NaN around it.  f32 keeps
    the absolute 1e-5 of test_gated_blend_and_sin_first_encoding (same data scale: the fast exponential's ~1e-6 relative
    error in the gate times |m - x| < 10, plus three roundings of values below 8), bf16 takes tests/util.py:TOL."""
    ops = _ops()
    Fr, H, W = 3, 5, 7
    gr = _g(dtype)
    g = torch.Generator().manual_seed(C)
    x, m = (rb(torch.randn(Fr, H, W, C, generator=g), dtype) for _ in range(2))
    gate = torch.randn(Fr, C, generator=g)
    s = torch.sigmoid(gate.double()).view(Fr, 1, 1, C)
    ref = x.double() + s * (m.double() - x.double())
    gbuf = torch.full((Fr + 2, C + 24), IN_FILL, device=dev)
    gv = gbuf[1:Fr + 1, 8:8 + C]
    gv.copy_(gate.to(dev))
    gbefore = gbuf.clone()
    ins = {"x": (x, dtype, gr, C + 2 * gr), "m": (m, dtype, 2 * gr, C + 3 * gr)}
    outs = {"y": ((Fr, H, W, C), dtype, gr, C + gr)}
    got = run_both(dev, ins, outs, lambda x, m, y: ops.gated_blend(x, m, gv, out=y), f"gated_blend C={C} {dtype}")["y"]
    assert torch.equal(bits(gbuf), bits(gbefore))
    if dtype == FP:
        err = (got - ref).abs().max().item()
        assert err <= 1e-5, f"gated_blend C={C}: max|err|={err:.3e} > 1e-5"
    else:
        close(got, ref, dtype, f"gated_blend C={C}")


# ------------------------------------------------------------------------------------------------ SFT tail
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nvec", [15, 2 * 4096 * 256 + 777], ids=["small", "two_grids_and_a_bit"])
def test_sft_fuse_flat_guarded(dev, dtype, nvec):
    """Dense by contract: the four tensors are slices of longer allocations (NaN around the inputs, the sentinel around
    y).  The launch is at most 4096 x 256 threads of one 16-byte piece each: 15 pieces leave most of one workgroup
    idle, the long case takes every thread through the grid-stride loop twice and some a third time."""
    ops = _ops()
    n = nvec * _g(dtype)
    g = torch.Generator().manual_seed(nvec % 1000)
    dec, sc, sh = (rb(torch.randn(n, generator=g), dtype) for _ in range(3))
    ref = dec.double() + 0.7 * (dec.double() * sc.double() + sh.double())
    shape = (1, 1, nvec, _g(dtype))
    placed = [flat_guarded(shape, dtype, dev, IN_FILL, t) for t in (dec, sc, sh)]
    ybuf, yv, ybefore = flat_guarded(shape, dtype, dev, OUT_FILL)
    ops.sft_fuse(placed[0][1], placed[1][1], placed[2][1], 0.7, out=yv)
    torch.cuda.synchronize()
    assert_flat_untouched(ybuf, ybefore, yv, "sft_fuse y")
    for name, (buf, _, before) in zip(("dec", "scale", "shift"), placed):
        assert_flat_untouched(buf, before, None, f"sft_fuse {name}")
    close(yv.double().cpu().reshape(-1), ref, dtype, f"sft_fuse n={n}", scale=2.0)


# ------------------------------------------------------------------------------------------------ BasicVSR++ warps
def _edge_flows(f, H, W):
    """Rows 5-10 of a (1,H,W,2) flow field aimed exactly at the frame's edges: integer flows, so the sampling point is a
    pixel centre (fraction 0) on row H / column W (one past the frame: everything reads as zero), on row H - 1 / column
    W - 1 (the +1 corners are outside with weight 0: a corner fetched from the guard would make the result NaN), and on
    column -1."""
    ws = torch.arange(W, dtype=torch.float32)
    f[0, 5, :, 0], f[0, 5, :, 1] = W - ws, 0.0                               # column W
    f[0, 6, :, 0], f[0, 6, :, 1] = W - 1 - ws, 0.0                           # column W - 1
    f[0, 7, :, 0], f[0, 7, :, 1] = 0.0, float(H - 7)                         # row H
    f[0, 8, :, 0], f[0, 8, :, 1] = 0.0, float(H - 1 - 8)                     # row H - 1
    f[0, 9, :, 0], f[0, 9, :, 1] = W - 1 - ws, float(H - 1 - 9)              # the last pixel
    f[0, 10, :, 0], f[0, 10, :, 1] = -1 - ws, 0.0                            # column -1
    return f


def _warp_layout(dtype, C, second):
    gr = _g(dtype)
    ins = {"prop": (None, dtype, gr, C + 2 * gr)}
    outs = {"c1": (None, dtype, 2 * gr, C + 3 * gr)}
    if second:
        ins["feat2"] = (None, dtype, 3 * gr, C + 4 * gr)
        outs["c2"] = (None, dtype, gr, C + 2 * gr)
    return ins, outs


VSRPP_SHAPES = [(20, 24, 64), (32, 32, 128)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("second", [False, True], ids=["first_order", "second_order"])
@pytest.mark.parametrize("shape", VSRPP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vsrpp_warp2_strided(dev, dtype, second, shape):
    """Sources and results as channel views (the sources' buffer descriptor of H * W * ld elements from the view's base
    then reaches into the NaN frame after them); flows that push whole rows outside, and the edge landings of
    _edge_flows.  The flows have no stride argument: dense."""
    from oracle.thirdparty import flow_warp
    ops = _ops()
    H, W, C = shape
    g = torch.Generator().manual_seed(11 + C)
    prop, feat2 = (rb(torch.randn(1, H, W, C, generator=g), dtype) for _ in range(2))
    f1 = torch.randn(1, H, W, 2, generator=g) * 4.0
    f2 = torch.randn(1, H, W, 2, generator=g) * 9.0
    f1[:, :3] += 30.0                                   # rows whose four corners all fall outside
    f1, f2 = _edge_flows(f1, H, W), _edge_flows(f2, H, W)
    ins, outs = _warp_layout(dtype, C, second)
    ins["prop"] = (prop, *ins["prop"][1:])
    outs = {k: ((1, H, W, C), *v[1:]) for k, v in outs.items()}
    if second:
        ins["feat2"] = (feat2, *ins["feat2"][1:])
    f1d, f2d = f1.to(dev), f2.to(dev)

    def call(prop, c1, feat2=None, c2=None):
        ops.vsrpp_warp2(prop, feat2, f1d, f2d if second else None, c1, c2)
    got = run_both(dev, ins, outs, call, f"vsrpp_warp2 {shape} {dtype}")
    close(nchw(got["c1"]), flow_warp(nchw(prop.double()), f1.double(), padding_mode="zeros"), dtype, "warp2 cond1", scale=4.0)
    if second:
        close(nchw(got["c2"]), flow_warp(nchw(feat2.double()), f2.double(), padding_mode="zeros"), dtype, "warp2 cond2",
              scale=4.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("second", [False, True], ids=["first_order", "second_order"])
@pytest.mark.parametrize("shape", VSRPP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vsrpp_prep_strided(dev, dtype, second, shape):
    """flair_vsrpp_prep with every strided argument a view.  flowpad is 2 x 16 bytes wide: channels 0-3 receive
    (flow1, flow2) in the activation dtype (flow2 = 0 on a first-order step), the channels above keep what they held.
    flow2_out against f1 + warp(f_prev, f1) in float64 (flow_compose's bound); cond2 against the warp by the flow the
    kernel itself reported (checked just before), so that an f32 rounding of the flow is not charged to the warp.
    Then flair_vsrpp_warp2 with that flow on the same views: bit-equal to prep (a replayed graph must equal the eager
    first step)."""
    from oracle.thirdparty import flow_warp
    ops = _ops()
    H, W, C = shape
    gr = _g(dtype)
    P = 2 * gr
    g = torch.Generator().manual_seed(5 + C)
    prop, feat2 = (rb(torch.randn(1, H, W, C, generator=g), dtype) for _ in range(2))
    f1 = _edge_flows(torch.randn(1, H, W, 2, generator=g) * 3, H, W)
    fprev = torch.randn(1, H, W, 2, generator=g) * 3
    f1[:, :3] += 30.0
    pad0 = torch.full((1, H, W, P), 7.0)
    ins, outs = _warp_layout(dtype, C, second)
    ins["prop"] = (prop, *ins["prop"][1:])
    outs = {k: ((1, H, W, C), *v[1:]) for k, v in outs.items()}
    outs["pad"] = ((1, H, W, P), dtype, gr, P + 2 * gr, pad0)
    if second:
        ins["feat2"] = (feat2, *ins["feat2"][1:])
        outs["f2"] = ((1, H, W, 2), FP, 0, 2)           # dense, between two guard frames
    f1d, fpd = f1.to(dev), fprev.to(dev)

    def call(prop, c1, pad, feat2=None, c2=None, f2=None):
        ops.vsrpp_prep(prop, feat2, f1d, fpd if second else None, c1, c2, f2, pad)
    what = f"vsrpp_prep {shape} {dtype}"
    got = run_both(dev, ins, outs, call, what)
    close(nchw(got["c1"]), flow_warp(nchw(prop.double()), f1.double(), padding_mode="zeros"), dtype, what + " cond1", scale=4.0)
    want_pad = torch.full((1, H, W, P), 7.0, dtype=torch.float64)
    want_pad[..., 0:2] = rb(f1, dtype).double()
    want_pad[..., 2:4] = 0.0
    if second:
        f2_ref = f1.double() + clip(flow_warp(nchw(fprev.double()), f1.double(), padding_mode="zeros"))
        close(got["f2"], f2_ref, FP, what + " flow2_out", scale=8.0)
        f2 = got["f2"].float()                           # exactly the kernel's f32 flow
        close(nchw(got["c2"]), flow_warp(nchw(feat2.double()), f2.double(), padding_mode="zeros"), dtype, what + " cond2",
              scale=4.0)
        want_pad[..., 2:4] = rb(f2, dtype).double()
    assert torch.equal(got["pad"], want_pad), what + ": flowpad"
    # the cached-flow launch of the later steps
    outs_w = {k: v for k, v in outs.items() if k in ("c1", "c2")}
    f2d = f2.to(dev) if second else None

    def call_w(prop, c1, feat2=None, c2=None):
        ops.vsrpp_warp2(prop, feat2, f1d, f2d, c1, c2)
    again = run_both(dev, ins, outs_w, call_w, what + " / warp2")
    for k in outs_w:
        assert torch.equal(bits(again[k]), bits(got[k])), f"{what}: {k} of vsrpp_warp2 differs from vsrpp_prep"


# ------------------------------------------------------------------------------------------------ flows / embeddings
def test_flow_compose_flat_guarded(dev):
    """Dense by contract: the three flow fields are frames 1-2 of four-frame allocations (NaN frames around the inputs,
    sentinel frames around the result); edge landings as for the warps."""
    from oracle.thirdparty import flow_warp
    ops = _ops()
    Fr, H, W = 2, 11, 13
    g = torch.Generator().manual_seed(4)
    f1 = torch.randn(Fr, H, W, 2, generator=g) * 2
    f1[:1] = _edge_flows(f1[:1].clone(), H, W)
    f2 = torch.randn(Fr, H, W, 2, generator=g) * 2
    ref = f1.double() + clip(flow_warp(nchw(f2.double()), f1.double(), padding_mode="zeros"))
    b1, v1, k1 = _placed(dev, f1, FP, 0, 2, IN_FILL)
    b2, v2, k2 = _placed(dev, f2, FP, 0, 2, IN_FILL)
    ob, ov = guarded(Fr, H, W, 2, FP, dev, fill=OUT_FILL)
    ok = ob.clone()
    ops.flow_compose(v1, v2, out=ov)
    torch.cuda.synchronize()
    assert_untouched(ob, ok, ov, "flow_compose out")
    assert_untouched(b1, k1, None, "flow_compose f1")
    assert_untouched(b2, k2, None, "flow_compose f2")
    close(ov.double().cpu(), ref, FP, "flow_compose", scale=8.0)


@pytest.mark.parametrize("act_in", [0, 3], ids=["in_none", "in_silu"])
@pytest.mark.parametrize("act_out", [0, 3], ids=["out_none", "out_silu"])
@pytest.mark.parametrize("M,K,N", [(1, 1031, 131), (32, 77, 131), (32, 511, 5)])
def test_linear_guarded(dev, act_in, act_out, M, K, N):
    """Odd K and N (K = 1031: three rounds of the 512-wide k loop, the last ragged; N = 5: fewer features than waves),
    y rows y_ld = N + 5 apart inside a sentinel buffer, x between NaN rows."""
    ops = _ops()
    act = {0: lambda v: v, 3: F.silu}
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    ref = act[act_out](act[act_in](x.double()) @ w.double().t() + b.double())
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
    assert not changed.any(), f"linear: {int(changed.sum())} element(s) changed outside y, first {changed.nonzero()[0].tolist()}"
    assert torch.equal(bits(xbuf), bits(xbefore))
    close(yv.double().cpu(), ref, FP, f"linear M={M} K={K} N={N}")


def test_linear_short_rows_after_a_launch_that_left_nan_in_lds(dev):
    """K = 33 is shorter than a wave: the lanes past K multiply a zero weight with whatever input element their fallback
    index names, which must be a staged one.  A first launch stages rows of NaN on every CU (LDS keeps what a finished
    workgroup left), so a fallback read past the M * K staged values would turn 0 * NaN into the result."""
    ops = _ops()
    g = torch.Generator().manual_seed(33)
    nan_x = torch.full((32, 511), IN_FILL, device=dev)
    ops.linear(nan_x, torch.zeros(4096, 511, device=dev), None)
    for M, K, N in ((32, 33, 7), (1, 33, 7), (9, 5, 3)):
        x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        y = ops.linear(x.to(dev), w.to(dev), b.to(dev), act_in=3)
        torch.cuda.synchronize()
        close(y.double().cpu(), F.silu(x.double()) @ w.double().t() + b.double(), FP, f"linear M={M} K={K} N={N}")


@pytest.mark.parametrize("sin_first", [False, True], ids=["cos_sin", "sin_cos"])
@pytest.mark.parametrize("dim", [6, 33, 1280])
def test_timestep_embedding_guarded(dev, sin_first, dim):
    """N = 5 rows (odd), a small, an odd (last column zero) and a large dim, in both orders, between sentinel rows.
    Reference: the frequencies and arguments in f32 as nn_new.py:103-121 forms them, their cos / sin in float64; the bound
    of test_embedding_linear_layout (an f32 argument near 1000 carries 6e-5 of rounding on its own)."""
    ops = _ops()
    t = torch.tensor([0., 1., 37., 999., 500.5])
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    args = (t[:, None] * freqs[None]).double()
    ref = torch.zeros(5, dim, dtype=torch.float64)
    ref[:, :half], ref[:, half:2 * half] = (torch.sin(args), torch.cos(args)) if sin_first else (torch.cos(args), torch.sin(args))
    buf, v, before = flat_guarded((5, dim), FP, dev, OUT_FILL)
    ops.timestep_embedding(t.to(dev), dim, out=v, sin_first=sin_first)
    torch.cuda.synchronize()
    assert_flat_untouched(buf, before, v, "timestep_embedding")
    close(v.double().cpu(), ref, FP, f"timestep_embedding dim={dim}", scale=50.0)
