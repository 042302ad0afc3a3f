"""Helpers shared by the parity tests."""
import math

import pytest
import torch


def to_clip(x, dtype, device, pad_to=None):
    """(N,C,H,W) f32 cpu -> (N,H,W,C[padded]) clip tensor on device."""
    y = x.permute(0, 2, 3, 1).contiguous()
    if pad_to is not None and pad_to > y.shape[3]:
        y = torch.cat([y, y.new_zeros(*y.shape[:3], pad_to - y.shape[3])], dim=3)
    return y.to(device=device, dtype=dtype).contiguous()


def from_clip(y, c=None):
    y = y.float().cpu()
    if c is not None:
        y = y[..., :c]
    return y.permute(0, 3, 1, 2).contiguous()


def rb(x, dtype):
    """Round an f32 cpu tensor through `dtype` (so the CPU reference sees what the GPU sees)."""
    return x.to(dtype).float()


# Tolerances (stated per dtype, relative to the reference's max magnitude):
#   f32 : accumulation-order differences only            -> 2e-5 * max|ref| + 1e-6
#   bf16: output rounding (2^-9 rel) + bf16 intermediates -> 1.6e-2 * max|ref| + 1e-3
TOL = {torch.float32: (2e-5, 1e-6), torch.bfloat16: (1.6e-2, 1e-3)}


def assert_close(got, ref, dtype, what="", scale=1.0):
    rel, ab = TOL[dtype]
    err = (got - ref).abs().max().item()
    bound = scale * rel * ref.abs().max().item() + ab
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e} (max|ref|={ref.abs().max().item():.3e})"
    return err


def parity_log(line):
    """Append one measured-error line to gpurun_out/r04_parity.txt (merged back from the GPU box; the copy under
    profiles/ is the committed record).  Never fails a test."""
    import os
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = os.path.join(root, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "r04_parity.txt"), "a") as f:
            f.write(line.rstrip() + "\n")
    except OSError:
        pass
    print(line)


# The fp32 fixtures under tests/golden/ were written by tests/golden/make_golden.py with torch on 8 intra-op CPU threads.
# How torch splits a CPU reduction over threads sets its summation order, and the networks amplify that last-bit
# difference about a thousandfold (a whole-network output moves by ~1e-3 relative at 1, 3 or 16 threads), so the CPU
# oracle is compared with a fixture on the fixture's own thread count.
FIXTURE_THREADS = 8


@pytest.fixture
def fixture_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    yield
    torch.set_num_threads(n)


# Guarded views: a clip tensor placed as a channel slice [coff, coff + C) of a wider buffer, with one guard frame before
# and one after it.  Everything outside the view holds a sentinel: NaN around inputs (a kernel that reads outside its
# input turns its result into NaN), a finite, bf16-exact value around outputs (a kernel that writes outside its output
# changes it).  The guards also keep stray accesses inside the test's own allocation.
IN_FILL = float("nan")
OUT_FILL = -1232.0          # exact in bf16 and f32
# Around the logits of an arg-max: `NaN > best` is false, so a NaN guard never shows a read past the last class; a finite
# value above every logit (exact in bf16) wins instead and changes the index.
ARGMAX_FILL = 30720.0       # 15 * 2^11


def guarded(T, H, W, C, dtype, dev, *, coff=0, ld=None, fill=OUT_FILL):
    """-> (buf, view): buf (T + 2, H, W, ld) filled with `fill`; view = buf[1:T + 1, :, :, coff:coff + C]."""
    ld = coff + C if ld is None else ld
    assert coff >= 0 and coff + C <= ld, (coff, C, ld)
    buf = torch.full((T + 2, H, W, ld), fill, dtype=dtype, device=dev)
    return buf, buf[1:T + 1, :, :, coff:coff + C]


def bits(t):
    """Integer view of a tensor's bits (NaN patterns compare as numbers)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def view_mask(buf, view):
    """Boolean mask over buf of the elements of `view` (a [f0:f0 + T, :, :, c0:c0 + C] slice of buf)."""
    assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    off = view.storage_offset() - buf.storage_offset()
    frame = buf.shape[1] * buf.shape[2] * buf.shape[3]
    f0, c0 = off // frame, off % frame
    assert c0 < buf.shape[3] and tuple(view.shape[1:3]) == tuple(buf.shape[1:3])
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    m[f0:f0 + view.shape[0], :, :, c0:c0 + view.shape[3]] = True
    return m


def assert_untouched(buf, before, view=None, what=""):
    """buf is bitwise equal to `before` (its copy taken before the launch) outside `view`; everywhere when view is None."""
    changed = bits(buf) != bits(before)
    if view is not None:
        changed &= ~view_mask(buf, view)
    n = int(changed.sum().item())
    if n:
        idx = changed.nonzero()[0].tolist()
        where = "outside the view" if view is not None else "in a read-only buffer"
        raise AssertionError(f"{what}: {n} element(s) changed {where}, first at {idx}: "
                             f"{before[tuple(idx)].item()!r} -> {buf[tuple(idx)].item()!r}")


def flat_guarded(shape, dtype, dev, fill, src=None, pad=64):
    """A dense tensor of `shape` inside a longer 1-D allocation of `fill`, for entries that take no stride: pad elements
    before and after (a multiple of 16 bytes in every dtype here, so the slice keeps the allocation's alignment).
    -> (buf, dense view, copy of buf taken after `src` was written)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    v = buf[pad:pad + n].view(shape)
    if src is not None:
        v.copy_(src.to(dev, dtype).view(shape))
    return buf, v, buf.clone()


def assert_flat_untouched(buf, before, view=None, what=""):
    """The 1-D allocation is bitwise equal to `before` outside the dense slice `view` (everywhere when view is None)."""
    changed = bits(buf) != bits(before)
    if view is not None:
        o = view.storage_offset() - buf.storage_offset()
        changed[o:o + view.numel()] = False
    n = int(changed.sum().item())
    if n:
        i = int(changed.nonzero()[0].item())
        where = "outside the tensor" if view is not None else "in a read-only buffer"
        raise AssertionError(f"{what}: {n} element(s) changed {where}, first at {i}: {before[i].item()!r} -> {buf[i].item()!r}")


# Exact arithmetic (tests/test_gpu_exact.py, tests/test_exact_cpu.py): on integer-valued data every product and every
# partial sum of a convolution is an integer below 2^24, hence exact in f32 in ANY accumulation order, tile shape, split
# or matrix instruction; the one correct output is the exact value (f32) or its round-to-nearest-even (bf16).
def int_tensor(shape, lo, hi, g):
    """Uniform integers in [lo, hi] as float32 (exact in bf16 for |v| <= 256)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def assert_exact_headroom(abs_sum):
    """abs_sum: the float64 tensor conv(|x|, |w|) + |bias| + |frame_bias| + sum |res| -- a bound on every partial sum in
    every order.  Below 2^24 all of them are integers (or multiples of the data's power-of-two step) that f32 holds exactly."""
    assert abs_sum.dtype == torch.float64
    m = abs_sum.max().item()
    assert m < 2 ** 24, f"partial sums up to {m:.0f} >= 2^24: not exact in f32"
    return m


def assert_bits_equal(got, ref, what="", tile=None):
    """got and ref (same shape and dtype, (T, H, W, C) clip layout when `tile` is given) are equal bit for bit, compared
    through bits().  The sign of a zero is left open: it is no part of the arithmetic contract, and the kernels' two
    spellings of ReLU differ in it (`v > 0 ? v : 0` gives +0, `fmaxf(v, v * 0)` gives -0 for v < 0).
    tile = (rows, cols, couts): also counts the differing elements by (h % rows, w % cols, c % couts), so that a failure
    names the lane, the row or the store group at fault."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    ne = (bits(got) != bits(ref)) & ~((got == 0) & (ref == 0))
    n = int(ne.sum().item())
    if not n:
        return
    idx = ne.nonzero()
    first = tuple(idx[0].tolist())
    d = (got.double() - ref.double()).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    msg = (f"{what}: {n} of {ne.numel()} element(s) differ in bits; first at {list(first)}: got {got[first].item()!r}, "
           f"expected {ref[first].item()!r}; largest |difference| {d[ne].max().item():.6g}")
    if tile is not None and got.dim() == 4:
        msg += tile_histogram(idx, tile)
    raise AssertionError(msg)


def tile_histogram(idx, tile):
    """idx: (n, 4) positions in a (T, H, W, C) clip tensor, tile = (rows, cols, couts) -> the lines that count them by
    (h % rows, w % cols, c % couts)."""
    rows, cols, couts = tile
    key = (idx[:, 1] % rows) * (cols * couts) + (idx[:, 2] % cols) * couts + idx[:, 3] % couts
    cnt = torch.bincount(key, minlength=rows * cols * couts).view(rows, cols, couts)
    msg = (f"\n  by h % {rows}: {cnt.sum((1, 2)).tolist()}\n  by w % {cols}: {cnt.sum((0, 2)).tolist()}"
           f"\n  by c % {couts}: {cnt.sum((0, 1)).tolist()}")
    top = cnt.flatten().argsort(descending=True)[:8].tolist()
    return msg + "\n  most hit (h % rows, w % cols, c % couts): " + ", ".join(
        f"({k // (cols * couts)}, {k // couts % cols}, {k % couts}): {int(cnt.flatten()[k])}" for k in top if cnt.flatten()[k] > 0)


# Attention with a known softmax (tests/test_gpu_attn_exact.py, tests/test_attn_exact_cpu.py).  q, k, v are float32 CPU
# tensors of shape (frames, heads, L, d).  Three families of inputs:
#   selection: the softmax is one-hot (every other probability is below 2^-149: nothing in f32 or bf16), so the one
#              correct output row is a V row, bit for bit;
#   tie:       all real keys of a query score the same bit for bit, so the output is the mean of the V rows (integers:
#              every partial sum is exact) within one unit in the last place;
#   staircase: the running maximum moves (or never moves) from one 32-key tile to the next; compared per element with
#              S = sum_j p_j |v_j|, the magnitude that the roundings of p and of the accumulator act on.
SIGNIFICAND = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
MIN_NORMAL = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}


def round_to(x64, dtype):
    """float64 -> the nearest value of `dtype` (ties to even), still as float64.  One rounding: a cast through float32
    would round twice.  Normal range only."""
    assert x64.dtype == torch.float64
    fin = x64[~torch.isnan(x64)].abs()
    assert bool(((fin == 0) | ((fin >= MIN_NORMAL[dtype]) & (fin <= torch.finfo(dtype).max))).all()), "outside the normal range"
    m, e = torch.frexp(x64)
    p = SIGNIFICAND[dtype]
    return torch.ldexp(torch.round(m * 2.0 ** p), e - p)


def ordered_bits(t):
    """The bits of a float tensor as int64 in the order of the values (sign-magnitude -> two's complement; +0 = -0 = 0):
    neighbouring values differ by 1."""
    b = bits(t).to(torch.int64)
    mag = b & ((1 << (8 * t.element_size() - 1)) - 1)
    return torch.where(b < 0, -mag, mag)


def _hist_32_64(bad):
    """Failing positions of a (F, 1, L, C) clip tensor by query % 32 and channel % 64."""
    if bad.dim() != 4:
        return ""
    idx = bad.nonzero()
    return (f"\n  by query % 32: {torch.bincount(idx[:, 2] % 32, minlength=32).tolist()}"
            f"\n  by channel % 64: {torch.bincount(idx[:, 3] % 64, minlength=64).tolist()}"
            f"\n  by frame: {torch.bincount(idx[:, 0], minlength=bad.shape[0]).tolist()}")


def assert_within_ulps(got, ref64, n, what=""):
    """got (float32, bfloat16 or float16) is within n units in the last place of ref64 rounded to got's type: the distance
    is taken on the ordered integer view of the bits.  NaN on either side fails.  -> the largest distance."""
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape, (what, got.dtype, ref64.dtype, got.shape, ref64.shape)
    got = got.detach().cpu().contiguous()
    want = round_to(ref64.contiguous(), got.dtype).to(got.dtype)
    nan = torch.isnan(got) | torch.isnan(want)
    dist = (ordered_bits(got) - ordered_bits(want)).abs()
    dist = torch.where(nan, torch.full_like(dist, 1 << 40), dist)
    bad = dist > n
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} element(s) more than {n} ulp from the reference "
                             f"({int(nan.sum())} NaN); first at {list(first)}: got {got[first].item()!r}, expected "
                             f"{want[first].item()!r} ({ref64[first].item()!r}); largest distance "
                             f"{int(dist[~nan].max()) if bool((~nan).any()) else 'NaN'} ulp" + _hist_32_64(bad))
    return int(dist.max())


def assert_attn_close(got, ref64, S, bound_rel, what="", ab=0.0):
    """|got - ref64| <= bound_rel * S (+ ab, an absolute rounding floor of the output type) for every element, S =
    sum_j p_j |v_j| of that element (float64).  NaN fails.  -> max((err - ab) / S) / bound_rel."""
    assert ref64.dtype == torch.float64 and S.dtype == torch.float64 and got.shape == ref64.shape == S.shape, what
    err = (got.detach().cpu().double() - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), (err - ab).clamp_min(0.0))
    bad = err > bound_rel * S
    ratio = (err / S.clamp_min(1e-300)).max().item() / bound_rel
    if bool(bad.any()):
        worst = tuple((err / S.clamp_min(1e-300)).flatten().argmax().unsqueeze(0).tolist())
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} element(s) beyond {bound_rel:.3e} * S; largest "
                             f"err / (bound_rel * S) = {ratio:.3f} (flat index {worst[0]}); first at {list(first)}: got "
                             f"{got[first].item()!r}, expected {ref64[first].item()!r}, S {S[first].item():.6g}"
                             + _hist_32_64(bad))
    return ratio


def sign_code(n, d):
    """(n, d) of +-1: the bits of the row index (0 -> -1, 1 -> +1), each repeated d // ceil(log2 n) times, the remaining
    channels +1.  Two rows differ in at least d // ceil(log2 n) channels."""
    nb = max(1, math.ceil(math.log2(n))) if n > 1 else 1
    rep = d // nb
    assert rep >= 1, (n, d)
    code = torch.ones(n, d)
    j = torch.arange(n)
    for b in range(nb):
        code[:, b * rep:(b + 1) * rep] = (((j >> b) & 1).float() * 2 - 1)[:, None]
    return code


MARGIN = 110.0      # natural-log units: exp(-110) < 2^-149, the smallest f32 (and bf16) denormal


def selection_strength(n, d):
    """The smallest power of two A <= 256 at which q = A * code separates the codes of sign_code(n, d) by >= MARGIN after
    the 1/sqrt(d) scale: rows differ in >= rep channels, each worth 2A."""
    if n == 1:
        return 1
    nb = max(1, math.ceil(math.log2(n)))
    for A in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        if 2 * A * (d // nb) / math.sqrt(d) >= MARGIN:
            return A
    raise AssertionError(f"no A <= 256 separates {n} codes of width {d} by {MARGIN}: shorten L")


def _signs(shape, g):
    return torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1


def attn_selection(frames, heads, L, d, g, last=False):
    """-> q, k, v, sel: query i of every (frame, head) selects key sel[i] (a seeded permutation, or L - 1 for all with
    `last`).  k = code * u with a sign vector u per (frame, head), q = A * code[sel] * u, v integers in [-256, 256]."""
    u = _signs((frames, heads, 1, d), g)
    code = sign_code(L, d)
    if last:
        sel = torch.full((frames, heads, L), L - 1, dtype=torch.long)
    else:
        sel = torch.stack([torch.randperm(L, generator=g) for _ in range(frames * heads)]).view(frames, heads, L)
    A = selection_strength(L, d)
    return A * code[sel] * u, (code * u).contiguous(), int_tensor((frames, heads, L, d), -256, 256, g), sel


def attn_tie(frames, heads, L, d, g):
    """-> q, k, v, a: every key of a (frame, head) is the sign vector u, query i is a_i * u with integer levels a_i in
    [-64, 64] (the first three are -64, 0, 64), v integers in [0, 256].  All keys of a query tie at a_i * sqrt(d)."""
    u = _signs((frames, heads, 1, d), g)
    a = torch.randint(-64, 65, (frames, heads, L), generator=g).float()
    a[..., :3] = torch.tensor([-64.0, 0.0, 64.0])[:L]
    return a[..., None] * u, u.expand(frames, heads, L, d).contiguous(), int_tensor((frames, heads, L, d), 0, 256, g), a


STAIRS = ("up", "down", "alt")


def stair_levels(n, d, variant, jitter):
    """g_j = s * step(j // 32) + jitter_j / 8 for n keys, s = round(32 * 3 / sqrt(d)) / 32 (about 3 nats per 32-key tile
    at a = 1).  up: step = tile; down: the reverse (the maximum never moves after tile 0); alt: up on even tiles, down on
    odd ones.  Every level is a multiple of 1/32 below 8: exact in bf16 and fp16."""
    s32 = max(1, round(32 * 3 / math.sqrt(d)))
    tile = torch.arange(n) // 32
    nt = (n + 31) // 32
    step = {"up": tile, "down": nt - 1 - tile, "alt": torch.where(tile % 2 == 0, tile, nt - 1 - tile)}[variant]
    num = s32 * step + 4 * jitter
    assert int(num.max()) < 256, (n, d, int(num.max()))
    return num.float() / 32


def attn_staircase(frames, heads, L, d, g, variant, dtype):
    """-> q, k, v rounded through `dtype`: k_j = g_j * u, q_i = a_i * u with a_i in {1, 2}, v randn."""
    u = _signs((frames, heads, 1, d), g)
    jitter = torch.randint(0, 4, (frames, heads, L), generator=g)
    lev = stair_levels(L, d, variant, jitter)
    a = torch.randint(1, 3, (frames, heads, L), generator=g).float()
    v = torch.randn(frames, heads, L, d, generator=g)
    return rb(a[..., None] * u, dtype), rb(lev[..., None] * u, dtype), rb(v, dtype)


def attn_scores64(q, k, d):
    return q.double() @ k.double().transpose(-1, -2) / math.sqrt(d)


def attn_ref64(q, k, v, extra_key_score=None, scale_error=0.0):
    """float64 softmax attention of (..., L, d) tensors -> (out, S, R): S = sum_j p_j |v_j| per output element, R the
    largest spread of one query's scores in log2 units.  The two arguments emulate kernel faults for the written record of
    tests/test_attn_exact_cpu.py: a phantom key with this score and v = 0, a relative error of the softmax scale."""
    s = attn_scores64(q, k, q.shape[-1]) * (1.0 + scale_error)
    R = (s.max(-1).values - s.min(-1).values).max().item() / math.log(2.0)
    vv = v.double()
    if extra_key_score is not None:
        s = torch.cat([s, torch.full_like(s[..., :1], extra_key_score)], dim=-1)
        vv = torch.cat([vv, torch.zeros_like(vv[..., :1, :])], dim=-2)
    p = torch.softmax(s, dim=-1)
    return p @ vv, p @ vv.abs(), R


def selection_margin(scores, hit):
    """scores (..., n) float64, hit (..., n) bool (the keys a query selects; they must tie exactly): the smallest lead of
    a selected key over the best other key, inf where there is no other."""
    top = torch.where(hit, scores, torch.full_like(scores, float("inf"))).min(-1).values
    assert torch.equal(top, torch.where(hit, scores, torch.full_like(scores, float("-inf"))).max(-1).values), "selected keys differ"
    rest = torch.where(hit, torch.full_like(scores, float("-inf")), scores).max(-1).values
    return (top - rest).min().item()


QKV_LAYOUTS = ("legacy", "new", "vqk")


def pack_qkv(q, k, v, layout, fill=float("nan")):
    """(frames, heads, L, d) x 3 -> ((frames, 1, L, ld) float32, offsets): legacy = per head q | k | v, new = all q | all k |
    all v (the two orders of qkv_attention), vqk = per head v | q | k | 8 channels of `fill` (attention_wide only)."""
    Fr, heads, L, d = q.shape
    if layout == "new":
        x = torch.stack([q, k, v], dim=1)                               # Fr, 3, heads, L, d
        x = x.permute(0, 3, 1, 2, 4).reshape(Fr, 1, L, 3 * heads * d)
        return x.contiguous(), dict(q_off=0, k_off=heads * d, v_off=2 * heads * d, head_stride=d)
    parts = [q, k, v] if layout == "legacy" else [v, q, k, torch.full((Fr, heads, L, 8), fill)]
    x = torch.cat(parts, dim=-1)                                        # Fr, heads, L, 3d (+ 8)
    hs = x.shape[-1]
    x = x.permute(0, 2, 1, 3).reshape(Fr, 1, L, heads * hs)
    off = dict(q_off=0, k_off=d, v_off=2 * d) if layout == "legacy" else dict(q_off=d, k_off=2 * d, v_off=0)
    return x.contiguous(), dict(off, head_stride=hs)


def heads_to_clip(o):
    """(frames, heads, L, d) -> (frames, 1, L, heads * d), the layout of the attention output."""
    Fr, heads, L, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(Fr, 1, L, heads * d).contiguous()


# Temporal window attention: q, k, v (T, P, heads, d) over P pixels, kpos (window - 1, heads, d); slot j of frame t reads
# frame clamp(t + off_j), off = -half .. half without 0.
def window_frames(T, window):
    half = window // 2
    offs = torch.tensor([j for j in range(-half, half + 1) if j != 0])
    return (torch.arange(T).view(T, 1) + offs.view(1, -1)).clamp(0, T - 1)       # (T, n)


def temporal_windows(q, k, v, kpos, window, round_fp16):
    """-> q (T, P, heads, d), kw and vw (T, n, P, heads, d) as the kernel sees them: k + kpos added in f32, then q, k + kpos
    and v rounded through fp16 when round_fp16."""
    idx = window_frames(q.shape[0], window)
    kw = k[idx] + kpos[None, :, None]
    vw = v[idx]
    if round_fp16:
        q, kw, vw = rb(q, torch.float16), rb(kw, torch.float16), rb(vw, torch.float16)
    return q, kw, vw


def temporal_scores64(q, kw):
    return torch.einsum("tphd,tnphd->tphn", q.double(), kw.double()) / math.sqrt(q.shape[-1])


def temporal_ref64(q, k, v, kpos, window, round_fp16=False):
    """float64 reference of the temporal window attention -> (out, S, R) as attn_ref64."""
    q, kw, vw = temporal_windows(q, k, v, kpos, window, round_fp16)
    s = temporal_scores64(q, kw)
    R = (s.max(-1).values - s.min(-1).values).max().item() / math.log(2.0)
    p = torch.softmax(s, dim=-1)
    return (torch.einsum("tphn,tnphd->tphd", p, vw.double()), torch.einsum("tphn,tnphd->tphd", p, vw.double().abs()), R)


def pack_temporal(q, k, v, H, W):
    """(T, P, heads, d) x 3 -> (T, H, W, 3C) float32: q | k | v, channel = head * d + c."""
    T, P, heads, d = q.shape
    assert P == H * W
    return torch.cat([z.reshape(T, H, W, heads * d) for z in (q, k, v)], dim=-1).contiguous()


def temporal_slot_selection(T, P, heads, d, window, g):
    """k = 0, kpos[slot] = the sign code of the slot (rotated by the head), q = A * kpos[sigma] for a seeded slot sigma per
    (t, pixel, head) -> q, k, v, kpos, hit (T, P, heads, n) bool, expected (T, P, heads, d) = v[clamp(t + off_sigma)]."""
    n = window - 1
    code = sign_code(n, d)
    kpos = torch.stack([code[(torch.arange(n) + h) % n] for h in range(heads)], dim=1)      # n, heads, d
    sigma = torch.randint(0, n, (T, P, heads), generator=g)
    q = selection_strength(n, d) * kpos[sigma, torch.arange(heads).view(1, 1, heads)]
    v = int_tensor((T, P, heads, d), -256, 256, g)
    idx = window_frames(T, window)                                                          # T, n
    src = idx.gather(1, sigma.reshape(T, -1)).view(T, P, heads)
    want = v[src, torch.arange(P).view(1, P, 1), torch.arange(heads).view(1, 1, heads)]
    hit = torch.arange(n).view(1, 1, 1, n) == sigma[..., None]
    return q, torch.zeros_like(v), v, kpos, hit, want


def temporal_frame_selection(T, P, heads, d, window, g):
    """kpos = 0, k[t] = the sign code of frame t (times a sign vector per pixel and head), q selects the frame of a seeded
    slot of its window -> q, k, v, kpos, hit (every slot that the clamp sends to that frame), expected = v[that frame]."""
    n = window - 1
    u = _signs((1, P, heads, d), g)
    code = sign_code(T, d)
    k = (code.view(T, 1, 1, d) * u).contiguous()
    sigma = torch.randint(0, n, (T, P, heads), generator=g)
    idx = window_frames(T, window)
    src = idx.gather(1, sigma.reshape(T, -1)).view(T, P, heads)
    q = selection_strength(T, d) * code[src] * u
    v = int_tensor((T, P, heads, d), -256, 256, g)
    want = v[src, torch.arange(P).view(1, P, 1), torch.arange(heads).view(1, 1, heads)]
    hit = idx.view(T, 1, 1, n) == src[..., None]
    return q, k, v, torch.zeros(n, heads, d), hit, want


def temporal_tie(T, P, heads, d, window, g):
    """k = u in every frame, kpos = 0, q = a * u with integer levels a in [-64, 64], v integers in [0, 256] -> q, k, v,
    kpos, the float64 mean over the window's slots of the clamped V rows."""
    n = window - 1
    u = _signs((1, P, heads, d), g)
    a = torch.randint(-64, 65, (T, P, heads), generator=g).float()
    a.view(-1)[:3] = torch.tensor([-64.0, 0.0, 64.0])
    v = int_tensor((T, P, heads, d), 0, 256, g)
    want = v[window_frames(T, window)].double().sum(1) / n
    return a[..., None] * u, u.expand(T, P, heads, d).contiguous(), v, torch.zeros(n, heads, d), want


def temporal_staircase(T, P, heads, d, window, g, dtype):
    """kpos[slot] = g_slot * u with g rising to the middle slots and falling again (about 3 nats per slot at a = 1),
    k = (0, 1 or 2) / 8 * u, q = a * u with a in {1, 2}, v randn; q, k, v rounded through `dtype` (kpos stays f32)."""
    n = window - 1
    u = _signs((1, 1, heads, d), g)
    s32 = max(1, round(32 * 3 / math.sqrt(d)))
    slot = torch.arange(n)
    lev = (s32 * torch.minimum(slot, n - 1 - slot) + 4 * torch.randint(0, 4, (n,), generator=g)).float() / 32
    kpos = lev.view(n, 1, 1) * u[0]
    k = torch.randint(0, 3, (T, P, heads, 1), generator=g).float() / 8 * u
    a = torch.randint(1, 3, (T, P, heads, 1), generator=g).float()
    v = torch.randn(T, P, heads, d, generator=g)
    return rb(a * u, dtype), rb(k, dtype), rb(v, dtype), kpos.contiguous()


# Normalisation kernels on inputs whose statistics are known (tests/test_gpu_norm_exact.py, tests/test_norm_exact_cpu.py).
# x is a float32 CPU clip tensor (T, H, W, C); a statistic spans `fps` consecutive frames and the C / groups channels of a
# group, so the (statistic, group) sets are the [:, :, g, :] slices of x.reshape(T / fps, fps * H * W, groups, C / groups).
U24 = 2.0 ** -24            # unit roundoff of f32
ACT_NONE, ACT_RELU, ACT_LRELU01, ACT_SILU, ACT_LRELU02, ACT_GELU = 0, 1, 2, 3, 5, 6
ACT_LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LRELU01: 1.0, ACT_LRELU02: 1.0, ACT_SILU: 1.1, ACT_GELU: 1.13}



def out_rounding(ref64, dtype):
    """What rounding a value near ref64 to `dtype` may add: nothing for f32 (its roundings are counted in units of 2^-24
    by the callers), half a unit in the last place of ref64 for bf16 -- 2^(e - 8) for 2^e <= |ref| < 2^(e + 1), between
    2^-9 |ref| at the top of a binade and 2^-8 |ref| at its bottom.  (2^-9 |ref| alone is not a bound: the correctly
    rounded 1.1275 is 1.125, off by 2.3 * 2^-9.)"""
    if dtype != torch.bfloat16:
        return torch.zeros_like(ref64)
    _, e = torch.frexp(ref64)                       # |ref| = m * 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(ref64), torch.where(ref64 == 0, torch.full_like(e, -125), e).clamp_min(-125) - 9)


assert_elem_close = assert_attn_close       # |got - ref| <= rel * S (+ ab) per element: nothing in it is about attention


def gn_sets(x, fps, groups):
    """(T, H, W, C) -> (T / fps, fps * H * W, groups, C / groups): a view for contiguous x."""
    T, H, W, C = x.shape
    assert T % fps == 0 and C % groups == 0, (x.shape, fps, groups)
    return x.reshape(T // fps, fps * H * W, groups, C // groups)


def gn_from_sets(s, T, H, W):
    return s.reshape(T, H, W, s.shape[2] * s.shape[3])


def balanced_signs(T, H, W, C, fps, groups, g):
    """+-1, exactly half of each in every (statistic, group), placed by a seeded random permutation per set: mean 0 and
    variance 1 in any summation order, while every proper contiguous sub-range is (almost surely) unbalanced."""
    ns, n, cpg = T // fps, fps * H * W, C // groups
    cnt = n * cpg
    assert cnt % 2 == 0, (T, H, W, C, fps, groups)
    order = torch.rand(ns, groups, cnt, generator=g).argsort(-1)
    s = torch.ones(ns, groups, cnt)
    s.scatter_(-1, order[..., :cnt // 2], -1.0)
    return gn_from_sets(s.view(ns, groups, n, cpg).permute(0, 2, 1, 3), T, H, W).contiguous()


def pow2_affine(C, g):
    """gamma = +-1, +-2 or +-4; beta = -gamma on even channels and +gamma on odd ones: gamma * (+-1) + beta is 0 or
    +-2 gamma."""
    gamma = (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1) * 2.0 ** torch.randint(0, 3, (C,), generator=g).float()
    return gamma, torch.where(torch.arange(C) % 2 == 0, -gamma, gamma)


def exact_film(T, C, ld, g):
    """(T, ld) float32 rows scale[C] | shift[C] | NaN padding: scale in {0, 1, -0.5, 3}, shift an integer in [-3, 3]."""
    assert ld >= 2 * C
    film = torch.full((T, ld), float("nan"))
    film[:, :C] = torch.tensor([0.0, 1.0, -0.5, 3.0])[torch.randint(0, 4, (T, C), generator=g)]
    film[:, C:2 * C] = torch.randint(-3, 4, (T, C), generator=g).float()
    return film


def spiked_ints(T, H, W, C, fps, groups, g):
    """Integers in [-3, 3] and, in every (statistic, group), one element of 64 at a pixel, channel and frame of its own:
    the first and the last pixel of the statistic for the first two groups, the last pixel of the first frame and the first
    pixel of the last frame for the next two, seeded positions for the rest.  -> x, positions (ns, groups) in the set."""
    ns, n, cpg = T // fps, fps * H * W, C // groups
    s = torch.randint(-3, 4, (ns, n, groups, cpg), generator=g).float()
    pix = torch.randint(0, n, (ns, groups), generator=g)
    edge = [0, n - 1, H * W - 1, n - H * W]
    for j in range(min(groups, 4)):
        pix[:, j] = edge[j]
    ch = torch.randint(0, cpg, (ns, groups), generator=g)
    s[torch.arange(ns)[:, None], pix, torch.arange(groups)[None, :], ch] = 64.0
    return gn_from_sets(s, T, H, W).contiguous(), pix * cpg + ch


def act64(v, act):
    """The activations of apply_act in float64 (the leaky slopes are the f32 constants of the kernels)."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act in (ACT_LRELU01, ACT_LRELU02):
        slope = torch.tensor(0.1 if act == ACT_LRELU01 else 0.2, dtype=torch.float32).double().item()
        return torch.where(v > 0, v, slope * v)
    if act == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    raise ValueError(act)


def gn_ref64(x, gamma, beta, fps, groups, eps, film=None):
    """GroupNorm (+ FiLM) before the activation, written out in float64 -> dict of (T, H, W, C) float64 tensors:
      pre   ((x - mean) * rstd * gamma + beta) * (1 + scale) + shift
      S     ((|x| + |mean|) * rstd * |gamma| + |beta|) * |1 + scale| + |shift|: what the f32 roundings of the fold act on
      slope (x - mean) * rstd * gamma * (1 + scale): the part of pre that is proportional to rstd
    and mean, var, rstd, ex2 = E[x^2] of the element's (statistic, group)."""
    T, H, W, C = x.shape
    s = gn_sets(x.double(), fps, groups)
    mean = s.mean((1, 3), keepdim=True)
    var = (s - mean).pow(2).mean((1, 3), keepdim=True)
    ex2 = s.pow(2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    full = lambda t: gn_from_sets(t.expand_as(s), T, H, W)
    mean, var, ex2, rstd = full(mean), full(var), full(ex2), full(rstd)
    ga, be = gamma.double(), beta.double()
    if film is not None:
        m = 1.0 + film[:, None, None, :C].double()
        sh = film[:, None, None, C:2 * C].double()
    else:
        m, sh = torch.ones(1, 1, 1, 1, dtype=torch.float64), torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    xd = x.double()
    slope = (xd - mean) * rstd * ga * m
    return dict(pre=slope + be * m + sh, S=((xd.abs() + mean.abs()) * rstd * ga.abs() + be.abs()) * m.abs() + sh.abs(),
                slope=slope, mean=mean, var=var, rstd=rstd, ex2=ex2)


def pool2(t):
    """2x2 mean of a (T, H, W, C) tensor."""
    T, H, W, C = t.shape
    return t.reshape(T, H // 2, 2, W // 2, 2, C).mean((2, 4))


def up2(t):
    """Nearest x2 of a (T, H, W, C) tensor."""
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


def resample_ref(t, mode):
    return t if mode == 0 else (pool2(t) if mode == 1 else up2(t))


def layernorm_ref64(x, gamma, beta, eps):
    """nn.LayerNorm over the last axis in float64 -> (y, S), S = (|x| + |mean|) * rstd * |gamma| + |beta|."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xd - mean).pow(2).mean(-1, keepdim=True) + eps)
    return ((xd - mean) * rstd * gamma.double() + beta.double(),
            (xd.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs())


def adain_ref64(content, style, eps):
    """adaptive_instance_normalization on (F, H, W, C) in float64 with the unbiased variance + eps -> (y, S),
    S = (|c| + |mean_c|) * std_s / std_c + |mean_s|."""
    c, s = content.double(), style.double()
    mc, ms = c.mean((1, 2), keepdim=True), s.mean((1, 2), keepdim=True)
    sc = torch.sqrt(c.var((1, 2), unbiased=True, keepdim=True) + eps)
    ss = torch.sqrt(s.var((1, 2), unbiased=True, keepdim=True) + eps)
    return (c - mc) / sc * ss + ms, (c.abs() + mc.abs()) / sc * ss + ms.abs()


def gn_fold_f32(x, mean64, var64, gamma, beta, eps, film=None):
    """The arithmetic of the GroupNorm kernels after their f64 statistics, step by step in float32 on the CPU: mean and
    1 / sqrt(var + eps) cast to f32, A = gamma * rstd, B = beta - mean * A, the FiLM step, y = fma(x, A, B).  mean64 and
    var64 are (T, H, W, C)-broadcastable float64 tensors, so a test can hand in faulty statistics.  -> float32 (T, H, W, C)
    before the activation (the fma is emulated in float64 and rounded once)."""
    C = x.shape[3]
    mean = mean64.float()
    rstd = (1.0 / torch.sqrt(var64.clamp_min(0.0) + eps)).float()
    A = gamma.float() * rstd
    B = beta.float() - mean * A
    if film is not None:
        m = 1.0 + film[:, None, None, :C]
        A = A * m
        B = (B.double() * m.double() + film[:, None, None, C:2 * C].double()).float()
    return (x.double() * A.double() + B.double()).float()


# Activation epilogues on an exact pre-activation (tests/test_gpu_act_exact.py, tests/test_act_exact_cpu.py).  v is a float64
# tensor whose last axis is the output channel; co is the channel index along that axis.
ACT_DCN_OFFSETS = 4
ACT_FLOOR = 2.0 ** -120     # a few f32 denormal steps: what an underflowing tail may leave


def dcn_is_residue(co, period):
    """The class map of FLAIR_ACT_DCN_OFFSETS in the tap-major channel order: of every `period` = 3 G channels the first
    2 G are residues (mag * tanh), the last G masks (sigmoid)."""
    return 3 * (co % period) < 2 * period


def dcn_act64(v, co, mag, period):
    assert v.dtype == torch.float64 and v.shape[-1] == co.numel()
    return torch.where(dcn_is_residue(co, period), mag * torch.tanh(v), torch.sigmoid(v))


def act_sens64(v, act, co=None, mag=10.0, period=48):
    """S of |got - act(v)| <= k 2^-24 S: the magnitude that the f32 roundings of the formula act on, in float64.
    |a| + |v a'(v)| (the value, and what a relative error of the exponential's argument does to it), plus the cancellation
    term of the formula where it has one: GELU = 0.5 v (1 + erf) carries 0.5 |v| (1 + |erf|) in place of |a|, and
    mag tanh = mag (1 - 2 r) carries mag (1 - tanh) beside mag |tanh|."""
    assert v.dtype == torch.float64
    if act == ACT_SILU:
        s = torch.sigmoid(v)
        return (v * s).abs() + (v * (s + v * s * (1 - s))).abs()
    if act == ACT_GELU:
        erf = torch.erf(v * 0.7071067811865476)
        da = 0.5 * (1 + erf) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327
        return 0.5 * v.abs() * (1 + erf.abs()) + (v * da).abs()
    if act == ACT_DCN_OFFSETS:
        t, s = torch.tanh(v), torch.sigmoid(v)
        return torch.where(dcn_is_residue(co, period), mag * (t.abs() + (1 - t) + (v * (1 - t * t)).abs()),
                           s + (v * s * (1 - s)).abs())
    raise ValueError(act)


def assert_act_close(got, ref64, S, k, dtype, what="", tile=None, extra=None):
    """|got - ref64| <= k 2^-24 S + out_rounding(ref64, dtype) + ACT_FLOOR (+ extra, the roundings of what follows the
    activation) for every element; NaN and Inf fail.  On failure the message counts the failing elements by tile position
    like assert_bits_equal.  -> the largest (err - those terms) / (2^-24 S)."""
    ab = out_rounding(ref64, dtype) + ACT_FLOOR
    if extra is not None:
        ab = ab + extra
    try:
        return k * assert_elem_close(got, ref64, S, k * U24, what, ab=ab)
    except AssertionError as e:
        if tile is None or ref64.dim() != 4:
            raise
        err = (got.detach().cpu().double() - ref64).abs()
        bad = ~(err - ab <= k * U24 * S)
        raise AssertionError(str(e) + tile_histogram(bad.nonzero(), tile)) from None
