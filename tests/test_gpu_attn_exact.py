"""The four attention implementations on inputs whose softmax is known exactly: flair_qkv_attention's native bf16 MFMA
kernel (d = 32 / 64 / 128, NW = 2 and 4), its split-channel MFMA kernel (d = 192 ... 1024, three (NW, CPW) builds), its two
f32 row kernels, flair_attention_wide and flair_temporal_attention.

The tolerance tests of this family (test_gpu_kernels, test_gpu_attn_widths, test_gpu_attn_wide_heads,
test_gpu_prior_strides) bound max|err| by a multiple of max|ref| on randn data; a typical output there is ten times
smaller than max|ref|, and a phantom key beyond L, or a softmax scale off by 1 %, stays below every one of those bounds
(tests/test_attn_exact_cpu.py keeps the figures).  Here:
  * selection: the softmax is one-hot with a lead of >= 110 nats (asserted in float64 for every query), so every other
    probability is below 2^-149 and the output is one V row: assert_bits_equal;
  * tie: all real keys of a query tie bit for bit at a level between -64 sqrt(d) and +64 sqrt(d), so the output is the
    mean of integer V rows: within 1 ulp of the output type.  At a negative level a phantom key with score 0 outweighs all
    real keys and the output collapses to about 0 instead of about 128;
  * staircase: the maximum moves in every 32-key tile (up), never after the first (down: the ballot-skip path) or on
    alternate tiles (alt); judged per element against S = sum_j p_j |v_j|:
      bf16: P is rounded to bf16 while l sums the unrounded p, the output is rounded once more: 3 * 2^-9 * S;
      f32:  (L + 2d + 4R) * 2^-24 * S: L roundings of acc * alpha + p * v, 2d for the dot product, R = the spread of a
            query's scores in log2 units for __expf's argument product (alpha and p, twice each);
      round_fp16 (temporal, f32): the f32 bound + 2^-11 for the fp16 output, + 2^-25 absolute: below 2^-14 the fp16
            values are 2^-24 apart, so an output there is rounded by up to half of that whatever its size.
With round_fp16 the kernel leaves fp16 values in an f32 tensor: bits and ulps are then those of fp16.
Shapes are the smallest at which each code path exists; test_cases_reach_every_attention_build recomputes the launchers'
selection rules and checks that every build gets a selection, a tie and a staircase case.  Measured err / bound go to
parity_log."""
import functools

import pytest
import torch

from tests.util import (MARGIN, QKV_LAYOUTS, STAIRS, assert_attn_close, assert_bits_equal, assert_within_ulps, attn_ref64,
                        attn_scores64, attn_selection, attn_staircase, attn_tie, heads_to_clip, pack_qkv, pack_temporal,
                        parity_log, selection_margin, temporal_frame_selection, temporal_ref64, temporal_scores64,
                        temporal_slot_selection, temporal_staircase, temporal_tie, temporal_windows)

FP, BF = torch.float32, torch.bfloat16
KINDS = ("selection", "tie", "staircase")
BF16_REL = 3 * 2.0 ** -9
FP16_REL = 2.0 ** -11
FP16_AB = 2.0 ** -25         # half the spacing of the fp16 subnormals: rounding an output below 2^-14 through fp16


def f32_rel(L, d, R):
    return (L + 2 * d + 4 * R) * 2.0 ** -24


def _ops():
    from flair_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ case table
# (family, d, ((frames, heads), ...), L, dtype).  Families: native = flair_qkv_attention at d = 32 / 64 / 128, wide = the
# same entry at d = 64 * nc, prior = flair_attention_wide (through qkv_attention at d = 40 and 96 and directly with
# interleaved offsets).
def _spatial_cases():
    cases = []
    for d in (32, 64, 128):
        # single key; last tile masked at each half; odd and even tile counts of the two-tile unrolled loop; odd L for
        # d = 32 f32 (two queries per wave)
        for L in (1, 31, 33, 65, 97, 130):
            for dt in (FP, BF):
                cases.append(("native", d, ((1, 2),), L, dt))
        # ceil(L / 128) * frames * heads >= 256: 128-query workgroups with a nearly empty last block; 7 KV tiles at d = 64
        cases.append(("native", d, ((16, 8),), 130, BF))
        cases.append(("native", d, ((8, 8),), 400, BF))
    for d in (192, 320, 512, 576, 1024):          # nc = 3, 5, 8, 9, 16
        for L in (1, 33, 100):                    # row clamping to L - 1; cross-wave exchange parity
            for dt in (FP, BF):
                cases.append(("wide", d, ((2, 1), (1, 2)), L, dt))
    for d in (40, 96):
        for L in (1, 15, 17, 35, 300):            # 16-query tile tail; more than 256 keys per thread loop
            for dt in (FP, BF):
                cases.append(("prior", d, ((2, 3),), L, dt))
    return cases


SPATIAL = _spatial_cases()


def _id(case):
    fam, d, shapes, L, dt = case
    return f"{fam}-d{d}-L{L}-{'x'.join(f'{f}.{h}' for f, h in shapes)}-{str(dt)[6:]}"


def spatial_build(case, frames, heads):
    """The kernel build that the launchers of attn.hip / prior.hip pick for a case (their selection rules, restated)."""
    fam, d, _, L, dt = case
    if fam == "prior":
        assert d not in (32, 64, 128) and not (d % 64 == 0 and 192 <= d <= 1024) and d % 8 == 0 and d + L <= 2048
        return ("attn_wide_kernel", dt)
    if fam == "native":
        assert d in (32, 64, 128)
        if dt == FP:
            return ("attn_rowwise_kernel", d)
        wg128 = (L + 127) // 128 * frames * heads
        return ("attn_mfma_bf16_v2_kernel", 4 if wg128 >= 256 else 2, d)
    assert d % 64 == 0 and 192 <= d <= 1024
    if dt == FP:
        return ("attn_rowwise_wide_kernel",)
    nc = d // 64
    return ("attn_mfma_bf16_wide_kernel",) + ((4, 1) if nc <= 4 else (4, 2) if nc <= 8 else (8, 2))


SPATIAL_BUILDS = ({("attn_wide_kernel", dt) for dt in (FP, BF)} | {("attn_rowwise_kernel", d) for d in (32, 64, 128)}
                  | {("attn_mfma_bf16_v2_kernel", nw, d) for nw in (2, 4) for d in (32, 64, 128)}
                  | {("attn_rowwise_wide_kernel",)}
                  | {("attn_mfma_bf16_wide_kernel", 4, 1), ("attn_mfma_bf16_wide_kernel", 4, 2), ("attn_mfma_bf16_wide_kernel", 8, 2)})

# temporal: d -> G = d / 8 rounded up to a power of two, MASKED when d < 8 G.  The first five widths (G = 1 ... 32, masked
# and unmasked groups) run every T and window; the others complete the set of builds at one T and one window.
TEMPORAL_D = (8, 24, 64, 96, 256)
TEMPORAL_D_MORE = (16, 32, 40, 128, 200)
TEMPORAL_T = (1, 2, 3, 6)                         # T smaller than the window: every slot clamps
TEMPORAL_WINDOWS = (3, 5, 7)
TEMPORAL_HW, TEMPORAL_HEADS = (3, 5), 2
TEMPORAL_MODES = ("float32", "float32-fp16", "bfloat16")


def temporal_build(d, mode):
    n = d // 8
    G = next(g for g in (1, 2, 4, 8, 16, 32) if n <= g)
    return ("temporal_attn_kernel", BF if mode == "bfloat16" else FP, G, d != 8 * G)


TEMPORAL_BUILDS = {("temporal_attn_kernel", dt, G, masked) for dt in (FP, BF)
                   for G, masked in ((1, False), (2, False), (4, False), (8, False), (16, False), (32, False),
                                     (4, True), (8, True), (16, True), (32, True))}     # d = 8 G, or 4 G < d < 8 G


def temporal_shapes(d):
    if d in TEMPORAL_D:
        return [(T, w) for T in TEMPORAL_T for w in TEMPORAL_WINDOWS]
    return [(3, 5)]


@pytest.mark.gpu
def test_cases_reach_every_attention_build():
    """Needs no device (tests/test_attn_exact_cpu.py runs it too): the case table, through the launchers' selection rules, reaches every build of every attention kernel with
    a selection, a tie and a staircase case (each test below runs all cases of its kind), the wide MFMA builds with the
    last chunk of a wave both owned and not owned."""
    reached = {}
    for case in SPATIAL:
        for frames, heads in case[2]:
            reached.setdefault(spatial_build(case, frames, heads), set()).update(KINDS)
    assert set(reached) == SPATIAL_BUILDS, set(reached) ^ SPATIAL_BUILDS
    assert all(kinds == set(KINDS) for kinds in reached.values())
    owned = {}
    for case in SPATIAL:
        if case[0] == "wide" and case[4] == BF:
            b = spatial_build(case, *case[2][0])
            owned.setdefault(b, set()).add(case[1] // 64 == b[1] * b[2])       # every wave owns all of its CPW chunks
    assert owned[("attn_mfma_bf16_wide_kernel", 4, 1)] == {False}          # nc = 3 (nc = 4 is d = 256: every wave owns)
    assert owned[("attn_mfma_bf16_wide_kernel", 4, 2)] == {False, True}    # nc = 5, 8
    assert owned[("attn_mfma_bf16_wide_kernel", 8, 2)] == {False, True}    # nc = 9, 16
    treached = {temporal_build(d, mode) for d in TEMPORAL_D + TEMPORAL_D_MORE for mode in TEMPORAL_MODES}
    assert treached == TEMPORAL_BUILDS, treached ^ TEMPORAL_BUILDS
    assert {temporal_build(d, "float32")[2:] for d in TEMPORAL_D} == {(1, False), (4, True), (8, False), (16, True), (32, False)}
    assert min(TEMPORAL_T) == 1 and min(TEMPORAL_WINDOWS) == 3          # one frame: every slot of every window clamps


# ------------------------------------------------------------------------------------------------ spatial inputs
def _seed(case, frames, heads, salt):
    fam, d, _, L, dt = case
    return (d * 1009 + L * 31 + frames * 7 + heads) * 10 + salt


@functools.lru_cache(maxsize=None)
def selection_case(fam, d, frames, heads, L, last):
    """-> q, k, v, expected (frames, heads, L, d), margin; shared by both dtypes (every value is exact in bf16)."""
    g = torch.Generator().manual_seed(_seed((fam, d, None, L, None), frames, heads, 1 + last))
    q, k, v, sel = attn_selection(frames, heads, L, d, g, last=last)
    hit = torch.arange(L).view(1, 1, 1, L) == sel[..., None]
    margin = selection_margin(attn_scores64(q, k, d), hit)
    want = v.gather(2, sel[..., None].expand(-1, -1, -1, d))
    return q, k, v, want, margin


@functools.lru_cache(maxsize=None)
def tie_case(fam, d, frames, heads, L):
    g = torch.Generator().manual_seed(_seed((fam, d, None, L, None), frames, heads, 3))
    q, k, v, a = attn_tie(frames, heads, L, d, g)
    want = (v.double().sum(2, keepdim=True) / L).expand(-1, -1, L, -1).contiguous()
    return q, k, v, want, a


@functools.lru_cache(maxsize=None)
def staircase_case(fam, d, frames, heads, L, variant, dt):
    g = torch.Generator().manual_seed(_seed((fam, d, None, L, None), frames, heads, 4 + STAIRS.index(variant)))
    q, k, v = attn_staircase(frames, heads, L, d, g, variant, dt)
    ref, S, R = attn_ref64(q, k, v)
    return q, k, v, ref, S, R


def layouts_of(fam):
    """qkv_attention in both orders; the prior family also directly through attention_wide with interleaved offsets."""
    return QKV_LAYOUTS if fam == "prior" else QKV_LAYOUTS[:2]


def run_spatial(q, k, v, layout, dt, dev):
    """-> the output as (frames, 1, L, heads * d) on the CPU, in dtype dt."""
    Fr, heads, L, d = q.shape
    x, off = pack_qkv(q, k, v, layout)
    x = x.to(device=dev, dtype=dt)
    if layout == "vqk":
        y = _ops().attention_wide(x, heads, d, **off)
    else:
        y = _ops().qkv_attention(x, heads, new_order=(layout == "new"))
    torch.cuda.synchronize()
    assert y.dtype == dt and tuple(y.shape) == (Fr, 1, L, heads * d)
    return y.cpu()


# ------------------------------------------------------------------------------------------------ spatial tests
@pytest.mark.gpu
@pytest.mark.parametrize("case", SPATIAL, ids=_id)
def test_selection_returns_the_selected_v_row_bit_for_bit(dev, case):
    fam, d, shapes, L, dt = case
    for frames, heads in shapes:
        for last in (False, True):
            q, k, v, want, margin = selection_case(fam, d, frames, heads, L, last)
            assert margin >= MARGIN, (case, margin)
            for layout in layouts_of(fam):
                got = run_spatial(q, k, v, layout, dt, dev)
                assert_bits_equal(got, heads_to_clip(want).to(dt),
                                  f"selection {_id(case)} {frames}x{heads} {layout} {'last key' if last else 'permutation'}",
                                  tile=(1, 32, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPATIAL, ids=_id)
def test_tie_returns_the_mean_of_the_v_rows_within_one_ulp(dev, case):
    fam, d, shapes, L, dt = case
    for frames, heads in shapes:
        q, k, v, want, _ = tie_case(fam, d, frames, heads, L)
        for layout in layouts_of(fam):
            got = run_spatial(q, k, v, layout, dt, dev)
            assert_within_ulps(got, heads_to_clip(want), 1, f"tie {_id(case)} {frames}x{heads} {layout}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPATIAL, ids=_id)
def test_staircase_per_element(dev, case):
    fam, d, shapes, L, dt = case
    worst = 0.0
    for frames, heads in shapes:
        for variant in STAIRS:
            q, k, v, ref, S, R = staircase_case(fam, d, frames, heads, L, variant, dt)
            rel = BF16_REL if dt == BF else f32_rel(L, d, R)
            for layout in layouts_of(fam):
                got = run_spatial(q, k, v, layout, dt, dev)
                what = f"staircase {_id(case)} {frames}x{heads} {variant} {layout}"
                try:
                    ratio = assert_attn_close(got, heads_to_clip(ref), heads_to_clip(S), rel, what)
                except AssertionError:
                    parity_log(f"attn_exact {what}: FAILED (bound_rel {rel:.3e}, R {R:.1f})")
                    raise
                worst = max(worst, ratio)
    parity_log(f"attn_exact staircase {_id(case)}: max(err / S) / bound_rel = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ temporal
def run_temporal(q, k, v, kpos, window, mode, dev):
    """-> (T, P, heads, d) on the CPU in the kernel's dtype."""
    T, P, heads, d = q.shape
    H, W = TEMPORAL_HW
    dt = BF if mode == "bfloat16" else FP
    x = pack_temporal(q, k, v, H, W).to(device=dev, dtype=dt)
    y = _ops().temporal_attention(x, kpos.reshape(window - 1, heads * d).to(dev), window,
                                  round_fp16=(mode == "float32-fp16"), head_dim=d)
    torch.cuda.synchronize()
    assert y.dtype == dt and tuple(y.shape) == (T, H, W, heads * d)
    return y.cpu().view(T, P, heads, d)


def out_type(got, mode):
    """The kernel's output in the type it was rounded to: round_fp16 leaves fp16 values in an f32 tensor."""
    if mode != "float32-fp16":
        return got
    assert torch.equal(got.half().float(), got), "round_fp16 output is not fp16-representable"
    return got.half()


def _tseed(d, T, window, salt):
    return (d * 101 + T * 11 + window) * 10 + salt


TEMPORAL_PARAMS = [(d, mode) for d in TEMPORAL_D + TEMPORAL_D_MORE for mode in TEMPORAL_MODES]
TEMPORAL_IDS = [f"d{d}-{mode}" for d, mode in TEMPORAL_PARAMS]
P_ = TEMPORAL_HW[0] * TEMPORAL_HW[1]


@functools.lru_cache(maxsize=None)
def temporal_selection_case(kind, d, T, window):
    g = torch.Generator().manual_seed(_tseed(d, T, window, 1 if kind == "slot" else 2))
    build = temporal_slot_selection if kind == "slot" else temporal_frame_selection
    q, k, v, kpos, hit, want = build(T, P_, TEMPORAL_HEADS, d, window, g)
    margins = []
    for fp16 in (False, True):         # every value is exact in fp16, so both modes see the same scores
        qq, kw, _ = temporal_windows(q, k, v, kpos, window, fp16)
        margins.append(selection_margin(temporal_scores64(qq, kw), hit))
    return q, k, v, kpos, hit, want, min(margins)


@pytest.mark.gpu
@pytest.mark.parametrize("d,mode", TEMPORAL_PARAMS, ids=TEMPORAL_IDS)
def test_temporal_slot_selection_bit_for_bit(dev, d, mode):
    for T, window in temporal_shapes(d):
        q, k, v, kpos, hit, want, margin = temporal_selection_case("slot", d, T, window)
        assert margin >= MARGIN and bool((hit.sum(-1) == 1).all()), (d, T, window, margin)
        got = out_type(run_temporal(q, k, v, kpos, window, mode, dev), mode)
        assert_bits_equal(got, want.to(got.dtype), f"temporal slot selection d={d} T={T} window={window} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("d,mode", TEMPORAL_PARAMS, ids=TEMPORAL_IDS)
def test_temporal_frame_selection(dev, d, mode):
    """Bit for bit where one slot reaches the selected frame; within 1 ulp where the clamp sends several slots to it
    (m v * (1 / m) is not exact for m = 3, 5, 6)."""
    for T, window in temporal_shapes(d):
        q, k, v, kpos, hit, want, margin = temporal_selection_case("frame", d, T, window)
        assert margin >= MARGIN and bool((hit.sum(-1) >= 1).all()), (d, T, window, margin)
        got = out_type(run_temporal(q, k, v, kpos, window, mode, dev), mode)
        what = f"temporal frame selection d={d} T={T} window={window} {mode}"
        assert_within_ulps(got, want.double(), 1, what)
        single = (hit.sum(-1) == 1)[..., None].expand_as(want)
        assert_bits_equal(torch.where(single, got, want.to(got.dtype)), want.to(got.dtype), what + " (one slot)")


@pytest.mark.gpu
@pytest.mark.parametrize("d,mode", TEMPORAL_PARAMS, ids=TEMPORAL_IDS)
def test_temporal_tie_within_one_ulp(dev, d, mode):
    for T, window in temporal_shapes(d):
        g = torch.Generator().manual_seed(_tseed(d, T, window, 3))
        q, k, v, kpos, want = temporal_tie(T, P_, TEMPORAL_HEADS, d, window, g)
        got = out_type(run_temporal(q, k, v, kpos, window, mode, dev), mode)
        assert_within_ulps(got, want, 1, f"temporal tie d={d} T={T} window={window} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("d,mode", TEMPORAL_PARAMS, ids=TEMPORAL_IDS)
def test_temporal_staircase_per_element(dev, d, mode):
    worst = 0.0
    for T, window in temporal_shapes(d):
        g = torch.Generator().manual_seed(_tseed(d, T, window, 4))
        q, k, v, kpos = temporal_staircase(T, P_, TEMPORAL_HEADS, d, window, g, BF if mode == "bfloat16" else FP)
        ref, S, R = temporal_ref64(q, k, v, kpos, window, round_fp16=(mode == "float32-fp16"))
        rel = BF16_REL if mode == "bfloat16" else f32_rel(window - 1, d, R) + (FP16_REL if mode == "float32-fp16" else 0.0)
        got = run_temporal(q, k, v, kpos, window, mode, dev)
        what = f"temporal staircase d={d} T={T} window={window} {mode}"
        try:
            worst = max(worst, assert_attn_close(got, ref, S, rel, what, ab=FP16_AB if mode == "float32-fp16" else 0.0))
        except AssertionError:
            parity_log(f"attn_exact {what}: FAILED (bound_rel {rel:.3e}, R {R:.1f})")
            raise
    parity_log(f"attn_exact temporal staircase d={d} {mode}: max(err / S) / bound_rel = {worst:.3f}")
