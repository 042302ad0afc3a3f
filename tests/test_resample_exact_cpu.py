"""The inputs and bounds of tests/test_gpu_resample_exact.py, proved without a GPU:

  * the f32 reference on the CPU (oracle.thirdparty.flow_warp, F.interpolate, F.avg_pool2d) stays within the bound that the
    kernels get of the float64 closed forms of tests/resample_ref.py, on every case the GPU tests use: the closed forms are
    the reference's semantics, and the bound is not too tight for a correct f32 implementation;
  * the flows keep most samples in or on the edge of the frame (a test on zeros sees nothing), and the pinned landings are
    where they should be;
  * every mutant of a closed form -- a plausible kernel bug -- exceeds the bound on some element of every case that covers
    it, so the GPU tests would fail on a kernel with that bug.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import resample_ref as R
from tests.util import round_to

BF, FP = torch.bfloat16, torch.float32
SMALL = R.WARP_CASES
ALL_WARP = R.WARP_CASES + [R.BIG_WARP]
ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def clip(t):
    return t.permute(0, 2, 3, 1).contiguous()


def oracle_warp(x, flow, border):
    from oracle.thirdparty import flow_warp
    return clip(flow_warp(nchw(x), flow, padding_mode="border" if border else "zeros"))


# ----------------------------------------------------------------------------------------------- reference checks
@pytest.mark.parametrize("border", [False, True], ids=["zeros", "border"])
@pytest.mark.parametrize("case", ALL_WARP, ids=ids)
def test_warp_reference_within_bound(case, border):
    H, W, C = case
    d = R.warp_case(H, W, C)
    ref = R.warp_ref64(d["x"], d["flow"], border)
    r = R.assert_within(oracle_warp(d["x"], d["flow"], border), ref, FP, max(H, W), f"flow_warp f32 reference {case}")
    print(f"f32 reference / bound, warp {case} border={border}: {r:.3f}")
    R.assert_within(oracle_warp(d["x2"], d["flow2"], border), R.warp_ref64(d["x2"], d["flow2"], border), FP, max(H, W),
                    f"flow_warp f32 reference {case}, second field")
    # quarter-pixel flows on integers: the exact result is a bf16 number, so the bf16 bound is the coordinate term alone
    assert torch.equal(round_to(ref, BF), ref)


@pytest.mark.parametrize("case", ALL_WARP, ids=ids)
def test_prep_reference_within_bound(case):
    H, W, C = case
    d = R.warp_case(H, W, C)
    m = max(H, W)
    f2_32 = d["flow"] + oracle_warp(d["flow_prev"], d["flow"], False)
    ref = R.prep_ref64(d["x"], d["x2"], d["flow"], d["flow_prev"], FP, flow2=f2_32)
    # the composed flow samples flow_prev, whose neighbours differ by at most DP: the same bound with DP in the place of D
    R.assert_within(f2_32, ref["flow2"], FP, m * R.DP / R.D, f"flow2 f32 reference {case}")
    R.assert_within(oracle_warp(d["x2"], f2_32, False), ref["cond2"], FP, m, f"cond2 f32 reference {case}")


@pytest.mark.parametrize("hw", [c[:2] for c in SMALL] + [R.BIG_COMPOSE], ids=ids)
def test_compose_reference_within_bound(hw):
    H, W = hw
    d = R.compose_case(H, W)
    got = d["f1"] + oracle_warp(d["f2"], d["f1"], False)
    # the f32 sum f1 + warp rounds on |f1| + 8 <= m + 11 where the warp is not 0 (a flow far outside adds exactly 0): a
    # hundredth of the bound
    R.assert_within(got, R.compose_ref64(d["f1"], d["f2"]), FP, max(H, W), f"flow_compose f32 reference {hw}")


def interp32(x, size, mode):
    xn = nchw(x)
    if mode == 0:
        y = F.interpolate(xn, size=size, mode="bilinear", align_corners=False)
    elif mode == 1:
        y = F.interpolate(xn, size=size, mode="bilinear", align_corners=True)
    elif mode == 2:
        y = F.interpolate(xn, size=size, mode="bicubic", align_corners=False)
    elif mode == 3:
        y = F.avg_pool2d(xn, 2, 2)
    else:
        y = F.interpolate(xn, size=size, mode="nearest")
    return clip(y)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resize_reference_within_bound(mode):
    worst = 0.0
    for hi in R.RESIZE_IN:
        for ho in R.RESIZE_OUT:
            x = R.resize_source(R.RESIZE_FRAMES, *hi, 3)
            ref = R.resize_ref64(x, ho, mode)
            worst = max(worst, R.assert_within(interp32(x, ho, mode), ref, FP, R.resize_extent(hi, ho),
                                               f"F.interpolate mode {mode} {hi}->{ho}"))
    print(f"f32 reference / bound, resize mode {mode}: {worst:.3f}")


def test_resize_vec_avgpool_and_big_references_within_bound():
    for hi, ho in R.VEC_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, 32)
        R.assert_within(interp32(x, ho, 0), R.resize_ref64(x, ho, 0), FP, R.resize_extent(hi, ho), f"vec {hi}->{ho}")
    for ho in R.RESIZE_OUT:
        hi = (2 * ho[0], 2 * ho[1])
        x = R.resize_source(R.RESIZE_FRAMES, *hi, 3)
        ref = R.resize_ref64(x, ho, 3)
        assert torch.equal(interp32(x, ho, 3).double(), ref) and torch.equal(round_to(ref, BF), ref)   # quarters below 16
    for hi, ho, C in (R.BIG_RESIZE, R.BIG_RESIZE_VEC):
        x = R.resize_source(1, *hi, C, big=True)
        R.assert_within(interp32(x, ho, 0), R.resize_ref64(x, ho, 0), FP, R.resize_extent(hi, ho), f"big {hi}->{ho}")


def test_nearest_closed_form_is_the_f32_reference():
    for hi, ho, C in R.NEAREST_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, C)
        assert torch.equal(R.nearest_ref(x, ho), interp32(x, ho, 4)), (hi, ho)
    # where the f32 index is not the exact rational floor(dst * n_in / n_out)
    assert int(R.nearest_index(2, 82)[41]) == 0 and 41 * 2 // 82 == 1
    exact = torch.arange(82) * 4 // 82
    assert not torch.equal(R.nearest_index(4, 82), exact)
    covered = [h for h, _, _ in R.NEAREST_CASES]
    assert (2, 3) in covered and (4, 3) in covered


def test_sources_are_exact_and_differ_by_frame_and_channel():
    for H, W, C in ALL_WARP:
        d = R.warp_case(H, W, C)
        for k in ("x", "x2"):
            x = d[k]
            assert torch.equal(x.to(BF).float(), x) and x.abs().max().item() <= 8 and torch.equal(x, x.round())
            assert all(not torch.equal(x[..., 0], x[..., c]) for c in range(1, C))
            assert all(not torch.equal(x[0], x[f]) for f in range(1, x.shape[0]))
        for k in ("flow", "flow2", "flow_prev"):
            assert torch.equal(d[k] * 4, (d[k] * 4).round()) and bool(torch.isfinite(d[k]).all())
        assert d["flow_prev"].abs().max().item() <= R.FLOW_PREV_SPAN


# ----------------------------------------------------------------------------------------------------- case checks
@pytest.mark.parametrize("case", ALL_WARP + [(H, W, 2) for H, W, _ in SMALL] + [(*R.BIG_COMPOSE, 2)], ids=ids)
def test_flows_stay_near_the_frame(case):
    H, W, C = case
    d = R.compose_case(H, W) if C == 2 else R.warp_case(H, W, C)
    for k in (("f1",) if C == 2 else ("flow", "flow2")):
        all_out, part = R.corner_shares(d[k], H, W)
        print(f"{case} {k}: all corners outside {all_out:.3f}, one to three outside {part:.3f}")
        assert all_out <= 0.5, (case, k, all_out)
        assert part >= 0.1, (case, k, part)            # every field is used with zeros padding


@pytest.mark.parametrize("case", SMALL, ids=ids)
def test_pinned_pixels_land_where_stated(case):
    H, W, C = case
    flow = R.warp_case(H, W, C)["flow"]
    n = flow.numel() // 2
    px, py = R._pixel_coords(flow)
    px, py = px.flatten(), py.flatten()
    pins = R.pinned_flows(H, W)
    assert len(pins) == 14
    for j, (lx, ly, fl) in enumerate(pins):
        p = j * (n // len(pins))
        if lx is not None:
            assert px[p].item() == lx
        if ly is not None:
            assert py[p].item() == ly
        if lx is None and ly is None:
            assert abs(flow.view(n, 2)[p, 0].item()) == abs(fl[0]) >= 1e4
    x = R.warp_case(H, W, C)["x"]
    far = [j * (n // len(pins)) for j in range(10, 14)]
    zeros, edge = R.warp_ref64(x, flow, False).view(n, C), R.warp_ref64(x, flow, True).view(n, C)
    for p, (cx, cy) in zip(far, [(W - 1, H - 1), (0, 0), (W - 1, H - 1), (0, 0)]):
        assert bool((zeros[p] == 0).all())
        assert torch.equal(edge[p], x[p // (H * W), cy, cx].double())


# ------------------------------------------------------------------------------------------------------ sensitivity
def seen(mutant, ref, m):
    """The mutant differs from the closed form by more than the loosest bound a kernel gets (bf16) on some element."""
    return bool(((mutant - ref).abs() > R.bound(ref, BF, m)).any())


WARP_MUTANTS = [   # fault, border settings, cases that cover it
    ("swap_xy", (False, True), SMALL),
    ("corner_x", (False, True), SMALL),
    ("corner_y", (False, True), SMALL),
    ("weights", (False, True), SMALL),
    ("clamp_after_floor", (True,), SMALL),
    ("size1_follows", (False,), [(1, 6, 32), (6, 1, 64)]),      # border padding clamps the stray coordinate back to 0
]


@pytest.mark.parametrize("fault,borders,cases", WARP_MUTANTS, ids=[m[0] for m in WARP_MUTANTS])
def test_warp_bound_sees_mutant(fault, borders, cases):
    for H, W, C in cases:
        d = R.warp_case(H, W, C)
        for border in borders:
            ref = R.warp_ref64(d["x"], d["flow"], border)
            assert seen(R.warp_ref64(d["x"], d["flow"], border, fault=fault), ref, max(H, W)), (fault, (H, W, C), border)
        if False in borders:        # flow_compose pads with zeros
            f = R.compose_case(H, W)
            assert seen(R.compose_ref64(f["f1"], f["f2"], fault=fault), R.compose_ref64(f["f1"], f["f2"]), max(H, W)), \
                (fault, "compose", (H, W))


def test_warp_bound_sees_the_wrong_padding():
    for H, W, C in SMALL:
        d = R.warp_case(H, W, C)
        z, b = R.warp_ref64(d["x"], d["flow"], False), R.warp_ref64(d["x"], d["flow"], True)
        assert seen(z, b, max(H, W)) and seen(b, z, max(H, W)), (H, W, C)


def test_prep_bound_sees_a_flow_composed_without_flow1():
    for H, W, C in SMALL:
        d = R.warp_case(H, W, C)
        ref = R.prep_ref64(d["x"], d["x2"], d["flow"], d["flow_prev"], BF)
        mut = R.prep_ref64(d["x"], d["x2"], d["flow"], d["flow_prev"], BF, fault="no_add")
        assert seen(mut["flow2"], ref["flow2"], max(H, W))      # even with D in the place of DP
        assert seen(mut["cond2"], ref["cond2"], max(H, W))
        assert not torch.equal(mut["flowpad"], ref["flowpad"])
        f = R.compose_case(H, W)
        assert seen(R.compose_ref64(f["f1"], f["f2"], fault="no_add"), R.compose_ref64(f["f1"], f["f2"]), max(H, W))


RESIZE_MUTANTS = [("no_half_pixel", 0), ("half_pixel_ac", 1), ("cubic_unclamped", 2), ("cubic_a05", 2)]


@pytest.mark.parametrize("fault,mode", RESIZE_MUTANTS, ids=[m[0] for m in RESIZE_MUTANTS])
def test_resize_bound_sees_mutant(fault, mode):
    hit = 0
    for hi in R.RESIZE_IN:
        for ho in R.RESIZE_OUT:
            x = R.resize_source(R.RESIZE_FRAMES, *hi, 3)
            hit += seen(R.resize_ref64(x, ho, mode, fault=fault), R.resize_ref64(x, ho, mode), R.resize_extent(hi, ho))
    # (1, 1) -> anything and the like leave nothing to get wrong; most of the 36 size pairs must see it
    assert hit >= 24, (fault, hit)
    if fault == "cubic_unclamped":      # an input narrower than the four taps
        x = R.resize_source(R.RESIZE_FRAMES, 2, 3, 3)
        assert seen(R.resize_ref64(x, (13, 11), 2, fault=fault), R.resize_ref64(x, (13, 11), 2), 13)


@pytest.mark.parametrize("fault", ["scale_swap", "scale_c2"])
def test_resize_bound_sees_wrong_channel_scales(fault):
    for hi, ho in R.SCALED_CASES:
        for mode in (0, 1, 2):
            x = R.resize_source(R.RESIZE_FRAMES, *hi, 3)
            ref = R.resize_ref64(x, ho, mode, 1.5, 0.75)
            assert seen(R.resize_ref64(x, ho, mode, 1.5, 0.75, fault=fault), ref, R.resize_extent(hi, ho))
            assert torch.equal(ref[..., 2], R.resize_ref64(x, ho, mode)[..., 2])


def test_nearest_bits_see_round_instead_of_floor():
    for hi, ho, C in R.NEAREST_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, C)
        assert not torch.equal(R.nearest_ref(x, ho, fault="round"), R.nearest_ref(x, ho)), (hi, ho)
