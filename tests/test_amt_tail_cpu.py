"""The references, inputs and bounds of tests/test_gpu_amt_tail.py, proved without a GPU:

  a. the closed forms of tests/amt_tail_ref.py are the reference: tests/amt_cpu.multi_flow_combine and multi_flow_decoder
     themselves, run in float64 with a float64 linspace in their warp, give the same numbers to 1e-12;
  b. the "exact" inputs are exact: every value the combine kernel forms on them, the five-term sum included, is an f32
     number, so the float64 closed form rounded once is the one correct answer (avg rounds in its division alone), and the
     pinned landings are where they should be;
  c. an f32 emulation of each kernel's documented operation order meets every bound the GPU tests apply, with room (the
     ratios are printed);
  d. every mutant of a closed form -- a plausible kernel bug -- is rejected by those same comparisons.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import amt_tail_ref as R
from tests.util import gn_fold_f32

N = R.N
ids = R.ids


# ------------------------------------------------------------------------------------------------ a. the reference
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 24, 40), (1, 1, 9), (1, 9, 1)], ids=ids)
def test_combine64_is_the_reference_in_float64(shape):
    for d in (R.combine_seeded_case(*shape), R.combine_exact_case(*shape) if shape in R.TAIL_SHAPES else None):
        if d is None:
            continue
        if 1 in shape[1:] and (d["prep"][..., :4 * N] == 0).any():
            continue        # the reference divides a flow by (size - 1) / 2 = 0: a flow of exactly 0 gives it NaN
        x, avg = R.combine64(**d)
        rx, ravg = R.reference_combine(**d, dtype=R.F64, warp=R.warp64)
        assert R.max_err(rx, x[..., :3 * N]) <= 1e-12 and R.max_err(ravg, avg[..., :3]) <= 1e-12
        assert (x[..., 15] == 0).all() and (avg[..., 3] == 0).all()
    # ... and amt_cpu.warp's own grid is f32 even on float64 tensors: not a float64 reference
    d = R.combine_seeded_case(*shape)
    if 1 not in shape[1:]:
        off = R.max_err(R.reference_combine(**d, dtype=R.F64)[0], R.combine64(**d)[0][..., :3 * N])
        print(f"amt_cpu.warp in float64 through its f32 grid, {shape}: {off:.2e} from the closed form")
        assert off > 1e-9


def test_prepare64_is_the_reference_in_float64():
    g = torch.Generator().manual_seed(9)
    dec = torch.randn(2, 6, 10, R.MF_C, generator=g) * 2
    ref, up = R.reference_prepare(dec, torch.randn(2, 3, 5, 4, generator=g) * 3)
    assert tuple(up.shape) == (2, 6, 10, 4)
    assert R.max_err(R.prepare64(dec, up), ref) <= 1e-12


# ------------------------------------------------------------------------------------------------ b. exactness
@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_exact_combine_inputs_are_exact(shape):
    B, H, W = shape
    d = R.combine_exact_case(*shape)
    x, avg, s = R.combine_exact_reference(*shape)
    assert torch.equal(x.float().double(), x) and torch.equal(s.float().double(), s)
    # so avg's only rounding is the division: the f32 quotient of the f32 sum is the float64 quotient rounded once
    assert R.same_bits((s.float() / 5.0), avg[..., :3].float())
    ex, eavg = R.combine_emul32(**d)
    assert R.same_bits(ex, x.float()) and R.same_bits(eavg, avg.float())
    assert all(R.landing_classes(d["prep"], H, W).values()), R.landing_classes(d["prep"], H, W)
    assert len(set(R.pinned_pixels(*shape).values())) == 5
    px, py = R.landings(d["prep"], H, W)
    outside = ((px < 0) | (px > W - 1) | (py < 0) | (py > H - 1)).double().mean().item()
    assert 0.02 < outside < 0.98, outside
    assert not torch.equal(d["pair"][..., 0:3], d["pair"][..., 3:6])
    assert torch.isnan(d["neg_mean"][:, 1:]).all() and d["neg_mean"].stride(0) > 1
    if B > 1:
        assert d["neg_mean"][0, 0] != d["neg_mean"][1, 0] and d["neg_mean"][0, 0] != -d["neg_mean"][0, 0]


@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_exact_prepare_channels_are_exact(shape):
    d = R.prepare_case(*shape)
    want, dev = R.prepare_reference(*shape)
    flows = R.not_mask(want)
    assert torch.equal(flows.float().double(), flows) and d["dec"].abs().max() <= 64 and d["up"].abs().max() <= 64
    assert R.same_bits(R.not_mask(R.prepare_emul32(**d)), flows.float())
    assert dev > 0
    up = d["up"]
    assert not torch.equal(up[..., 0], up[..., 1]) and not torch.equal(up[..., 0:2], up[..., 2:4])


def test_balanced_planes_have_one_answer():
    """On +-1 planes with as many of each, the closed form rounded to f32, the emulation and the expression of
    tests/test_gpu_amt.py's balanced test agree bit for bit; every chunk's sum is a nonzero integer."""
    for shape in R.INSTNORM_SHAPES[:4]:
        F_, H, W, C = shape
        x = R.instnorm_balanced_case(shape)
        assert (x.sum((1, 2)) == 0).all()
        zero, one = torch.zeros(1, 1, 1, 1, dtype=R.F64), torch.ones(1, 1, 1, 1, dtype=R.F64)
        fold = gn_fold_f32(x, zero, one, torch.ones(C), torch.zeros(C), 1e-5)
        for relu in (False, True):
            want = R.instnorm64(x, relu=relu).float()
            assert R.same_bits(want, F.relu(fold) if relu else fold)
            assert R.same_bits(want, R.instnorm_emul32(x, relu=relu))
        parts = torch.stack([c.sum(1) for c in x.reshape(F_, H * W, C).split(R.chunks(H * W), dim=1)])
        assert len(R.chunks(H * W)) == R.in_split(H * W) > 1 and (parts != 0).float().mean() > 0.9


def test_instance_norm_shapes_reach_what_they_claim():
    assert [R.chunks(h * w) for _, h, w, _ in R.INSTNORM_SHAPES[:3]] == [[512, 512], [594, 594], [547, 547, 546]]
    big = R.chunks(182 * 182)
    assert len(big) == 64 and big[0] == 518 and big[-1] == 182 * 182 - 63 * 518 and sum(big) == 182 * 182
    assert R.chunks(33 * 35) == [578, 577]
    assert R.in_split(16 * 18) == 1                     # the maps of tests/test_gpu_amt.py never split
    for shape in R.INSTNORM_SHAPES:
        x = R.instnorm_seeded_case(shape, 30).double()
        m, s = x.mean((1, 2)), x.std((1, 2))
        assert (m[:, 1:] - m[:, :-1]).abs().min() > 0 and (s[:, 1:] - s[:, :-1]).abs().min() > 0
        if shape[0] > 1:
            assert ((s[1] / s[0]) > 2).all()


# ------------------------------------------------------------------------------------------------ c. headroom
@pytest.mark.parametrize("shape", R.TAIL_SHAPES, ids=ids)
def test_emulated_tail_meets_the_seeded_bounds(shape):
    d = R.combine_seeded_case(*shape)
    x, avg, dev_x, dev_avg = R.combine_seeded_reference(*shape)
    ex, eavg = R.combine_emul32(**d)
    rx, ra = R.max_err(ex, x) / (4 * dev_x), R.max_err(eavg, avg) / (4 * dev_avg)
    print(f"combine {shape}: f32 ATen deviation x {dev_x:.2e} avg {dev_avg:.2e}; emulation err / bound x {rx:.3f} avg {ra:.3f}")
    assert 0 < rx <= 0.5 and 0 < ra <= 0.5
    p = R.prepare_case(*shape)
    want, dev = R.prepare_reference(*shape)
    r = R.max_err(R.prepare_emul32(**p)[..., 4 * N:5 * N], want[..., 4 * N:5 * N]) / (4 * dev)
    print(f"prepare {shape}: f32 sigmoid deviation {dev:.2e}; emulation err / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("offset", R.INSTNORM_OFFSETS)
@pytest.mark.parametrize("shape", R.INSTNORM_SHAPES, ids=ids)
def test_emulated_instance_norm_meets_the_seeded_bound(shape, offset):
    x = R.instnorm_seeded_case(shape, offset)
    want, dev = R.instnorm_seeded_reference(shape, offset)
    r = R.max_err(R.instnorm_emul32(x), want) / (4 * dev)
    print(f"instance norm {shape} offset {offset}: f32 ATen deviation {dev:.2e}; emulation err / bound {r:.3f}")
    assert 0 < r <= 0.5


def test_saturated_sigmoid_in_the_emulation():
    y = R.prepare_emul32(**R.saturation_case())[0, 0, :, 4 * N]
    assert not torch.isnan(y).any() and y[0] == 0 and y[3] == 0.5 and y[-1] == 1 and (y[1:] >= y[:-1]).all()


# ------------------------------------------------------------------------------------------------ d. sharpness
def combine_rejections(fault):
    """-> the cases whose comparison rejects the mutant: 'exact B H W' (bit for bit) or 'seeded B H W' (4 x deviation)."""
    hit = []
    for shape in R.TAIL_SHAPES:
        x, avg, _ = R.combine_exact_reference(*shape)
        mx, mavg = R.combine64(**R.combine_exact_case(*shape), fault=fault)
        if not (R.same_bits(mx.float(), x.float()) and R.same_bits(mavg.float(), avg.float())):
            hit.append(("exact",) + shape)
        x, avg, dev_x, dev_avg = R.combine_seeded_reference(*shape)
        mx, mavg = R.combine64(**R.combine_seeded_case(*shape), fault=fault)
        if R.max_err(mx, x) > 4 * dev_x or R.max_err(mavg, avg) > 4 * dev_avg:
            hit.append(("seeded",) + shape)
    return hit


@pytest.mark.parametrize("fault", R.COMBINE_FAULTS)
def test_combine_comparison_rejects_mutant(fault):
    hit = combine_rejections(fault)
    print(f"combine mutant {fault}: rejected by {hit}")
    assert any(h[0] == "exact" for h in hit), hit                       # the bit-for-bit cases alone see it
    if fault != "unclamped":
        # (a neighbour left unclamped weighs nothing: it shows only where it reads the NaN behind the last frame)
        assert any(h[0] == "seeded" for h in hit), hit
    if fault == "mean_frame0":
        assert all(h[1] == 2 for h in hit)                              # needs a second frame


def test_unfaulted_combine_is_not_rejected():
    assert combine_rejections(None) == []


@pytest.mark.parametrize("fault", R.PREPARE_FAULTS)
def test_prepare_comparison_rejects_mutant(fault):
    hit = []
    for shape in R.TAIL_SHAPES:
        d = R.prepare_case(*shape)
        want, dev = R.prepare_reference(*shape)
        mut = R.prepare64(**d, fault=fault)
        if not R.same_bits(R.not_mask(mut).float(), R.not_mask(want).float()):
            hit.append(("bits",) + shape)
        if R.max_err(mut[..., 4 * N:5 * N], want[..., 4 * N:5 * N]) > 4 * dev:
            hit.append(("sigmoid",) + shape)
    print(f"prepare mutant {fault}: rejected by {hit}")
    assert len([h for h in hit if h[0] == "bits"]) == len(R.TAIL_SHAPES), hit


@pytest.mark.parametrize("shape", R.AXPBY_P, ids=ids)
@pytest.mark.parametrize("C", R.AXPBY_C)
def test_axpby_bits_reject_a_fused_multiply_add(C, shape):
    x0, x1 = R.axpby_case(shape, C)
    a, b = R.AXPBY_COEFS[1]
    want = R.axpby_emul32(x0, a, x1, b)
    fused = R.axpby_emul32(x0, a, x1, b, fault="fma")
    share = (want != fused).float().mean().item()
    also = (want != torch.addcmul(x0 * R.f32_scalar(a), x1, R.f32_scalar(b))).float().mean().item()
    print(f"axpby C = {C} {shape}: a fused multiply-add changes {share:.1%} of the elements (torch.addcmul: {also:.1%})")
    assert share >= 0.05
    # the rounded products stay within an ulp and a half of the float64 value; (1, 2) is exact in its products
    w64 = R.axpby64(x0, a, x1, b)
    assert R.max_err(want, w64) <= 1.5 * 2.0 ** -24 * (2 * w64.abs().max().item() + 4)
    assert R.same_bits(R.axpby_emul32(x0, 1.0, x1, 2.0), R.axpby_emul32(x0, 1.0, x1, 2.0, fault="fma"))
    assert R.same_bits(R.axpby_emul32(x0, 1.0 / 3.0), (x0.double() * R.f32_scalar(1.0 / 3.0).double()).float())


def instnorm_rejections(fault, stop_early=True):
    hit = []
    for shape in R.INSTNORM_SHAPES[:4]:
        x = R.instnorm_balanced_case(shape)
        if not R.same_bits(R.instnorm64(x, fault=fault).float(), R.instnorm64(x).float()):
            hit.append(("balanced",) + shape)
    for offset in R.INSTNORM_OFFSETS:
        for shape in sorted(R.INSTNORM_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3]):
            if stop_early and any(h[0] == offset for h in hit):
                break
            want, dev = R.instnorm_seeded_reference(shape, offset)
            if R.max_err(R.instnorm64(R.instnorm_seeded_case(shape, offset), fault=fault), want) > 4 * dev:
                hit.append((offset,) + shape)
    return hit


@pytest.mark.parametrize("fault", R.INSTNORM_FAULTS)
def test_instance_norm_comparison_rejects_mutant(fault):
    hit = instnorm_rejections(fault)
    print(f"instance norm mutant {fault}: rejected by {hit}")
    assert hit
    balanced = [h[1:] for h in hit if h[0] == "balanced"]
    if fault == "double_count":                     # a doubled pixel shows on every split plane
        assert balanced == R.INSTNORM_SHAPES[:4]
    if fault == "drop_remainder":                   # a dropped remainder wherever the chunks are uneven
        assert balanced == [s for s in R.INSTNORM_SHAPES[:4] if (s[1] * s[2]) % R.in_split(s[1] * s[2])]
        assert balanced
    if fault in ("var_n1", "eps_outside"):
        assert len(balanced) == 4
    if fault in ("neighbour_channel", "neighbour_frame", "one_pass_f32"):
        assert not balanced and any(h[0] in R.INSTNORM_OFFSETS for h in hit)    # the seeded bound's to see


def test_unfaulted_instance_norm_is_not_rejected():
    assert instnorm_rejections(None, stop_early=False) == []
