"""tests/dcn_frac_ref.py checked without a GPU: the four-corner reference against the two DCN oracles and against the
integer gather of tests/test_gpu_exact.py, the conditions that make the dyadic data exact (for every case that
tests/test_gpu_dcn_frac.py runs), and the one-hot bound: emulations of the kernel's three blend forms stay within it,
three faults of one (group, tap) leave it by more than a factor of ten."""
import math

import pytest
import torch

from tests import dcn_frac_ref as R
from tests.dcn_frac_ref import BF, FP
from tests.test_gpu_exact import assert_rounding_exercised, dcn_gather_ref, dcn_total_offset
from tests.util import assert_exact_headroom, int_tensor, rb

SMALL = (1, FP, 2, 11, 13, 32, 48, 8)


def test_cases_are_the_21_strided_cases_and_the_mode_2_shapes():
    assert len(R.strided_cases()) == 21 and len(R.pack_cases()) == 8 and len(R.onehot_cases()) == 14 + 8
    dot2 = [c for c in R.strided_cases() if R.is_dot2(c)]
    assert [c[2:5] for c in dot2] == [(2, 64, 128), (2, 64, 128), (1, 12, 16), (4, 128, 128), (1, 16, 32)]   # the bf16 <.., A, 1F> rows


def test_corner_ref_agrees_with_deform_conv2d_on_dyadic_positions():
    """Dyadic positions, random real x, w and masks: oracle.thirdparty.deform_conv2d in float64 agrees to rounding
    (its grid_sample normalises the positions inexactly): 1e-11 of max|ref|."""
    from oracle.thirdparty import deform_conv2d
    d = R.dyadic_data(SMALL, 1)
    mode, dtype, Fr, H, W, half, cout, G = SMALL
    g = torch.Generator().manual_seed(3)
    x = torch.randn(Fr, 2 * half, H, W, generator=g)
    w = torch.randn(cout, 2 * half, 3, 3, generator=g)
    b = torch.randn(cout, generator=g)
    mask = torch.rand(Fr, 9 * G, H, W, generator=g)
    got = R.dcn_corner_ref(x, d.residues, d.flows, mask, w, b, G)
    assert got.frac >= 0.5
    ref = deform_conv2d(x.double(), dcn_total_offset(d.residues, d.f1, d.f2).double(), w.double(), b.double(), (1, 1), (1, 1),
                        (1, 1), mask.double())
    err, top = (got.out - ref).abs().max().item(), ref.abs().max().item()
    print(f"corner ref against deform_conv2d: {err:.2e} absolute at max|ref| = {top:.1f}")
    assert err <= 1e-11 * top


def test_corner_ref_agrees_with_the_reference_source_on_its_edge_targets():
    """The edge targets of test_gpu_kernels.test_dcn_vs_reference_source against oracle/dcn_ref.py run in float32: the two
    compute the same float32 positions, so they differ by that oracle's float32 blend and its K = 9 C term sum only:
    (K + 16) 2^-24 of the magnitude run per element."""
    from oracle import dcn_ref
    c, H, W, G = 16, 11, 13, 16
    g = torch.Generator().manual_seed(77 + c)
    x = torch.randn(1, 2 * c, H, W, generator=g)
    w = torch.randn(c, 2 * c, 3, 3, generator=g) / math.sqrt(18 * c)
    b = torch.randn(c, generator=g) * 0.1
    offset = torch.randn(1, 2 * G * 9, H, W, generator=g) * 3
    mask = torch.rand(1, G * 9, H, W, generator=g)
    off = offset.view(1, G, 9, 2, H, W)
    hh = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    ww = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    targets = [(-0.5, 0.25), (-1.0, 2.0), (-0.999, -0.001), (H - 1.0, W - 1.0), (H - 0.5, W - 0.25),
               (float(H), 1.0), (2.0, 3.0), (H - 1.25, -1.0), (-3.0, 1.5)]
    for k in range(9):
        i, j = divmod(k, 3)
        off[:, k, k, 0] = (targets[k][0] - (hh - 1 + i)).expand(1, H, W)
        off[:, k, k, 1] = (targets[k][1] - (ww - 1 + j)).expand(1, H, W)
    off[:, G - 1] = torch.round(off[:, G - 1])
    ref = torch.from_numpy(dcn_ref.modulated_deform_conv_forward(x.numpy(), w.numpy(), b.numpy(), offset.numpy(),
                                                                 mask.numpy(), deformable_group=G)).double()
    got = R.dcn_corner_ref(x, offset, None, mask, w, b, G)
    ratio = ((got.out - ref).abs() / ((18 * c + 16) * R.U24 * got.mag)).max().item()
    print(f"corner ref against oracle/dcn_ref.py (float32) on its edge targets: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0
    for k, want in enumerate([2, 2, 1, 1, 1, 0, 4, 2, 0]):          # corners inside: (-0.5, 0.25) keeps the pair on row 0, ...
        assert bool((got.inside[0, k, k] == want).all()), (k, targets[k], got.inside[0, k, k].unique())


def test_corner_ref_equals_the_integer_gather_bit_for_bit():
    H, W, G, cin, cout = 9, 11, 8, 32, 12
    g = torch.Generator().manual_seed(9 * 11 + G)
    x = int_tensor((2, cin, H, W), -3, 3, g)
    w = int_tensor((cout, cin, 3, 3), -3, 3, g)
    b = int_tensor((cout,), -8, 8, g)
    offset = int_tensor((2, 18 * G, H, W), -7, 7, g)
    mask = int_tensor((2, 9 * G, H, W), 0, 2, g) * 0.5
    f1, f2 = int_tensor((2, H, W, 2), -3, 3, g), int_tensor((2, H, W, 2), -3, 3, g)
    want, inside, _ = dcn_gather_ref(x, dcn_total_offset(offset, f1, f2), mask, w, b, G)
    got = R.dcn_corner_ref(x, offset, (f1, f2), mask, w, b, G)
    assert got.frac == 0.0 and torch.equal(got.out, want)
    assert bool((got.inside[inside] >= 1).all())                    # an integer position inside the frame is its own corner


@pytest.mark.parametrize("case", R.exact_cases(), ids=R.case_id)
def test_dyadic_data_is_exact_and_reaches_the_edges(case):
    """What makes the bit-for-bit comparison of tests/test_gpu_dcn_frac.py valid and worth running, from the reference
    alone, for every case run there."""
    mode, dtype, Fr, H, W, half, cout, G = case
    d = R.dyadic_data(case, mode)
    r = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G)
    assert r.cols_bf16_exact, "a blended sample is not representable in bf16"
    top = assert_exact_headroom(r.mag * 32)                                        # every partial sum is a multiple of 1/32
    assert torch.equal(r.out * 32, (r.out * 32).round())
    pre = r.out.float()
    assert torch.equal(pre.double(), r.out)
    assert_rounding_exercised(pre, BF, R.case_id(case))
    share = R.partly_outside_share(r.inside)
    rows = R.band_report(r.inside, d.bands)
    print(f"{R.case_id(case)}: {100 * r.frac:.0f} % of the coordinates fractional, {100 * share:.1f} % of the samples partly "
          f"outside, partial sums up to {top:.0f} / 32; bands (covered of pixels): "
          + ", ".join(f"{n} {c}/{t}" for n, c, t, _ in rows))
    assert r.frac >= 0.5 and share >= R.partly_outside_floor(H, W), (r.frac, share)
    assert (mode == 0) == (not rows)
    for name, covered, total, wrong in rows:
        assert wrong == 0, (name, wrong)
        assert covered == total if dtype == FP or max(H, W) <= 32 else covered >= total // 4, (name, covered, total)
    for f in range(1, Fr):                                                         # frames differ
        assert not torch.equal(d.x[f], d.x[0]) and not torch.equal(r.out[f], r.out[0])
    if mode != 1:                                                                  # what the kernel's activation has to give
        o, m = d.raw[:, :18 * G].double(), d.raw[:, 18 * G:].double()
        assert torch.equal(torch.sigmoid(m).round(decimals=12), d.mask)
        if mode == 0:
            assert torch.equal((R.MAX_MAG * torch.tanh(o)).float(), d.residues)


# ------------------------------------------------------------------------------------------------ the one-hot bound
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate(form):
    """The kernel's blend in torch, as dcn_corner_ref's `blend`: f32 -- float32 weights, four fused multiply-adds; bf16 -- the
    same, the sample rounded to bf16; dot2 -- the ONEFRAME weights rounded to bf16, float32 accumulation, sample rounded."""
    def blend(k, ay, ax, m, v, cpg):
        m = m.float()
        if form == "dot2":
            wx0, wx1 = (1 - ax) * m, ax * m
            wt = rb(torch.stack([(1 - ay) * wx0, (1 - ay) * wx1, ay * wx0, ay * wx1]), BF)
            s = (wt.repeat_interleave(cpg, dim=1).double() * v.double()).sum(0).float()
        else:
            wt = R.corner_weights(ay, ax, m).repeat_interleave(cpg, dim=1)
            s = torch.zeros_like(v[0])
            for i in range(4):
                s = _fma32(wt[i], v[i], s)
        return (s if form == "f32" else rb(s, BF)).double()
    return blend


ONEHOT_CPU = [(1, FP, 2, 11, 13, 32, 48, 8), (1, BF, 2, 11, 13, 64, 32, 8), (1, BF, 1, 16, 32, 64, 64, 16),
              (2, BF, 2, 9, 13, 32, 64, 4), (2, FP, 2, 9, 13, 32, 64, 4)]


def _form(case):
    return "f32" if case[1] == FP else "dot2" if R.is_dot2(case) else "bf16"


@pytest.mark.parametrize("case", ONEHOT_CPU, ids=R.case_id)
def test_onehot_bound_holds_for_the_emulated_blend(case):
    mode, dtype, Fr, H, W, half, cout, G = case
    d = R.generic_data(case)
    ref = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G)
    for name, covered, total, wrong in R.band_report(ref.inside, d.bands):
        assert wrong == 0 and covered == total, (name, covered, total, wrong)
    mask = d.mask if mode == 1 else torch.sigmoid(d.raw[:, 18 * G:]).double()     # mode 2: a float32 sigmoid
    emu = R.dcn_corner_ref(d.x, d.residues, d.flows, mask, d.w, d.b, G, blend=emulate(_form(case)))
    got = emu.out.float().to(dtype).double()
    err = (got - ref.out).abs()
    ratio = (err / R.onehot_bound(case, ref.out, ref.mag)).max().item()
    issued = (err / R.onehot_bound(case, ref.out, ref.mag, as_issued=True)).max().item()
    print(f"one-hot bound, {_form(case)} blend emulated, {R.case_id(case)}: worst err / bound {ratio:.3f} "
          f"({issued:.3f} with 2^-9 per bf16 rounding)")
    assert ratio <= 1.0
    # The written record of why a bf16 rounding counts 2^-8 here: these emulations round every value correctly, once, and
    # still leave the bound that counts 2^-9 (the kernel comment's figure before this test) on a few hundred elements.
    assert (issued > 1.0) == (dtype == BF), issued


def _mutation(kind, g, kk):
    def blend(k, ay, ax, m, v, cpg):
        ay, ax = ay.double().clone(), ax.double().clone()
        if kind == "swap" and k == kk:
            ax[g] = 1 - ax[g]
        wt = R.corner_weights(ay, ax, m)
        if kind == "drop" and k == kk:
            wt[3, g] = 0.0
        if kind == "weight" and k == kk:
            wt[1, g] += 2.0 ** -6
        return (wt.repeat_interleave(cpg, dim=1) * v.double()).sum(0)
    return blend


@pytest.mark.parametrize("case", ONEHOT_CPU[1:4], ids=R.case_id)
@pytest.mark.parametrize("kind", ["drop", "swap", "weight"])
def test_onehot_bound_sees_one_faulty_group_and_tap(case, kind):
    """A reference with one corner dropped, with ax and 1 - ax swapped, or with one weight off by 2^-6 -- each for ONE
    (group, tap) -- leaves the bound by more than a factor of ten at the output channels that read that (group, tap), and
    changes no other element."""
    mode, dtype, Fr, H, W, half, cout, G = case
    d = R.generic_data(case)
    ref = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G)
    cpg = 2 * half // G
    # the first output channel past the nine that aim at the bands whose (group, tap) is no band pair
    co = next(c for c in range(9, cout) if (c % G, c % 9) not in R.band_pairs(G))
    k, ci = co % 9, int(d.w[co].reshape(2 * half, 9)[:, co % 9].nonzero()[0])
    g = ci // cpg
    assert g == co % G
    hit = [c for c in range(cout) if d.w[c].reshape(2 * half, 9)[g * cpg:(g + 1) * cpg, k].abs().sum() > 0]
    assert co in hit
    mut = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G, blend=_mutation(kind, g, k))
    ratio = (mut.out - ref.out).abs() / R.onehot_bound(case, ref.out, ref.mag)
    rest = [c for c in range(cout) if c not in hit]
    assert bool((ratio[:, rest] == 0).all())
    worst, beyond = ratio[:, hit].max().item(), (ratio[:, hit] > 1).float().mean().item()
    print(f"{kind} at group {g}, tap {k}, {R.case_id(case)}: worst err / bound {worst:.0f}, beyond the bound at "
          f"{100 * beyond:.0f} % of the {len(hit)} x {Fr * H * W} elements that read it")
    assert worst > 10.0 and beyond >= 0.25
