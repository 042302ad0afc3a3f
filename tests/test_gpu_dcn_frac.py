"""flair_dcn_align at the positions it really samples, which lie between pixels (reference and data: tests/dcn_frac_ref.py,
checked without a GPU by tests/test_dcn_frac_cpu.py).

A. Bit for bit on dyadic data.  Positions on a grid of 1/4 pixel, masks in {0, 0.5, 1}, integer features and weights: the
   four corner weights are multiples of 1/32 (exact in bf16, so the v_dot2c blend with its bf16 weights is exact too), the
   blended samples are exact in bf16, every partial sum is exact in f32 -- one wrong or dropped corner, two swapped
   weights, a neighbour's row read instead of zero, a weight that did not survive its rounding change bits.  Every entry of
   tests/test_gpu_strides.DCN_CASES (activated: raw_activated = 1; the others: mode 0 with max_mag = 2, where the kernel's
   own tanh and sigmoid have to give -2, 0, 2 and 0, 0.5, 1 exactly) and ops.dcn_pack (raw_activated = 2) at four shapes
   in both dtypes; every frame is compared, and the frames differ.
B. Per element at arbitrary positions.  Randn data and a weight matrix with ONE nonzero per output channel:
   y[p, co] = bias + w * (one blended sample), compared with the float64 reference against dcn_frac_ref.onehot_bound.
"""
import pytest
import torch

from tests import dcn_frac_ref as R
from tests.dcn_frac_ref import BF, FP
from tests.test_gpu_exact import assert_rounding_exercised, nhwc
from tests.util import assert_bits_equal, assert_exact_headroom, parity_log, tile_histogram

pytestmark = pytest.mark.gpu


def _ops():
    from flair_amd import ops
    return ops


def run_kernel(dev, case, d, raw=None, f2=None):
    """flair_dcn_align on the data d (raw and flow2 replaceable) -> (F, H, W, Cout) on the CPU."""
    ops = _ops()
    mode, dtype, Fr, H, W, half, cout, G = case
    raw = (d.raw if raw is None else raw)[:, ops.dcn_raw_permutation(G)]
    wp = ops.pack_conv_weight(d.w, [(2 * half, 2 * half)], dtype).to(dev)
    if mode == 2:
        ld = (27 * G + 7) // 8 * 8                                    # 16-byte granular rows in both dtypes
        rawp = torch.zeros(Fr, H, W, ld, dtype=dtype)
        rawp[..., :27 * G] = raw.permute(0, 2, 3, 1)
        y = ops.dcn_pack(nhwc(d.x, dtype, dev), rawp.to(dev), wp, d.b.to(dev), cout, groups=G)
    else:
        f2 = d.f2 if f2 is None else f2
        y = ops.dcn_align(nhwc(d.x[:, :half], dtype, dev), nhwc(d.x[:, half:], dtype, dev), nhwc(raw, dtype, dev),
                          d.f1.to(dev), f2.to(dev), wp, d.b.to(dev), cout, groups=G, max_mag=R.MAX_MAG,
                          raw_activated=bool(mode))
    torch.cuda.synchronize()
    return y.cpu()


# ------------------------------------------------------------------------------------------------ A: bit for bit
@pytest.mark.parametrize("case", R.exact_cases(), ids=R.case_id)
def test_dcn_frac_exact(dev, case):
    """Every frame bit for bit against the float64 reference rounded once to the output type; the tiles of test_dcn_exact,
    so that a failure names the lane or the store group.  If a mode 0 or mode 2 case fails while its mode 1 neighbour
    passes, look at the activation first: these cases need __expf(+-100 and beyond) = inf and 0 and v_rcp_f32 exact at 1
    and 2 (tests/test_gpu_act_exact.py rests on the same kind of fact)."""
    mode, dtype, Fr, H, W, half, cout, G = case
    d = R.dyadic_data(case, mode)
    r = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G)
    assert r.cols_bf16_exact
    assert_exact_headroom(r.mag * 32)
    pre = r.out.float()
    assert torch.equal(pre.double(), r.out)
    assert_rounding_exercised(pre, dtype, R.case_id(case))
    share = R.partly_outside_share(r.inside)
    rows = R.band_report(r.inside, d.bands)
    print(f"dcn frac {R.case_id(case)}: {100 * share:.1f} % of the samples partly outside, {100 * r.frac:.0f} % of the coordinates "
          f"fractional; bands (covered pixels): " + ", ".join(f"{n} {c}" for n, c, _, _ in rows))
    assert share >= R.partly_outside_floor(H, W) and all(wrong == 0 and c > 0 for _, c, _, wrong in rows)
    y = run_kernel(dev, case, d)
    assert_bits_equal(y, pre.to(dtype).permute(0, 2, 3, 1).contiguous(), f"dcn frac {R.case_id(case)}", tile=(1, 32, 32))


def test_dcn_frac_sees_a_quarter_pixel(dev):
    """One residue of one (frame, pixel, tap, group) changed by a quarter of a pixel, of 2 * 11 * 13 * 9 * 8 samples, fails
    the comparison at that pixel."""
    case = (1, BF, 2, 11, 13, 64, 32, 8)
    mode, dtype, Fr, H, W, half, cout, G = case
    assert case in R.exact_cases()
    d = R.dyadic_data(case, mode)
    g, k = 5, 4                                                      # second input half, centre tap; no band pair
    assert (g, k) not in R.band_pairs(G)
    raw, f2 = d.raw.clone(), d.f2.clone()
    res, mask = d.residues.clone(), d.mask.clone()
    for t in (raw, res):
        t[1, 2 * (g * 9 + k):2 * (g * 9 + k) + 2, 5, 6] = 0.0        # the sample of pixel (5, 6) of frame 1 is x[5, 6] itself
    raw[1, 18 * G + g * 9 + k, 5, 6] = mask[1, g * 9 + k, 5, 6] = 1.0
    f2[1, 5, 6] = 0.0
    r = R.dcn_corner_ref(d.x, res, (d.f1, f2), mask, d.w, d.b, G)
    want = r.out.float().to(dtype).permute(0, 2, 3, 1).contiguous()
    wrong = raw.clone()
    wrong[1, 2 * (g * 9 + k) + 1, 5, 6] = 0.25                       # a quarter of a pixel to the right
    cpg = 2 * half // G
    assert not torch.equal(d.x[1, g * cpg:(g + 1) * cpg, 5, 6], d.x[1, g * cpg:(g + 1) * cpg, 5, 7])
    assert_bits_equal(run_kernel(dev, case, d, raw=raw, f2=f2), want, "right offsets")
    with pytest.raises(AssertionError, match="first at \\[1, 5, 6, "):
        assert_bits_equal(run_kernel(dev, case, d, raw=wrong, f2=f2), want, "a quarter of a pixel")


# ------------------------------------------------------------------------------------------------ B: one-hot weights
def _form(case):
    return ("f32" if case[1] == FP else "dot2" if R.is_dot2(case) else "bf16") + ("" if case[0] == 1 else ", raw offsets")


@pytest.mark.parametrize("case", R.onehot_cases(), ids=R.case_id)
def test_dcn_frac_onehot(dev, case):
    """|y - ref| <= dcn_frac_ref.onehot_bound per element.  Mode 0 is left to family A and to the tolerance tests: its tanh
    moves the positions themselves.
    Measured worst err / bound on an MI355X, per form over its cases (every case: profiles/dcn_frac_parity.txt):
      f32                        0.292 .. 0.369          f32, raw offsets      0.155 .. 0.213
      bf16 (batched forms)       0.814 .. 0.977          bf16, raw offsets     0.901 .. 0.964
      dot2 (bf16, ONEFRAME)      0.718 .. 0.915
    The bound counts 2^-8 per bf16 rounding.  Against the same formula with 2^-9 (dcn.hip's comment said 2^-9 for the dot2
    weights until this test) the bf16 forms reach 1.57 .. 1.94 and the dot2 forms 1.42 .. 1.80, no more than the correctly
    rounded emulations of tests/test_dcn_frac_cpu.py do (1.57 .. 1.75 on three small cases): the kernel is right, a
    round-to-nearest to bf16 is worth half a unit in the last place, which is 2^-8 of a value at the bottom of its binade."""
    mode, dtype, Fr, H, W, half, cout, G = case
    d = R.generic_data(case)
    r = R.dcn_corner_ref(d.x, d.residues, d.flows, d.mask, d.w, d.b, G)
    rows = R.band_report(r.inside, d.bands)
    assert all(wrong == 0 and c > 0 for _, c, _, wrong in rows), rows
    y = run_kernel(dev, case, d).permute(0, 3, 1, 2).double()
    err = (y - r.out).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = err / R.onehot_bound(case, r.out, r.mag)
    issued = (err / R.onehot_bound(case, r.out, r.mag, as_issued=True)).max().item()
    worst = ratio.max().item()
    parity_log(f"dcn frac one-hot {R.case_id(case)} ({_form(case)}): worst err / bound {worst:.3f} ({issued:.3f} with 2^-9 per bf16 "
               f"rounding), {100 * R.partly_outside_share(r.inside):.1f} % of the samples partly outside")
    if worst > 1.0:
        bad = (ratio > 1.0).permute(0, 2, 3, 1)
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"dcn frac one-hot {R.case_id(case)}: {int(bad.sum())} of {bad.numel()} element(s) beyond the bound, "
                             f"worst err / bound {worst:.3f}; first at {first}" + tile_histogram(bad.nonzero(), (1, 32, 32)))
