"""The references and cases of tests/test_gpu_face_exact.py, checked without a GPU.

  * tests/face_ref.py (written from the definition) and oracle/facewarp.py (the numpy restatement the older tests use)
    agree bit for bit on every exact case and within the GPU tests' per-element bound on the random ones;
  * every warp case reaches the window classes it claims, with partial windows over all four edges and a corner;
    sources narrower or shorter than 4 pixels have no inner window;
  * each alternative rounding rule of the coordinates (half away from zero, floor, rounding the sum of the two parts)
    changes output elements of some case, so the bit-for-bit GPU comparison tells them from the specified rule;
  * every expected output of an exact case is an f32 number (asserted in integer arithmetic inside face_ref.warp_exact
    and face_ref.blur_exact), and the small blur cases reflect an index twice.

Window classes per case, outside / inner / partial (printed by test_case_classes, which also counts the partial windows
over each edge):
    7x9-scale 980/192/748    7x9-turn 1140/192/588   7x9-shift 1836/24/60    1x9-scale 1544/0/376
    9x2-turn 1440/0/480      3x3-scale 1644/0/276    4x4-scale 1542/8/370
    tie-x-neg 112/24/56      tie-x-pos 102/24/66     tie-y-neg 104/24/64     tie-y-pos 96/24/72
    parts-x-pos 112/24/56    parts-x-neg 102/20/70   parts-y-pos 156/10/26
    random (23x37 -> 45x61): 572/1431/742, 6/2475/264, 1896/582/267, 1729/725/291
7x9-shift moves the source down, so no window hangs over its top edge; every other case has partial windows over all
four edges and a corner.  A 4x4 source has one inner position (first tap 0, 0), reached by 8 pixels.
Output elements (of C = 2 planes) that an alternative coordinate rule changes, per case (test_rounding_rules):
    half_away  tie-x-neg 154, tie-y-neg 18, parts-x-neg 28, none elsewhere
    floor      tie-x-neg 154, tie-x-pos 140, tie-y-neg 162, tie-y-pos 144, parts-x-pos 42, parts-x-neg 42, parts-y-pos 24
    sum        parts-x-pos 14, parts-x-neg 14, parts-y-pos 10, none elsewhere
The numpy restatement (oracle) against the float64 reference on the random cases: worst |err| / (2^-24 S) = 3.85 on the
f32 path, |err| / (2^-53 S) = 4.61 on the f64 path; the GPU tests allow 18.  Blur restatement against fsum, worst err
over repeats (ksize + 2) 2^-53 sum |k| |v|: 0.26 (9 taps, 1 repeat), 0.08 (9, 3), 0.17 (9, 2, 64x64), 0.04 (101, 2).
"""
from unittest import mock

import numpy as np
import pytest

from tests import face_ref as R


def oracle_warp(img_chw, minv, out_hw, border):
    """oracle/facewarp.py's warp of a (C, Hs, Ws) image under a dst -> src matrix: its inversion step is replaced by the
    identity, so that it sees the matrix the kernels get.  -> (C, Hd, Wd) in the image's type."""
    from oracle import facewarp as fw
    img = np.ascontiguousarray(np.moveaxis(np.asarray(img_chw), 0, 2))
    with mock.patch.object(fw, "invert_affine", lambda M: np.asarray(M, dtype=np.float64).reshape(2, 3)):
        out = fw.warp_affine_cubic(img, minv, (out_hw[1], out_hw[0]), tuple(float(b) for b in border))
    return np.ascontiguousarray(np.moveaxis(out, 2, 0))


def random_source(C, dtype, seed, signed=False):
    rng = np.random.default_rng(seed)
    Hs, Ws = R.RANDOM_SRC
    v = rng.random((C, Hs, Ws))
    return ((v * 2.6 - 1.3) if signed else v * 255.0).astype(dtype)


def test_weight_table():
    tab32, num = R.cubic_table()
    assert tab32.dtype == np.float32 and np.array_equal(tab32[0], np.array([0, 1, 0, 0], dtype=np.float32))
    assert (num.sum(1) == 1 << R.TAB_BITS).all()                  # every row sums to exactly 1
    assert np.array_equal(tab32[1:][::-1, ::-1], tab32[1:])       # fraction f and 1 - f mirror each other
    from oracle import facewarp as fw
    assert np.array_equal(fw._TAB, tab32)


@pytest.mark.parametrize("name", list(R.WARP_CASES))
def test_case_classes(name):
    (Hs, Ws), (Hd, Wd), minv, claims = R.WARP_CASES[name]
    sx, sy, fx, fy = R.tap_geometry(minv, Hd, Wd)
    cls = R.classify(sx, sy, Hs, Ws)
    counts = R.class_counts(cls)
    sides = R.partial_sides(cls, sx, sy, Hs, Ws)
    print(f"{name}: outside/inner/partial = {counts[0]}/{counts[1]}/{counts[2]}, partial windows over {sides}")
    for c in claims:
        assert counts[c] >= 20, (name, R.CLASS_NAMES[c], counts)
    assert all((v > 0) != (k in R.SIDES_NOT_REACHED.get(name, ())) for k, v in sides.items()), (name, sides)
    if Hs <= 3 or Ws <= 3:
        assert counts[R.INNER] == 0 and counts[R.PARTIAL] > 0
    if (Hs, Ws) == (4, 4):
        assert counts[R.INNER] > 0 and set(sx[cls == R.INNER]) == {0} and set(sy[cls == R.INNER]) == {0}
    if name in R.EXACT_CASES:
        assert set(np.unique(fx)) | set(np.unique(fy)) <= {0, 8, 16, 24}          # quarter-pixel positions only
        assert "shift" in name or len(set(np.unique(fx)) | set(np.unique(fy))) == 4
    else:
        assert set(np.unique(fx)) == {0} or set(np.unique(fy)) == {0}             # one coordinate on whole pixels
    if name == "7x9-scale":
        assert counts == (980, 192, 748)
    if name == "7x9-turn":
        assert counts == (1140, 192, 588)


@pytest.mark.parametrize("name", list(R.WARP_CASES))
def test_exact_cases_are_exact_and_match_the_oracle(name):
    """warp_exact asserts in integer arithmetic that the f32 weight products are exact, that every partial sum fits f32
    and that the result is an f32 number; the float64 reference and the oracle (f32 and f64 sources) then agree with it
    bit for bit."""
    (Hs, Ws), out_hw, minv, _ = R.WARP_CASES[name]
    for C in (1, 2, 3, 4):
        src = R.int_source(1, C, Hs, Ws, 10 + C)[0]
        ex = R.warp_exact(src, minv, out_hw, R.BORDER)
        r64 = R.warp_ref64(src.astype(np.float32), minv, out_hw, R.BORDER)
        assert np.array_equal(r64["value"], ex["value"]) and np.array_equal(r64["cls"], ex["cls"])
        assert (ex["value"][:, ex["cls"] == R.OUTSIDE] == np.array(R.BORDER[:C], dtype=np.float64)[:, None]).all()
        for dtype in (np.float32, np.float64):
            got = oracle_warp(src.astype(dtype), minv, out_hw, R.BORDER)
            assert got.dtype == dtype
            ne = got.astype(np.float64) != ex["value"]
            if ne.any():
                idx = tuple(np.argwhere(ne)[0])
                raise AssertionError(f"{name} C={C} {np.dtype(dtype).name}: oracle {got[idx]!r} != exact {ex['value'][idx]!r} at "
                                     f"{idx}: {R.describe(ex, idx)}")


def test_rounding_rules():
    """Each alternative rule moves output elements of some case; half-even on the parts is the one that is asserted."""
    changed = {rule: {} for rule in R.RULES[1:]}
    for name, ((Hs, Ws), out_hw, minv, _) in R.ROUNDING_CASES.items():
        src = R.int_source(1, 2, Hs, Ws, 12)[0]
        want = R.warp_exact(src, minv, out_hw, R.BORDER)["value"]
        for rule in R.RULES[1:]:
            alt = R.warp_ref64(src.astype(np.float64), minv, out_hw, R.BORDER, rule=rule)["value"]
            changed[rule][name] = int((alt != want).sum())
    for rule, per in changed.items():
        print(f"rule {rule}: changed elements per case {per}")
    for rule in R.RULES[1:]:
        assert sum(changed[rule].values()) > 0, rule
    # which case catches what, as designed: the negative ties catch half-away, all ties catch floor, the `parts` cases
    # catch the rounded sum -- in x and in y, at both signs
    for axis in "xy":
        assert changed["half_away"][f"tie-{axis}-neg"] > 0 and changed["half_away"][f"tie-{axis}-pos"] == 0
        assert changed["floor"][f"tie-{axis}-neg"] > 0 and changed["floor"][f"tie-{axis}-pos"] > 0
        assert changed["sum"][f"parts-{axis}-pos"] > 0
    assert changed["sum"]["parts-x-neg"] > 0


@pytest.mark.parametrize("k", range(4))
def test_random_cases_oracle_within_bound(k):
    """The f32 (f64) restatement stays within 18 * 2^-24 (2^-53) * S of the float64 reference per element: the bound of the
    GPU test is not too tight for a correct implementation.  Also the class counts of the random cases."""
    minv = R.invert(R.RANDOM_MATS[k])
    border = (135.0, 133.0, 132.0)
    src = random_source(3, np.float32, 20 + k)
    ref = R.warp_ref64(src, minv, R.RANDOM_DST, border)
    counts = R.class_counts(ref["cls"])
    print(f"random case {k}: outside/inner/partial = {counts}")
    assert counts[R.INNER] >= 20 and counts[R.PARTIAL] >= 20
    if k == 3:
        assert counts[R.OUTSIDE] >= 20                             # the face partly outside the source
    got = oracle_warp(src, minv, R.RANDOM_DST, border)
    r32 = (np.abs(got.astype(np.float64) - ref["value"]) / (R.U24 * ref["S"])).max()
    src64 = random_source(2, np.float64, 30 + k)
    ref = R.warp_ref64(src64, minv, R.RANDOM_DST, border)
    got = oracle_warp(src64, minv, R.RANDOM_DST, border)
    r64 = (np.abs(got - ref["value"]) / (R.U53 * ref["S"])).max()
    print(f"random case {k}: f32 restatement worst err / (2^-24 S) = {r32:.2f}, f64 worst err / (2^-53 S) = {r64:.2f}")
    assert r32 <= 18 and r64 <= 18
    assert (got[:, ref["cls"] == R.OUTSIDE] == np.array(border[:2])[:, None]).all()


def test_pre_and_post():
    v = np.array([-1.3, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 1.3], dtype=np.float32)
    assert np.array_equal(R.pre32(v), np.array([0, 0, 63.75, 127.5, 159.375, 191.25, 255, 255], dtype=np.float32))
    assert np.array_equal(R.post64(R.pre32(v)), np.clip(v.astype(np.float64), -1, 1))
    assert np.array_equal(R.post64([300.0, -4.0]), [1.0, -1.0])


# --------------------------------------------------------------------------------------------------------------- blur
def test_reflect101():
    assert [R.reflect101(i, 3)[0] for i in range(-4, 8)] == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert R.reflect101(-4, 3) == (0, 2) and R.reflect101(6, 3) == (2, 2) and R.reflect101(-2, 2) == (0, 2)
    for (N, H, W, ksize), twice in R.EXACT_BLUR:
        most = max(R.reflect_table(H, ksize // 2)[1], R.reflect_table(W, ksize // 2)[1])
        assert (most >= 2) == twice, (H, W, ksize, most)
        assert ksize // 2 < 2 * H - 1 and ksize // 2 < 2 * W - 1          # a shape the entry accepts


@pytest.mark.parametrize("case", [c for c, _ in R.EXACT_BLUR], ids=lambda c: "x".join(map(str, c)))
def test_exact_blur_cases(case):
    """Integer arithmetic, the float64 restatement, the fsum reference and (101-free, one-reflection shapes aside) the
    oracle's blur agree bit for bit on dyadic kernels; labels outside the LUT read its first and last entry."""
    N, H, W, ksize = case
    kern_int, shift = R.BINOMIAL[ksize]
    kern = [t / 2.0 ** shift for t in kern_int]
    lab = R.exact_labels(N, H, W, 40)
    assert lab.min() < 0 and lab.max() >= len(R.EXACT_LUT)
    inside = np.clip(lab, 0, len(R.EXACT_LUT) - 1)
    for repeats in (1, 2, 3):
        for edge in (0, 1, 9):
            want = R.blur_exact(lab, R.EXACT_LUT, kern_int, shift, repeats, edge, 8)
            assert np.array_equal(R.blur_numpy(lab, R.EXACT_LUT, kern, repeats, edge, 256.0), want)
            assert np.array_equal(R.blur_fsum(lab, R.EXACT_LUT, kern, repeats, edge, 256.0)[0], want)
            assert np.array_equal(R.blur_exact(inside, R.EXACT_LUT, kern_int, shift, repeats, edge, 8), want)
            if edge == 9 and min(H, W) <= 18:
                assert not want.any()
            elif edge == 0:
                assert want.all() or want.min() == 0
                assert want.max() > 0
    # a constant image stays constant: the kernel sums to one and the reflection adds no weight
    const = R.blur_exact(np.full((1, H, W), 3), R.EXACT_LUT, kern_int, shift, 2, 0, 8)
    assert (const == R.EXACT_LUT[3] / 256.0).all()


def test_oracle_blur_is_the_restatement():
    """oracle/facewarp.py's blur (one repeat, no LUT, no edge, no division) equals blur_numpy bit for bit."""
    from oracle import facewarp as fw
    lab = R.blob_labels(1, 20, 28, 41)
    lut = np.asarray(R.GAUSS_LUT)
    assert np.array_equal(fw.gaussian_kernel(9, 26.0), R.gaussian_kernel(9, 26.0))
    got = fw.gaussian_blur(lut[lab[0]], 9, 26.0)
    assert np.array_equal(got, R.blur_numpy(lab, lut, R.gaussian_kernel(9, 26.0), 1, 0, 1.0)[0])


@pytest.mark.parametrize("case", R.GAUSS_BLUR, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_blur_restatement_within_bound(case):
    """The float64 restatement in the documented order is within repeats (ksize + 2) 2^-53 sum |k| |v| of the fsum
    reference: the bound the kernel gets is not too tight for a correct implementation."""
    ksize, H, W, repeats = case
    lab = R.blob_labels(2, H, W, 42)
    kern = R.gaussian_kernel(ksize, 26.0)
    ref, mag = R.blur_fsum(lab, R.GAUSS_LUT, kern, repeats, 2, 255.0)
    got = R.blur_numpy(lab, R.GAUSS_LUT, kern, repeats, 2, 255.0)
    bound = repeats * (ksize + 2) * R.U53 * mag
    assert (np.abs(got - ref) <= bound).all()
    assert (got[:, :2] == 0).all() and (got[:, :, -2:] == 0).all() and got[:, 2:-2, 2:-2].min() > 0
    ratio = (np.abs(got - ref)[:, 2:-2, 2:-2] / bound[:, 2:-2, 2:-2]).max()
    print(f"blur {case}: f64 restatement worst err / bound = {ratio:.3f}")
