"""The entries of csrc/face.hip against tests/face_ref.py, the reference written from the definition, through the ops
wrappers.  tests/test_face_exact_cpu.py proves the cases (window classes reached, exactness, that another rounding rule
of the coordinates changes outputs) and that the reference agrees with oracle/facewarp.py.

  flair_warp_affine_cubic(_indexed)
      bit for bit: integer sources in [0, 31] at quarter-pixel positions and at coordinate ties, C = 1 .. 4, f32 and f64
                   sources, 1x9 .. 7x9 sources; outside pixels = the border value; pre = post = 0 on random data against
                   the numpy restatement of oracle/facewarp.py, which never contracts a product into a sum
      per element: random data under four similarity transforms,
                   f32: |got - ref64| <= 18 * 2^-24 * S -- 16 products rounded once, one more subtraction each in a
                        partial window, summed along the documented order (the f32 restatement on the CPU stays below
                        4.3 * 2^-24 * S, tests/test_face_exact_cpu.py);
                   post: 2 / 255 of that + 3 * 2^-24 (three roundings of a value of at most 1);
                   f64: 18 * 2^-53 * S + half an ulp of the f32 result
  flair_face_blend      bit for bit against x0 (1 - m) + face m in numpy f32, one case beyond one grid pass
  flair_face_paste      bit for bit against warp(face), warp(mask), blend face by face for C = 1, 2, 4 and 3 x 5 faces;
                        bit for bit against x0's or the face's value on 0 / 1 masks under integer translations
  flair_face_mask_blur  bit for bit against integers on binomial kernels (reflections that reflect twice, repeats 1 .. 3,
                        edge 0 / 1 / all, labels outside the LUT); bit for bit against the float64 restatement in the
                        documented order and within repeats (ksize + 2) 2^-53 sum |k| |v| of the fsum reference on
                        Gaussian kernels; refusals exactly at ksize / 2 = 2 H - 1 and 2 W - 1

"Bit for bit" compares values of non-NaN floats, i.e. the bits up to the sign of a zero, which is no part of the contract
(tests/util.py assert_bits_equal).  The worst err / bound of every per-element assertion goes to parity_log
(profiles/face_exact_parity.txt is the record).
"""
import numpy as np
import pytest
import torch

from tests import face_ref as R
from tests.test_face_exact_cpu import oracle_warp, random_source
from tests.util import parity_log

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f64": np.float64}


def _ops():
    from flair_amd import ops
    return ops


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _minv(mats, dev):
    return _dev(np.stack([np.asarray(m, dtype=np.float64).reshape(6) for m in mats]), dev)


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def assert_same(got, want, what, refs=None):
    """got (torch, any device) equals want (numpy) element by element; refs: per leading index the warp reference whose
    class and tap position describe the first differing element."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    ne = got != want
    if ne.any():
        idx = tuple(int(i) for i in np.argwhere(ne)[0])
        where = f": {R.describe(refs[idx[0]], idx)}" if refs is not None else ""
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} element(s) differ; first at {list(idx)}: got {got[idx]!r}, "
                             f"expected {want[idx]!r}{where}")


def within(got, ref, bound, what):
    """|got - ref| <= bound per element -> the worst err / bound (0 / 0 counts as 0)."""
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)
    assert not np.isnan(err).any(), f"{what}: NaN"
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    if (err > bound).any():
        idx = tuple(int(i) for i in np.argwhere(err > bound)[0])
        raise AssertionError(f"{what}: {int((err > bound).sum())} of {err.size} element(s) beyond the bound, worst err / bound "
                             f"{ratio.max():.3f}; first at {list(idx)}: err {err[idx]:.3e} > {bound[idx]:.3e}, expected {ref[idx]!r}")
    return float(ratio.max())


# --------------------------------------------------------------------------------------------------------- warp, exact
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(R.WARP_CASES))
def test_warp_exact(dev, name, dtype):
    ops = _ops()
    (Hs, Ws), out_hw, minv, _ = R.WARP_CASES[name]
    for C in (1, 2, 3, 4):
        src = R.int_source(2, C, Hs, Ws, 50 + C)
        refs = [R.warp_exact(s, minv, out_hw, R.BORDER) for s in src]
        want = np.stack([r["value"] for r in refs]).astype(np.float32)
        got = ops.warp_affine_cubic(_dev(src.astype(DTYPES[dtype]), dev), _minv([minv, minv], dev), out_hw, border=R.BORDER[:C])
        assert_same(got, want, f"warp {name} C={C} {dtype}", refs)
        out = np.stack([r["cls"] for r in refs]) == R.OUTSIDE
        assert (got.cpu().numpy()[:, :, out[0]] == np.array(R.BORDER[:C], dtype=np.float32)[None, :, None]).all()


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_warp_exact_one_matrix_per_image_and_indexed(dev, dtype):
    """Four outputs with a matrix each: the plain entry on four sources, the indexed entry on three sources through the
    list (2, 0, 2, 1), which is no permutation of itself and names source 2 twice."""
    ops = _ops()
    names = ["7x9-scale", "7x9-turn", "7x9-shift", "tie-x-neg"]
    mats = [R.WARP_CASES[n][2] for n in names]
    out_hw = (40, 48)
    index = [2, 0, 2, 1]
    for C in (1, 2, 3, 4):
        src = R.int_source(4, C, 7, 9, 60 + C)
        sd = _dev(src.astype(DTYPES[dtype]), dev)
        refs = [R.warp_exact(src[k], mats[k], out_hw, R.BORDER) for k in range(4)]
        got = ops.warp_affine_cubic(sd, _minv(mats, dev), out_hw, border=R.BORDER[:C])
        assert_same(got, np.stack([r["value"] for r in refs]).astype(np.float32), f"warp, 4 matrices, C={C} {dtype}", refs)
        refs = [R.warp_exact(src[index[k]], mats[k], out_hw, R.BORDER) for k in range(4)]
        got = ops.warp_affine_cubic(sd[:3].contiguous(), _minv(mats, dev), out_hw, border=R.BORDER[:C],
                                    src_index=_i32(index, dev), src_index_host=index)
        assert got.shape == (4, C) + out_hw
        assert_same(got, np.stack([r["value"] for r in refs]).astype(np.float32), f"indexed warp C={C} {dtype}", refs)


# ------------------------------------------------------------------------------------------------- warp, random data
CROP_BORDER = (135.0, 133.0, 132.0)


def _random_refs(C, dtype, seed, signed, pre, border):
    minvs = [R.invert(M) for M in R.RANDOM_MATS]
    src = np.stack([random_source(C, dtype, seed + k, signed) for k in range(4)])
    refs = [R.warp_ref64(src[k], minvs[k], R.RANDOM_DST, border, pre=pre) for k in range(4)]
    return minvs, src, refs, np.stack([r["value"] for r in refs]), np.stack([r["S"] for r in refs])


@pytest.mark.parametrize("pre,post", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("indexed", [False, True], ids=["plain", "indexed"])
def test_warp_f32_per_element(dev, pre, post, indexed):
    ops = _ops()
    minvs, src, refs, value, S = _random_refs(3, np.float32, 70, pre, pre, CROP_BORDER)
    kw = dict(border=CROP_BORDER, pre=pre, post=post)
    if indexed:                                                   # the sources stored in another order, read back through the list
        order = [3, 1, 0, 2]
        index = [order.index(k) for k in range(4)]
        got = ops.warp_affine_cubic(_dev(src[order], dev), _minv(minvs, dev), R.RANDOM_DST, src_index=_i32(index, dev),
                                    src_index_host=index, **kw)
    else:
        got = ops.warp_affine_cubic(_dev(src, dev), _minv(minvs, dev), R.RANDOM_DST, **kw)
    bound = 18 * R.U24 * S
    if post:
        value, bound = R.post64(value), 2.0 / 255.0 * bound + 3 * R.U24
    what = f"warp f32 pre={pre} post={post} {'indexed' if indexed else 'plain'}"
    ratio = within(got, value, bound, what)
    parity_log(f"face_exact {what}: worst err/bound {ratio:.3f}")
    if not post:
        outside = np.stack([r["cls"] for r in refs]) == R.OUTSIDE
        assert outside.sum() >= 20
        g = got.cpu().numpy()
        for k in range(3):
            assert (g[:, k][outside] == np.float32(CROP_BORDER[k])).all()
    if not pre and not post:                                      # numpy never contracts: a fused multiply-add in face.hip fails here
        want = np.stack([oracle_warp(src[k], minvs[k], R.RANDOM_DST, CROP_BORDER) for k in range(4)])
        assert_same(got, want, what + " vs the numpy restatement", refs)


def test_warp_f64_per_element(dev):
    ops = _ops()
    border = (0.0, 7.0)
    minvs, src, refs, value, S = _random_refs(2, np.float64, 80, False, False, border)
    got = ops.warp_affine_cubic(_dev(src, dev), _minv(minvs, dev), R.RANDOM_DST, border=border)
    g = got.cpu().numpy()
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(g), np.abs(value.astype(np.float32)))).astype(np.float64)
    ratio = within(got, value, 18 * R.U53 * S + half_ulp, "warp f64")
    # the cast to f32 dominates that bound; the sum's own share: what exceeds the cast's half ulp, over 18 * 2^-53 * S
    own = (np.maximum(np.abs(g.astype(np.float64) - value) - half_ulp, 0.0) / np.maximum(18 * R.U53 * S, 1e-300)).max()
    parity_log(f"face_exact warp f64: worst err/bound {ratio:.3f}, beyond the cast's half ulp {own:.3f} of 18 * 2^-53 * S")
    outside = np.stack([r["cls"] for r in refs]) == R.OUTSIDE
    for k in range(2):
        assert (g[:, k][outside] == np.float32(border[k])).all()
    want = np.stack([oracle_warp(src[k], minvs[k], R.RANDOM_DST, border) for k in range(4)]).astype(np.float32)
    assert_same(got, want, "warp f64 vs the numpy restatement", refs)


# -------------------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("shape", [(2, 1, 40, 56), (2, 3, 40, 56), (1, 4, 40, 56), (1, 3, 600, 600)], ids=lambda s: "x".join(map(str, s)))
def test_blend_bits(dev, shape):
    """1 x 3 x 600 x 600 has 1,080,000 elements, more than the 4096 x 256 threads of the grid: the grid-stride loop takes
    a second step."""
    N, C, H, W = shape
    rng = np.random.default_rng(90)
    x0, face = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    m = rng.random((N, 1, H, W)).astype(np.float32)
    m.reshape(-1)[:3] = (0.0, 1.0, 0.5)
    want = x0 * (np.float32(1) - m) + face * m
    assert want.dtype == np.float32
    if H == 600:
        assert want.size > 4096 * 256
    got = _ops().face_blend(_dev(x0, dev), _dev(face, dev), _dev(m, dev))
    assert_same(got, want, f"blend {shape}")


# -------------------------------------------------------------------------------------------------------------- paste
PT, PH, PW = 3, 40, 56


def _paste_case(C, h, w, seed):
    """Four faces in three frames, frame_start = (0, 2, 2, 4): two overlapping faces in frame 0, none in frame 1, two in
    frame 2, the last one cut by the frame's left and top edge.  The dst -> src matrices are similarities frame -> face."""
    rng = np.random.default_rng(seed)
    s = w / 24.0
    minv = [R.similarity(s, 0.1, -6 * s, -4 * s), R.similarity(1.2 * s, -0.3, -14 * s, -2 * s),
            R.similarity(0.8 * s, 0.25, -20 * s, -9 * s), R.similarity(s, -0.15, 5 * s, 3 * s)]
    x0 = np.clip(rng.standard_normal((PT, C, PH, PW)) * 0.6, -1.3, 1.3).astype(np.float32)
    faces = np.clip(rng.standard_normal((4, C, h, w)) * 0.6, -1.3, 1.3).astype(np.float32)
    masks = rng.random((4, 1, h, w))
    return x0, faces, masks, minv, [0, 2, 2, 4]


@pytest.mark.parametrize("C,h,w", [(1, 10, 12), (2, 10, 12), (4, 10, 12), (3, 3, 5)], ids=lambda v: str(v))
def test_paste_equals_the_launch_sequence(dev, C, h, w):
    from tests.test_gpu_faces_all import _three_launches
    ops = _ops()
    x0, faces, masks, minv, fs = _paste_case(C, h, w, 100 + C)
    x0d, fd, md, mi = _dev(x0, dev), _dev(faces, dev), _dev(masks, dev), _minv(minv, dev)
    want = _three_launches(x0d, fd, md, mi, fs)
    got = ops.face_paste(x0d, fd, md, mi, _i32(fs, dev), fs)
    torch.cuda.synchronize()
    assert_same(got, want.cpu().numpy(), f"paste C={C} faces {h}x{w}")
    assert torch.equal(got[1], x0d[1])
    for t in (0, 2):
        assert (got[t] != x0d[t]).float().mean().item() > 0.05   # the faces cover a part of the frame worth testing


def test_paste_exact_translations(dev):
    """Masks of 0 and 1, integer translations, face values whose pre / post round trip is exact: every output element is
    the frame's value or the value of the last face in list order whose mask is 1 there."""
    C, h, w = 3, 8, 8
    rng = np.random.default_rng(110)
    x0 = rng.standard_normal((PT, C, PH, PW)).astype(np.float32)
    x0[x0 == 0] = 1.0
    levels = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32)
    assert np.array_equal(R.post64(R.pre32(levels)), levels.astype(np.float64))
    faces = levels[rng.integers(0, 5, (4, C, h, w))]
    masks = rng.integers(0, 2, (4, 1, h, w)).astype(np.float64)
    shifts = [(5, 3), (9, 6), (-3, -2), (51, 35)]                # face k sits at frame pixel (tx, ty): two overlap, two are cut
    fs = [0, 2, 2, 4]
    want = x0.copy()
    taken = 0
    for t in range(PT):
        for k in range(fs[t], fs[t + 1]):
            tx, ty = shifts[k]
            for y in range(max(ty, 0), min(ty + h, PH)):
                for x in range(max(tx, 0), min(tx + w, PW)):
                    if masks[k, 0, y - ty, x - tx] == 1.0:
                        want[t, :, y, x] = faces[k, :, y - ty, x - tx]
                        taken += 1
    assert taken > 60
    minv = [np.array([[1, 0, -tx], [0, 1, -ty]], dtype=np.float64) for tx, ty in shifts]
    got = _ops().face_paste(_dev(x0, dev), _dev(faces, dev), _dev(masks, dev), _minv(minv, dev), _i32(fs, dev), fs)
    assert_same(got, want, "paste, 0 / 1 masks under integer translations")


# --------------------------------------------------------------------------------------------------------- mask blur
def _blur(dev, lab, lut, kern, repeats, edge, div):
    N, H, W = lab.shape
    out = _ops().face_mask_blur(_dev(lab.astype(np.int32).reshape(-1), dev), N, H, W, _dev(np.asarray(lut, dtype=np.float64), dev),
                                _dev(np.asarray(kern, dtype=np.float64), dev), repeats=repeats, edge=edge, div=div)
    assert out.shape == (N, 1, H, W) and out.dtype == torch.float64
    return out[:, 0]


@pytest.mark.parametrize("case", [c for c, _ in R.EXACT_BLUR], ids=lambda c: "x".join(map(str, c)))
def test_blur_exact(dev, case):
    N, H, W, ksize = case
    kern_int, shift = R.BINOMIAL[ksize]
    kern = [t / 2.0 ** shift for t in kern_int]
    lab = R.exact_labels(N, H, W, 40)
    for repeats in (1, 2, 3):
        for edge in (0, 1, 9):
            want = R.blur_exact(lab, R.EXACT_LUT, kern_int, shift, repeats, edge, 8)
            got = _blur(dev, lab, R.EXACT_LUT, kern, repeats, edge, 256.0)
            assert_same(got, want, f"blur {case} repeats={repeats} edge={edge}")


@pytest.mark.parametrize("case", R.GAUSS_BLUR, ids=lambda c: "x".join(map(str, c)))
def test_blur_gaussian(dev, case):
    ksize, H, W, repeats = case
    lab = R.blob_labels(2, H, W, 42)
    kern = R.gaussian_kernel(ksize, 26.0)
    got = _blur(dev, lab, R.GAUSS_LUT, kern, repeats, 2, 255.0)
    assert_same(got, R.blur_numpy(lab, R.GAUSS_LUT, kern, repeats, 2, 255.0), f"blur {case} vs the f64 restatement")
    ref, mag = R.blur_fsum(lab, R.GAUSS_LUT, kern, repeats, 2, 255.0)
    ratio = within(got, ref, repeats * (ksize + 2) * R.U53 * mag, f"blur {case} vs fsum")
    parity_log(f"face_exact blur ksize={ksize} {H}x{W} repeats={repeats}: worst err/bound {ratio:.3f}")


def test_blur_refuses_exactly_at_two_reflections(dev):
    from flair_amd import _lib
    for H, W in ((3, 8), (8, 3)):
        lab = R.blob_labels(2, H, W, 43)
        with pytest.raises(_lib.FlairHipError, match="kernel wider than two reflections"):
            _blur(dev, lab, R.GAUSS_LUT, R.gaussian_kernel(11, 26.0), 1, 0, 255.0)      # 11 // 2 = 2 * 3 - 1
        kern = R.gaussian_kernel(9, 26.0)                                                # 9 // 2 = 2 * 3 - 2
        assert_same(_blur(dev, lab, R.GAUSS_LUT, kern, 1, 0, 255.0), R.blur_numpy(lab, R.GAUSS_LUT, kern, 1, 0, 255.0),
                    f"blur 9 taps on {H}x{W}")
    with pytest.raises(_lib.FlairHipError, match="kernel wider than two reflections"):  # 101 // 2 = 50 >= 2 * 20 - 1
        _blur(dev, R.blob_labels(2, 20, 28, 42), R.GAUSS_LUT, R.gaussian_kernel(101, 26.0), 2, 2, 255.0)
