"""GPU: flair_face_crop_u8 (csrc/facecrop.hip, include/flair_facescore.h) against tests/facecrop_ref.py, bit for bit: the crop is
integers after two float64 roundings, so every byte of every case is compared for equality and no tolerance exists."""
import ctypes

import numpy as np
import pytest
import torch

from tests import face_ref as F
from tests import facecrop_ref as R

pytestmark = pytest.mark.gpu


def on(dev, x):
    return None if x is None else torch.from_numpy(np.array(x)).to(dev)         # a copy: the shared arrays are read-only


def crop(dev, frames, minv, index, out_hw, frames2=None, **kw):
    """ops.face_crop_u8 on numpy inputs -> numpy crops of a (and of b)."""
    from flair_amd import ops
    minv = np.asarray(minv, dtype=np.float64).reshape(-1, 6)
    got = ops.face_crop_u8(on(dev, frames), on(dev, minv), minv, torch.tensor(list(index), dtype=torch.int32).to(dev), list(index), out_hw,
                           b=on(dev, frames2), **kw)
    return got.cpu().numpy() if frames2 is None else tuple(t.cpu().numpy() for t in got)


def assert_same(got, want, ref=None):
    if not np.array_equal(got, want):
        idx = tuple(int(v) for v in np.argwhere(got != want)[0])
        where = "" if ref is None else ": " + F.describe(ref, idx[-3:-1])
        raise AssertionError(f"{int((got != want).sum())} bytes differ, the first at {idx}: got {got[idx]}, want {want[idx]}{where}")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_case_bit_for_bit(dev, name):
    """The copy, the quarter-pixel translations, the half-pixel step with both clamps, the rotation with all three window
    classes, the crop wholly outside, the 1 x 1 and 3 x 5 sources, the 1 x 1 destination and the rounding ties."""
    _, out_hw, m = R.CASES[name]
    ref = R.case(name)
    if name == "step":
        assert (int(ref["raw"].min()), int(ref["raw"].max())) == R.STEP_RANGE               # on the reference first: both clamps act
    if name == "rotation":
        assert F.class_counts(ref["cls"]) == R.ROTATION_CLASSES and min(R.ROTATION_CLASSES) > 0
    got = crop(dev, R.case_source(name)[None], m, [0], out_hw)
    assert got.shape == (1,) + tuple(out_hw) + (3,) and got.dtype == np.uint8
    assert_same(got[0], ref["value"], ref)
    if name == "copy":
        assert np.array_equal(got[0], R.frames()[0][3:19, 5:29])
    if name == "outside":
        assert (got[0] == np.array(R.BORDER, dtype=np.uint8)).all()


def test_faces_of_two_frames_through_src_index_and_both_sets(dev):
    """Three faces cut from frame 1 and one from frame 0, at 21 x 70 (two column groups, a ragged last row group); one frame set
    against two gives the same bits for a; a face alone and as face 2 of 4; two runs give the same bits."""
    a, b = R.frames(), R.frames(2, R.HS, R.WS, seed=12)
    want_a = R.crop_batch(a, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW)
    want_b = R.crop_batch(b, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW)
    assert not np.array_equal(want_a, want_b)
    got_a, got_b = crop(dev, a, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW, frames2=b)
    assert_same(got_a, want_a)
    assert_same(got_b, want_b)
    alone = crop(dev, a, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW)
    assert np.array_equal(alone, got_a)                                             # one set against two
    face2 = crop(dev, a, R.MULTI_MINV[2:3], R.MULTI_INDEX[2:3], R.MULTI_HW)
    assert np.array_equal(face2[0], got_a[2])                                       # alone and as face 2 of 4
    again_a, again_b = crop(dev, a, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW, frames2=b)
    assert np.array_equal(again_a, got_a) and np.array_equal(again_b, got_b)        # two runs in a row


def test_no_face_is_a_no_op(dev):
    from flair_amd import _lib, ops
    a = on(dev, R.frames())
    out = ops.face_crop_u8(a, torch.zeros((0, 6), dtype=torch.float64, device=dev), np.zeros((0, 6)), torch.zeros(0, dtype=torch.int32, device=dev), [],
                           (16, 24))
    assert tuple(out.shape) == (0, 16, 24, 3) and out.dtype == torch.uint8
    # the entry itself: K = 0 enqueues nothing and leaves a guarded output alone
    guard = torch.full((64,), 77, dtype=torch.uint8, device=dev)
    _lib.call.flair_face_crop_u8(a, None, 2, R.HS, R.WS, None, None, 0, 16, 24, (ctypes.c_uint8 * 3)(*R.BORDER), guard, None)
    torch.cuda.synchronize()
    assert (guard == 77).all()


def test_sources_and_outputs_at_odd_byte_addresses(dev):
    """Every buffer starts at an odd address inside a larger one whose other bytes must stay what they were."""
    from flair_amd import ops
    a, b = R.frames(), R.frames(2, R.HS, R.WS, seed=12)
    K, (Hd, Wd) = len(R.MULTI_INDEX), R.MULTI_HW
    n_src, n_out = a.size, K * Hd * Wd * 3

    def odd(n, fill):
        buf = torch.full((n + 2,), fill, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 2 == 0
        return buf, buf[1:n + 1]
    buf_a, va = odd(n_src, 0)
    buf_b, vb = odd(n_src, 0)
    va.copy_(on(dev, a).reshape(-1))
    vb.copy_(on(dev, b).reshape(-1))
    buf_oa, oa = odd(n_out, 201)
    buf_ob, ob = odd(n_out, 202)
    ta, tb = va.view(a.shape), vb.view(b.shape)
    toa, tob = oa.view(K, Hd, Wd, 3), ob.view(K, Hd, Wd, 3)
    assert all(t.data_ptr() % 2 == 1 and t.is_contiguous() for t in (ta, tb, toa, tob))
    minv = np.asarray(R.MULTI_MINV, dtype=np.float64)
    got = ops.face_crop_u8(ta, on(dev, minv), minv, torch.tensor(R.MULTI_INDEX, dtype=torch.int32).to(dev), list(R.MULTI_INDEX), R.MULTI_HW, b=tb,
                           out_a=toa, out_b=tob)
    assert got[0].data_ptr() == toa.data_ptr() and got[1].data_ptr() == tob.data_ptr()
    assert_same(toa.cpu().numpy(), R.crop_batch(a, minv, R.MULTI_INDEX, R.MULTI_HW))
    assert_same(tob.cpu().numpy(), R.crop_batch(b, minv, R.MULTI_INDEX, R.MULTI_HW))
    for buf, fill in ((buf_oa, 201), (buf_ob, 202)):
        assert int(buf[0]) == fill and int(buf[-1]) == fill                        # the bytes around an output


def test_other_borders(dev):
    m = R.CASES["quarter-xy"][2]
    for border in ((0, 0, 0), (255, 1, 128)):
        got = crop(dev, R.frames()[:1], m, [0], (16, 24), border=border)
        assert_same(got[0], R.crop(R.frames()[0], m, (16, 24), border)["value"])


def test_every_refusal_of_the_header(dev):
    from flair_amd import _lib, ops
    lib = _lib.lib()
    for name, args, what in R.entry_refusals():
        R.assert_refused(lib, name, args, what)
    # on real tensors: an output inside a source is refused by the entry, a far matrix and a wrong index by the wrapper
    a = on(dev, R.frames())
    m = np.array([[1.0, 0, 5, 0, 1, 3]])
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    inside = a.view(-1)[7:7 + 4 * 5 * 3].view(1, 4, 5, 3)
    with pytest.raises(_lib.FlairHipError, match=r"flair_face_crop_u8: out overlaps a source"):
        ops.face_crop_u8(a, on(dev, m), m, idx, [0], (4, 5), out_a=inside)
    with pytest.raises(_lib.FlairHipError, match=r"flair_face_crop_u8: out overlaps a source"):
        ops.face_crop_u8(a[:1], on(dev, m), m, idx, [0], (4, 5), b=a[1:], out_b=inside)
    with pytest.raises(ValueError, match=r"face_crop_u8: src_index outside \[0, 2\)"):
        ops.face_crop_u8(a, on(dev, m), m, idx, [2], (4, 5))
    far = np.array([[1.0, 0, 40000, 0, 1, 3]])
    with pytest.raises(ValueError, match=r"face_crop_u8: matrix 0 maps a corner of the crop beyond \+-32000 source pixels"):
        ops.face_crop_u8(a, on(dev, far), far, idx, [0], (4, 5))
    assert np.array_equal(a.cpu().numpy(), R.frames())                              # nothing was written


def test_a_source_beyond_two_to_the_31_bytes(dev):
    """One frame of 26760 x 26760 pixels (2.15e9 bytes, never filled) with a patch of random bytes in its last corner: a crop
    over that corner reads at byte offsets past 2^31 and equals the crop of the patch alone under the shifted matrix."""
    from flair_amd import ops
    side, ph, pw = 26760, 32, 64
    assert side * side * 3 > 1 << 31
    patch = R.frames(1, ph, pw, seed=9)[0]
    big = torch.empty((1, side, side, 3), dtype=torch.uint8, device=dev)
    big[0, side - ph:, side - pw:] = on(dev, patch)
    m = np.array([[1.0, 0, side - 20.5, 0, 1, side - 12.25]])
    want = R.crop(patch, [1.0, 0, pw - 20.5, 0, 1, ph - 12.25], (16, 24))
    assert F.class_counts(want["cls"])[1] > 50 and F.class_counts(want["cls"])[2] > 50 and want["sx"].min() >= 0 and want["sy"].min() >= 0
    got = ops.face_crop_u8(big, on(dev, m), m, torch.zeros(1, dtype=torch.int32, device=dev), [0], (16, 24))
    assert_same(got[0].cpu().numpy(), want["value"], want)
