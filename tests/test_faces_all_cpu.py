"""CPU: several faces per frame / frames without a face -- the two ABI entries' declarations and refusals, the ops wrappers'
refusals, the host-side face selection (retinaface_utils.select_faces) and the command line options."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("flair_warp_affine_cubic_indexed", "flair_face_paste")
_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]])


def _face(cx, cy, size, score=0.9):
    """Box + score + five landmarks of a face of ``size`` pixels centred at (cx, cy) (the 512 template scaled)."""
    lm = (_TPL / 512.0 - 0.5) * size + np.array([cx, cy])
    return np.concatenate([[cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, score], lm.reshape(-1)]).astype(np.float32)


def _none():
    return np.zeros((0, 15), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_library_exports_both_entries():
    from flair_amd import _lib
    text = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for n in ENTRIES:
        assert n in names and hasattr(lib, n), n
    assert lib.flair_abi_version() >= 12


def _indexed(lib, *, src=16, idx=16, minv=16, dst=16, border=True, N=2, C=3, Nsrc=2):
    b = (ctypes.c_float * 4)(0, 0, 0, 0) if border else None
    return lib.flair_warp_affine_cubic_indexed(ctypes.c_void_p(src), 0, Nsrc, ctypes.c_void_p(idx), N, C, 8, 8,
                                               ctypes.c_void_p(minv), 8, 8, b, 0, 0, ctypes.c_void_p(dst), None)


def _paste(lib, *, x0=16, faces=16, masks=16, minv=16, fs=16, out=1 << 30, T=2, C=3, K=2, H=8, W=8, h=8, w=8):
    return lib.flair_face_paste(ctypes.c_void_p(x0), T, C, H, W, ctypes.c_void_p(faces), ctypes.c_void_p(masks),
                                ctypes.c_void_p(minv), K, h, w, ctypes.c_void_p(fs), ctypes.c_void_p(out), None)


@pytest.mark.parametrize("bad", [dict(src=0), dict(idx=0), dict(minv=0), dict(dst=0), dict(border=False), dict(N=-1), dict(C=5),
                                 dict(Nsrc=0)])
def test_indexed_warp_entry_refuses_before_any_launch(bad):
    from flair_amd import _lib
    lib = _lib.lib()
    assert _indexed(lib, **bad) == -1
    assert b"flair_warp_affine_cubic_indexed" in lib.flair_last_error()


@pytest.mark.parametrize("bad", [dict(x0=0), dict(out=0), dict(fs=0), dict(faces=0), dict(masks=0), dict(minv=0), dict(K=-1),
                                 dict(T=0), dict(C=5), dict(H=0), dict(w=0), dict(out=16)])
def test_face_paste_entry_refuses_before_any_launch(bad):
    from flair_amd import _lib
    lib = _lib.lib()
    assert _paste(lib, **bad) == -1
    msg = lib.flair_last_error()
    assert b"flair_face_paste" in msg
    if bad == dict(fs=0):
        assert b"frame_start" in msg
    if bad == dict(out=16):
        assert b"alias" in msg


# ----------------------------------------------------------------------------------------------------- ops wrappers
def _paste_args(T=2, K=2):
    return (torch.zeros(T, 3, 8, 8), torch.zeros(K, 3, 6, 6), torch.zeros(K, 1, 6, 6, dtype=torch.float64),
            torch.zeros(K, 6, dtype=torch.float64), torch.tensor([0, 1, 2], dtype=torch.int32))


def test_ops_face_paste_refusals():
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    x0, faces, masks, minv, fs = _paste_args()
    with pytest.raises(FlairHipError, match="HBM"):                          # CPU tensors
        ops.face_paste(x0, faces, masks, minv, fs, [0, 1, 2])
    with pytest.raises(FlairHipError, match="HBM"):                          # ... also for K = 0
        ops.face_paste(x0, None, None, None, fs, [0, 0, 0])
    with pytest.raises(ValueError, match="x0"):                              # non-contiguous
        ops.face_paste(torch.zeros(2, 3, 8, 16)[..., ::2], faces, masks, minv, fs, [0, 1, 2])
    with pytest.raises(ValueError, match="faces"):
        ops.face_paste(x0, torch.zeros(2, 3, 6, 12)[..., ::2], masks, minv, fs, [0, 1, 2])
    with pytest.raises(ValueError, match="masks"):                           # wrong dtype
        ops.face_paste(x0, faces, masks.float(), minv, fs, [0, 1, 2])
    with pytest.raises(ValueError, match="minv"):
        ops.face_paste(x0, faces, masks, minv.float(), fs, [0, 1, 2])
    with pytest.raises(ValueError, match="frame_start"):                     # not (T + 1,) int32
        ops.face_paste(x0, faces, masks, minv, fs.long(), [0, 1, 2])
    with pytest.raises(ValueError, match="frame_start"):
        ops.face_paste(x0, faces, masks, minv, fs[:2], [0, 1, 2])
    for host in ([0, 2, 1], [1, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2]):       # decreasing / not from 0 / not to K / short
        with pytest.raises(ValueError, match="non-decreasing"):
            ops.face_paste(x0, faces, masks, minv, fs, host)


def test_ops_indexed_warp_refusals():
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    src, minv = torch.zeros(2, 3, 8, 8), torch.zeros(3, 6, dtype=torch.float64)
    idx = torch.tensor([0, 0, 1], dtype=torch.int32)
    with pytest.raises(FlairHipError, match="HBM"):
        ops.warp_affine_cubic(src, minv, (4, 4), src_index=idx, src_index_host=[0, 0, 1])
    with pytest.raises(ValueError, match="src must"):
        ops.warp_affine_cubic(torch.zeros(2, 3, 8, 16)[..., ::2], minv, (4, 4), src_index=idx, src_index_host=[0, 0, 1])
    with pytest.raises(ValueError, match="src_index must"):
        ops.warp_affine_cubic(src, minv, (4, 4), src_index=idx.long(), src_index_host=[0, 0, 1])
    with pytest.raises(ValueError, match="minv"):
        ops.warp_affine_cubic(src, minv[:2], (4, 4), src_index=idx, src_index_host=[0, 0, 1])
    for host in ([0, 0, 2], [-1, 0, 1]):                                     # out of range
        with pytest.raises(ValueError, match="outside"):
            ops.warp_affine_cubic(src, minv, (4, 4), src_index=idx, src_index_host=host)
    with pytest.raises(ValueError, match="src_index_host"):
        ops.warp_affine_cubic(src, minv, (4, 4), src_index=idx)


# ------------------------------------------------------------------------------------------------------ select_faces
def test_select_faces_pairs_faces_with_frames_across_an_empty_frame():
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial, select_faces
    small, big, mid = _face(30, 34, 24), _face(70, 62, 72), _face(90, 40, 40)
    dets = [np.stack([small, big]), _none(), np.stack([mid]), np.stack([small, mid, big])]
    mats, frames = select_faces(dets, 128, 128, _TPL)
    assert frames == [0, 0, 2, 3, 3, 3]

    def fit(d):
        return estimate_affine_partial(d[5:15].reshape(5, 2), _TPL)
    want = [big, small, mid, big, mid, small]                                # per frame: decreasing area
    assert all(np.array_equal(m, fit(d)) for m, d in zip(mats, want))
    # the cap keeps the largest ones; the pairing after the empty frame is unchanged
    mats2, frames2 = select_faces(dets, 128, 128, _TPL, max_faces=2)
    assert frames2 == [0, 0, 2, 3, 3]
    assert all(np.array_equal(m, fit(d)) for m, d in zip(mats2, [big, small, mid, big, mid]))
    assert select_faces([_none(), _none()], 128, 128, _TPL) == ([], [])
    with pytest.raises(ValueError):
        select_faces(dets, 128, 128, _TPL, max_faces=0)


def test_select_faces_threshold_ties_and_clamped_area():
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial, select_faces
    small, big = _face(30, 34, 24), _face(70, 62, 72)
    eye = np.linalg.norm(small[5:7] - small[7:9])
    assert eye < 6 < np.linalg.norm(big[5:7] - big[7:9])
    mats, frames = select_faces([np.stack([small, big]), np.stack([small])], 128, 128, _TPL, eye_dist_threshold=6.0)
    assert frames == [0]                                                     # the small face is dropped in both frames
    assert np.array_equal(mats[0], estimate_affine_partial(big[5:15].reshape(5, 2), _TPL))
    # equal areas keep the detector's order
    a, b = _face(40, 40, 32), _face(90, 90, 32)
    mats, _ = select_faces([np.stack([b, a])], 128, 128, _TPL)
    assert np.array_equal(mats[0], estimate_affine_partial(b[5:15].reshape(5, 2), _TPL))
    # the area is that of the box clamped to the image: a large face mostly outside the frame ranks below a smaller one inside
    out, inside = _face(-20, 64, 80), _face(80, 64, 48)
    mats, _ = select_faces([np.stack([out, inside])], 128, 128, _TPL, max_faces=1)
    assert np.array_equal(mats[0], estimate_affine_partial(inside[5:15].reshape(5, 2), _TPL))


def test_select_faces_max_one_is_the_largest_face_rule():
    """max_faces=1 on frames that all have a face == get_crop_face(only_keep_largest=True)'s choice and matrices."""
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial, get_largest_face, select_faces
    rng = np.random.default_rng(3)
    dets = [np.stack([_face(*rng.uniform(10, 118, 2), rng.uniform(16, 90)) for _ in range(int(rng.integers(1, 5)))])
            for _ in range(6)]
    mats, frames = select_faces(dets, 128, 128, _TPL, eye_dist_threshold=0.1, max_faces=1)
    assert frames == list(range(6))
    for m, d in zip(mats, dets):
        _, k = get_largest_face([b[0:5] for b in d], 128, 128)
        assert np.array_equal(m, estimate_affine_partial(d[k][5:15].reshape(5, 2), _TPL))


def test_frame_starts_and_helper_refusals():
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    assert FaceRestoreHelper.frame_starts([0, 0, 2], 3) == [0, 2, 2, 3]
    assert FaceRestoreHelper.frame_starts([], 2) == [0, 0, 0]
    for bad in ([1, 0], [0, 3], [-1, 0]):
        with pytest.raises(ValueError):
            FaceRestoreHelper.frame_starts(bad, 3)
    h = FaceRestoreHelper(device="cpu", detector=object())
    with pytest.raises(NotImplementedError, match="detector"):               # an external detector has no per-frame pairing
        h.get_crop_faces_all(torch.zeros(1, 3, 64, 64))
    h = FaceRestoreHelper(device="cpu")
    with pytest.raises(ValueError, match="one frame index per affine matrix"):
        h.get_crop_face_from_affine_matrices(torch.zeros(2, 3, 8, 8), [np.eye(2, 3)], face_frames=[0, 1])


def test_window_faces_rejects_an_unknown_mode():
    from flair_amd import video
    with pytest.raises(ValueError, match="largest, all"):
        video.window_faces(None, torch.zeros(1, 3, 8, 8), faces="every")


# ------------------------------------------------------------------------------------------------------ command line
def test_command_line_parses_faces_options():
    from flair_amd.__main__ import faces_of, make_parser
    ap = make_parser()
    a = ap.parse_args(["restore", "gaussian", "in", "out"])
    assert a.faces == "largest" and a.max_faces == 4 and faces_of(a) == {}
    a = ap.parse_args(["restore", "gaussian", "in", "out", "--faces", "all", "--max-faces", "2"])
    assert a.faces == "all" and a.max_faces == 2 and faces_of(a) == dict(faces="all", max_faces=2)
    with pytest.raises(SystemExit):
        ap.parse_args(["restore", "gaussian", "in", "out", "--faces", "some"])
    with pytest.raises(SystemExit):
        faces_of(ap.parse_args(["restore", "gaussian", "in", "out", "--faces", "all", "--max-faces", "0"]))
    with pytest.raises(SystemExit):
        faces_of(ap.parse_args(["restore", "gaussian", "in", "out", "--faces", "all", "--aligned"]))
