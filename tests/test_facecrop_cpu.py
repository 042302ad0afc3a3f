"""CPU: the face score's crop by its definition (tests/facecrop_ref.py) on hand cases and against its mutants, the weight table of
csrc/facecrop.hip, the sixth header, the entry's refusals, the wrapper's refusals, and the host's arithmetic of the face score
(means, drift, report lines, command line) on hand-made records."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import face_ref as F
from tests import facecrop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the definition
def test_the_table_is_integers_over_2_17_and_every_row_sums_to_one():
    tab32, num = F.cubic_table()
    assert num.shape == (32, 4) and num.dtype == np.int64
    assert (num.sum(axis=1) == 1 << 17).all()
    assert np.array_equal(tab32.astype(np.float64) * 2.0 ** 17, num.astype(np.float64))
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "facecrop.hip")).read()
    body = re.search(r"FC_TAB\[32\]\[4\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [[int(v) for v in row.split(",")] for row in re.findall(r"\{([^{}]*)\}", body)]
    assert np.array_equal(np.array(rows, dtype=np.int64), num)                      # the kernel's table is the reference's
    assert "FC_TAB_BITS = 17" in src


def test_known_answers():
    copy = R.case("copy")
    assert np.array_equal(copy["value"], R.frames()[0][3:19, 5:29]) and F.class_counts(copy["cls"]) == (0, 16 * 24, 0)
    step = R.case("step")
    assert (int(step["raw"].min()), int(step["raw"].max())) == R.STEP_RANGE == (-24, 279)          # both clamps act
    assert step["value"].min() == 0 and step["value"].max() == 255
    rot = R.case("rotation")
    assert rot["value"].shape == (40, 24, 3) and F.class_counts(rot["cls"]) == R.ROTATION_CLASSES == (566, 307, 87)
    out = R.case("outside")
    assert F.class_counts(out["cls"]) == (9 * 13, 0, 0) and (out["value"] == np.array(R.BORDER, dtype=np.uint8)).all()
    assert F.class_counts(R.case("src1x1")["cls"])[1] == 0 and F.class_counts(R.case("src3x5")["cls"])[1] == 0     # too small for an inner window
    assert R.case("dst1x1")["value"].shape == (1, 1, 3)
    for name in ("quarter-x", "quarter-y", "quarter-xy"):
        g = R.case(name)
        assert set(np.unique(g["fx"])) | set(np.unique(g["fy"])) <= {0, 8, 16, 24}                # dyadic quarter pixels
        assert g["raw"].min() < 0 and g["raw"].max() > 255


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_the_integer_result_is_the_rounded_float64_sum(name):
    _, out_hw, m = R.CASES[name]
    assert np.array_equal(R.crop_float64(R.case_source(name), m, out_hw), R.case(name)["value"])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_a_named_case(mutant):
    changed = [n for n in sorted(R.CASES) if not np.array_equal(R.case(n, mutant)["value"], R.case(n)["value"])]
    print(f"{mutant}: changes {changed}")
    assert changed
    must = {"swap_xy": "quarter-x", "half_away": "tie-x-neg", "floor": "tie-x-pos", "no_clamp": "step", "no_half": "quarter-xy",
            "border_zero": "outside"}[mutant]
    assert must in changed


def test_multi_face_data_is_what_the_gpu_tests_assume():
    frames = R.frames()
    assert frames.shape == (2, 37, 70, 3) and R.MULTI_INDEX == (1, 1, 0, 1) and R.MULTI_HW == (21, 70)       # two column groups, a ragged last row group
    out = R.crop_batch(frames, R.MULTI_MINV, R.MULTI_INDEX, R.MULTI_HW)
    assert out.shape == (4, 21, 70, 3)
    assert np.array_equal(out[2], R.crop(frames[0], R.MULTI_MINV[2], R.MULTI_HW)["value"])
    assert not np.array_equal(out[2], R.crop(frames[1], R.MULTI_MINV[2], R.MULTI_HW)["value"])                # the index matters
    assert R.corners_outside(R.MULTI_MINV[0], R.MULTI_HW, 37, 70) and not R.corners_outside([1, 0, 5, 0, 1, 3], (16, 24), 37, 70)


# ------------------------------------------------------------------------------------------- the sixth header
def facescore_declared():
    text = open(os.path.join(ROOT, "include", "flair_facescore.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_facescore_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib
    assert facescore_declared() == sorted(_header.FACESCORE_PROTOS) == ["flair_face_crop_u8"]
    others = (set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS) | set(_header.IDENT_PROTOS)
              | set(_header.TEMPORAL_PROTOS))
    assert not set(_header.FACESCORE_PROTOS) & others and not set(_header.FACESCORE_PROTOS) & set(_lib.ALL_PROTOS)
    assert len(_header.STRUCTS) == 7 and _header.parse(open(_header.FACESCORE_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 22
    restype, params = _header.FACESCORE_PROTOS["flair_face_crop_u8"]
    f = lib.flair_face_crop_u8
    assert f.restype is ctypes.c_int and restype is ctypes.c_int and params[-1].name == "stream"
    assert list(f.argtypes) == [p.ctype for p in params]
    i, v = ctypes.c_int, ctypes.c_void_p
    assert [tuple(p) for p in params] == [
        ("a", v, "uint8_t"), ("b", v, "uint8_t"), ("Nsrc", i, None), ("Hs", i, None), ("Ws", i, None), ("minv", v, "double"),
        ("src_index", v, "int"), ("K", i, None), ("Hd", i, None), ("Wd", i, None), ("border", v, "uint8_t"), ("out_a", v, "uint8_t"),
        ("out_b", v, "uint8_t"), ("stream", v, None)]
    header = open(_header.FACESCORE_HEADER_PATH).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "facecrop.hip")).read()
    assert "is 22 from this header on" in header and "NOT cv2.warpAffine's uint8 path" in header
    assert "atomic" not in src.replace("no atomics", "") and "__shared__" not in src and "asm" not in src
    assert not re.search(r"\b(float|__half)\b", re.sub(r"//.*", "", src))                        # doubles in the position, integers after it
    assert not re.search(r"size_t\s+flair_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))         # nothing allocated, no workspace
    make = open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read()
    assert "flair_facescore.h" in make and re.search(r"(?m)^facecrop\.o: CXXFLAGS \+= -ffp-contract=off$", make)


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entry():
    from flair_amd import _lib
    call = _lib.call
    f32, f64, u8, i32 = (_device_tensor(t) for t in (torch.float32, torch.float64, torch.uint8, torch.int32))
    bd = (ctypes.c_uint8 * 3)(*R.BORDER)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_face_crop_u8(torch.zeros(2, dtype=torch.uint8), None, 1, 1, 1, f64, i32, 1, 1, 1, bd, u8, None)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_face_crop_u8: minv must be float64, got float32$"):
        call.flair_face_crop_u8(u8, None, 1, 1, 1, f32, i32, 1, 1, 1, bd, u8, None)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_face_crop_u8: src_index must be int32, got float64$"):
        call.flair_face_crop_u8(u8, None, 1, 1, 1, f64, f64, 1, 1, 1, bd, u8, None)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_face_crop_u8: out_b must be uint8, got float32$"):
        call.flair_face_crop_u8(u8, u8, 1, 1, 1, f64, i32, 1, 1, 1, bd, u8, f32)
    with pytest.raises(TypeError, match="flair_face_crop_u8 takes 13 arguments"):
        call.flair_face_crop_u8(u8, None)
    with pytest.raises(AttributeError, match="flair_face_crop_u8_workspace is not an entry"):
        call.flair_face_crop_u8_workspace


def test_the_entry_refuses_before_any_launch(monkeypatch):
    """Every refusal the header lists: status -1 and the entry's message, on a machine without a GPU; K = 0 enqueues nothing."""
    from flair_amd import _lib
    lib = _lib.lib()
    cases = R.entry_refusals()
    assert {n for n, _, _ in cases} == {"flair_face_crop_u8"} and len(cases) >= 24
    for name, args, what in cases:
        R.assert_refused(lib, name, args, what)
    for args in R.entry_accepts_without_launch():
        assert lib.flair_face_crop_u8(*args, None) == 0
    monkeypatch.setattr(_lib, "stream", lambda: None)
    u8, f64, i32 = _device_tensor(torch.uint8), _device_tensor(torch.float64), _device_tensor(torch.int32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_face_crop_u8 failed \(status -1\): flair_face_crop_u8: out overlaps a source"):
        _lib.call.flair_face_crop_u8(u8, None, 1, 8, 8, f64, i32, 1, 4, 4, (ctypes.c_uint8 * 3)(1, 2, 3), u8, None)


def test_the_wrapper_refuses_wrong_tensors_indices_and_far_matrices():
    from flair_amd import ops
    a = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    m = torch.tensor([[1.0, 0, 0, 0, 1, 0]], dtype=torch.float64)
    idx = torch.zeros(1, dtype=torch.int32)

    def run(a=a, minv=m, minv_host=m.numpy(), src_index=idx, src_index_host=(0,), out_hw=(4, 5), **kw):
        return ops.face_crop_u8(a, minv, minv_host, src_index, src_index_host, out_hw, **kw)
    with pytest.raises(ValueError, match=r"face_crop_u8: a is a dense \(Nsrc, Hs, Ws, 3\) uint8 tensor with Nsrc >= 1, got \(2, 8, 9, 3\) torch.float32"):
        run(a=a.float())
    with pytest.raises(ValueError, match=r"face_crop_u8: a is a dense"):
        run(a=a.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match=r"face_crop_u8: b is a frame set of a's shape \(2, 8, 9, 3\), got \(1, 8, 9, 3\)"):
        run(b=a[:1])
    with pytest.raises(ValueError, match=r"face_crop_u8: src_index must be a contiguous \(K,\) int32 tensor"):
        run(src_index=idx.long())
    with pytest.raises(ValueError, match=r"face_crop_u8: minv must be a contiguous \(1, 6\) float64 tensor"):
        run(minv=m.float())
    with pytest.raises(ValueError, match=r"face_crop_u8: src_index_host \(the 1 indices on the host\) is needed"):
        run(src_index_host=None)
    with pytest.raises(ValueError, match=r"face_crop_u8: src_index outside \[0, 2\)"):
        run(src_index_host=(2,))
    with pytest.raises(ValueError, match=r"face_crop_u8: src_index outside \[0, 2\)"):
        run(src_index_host=(-1,))
    with pytest.raises(ValueError, match=r"face_crop_u8: minv_host \(the 1 matrices on the host\) is needed"):
        run(minv_host=None)
    with pytest.raises(ValueError, match=r"face_crop_u8: a crop of 0x5 pixels"):
        run(out_hw=(0, 5))
    for far in ([1, 0, 32001, 0, 1, 0], [1, 0, 0, 0, 1, -32001], [8001, 0, 0, 0, 1, 0], [1, 0, 0, 0, 11001, 0], [1, 0, float("nan"), 0, 1, 0],
                [1, 0, 0, 0, 1, float("inf")]):
        with pytest.raises(ValueError, match=r"face_crop_u8: matrix 0 maps a corner of the crop beyond \+-32000 source pixels"):
            run(minv_host=np.array([far]))
    with pytest.raises(ValueError, match=r"face_crop_u8: border is three bytes"):
        run(border=(1, 2, 256))
    with pytest.raises(ValueError, match=r"face_crop_u8: border is three bytes"):
        run(border=(1, 2))
    with pytest.raises(ValueError, match=r"face_crop_u8: out_a is a dense \(1, 4, 5, 3\) uint8 tensor, got \(1, 4, 5\)"):
        run(out_a=torch.zeros(1, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"face_crop_u8: out_b without b"):
        run(out_b=torch.zeros(1, 4, 5, 3, dtype=torch.uint8))
    from flair_amd import _lib
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):          # every check passed: the launch is next
        run()
    # K = 0 launches nothing, on any device
    none = ops.face_crop_u8(a, m[:0], np.zeros((0, 6)), idx[:0], (), (4, 5), b=a)
    assert [tuple(t.shape) for t in none] == [(0, 4, 5, 3)] * 2


# ------------------------------------------------------------------------------------------- the host's arithmetic
def _face(psnr, ssim, clipped=False, **kw):
    return dict(psnr=psnr, ssim=ssim, **kw, clipped=clipped, matrix=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _result(frames, mean):
    return dict(frames=frames, mean=mean, count=len(frames))


def test_means_count_faces_not_frames():
    from flair_amd import facescore as ffs
    frames = [dict(name="0.png", psnr=30.0, ssim=0.9, faces=[_face(20.0, 0.5, lpips=0.25, ids=0.75), _face(40.0, 0.75, lpips=0.75, ids=None, clipped=True)]),
              dict(name="1.png", psnr=31.0, ssim=0.8, faces=[]),
              dict(name="2.png", psnr=32.0, ssim=0.7, faces=[_face(30.0, 0.25, lpips=0.5, ids=0.25)])]
    mean = ffs.means(frames, "all")
    assert mean == dict(face_psnr=30.0, face_ssim=0.5, face_lpips=0.5, face_ids=0.5, face_count=3, frames_with_faces=2)
    assert not [k for k in mean if "drift" in k]                                    # mode all reports no drift
    none = ffs.means([dict(name="0.png", psnr=1.0, ssim=1.0, faces=[])], "largest")
    assert none == dict(face_count=0, frames_with_faces=0)                          # no face: the value keys are absent
    plain = ffs.means([dict(faces=[_face(20.0, 0.5)])], "largest")
    assert plain == dict(face_psnr=20.0, face_ssim=0.5, face_count=1, frames_with_faces=1)


def test_drift_is_over_consecutive_frames_that_both_have_a_face():
    from flair_amd import facescore as ffs
    e0, e1, e2 = np.array([1.0, 0.0]), np.array([0.0, 2.0]), np.array([3.0, 3.0])
    assert ffs.drift([e0, e0, e0]) == 0.0
    assert ffs.drift([e0, e1]) == 1.0
    assert ffs.drift([e0, None, e1]) is None and ffs.drift([e0]) is None and ffs.drift([]) is None
    assert ffs.drift([e0, e1, None, e2, e2]) == pytest.approx((1.0 + 0.0) / 2)
    assert ffs.drift([e0, np.zeros(2), e0]) is None                                 # a zero embedding has no cosine
    emb = [(e0, e0), (e1, e0), None, (e2, e1)]
    frames = [dict(faces=[_face(20.0, 0.5, ids=1.0)]), dict(faces=[_face(20.0, 0.5, ids=0.0)]), dict(faces=[]), dict(faces=[_face(20.0, 0.5, ids=0.5)])]
    mean = ffs.means(frames, "largest", emb)
    assert mean["face_id_drift"] == 1.0 and mean["face_id_drift_truth"] == 0.0 and mean["face_ids"] == 0.5
    assert "face_id_drift" not in ffs.means(frames, "all", emb) and "face_id_drift" not in ffs.means(frames, "largest", None)


def test_format_report_prints_the_faces_under_their_frame():
    from flair_amd import facescore as ffs
    from flair_amd import metrics as fm
    frames = [dict(name="0.png", psnr=30.0, ssim=0.9, lpips=0.1, faces=[_face(20.0, 0.5, lpips=0.25, ids=0.75), _face(40.0, 0.7, lpips=0.75, ids=None, clipped=True)]),
              dict(name="1.png", psnr=31.0, ssim=0.8, lpips=0.2, faces=[])]
    mean = dict(psnr=30.5, ssim=0.85, lpips=0.15)
    mean.update(ffs.means(frames, "all"))
    lines = fm.format_report(_result(frames, mean))
    assert lines == ["0.png  psnr 30.0000  ssim 0.9000  lpips 0.1000",
                     "  face 0  psnr 20.0000  ssim 0.5000  lpips 0.2500  ids 0.7500",
                     "  face 1  psnr 40.0000  ssim 0.7000  lpips 0.7500  ids n/a  (clipped)",
                     "1.png  psnr 31.0000  ssim 0.8000  lpips 0.2000",
                     "  faces 0",
                     "mean of 2 frames  psnr 30.5000  ssim 0.8500  lpips 0.1500",
                     "mean of 2 faces in 1 of 2 frames  psnr 30.0000  ssim 0.6000  lpips 0.5000  ids 0.7500"]
    empty = [dict(name="0.png", psnr=30.0, ssim=0.9, faces=[])]
    lines = fm.format_report(_result(empty, dict(psnr=30.0, ssim=0.9, **ffs.means(empty, "largest"))))
    assert lines == ["0.png  psnr 30.0000  ssim 0.9000", "  faces 0", "mean of 1 frames  psnr 30.0000  ssim 0.9000", "mean of 0 faces in 0 of 1 frames"]
    drift = dict(psnr=1.0, ssim=1.0, face_psnr=2.0, face_ssim=0.5, face_ids=0.25, face_count=1, frames_with_faces=1, face_id_drift=0.125, face_id_drift_truth=None)
    assert ffs.format_mean(drift, 3) == "mean of 1 faces in 1 of 3 frames  psnr 2.0000  ssim 0.5000  ids 0.2500  id-drift 0.1250 (truth n/a)"
    assert ffs.face_tail(dict(mean=drift)) == "  faces 1 in 1 frames  face-psnr 2.0000  face-ssim 0.5000  face-ids 0.2500"
    assert ffs.face_tail(dict(mean=dict(psnr=1.0))) == ""
    # without faces the report is what it was
    old = [dict(name="0.png", psnr=30.0, ssim=0.9)]
    assert fm.format_report(_result(old, dict(psnr=30.0, ssim=0.9))) == ["0.png  psnr 30.0000  ssim 0.9000", "mean of 1 frames  psnr 30.0000  ssim 0.9000"]
    json.dumps(_result(frames, mean))                                               # the records are plain JSON


def test_clipped_is_a_closed_form_of_the_four_corners():
    from flair_amd import facescore as ffs
    assert not ffs.corners_outside([1, 0, 5, 0, 1, 3], (16, 24), 37, 70)
    assert not ffs.corners_outside([1, 0, 46, 0, 1, 21], (16, 24), 37, 70)          # the last corner lands on (69, 36), the last pixel
    assert ffs.corners_outside([1, 0, 46.5, 0, 1, 21], (16, 24), 37, 70) and ffs.corners_outside([1, 0, 5, 0, 1, -0.25], (16, 24), 37, 70)
    for m in R.MULTI_MINV:
        assert ffs.corners_outside(m, R.MULTI_HW, 37, 70) == R.corners_outside(m, R.MULTI_HW, 37, 70)


def test_scorer_refuses_bad_modes_and_small_crops():
    from flair_amd import facescore as ffs
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    helper = FaceRestoreHelper(face_size=64, device="cpu", face_det=object())
    assert ffs.FaceScorer(helper, "largest", max_faces=4).max_faces == 1 and ffs.FaceScorer(helper, "all", max_faces=4).max_faces == 4
    assert ffs.FaceScorer(helper, "all").max_faces is None and ffs.FaceScorer(helper, "all").out_hw == (64, 64)
    with pytest.raises(ValueError, match="mode='biggest', one of largest, all"):
        ffs.FaceScorer(helper, "biggest")
    with pytest.raises(ValueError, match="max_faces must be at least 1"):
        ffs.FaceScorer(helper, "all", max_faces=0)
    with pytest.raises(ValueError, match="crops of 10x10; SSIM's 11x11 window"):
        ffs.FaceScorer(FaceRestoreHelper(face_size=10, device="cpu", face_det=object()), "all")
    import types
    small = ffs.FaceScorer(FaceRestoreHelper(face_size=20, device="cpu", face_det=object()), "all")
    with pytest.raises(ValueError, match="face score: the face crops are 20x20; the alex trunk needs"):
        small.check_models(lpips=types.SimpleNamespace(net="alex"))
    small.check_models(lpips=types.SimpleNamespace(net="vgg"), identity=object())


# ------------------------------------------------------------------------------------------- the command line
def test_command_line_refuses_before_any_frame_is_decoded(tmp_path):
    from flair_amd.__main__ import main, make_parser
    from flair_amd import pipeline as pl
    args = make_parser().parse_args(["evaluate", "a", "b"])
    assert args.score_faces is None and args.max_faces == 4 and args.face_size == 512 and args.det_model == "retinaface_resnet50"
    args = make_parser().parse_args(["restore", "x8_bicubic", "v", "o"])
    assert args.score_faces is None and args.face_size == 512
    for model, (_, name) in pl.DETECTOR_FILES.items():
        with pytest.raises(SystemExit, match=re.escape(f"evaluate: --score-faces with --det-model {model} needs {tmp_path / name}")):
            main(["evaluate", str(tmp_path / "none"), str(tmp_path / "none2"), "--score-faces", "all", "--weights", str(tmp_path), "--det-model", model])
    with pytest.raises(SystemExit, match="evaluate: --score-faces reads the retinaface_resnet50 detector from --weights DIR; give one"):
        main(["evaluate", "a", "b", "--score-faces", "largest"])
    with pytest.raises(SystemExit, match="evaluate: --max-faces must be at least 1"):
        main(["evaluate", "a", "b", "--score-faces", "all", "--max-faces", "0", "--weights", str(tmp_path)])
    with pytest.raises(SystemExit, match="evaluate: --face-size must be at least 11"):
        main(["evaluate", "a", "b", "--score-faces", "all", "--face-size", "10", "--weights", str(tmp_path)])
    video = tmp_path / "video"
    video.mkdir()
    with pytest.raises(SystemExit, match="restore: --score-faces compares the written frames with --ground-truth DIR; give one"):
        main(["restore", "x8_bicubic", str(video), str(tmp_path / "out"), "--score-faces", "largest"])
    with pytest.raises(SystemExit):                                                 # argparse: not a mode
        main(["evaluate", "a", "b", "--score-faces", "some"])


def test_restore_scores_faces_with_the_detector_it_built(tmp_path, monkeypatch, capsys):
    """restore --ground-truth --score-faces: evaluate_dirs gets a FaceScorer around restore's own detector, the log line carries
    the faces' means and metrics.json the records."""
    import types
    from flair_amd import facescore as ffs
    from flair_amd import io as fio
    from flair_amd import metrics, pipeline
    from flair_amd.__main__ import main
    vid, truth, out = tmp_path / "video", tmp_path / "truth", tmp_path / "out"
    for d in (vid, truth):
        d.mkdir()
        fio.write_frame(str(d / "0000.png"), np.zeros((16, 16, 3), dtype=np.uint8))
    det, seen = object(), []

    class Fake:
        face_helper = types.SimpleNamespace(face_det=det)

        def restore_video_files(self, v, o, **hp):
            os.makedirs(o, exist_ok=True)
            fio.write_frame(os.path.join(o, "0000.png"), np.zeros((16, 16, 3), dtype=np.uint8))
            return 1

    def evaluate(restored, truth_dir, device, batch=8, faces=None):
        seen.append(faces)
        frames = [dict(name="0000.png", psnr=30.5, ssim=0.875, faces=[_face(20.0, 0.5)])]
        return dict(frames=frames, mean=dict(psnr=30.5, ssim=0.875, **ffs.means(frames, faces.mode)), count=1)

    monkeypatch.setattr(pipeline, "build_pipeline", lambda *a, **k: Fake())
    monkeypatch.setattr(metrics, "evaluate_dirs", evaluate)
    assert main(["restore", "gaussian", str(vid), str(out), "--ground-truth", str(truth), "--score-faces", "all", "--max-faces", "2",
                 "--face-size", "64", "--device", "cpu"]) == 0
    scorer, = seen
    assert isinstance(scorer, ffs.FaceScorer) and scorer.helper.face_det is det and (scorer.mode, scorer.max_faces, scorer.out_hw) == ("all", 2, (64, 64))
    assert "psnr 30.5000  ssim 0.8750  faces 1 in 1 frames  face-psnr 20.0000  face-ssim 0.5000" in capsys.readouterr().out
    got = json.load(open(out / "metrics.json"))
    assert got["mean"]["face_count"] == 1 and got["frames"][0]["faces"][0]["psnr"] == 20.0
