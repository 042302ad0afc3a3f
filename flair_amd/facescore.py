"""Face-region scores of unaligned footage: ``--score-faces largest|all`` of evaluate and restore --ground-truth.

``restore`` handles unaligned and rectangular frames with zero, one or several faces; over a whole frame the background
dominates PSNR, SSIM and LPIPS, and the identity score takes aligned crops only.  Here the faces are found on the TRUTH frames
(the restored set may be the damaged one), aligned to the helper's template exactly as ``restore`` aligns them
(``retinaface_utils.select_faces``), and ONE matrix per face cuts both frame sets, so that the crops are pixel-aligned.  The
cut is ``flair_face_crop_u8`` (include/flair_facescore.h, csrc/facecrop.hip): from the written bytes of both sets to aligned
byte crops, the exact a = -0.75 cubic rounded once, one launch per batch.  The byte-based scores then run on the crops
unchanged: ``metrics.psnr_ssim``, the LPIPS model, ``identity.embed``.

  * mode ``largest``: at most one face per frame, the one ``get_largest_face`` picks; ``all``: every face, largest first, at
    most ``max_faces`` per frame.
  * per face: ``psnr``, ``ssim``, ``lpips`` and ``ids`` where those models are given, ``clipped`` (a corner of the crop maps
    outside the frame, so a part of the crop is the border colour in BOTH sets) and ``matrix``, the 2 x 3 frame -> crop
    alignment.
  * the means are over faces, not frames: ``face_psnr``, ``face_ssim``, ``face_lpips``, ``face_ids``, with ``face_count`` and
    ``frames_with_faces``; without a face the value keys are absent.
  * ``face_id_drift`` / ``face_id_drift_truth``, mode ``largest`` with an identity model only: the mean of 1 - cos over
    consecutive frames that both have a face.  In mode ``all`` no drift is reported: the faces of a frame are ordered by size,
    not by person, and following people from frame to frame is a feature of its own.
"""
import os

import numpy as np
import torch

from . import ops

MODES = ("largest", "all")
BORDER = (135, 133, 132)                        # the helper's crop border (face_restoration_helper.py), as bytes
EYE_DIST_THRESHOLD = 0.1                        # video.window_faces' value


def detector_file(det_model, weights_dir):
    from .pipeline import DETECTOR_FILES
    if det_model not in DETECTOR_FILES:
        raise ValueError(f"det_model={det_model!r}: one of {', '.join(DETECTOR_FILES)}")
    return os.path.join(str(weights_dir), DETECTOR_FILES[det_model][1])


def build_detector(det_model, weights_dir, device):
    """The loaded detector ``det_model`` of pipeline.DETECTOR_FILES from its file in ``weights_dir``, as build_pipeline builds
    it (strict, weights_only); never a random one.  FileNotFoundError names a missing file."""
    from .checkpoint import load_reference_checkpoint
    from .pipeline import DETECTOR_FILES
    path = detector_file(det_model, weights_dir)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"detector checkpoint {os.path.basename(path)} not found in {weights_dir} ({path})")
    device = torch.device(device)
    if det_model.startswith("YOLOv5"):
        from .guided_diffusion.yolov5face import YoloDetector
        det = YoloDetector(DETECTOR_FILES[det_model][0], device="cpu")
        load_reference_checkpoint(det.detector, path, strict=True)
        det.detector = det.detector.to(device).eval()
    else:
        from .guided_diffusion.retinaface import RetinaFace
        det = RetinaFace(network_name=DETECTOR_FILES[det_model][0], half=False, device="cpu")
        load_reference_checkpoint(det, path, strict=True)
        det = det.to(device).eval()
    det.device = device
    return det


def load_face_scorer(det_model, weights_dir, device, mode, max_faces=None, face_size=512):
    """A FaceScorer around a helper of its own with the detector read from ``weights_dir``."""
    from .guided_diffusion.face_restoration_helper import FaceRestoreHelper
    det = build_detector(det_model, weights_dir, device)
    helper = FaceRestoreHelper(face_size=int(face_size), det_model=det_model, device=device, face_det=det)
    return FaceScorer(helper, mode, max_faces=max_faces)


def corners_outside(minv, out_hw, H, W):
    """Whether one of a crop's four corners maps outside the frame [0, W - 1] x [0, H - 1] under the dst -> src matrix."""
    m = [float(v) for v in np.asarray(minv, dtype=np.float64).reshape(6)]
    h, w = out_hw
    for x in (0, w - 1):
        for y in (0, h - 1):
            px, py = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
            if not (0.0 <= px <= W - 1 and 0.0 <= py <= H - 1):
                return True
    return False


class FaceScorer:
    """``FaceScorer(helper, mode, max_faces=None)`` around a ``FaceRestoreHelper`` (its detector, template and face size);
    ``mode`` "largest" or "all"; ``max_faces`` bounds the faces of a frame in mode "all" (None: every face)."""

    def __init__(self, helper, mode, max_faces=None):
        if mode not in MODES:
            raise ValueError(f"face score: mode={mode!r}, one of {', '.join(MODES)}")
        if max_faces is not None and int(max_faces) < 1:
            raise ValueError("face score: max_faces must be at least 1 (or None for every face)")
        self.helper, self.mode = helper, mode
        self.max_faces = 1 if mode == "largest" else (None if max_faces is None else int(max_faces))
        w, h = helper.face_size
        self.out_hw = (h, w)
        from .metrics import SSIM_WINDOW
        if min(h, w) < SSIM_WINDOW:
            raise ValueError(f"face score: crops of {h}x{w}; SSIM's {SSIM_WINDOW}x{SSIM_WINDOW} window needs at least {SSIM_WINDOW} pixels a side")

    def check_models(self, lpips=None, identity=None):
        """ValueError where the crops are smaller than the LPIPS trunk admits or not square for the identity network."""
        h, w = self.out_hw
        if lpips is not None:
            from . import lpips as flp
            flp.check_size(lpips.net, h, w, what="face score: the face crops")
        if identity is not None:
            from . import identity as fid
            fid.check_size(h, w, what="face score: a face crop")

    @torch.no_grad()
    def detect(self, truth_u8):
        """(N, H, W, 3) uint8 truth frames on the GPU -> (K frame -> crop matrices, face_frames): the faces of every frame,
        largest first, by the helper's detector on the frames as f32 NCHW in [-1, 1] (torch plumbing)."""
        x = truth_u8.permute(0, 3, 1, 2).to(torch.float32).mul_(1.0 / 127.5).sub_(1.0)
        return self.helper.get_face_matrices(x, eye_dist_threshold=EYE_DIST_THRESHOLD, max_faces=self.max_faces)

    def crops(self, a_u8, b_u8, matrices, face_frames):
        """Both frame sets cut by one launch -> (crops of a, crops of b, the K dst -> src matrices on the host)."""
        from .guided_diffusion.face_restoration_helper import invert_affine
        dev = a_u8.device
        minv_host = np.stack([invert_affine(m).reshape(6) for m in matrices])
        ca, cb = ops.face_crop_u8(a_u8, self.helper._minv(matrices, dev), minv_host, self.helper._index(face_frames, dev),
                                  [int(f) for f in face_frames], self.out_hw, b=b_u8, border=BORDER)
        return ca, cb, minv_host

    @torch.no_grad()
    def score(self, a_u8, b_u8, lpips=None, identity=None):
        """Restored frames a and truth frames b, (N, H, W, 3) uint8 on the GPU -> (faces, embeddings): per frame the list of
        its face records, and per frame (restored, truth) embeddings of its first face (None without a face or a model)."""
        from . import metrics as fm
        N, H, W, _ = a_u8.shape
        faces, emb = [[] for _ in range(N)], [None] * N
        matrices, face_frames = self.detect(b_u8)
        K = len(matrices)
        if K == 0:
            return faces, emb
        ca, cb, minv_host = self.crops(a_u8.contiguous(), b_u8.contiguous(), matrices, face_frames)
        got = fm.psnr_ssim(ca, cb)
        lp = lpips(ca, cb) if lpips is not None else None
        e = identity.embed(ca, cb) if identity is not None else None
        for k, t in enumerate(face_frames):
            rec = dict(psnr=got["psnr"][k], ssim=got["ssim"][k])
            if lp is not None:
                rec["lpips"] = lp[k]
            if e is not None:
                from . import identity as fid
                rec["ids"] = fid.cosine(e[k], e[K + k])
                if not faces[t]:
                    emb[t] = (e[k], e[K + k])
            rec["clipped"] = corners_outside(minv_host[k], self.out_hw, H, W)
            rec["matrix"] = [[float(v) for v in row] for row in np.asarray(matrices[k], dtype=np.float64).reshape(2, 3)]
            faces[t].append(rec)
        return faces, emb


# ------------------------------------------------------------------------------------------- the host's arithmetic (float64)
VALUE_KEYS = ("psnr", "ssim", "lpips", "ids")


def drift(embeddings):
    """The mean of 1 - cos over consecutive frames that both have a face (an entry None: no face); None without such a pair
    (or where every pair has a zero embedding)."""
    from .identity import cosine
    values = []
    for prev, cur in zip(embeddings, embeddings[1:]):
        if prev is None or cur is None:
            continue
        c = cosine(cur, prev)
        if c is not None:
            values.append(1.0 - c)
    return sum(values) / len(values) if values else None


def means(frames, mode, embeddings=None):
    """The ``mean`` keys of a result: frames is the list of frame dicts with their ``faces``; embeddings the per-frame
    (restored, truth) pairs of ``FaceScorer.score`` where an identity model ran."""
    faces = [f for fr in frames for f in fr["faces"]]
    out = {}
    for key in VALUE_KEYS:
        have = [f[key] for f in faces if key in f and f[key] is not None]
        if any(key in f for f in faces):
            out["face_" + key] = sum(have) / len(have) if have else None
    out["face_count"] = len(faces)
    out["frames_with_faces"] = sum(1 for fr in frames if fr["faces"])
    if mode == "largest" and embeddings is not None:
        out["face_id_drift"] = drift([None if e is None else e[0] for e in embeddings])
        out["face_id_drift_truth"] = drift([None if e is None else e[1] for e in embeddings])
    return out


def _value(name, v):
    if v is None:
        return f"  {name} n/a"
    return f"  {name} {v:.4f}"


def format_faces(faces):
    """The lines under a frame's line: ``  face 0  psnr ..  ssim ..  lpips ..  ids ..`` with ``(clipped)`` where true, or
    ``  faces 0`` for a frame without one."""
    if not faces:
        return ["  faces 0"]
    lines = []
    for k, f in enumerate(faces):
        text = f"  face {k}" + "".join(_value(key, f[key]) for key in VALUE_KEYS if key in f)
        lines.append(text + ("  (clipped)" if f.get("clipped") else ""))
    return lines


def format_mean(mean, count):
    """``mean of K faces in F of N frames  psnr .. ssim ..`` (and the drift of mode largest with an identity model)."""
    text = f"mean of {mean['face_count']} faces in {mean['frames_with_faces']} of {count} frames"
    text += "".join(_value(key, mean["face_" + key]) for key in VALUE_KEYS if "face_" + key in mean)
    if "face_id_drift" in mean:
        truth = "n/a" if mean["face_id_drift_truth"] is None else f"{mean['face_id_drift_truth']:.4f}"
        text += _value("id-drift", mean["face_id_drift"]) + f" (truth {truth})"
    return text


def face_tail(result):
    """``  faces K in F frames  face-psnr X  face-ssim Y ...`` of a result's mean for restore's one-line log ('' without the
    option)."""
    mean = result["mean"]
    if "face_count" not in mean:
        return ""
    text = f"  faces {mean['face_count']} in {mean['frames_with_faces']} frames"
    return text + "".join(_value("face-" + key, mean["face_" + key]) for key in VALUE_KEYS if "face_" + key in mean)
