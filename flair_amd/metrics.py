"""PSNR, SSIM and (on request) LPIPS of written frames against ground truth, and (on request) their no-reference NIQE, their
ArcFace identity similarity, their flow-warping error and the same scores over their face regions, on the GPU
(``flair_image_metrics``, csrc/metrics.hip; ``flair_amd.lpips``, csrc/lpips.hip; ``flair_amd.niqe``, csrc/niqe.hip;
``flair_amd.identity``, csrc/ident.hip; ``flair_amd.temporal``, csrc/temporal.hip; ``flair_amd.facescore``, csrc/facecrop.hip).

The reference ships no scoring tool; this is the restoration literature's usual pair, on the bytes that get written
(float images go through ``io.to_bytes`` first, so a metric always describes the files):

  * ``psnr = 10 log10(255^2 * 3 H W / sse)`` over the three channels of a frame together, ``inf`` where the frames agree;
  * ``ssim``: Wang et al.'s index as BasicSR computes it on RGB -- 11 x 11 Gaussian window, sigma 1.5, valid region only
    ((H - 10) x (W - 10), no padding), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, the mean over the map and the three
    channels.

  * ``lpips``, only with a model from ``flair_amd.lpips.load_lpips``: the ``lpips`` package's 0.1 metric on a VGG-16 or AlexNet
    trunk, as restated in include/flair_eval.h.

  * ``niqe``, only with a model from ``flair_amd.niqe.load_niqe``: the no-reference NIQE of the RESTORED frames (the truth is
    not scored), as restated in include/flair_noref.h; ``flair_amd.niqe.niqe_dir`` scores a directory without any truth.

  * ``ids``, only with a model from ``flair_amd.identity.load_identity``: the cosine of the ArcFace embeddings of a restored
    frame and its truth, as restated in include/flair_ident.h, with the identity drift from frame to frame of both sets.

  * ``warp_err``, only with a model from ``flair_amd.temporal``: the flow-warping error of every consecutive frame pair, as
    restated in include/flair_temporal.h, of the restored frames and of the truth under the truth's flows and mask.

  * ``faces``, only with a ``flair_amd.facescore.FaceScorer``: PSNR, SSIM and, where those models are given, LPIPS and the
    identity similarity of every face of unaligned frames, on aligned byte crops of both sets (include/flair_facescore.h).

Not measured: the Y-channel and border-cropped variants of PSNR / SSIM, NIQE's colour and border-cropped variants, other
no-reference scores (BRISQUE, PI), temporal metrics other than the identity drift and the flow-warping error (tOF, tLP,
warping errors over longer ranges than one frame).
"""
import math
import os

import torch

from . import io as fio
from . import ops

SSIM_WINDOW = 11
TILE_H, TILE_W = 32, 64         # the SSIM-map tile of one workgroup (MT_TH, MT_TW of csrc/metrics.hip): the tests size their shapes by it


def psnr_ssim(a_u8, b_u8):
    """a_u8, b_u8: (N, H, W, 3) uint8 on the GPU -> dict(psnr=[N floats], ssim=[N floats], sse=[N ints])."""
    N, H, W, _ = a_u8.shape
    rows = ops.image_metrics(a_u8, b_u8).cpu().tolist()
    sse = [int(round(r[0])) for r in rows]
    peak = 255.0 ** 2 * 3 * H * W
    psnr = [10.0 * math.log10(peak / e) if e else math.inf for e in sse]
    valid = 3.0 * (H - SSIM_WINDOW + 1) * (W - SSIM_WINDOW + 1)
    ssim = [(r[1] + r[2] + r[3]) / valid for r in rows]
    return dict(psnr=psnr, ssim=ssim, sse=sse)


def _pairs(restored_dir, truth_dir):
    """The (restored, truth) file pairs in list_frames order with their common (h, w); every refusal of evaluate_dirs."""
    ra, rb = fio.list_frames(restored_dir), fio.list_frames(truth_dir)
    for d, paths in ((restored_dir, ra), (truth_dir, rb)):
        if not paths:
            raise ValueError(f"evaluate: no frame files in {d}")
    if len(ra) != len(rb):
        raise ValueError(f"evaluate: {restored_dir} holds {len(ra)} frames and {truth_dir} holds {len(rb)}; "
                         "frames are paired in order and the counts must agree")
    sizes = []
    for pa, pb in zip(ra, rb):
        sa, sb = fio.frame_size(pa), fio.frame_size(pb)
        if sa != sb:
            raise ValueError(f"evaluate: {pa} is {sa[0]}x{sa[1]} and {pb} is {sb[0]}x{sb[1]}; paired frames must share one size")
        if min(sa) < SSIM_WINDOW:
            raise ValueError(f"evaluate: {pa} and {pb} are {sa[0]}x{sa[1]}; SSIM's {SSIM_WINDOW}x{SSIM_WINDOW} window needs "
                             f"frames of at least {SSIM_WINDOW} pixels a side")
        sizes.append(sa)
    return ra, rb, sizes


def _groups(sizes, batch):
    """Runs of at most ``batch`` consecutive frames of one size as (first, n)."""
    groups, first = [], 0
    while first < len(sizes):
        n = 1
        while n < batch and first + n < len(sizes) and sizes[first + n] == sizes[first]:
            n += 1
        groups.append((first, n))
        first += n
    return groups


def evaluate_dirs(restored_dir, truth_dir, device, batch=8, lpips=None, niqe=None, identity=None, warp_error=None, warp_skip=(),
                  faces=None):
    """Score the frames of ``restored_dir`` against those of ``truth_dir``, paired in ``io.list_frames`` order:
    ``dict(frames=[{name, psnr, ssim}], mean={psnr, ssim}, count)``; the means are those of the per-frame values.
    ValueError when a directory is empty, the counts differ, a pair differs in size or is smaller than 11 pixels a side
    (checked on the file headers, before anything is decoded).  The next batch is decoded and uploaded while the current
    one is measured (io.iter_frame_batches).  ``lpips``: a ``flair_amd.lpips.LPIPS`` model; every frame dict and ``mean``
    then gain ``lpips``, and frames below the trunk's minimum are refused with the others (without one the result is what
    it was before the option existed).  ``niqe``: a ``flair_amd.niqe.NIQE`` model; every frame dict then gains ``niqe`` of the
    restored frame (None where it has no score) and ``mean`` gains ``niqe``, over the ``niqe_frames`` frames that have one;
    frames with fewer than two 96 x 96 blocks are refused with the others.  ``identity``: a ``flair_amd.identity.ArcFace``
    model; every frame dict then gains ``ids`` (None where an embedding is zero) and ``mean`` gains ``ids``, ``id_drift`` and
    ``id_drift_truth``; every frame goes through the network once, and frames that are not square are refused with the others.
    ``warp_error``: a ``flair_amd.temporal.WarpError`` model; every frame dict then gains ``warp_err``, the flow-warping error of
    the restored frame and the one before it under the TRUTH's flows and mask (None for the first frame, after a change of
    size, for a pair with an empty mask and for the later-frame indices in ``warp_skip``: ``temporal.straddling`` of the scene
    cuts), and ``mean`` gains ``warp_err``, ``warp_err_truth``, ``warp_err_pairs`` and ``masked``; frames under 32 pixels a
    side are refused with the others.  ``faces``: a ``flair_amd.facescore.FaceScorer``; every frame dict then gains ``faces``, a
    list of ``{psnr, ssim, [lpips], [ids], clipped, matrix}`` per face found on the TRUTH frame and cut from both sets by one
    matrix, and ``mean`` gains ``face_psnr``, ``face_ssim``, ``[face_lpips]``, ``[face_ids]`` (means over faces; absent without a
    face), ``face_count`` and ``frames_with_faces`` and, in mode "largest" with ``identity``, ``face_id_drift`` and
    ``face_id_drift_truth``.  ``identity`` then applies to the crops only: the whole-frame ``ids`` and its squareness check
    are skipped; every other whole-frame value stays what it is without the scorer."""
    ra, rb, sizes = _pairs(restored_dir, truth_dir)
    face_identity = None
    if faces is not None:
        faces.check_models(lpips=lpips, identity=identity)
        face_identity, identity = identity, None
    if niqe is not None:
        from . import niqe as fnq
        for pa, (h, w) in zip(ra, sizes):
            fnq.check_size(h, w, what=f"evaluate: {pa}")
    if lpips is not None:
        from . import lpips as flp
        for pa, pb, (h, w) in zip(ra, rb, sizes):
            flp.check_size(lpips.net, h, w, what=f"evaluate: {pa} and {pb}")
    if identity is not None:
        from . import identity as fid
        for pa, (h, w) in zip(ra, sizes):
            fid.check_size(h, w, what=f"evaluate: {pa}")
    if warp_error is not None:
        from . import temporal as ftm
        for pa, (h, w) in zip(ra, sizes):
            ftm.check_size(h, w, what=f"evaluate: {pa}")
        pair_stream = ftm.PairStream(warp_error)
    frames, emb_a, emb_b, face_emb = [], [], [], []
    for first, (a, b) in fio.iter_frame_batches([ra, rb], _groups(sizes, max(1, int(batch))), device):
        got = psnr_ssim(a, b)
        for i, (p, s) in enumerate(zip(got["psnr"], got["ssim"])):
            frames.append(dict(name=os.path.basename(ra[first + i]), psnr=p, ssim=s))
        if lpips is not None:
            for i, d in enumerate(lpips(a, b)):
                frames[first + i]["lpips"] = d
        if niqe is not None:
            for i, v in enumerate(niqe(a)):
                frames[first + i]["niqe"] = None if math.isnan(v) else v
        if identity is not None:
            e = identity.embed(a, b)
            emb_a += list(e[:a.shape[0]])
            emb_b += list(e[a.shape[0]:])
        if warp_error is not None:
            pair_stream.push(a, b)
        if faces is not None:
            per_frame, emb = faces.score(a, b, lpips=lpips, identity=face_identity)
            for i, found in enumerate(per_frame):
                frames[first + i]["faces"] = found
            face_emb += emb
    n = len(frames)
    mean = dict(psnr=sum(f["psnr"] for f in frames) / n, ssim=sum(f["ssim"] for f in frames) / n)
    if lpips is not None:
        mean["lpips"] = sum(f["lpips"] for f in frames) / n
    if niqe is not None:
        mean.update(fnq.mean_of([f["niqe"] for f in frames]))
    if identity is not None:
        ids, id_mean = fid.scores(emb_a, emb_b)
        for f, v in zip(frames, ids):
            f["ids"] = v
        mean.update(id_mean)
    if warp_error is not None:
        values, warp_mean = ftm.scores(pair_stream.rows, pair_stream.pixels, set(warp_skip))
        for f, v in zip(frames, values):
            f["warp_err"] = v
        mean.update(warp_mean)
    if faces is not None:
        from . import facescore as ffs
        mean.update(ffs.means(frames, faces.mode, face_emb if face_identity is not None else None))
    return dict(frames=frames, mean=mean, count=n)


def format_report(result):
    """One line per frame and the means, four decimals each (``lpips``, then ``niqe``, then ``ids``, then ``warp-err``, where the
    result holds them; ``niqe n/a`` / ``ids n/a`` / ``warp-err n/a`` for a frame without a score, which the mean leaves out; the
    means' line carries the identity drift of the restored frames and, in brackets, of the truth, and ends with the
    flow-warping error (x 10^3), the truth's in brackets, and the masked-out share).  Where the frames hold ``faces``, one
    indented line per face follows a frame's line (``  faces 0`` for a frame without one) and the faces' means follow the
    means' line (``flair_amd.facescore.format_faces`` / ``format_mean``)."""
    def tail(d):
        text = f"  lpips {d['lpips']:.4f}" if "lpips" in d else ""
        if "niqe" in d:
            from .niqe import format_value
            text += format_value(d["niqe"])
        if "ids" in d:
            from . import identity as fid
            text += fid.format_mean(d) if "id_drift" in d else fid.format_value(d["ids"])
        if "warp_err" in d:
            from . import temporal as ftm
            text += ftm.format_mean(d) if "masked" in d else ftm.format_value(d["warp_err"])
        return text
    lines = []
    for f in result["frames"]:
        lines.append(f"{f['name']}  psnr {f['psnr']:.4f}  ssim {f['ssim']:.4f}" + tail(f))
        if "faces" in f:
            from . import facescore as ffs
            lines += ffs.format_faces(f["faces"])
    lines.append(f"mean of {result['count']} frames  psnr {result['mean']['psnr']:.4f}  ssim {result['mean']['ssim']:.4f}"
                 + tail(result["mean"]))
    if "face_count" in result["mean"]:
        from . import facescore as ffs
        lines.append(ffs.format_mean(result["mean"], result["count"]))
    return lines
