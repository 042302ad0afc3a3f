"""The command line on rectangular frames without the released checkpoints: random-weight equivalent of

    python -m flair_amd restore gaussian ./frames ./out --frame-size auto --faces all

Writes full-size random checkpoints (the gaussian network in its 512 layout, CodeFormer, RetinaFace ResNet-50, ParseNet), a
kernel file and --frames degraded frames of --degraded HxW (default 192x320 -> 768x1280) into a scratch directory and
runs the command line's own ``main()`` on them.  A random detector fires on thousands of anchors or on none, so the one
thing replaced is the detector of the pipeline ``main()`` builds: it reports two fixed faces per frame (boxes and the five
landmarks of the 512 template, drifting from frame to frame; the second one hangs over the frame's right edge).  Everything
after detection is the product's: alignment, 512 x 512 crops out of the rectangular frames, CodeFormer on the crops,
ParseNet masks and the paste.  The tool checks the PNGs and that the prior ran on 2 faces per frame in every step.
Run it under a time limit (``timeout -k 10 900 python tools/restore_rect_random.py``).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]]) / 512.0 - 0.5


class FixedFaces:
    """batched_detect_faces of a detector that finds the same two faces in every frame: rows of box, score and five
    landmarks (the 512 template scaled to the face), as the detectors return them."""

    def __init__(self, H, W):
        self.H, self.W = H, W

    def face(self, cx, cy, size, score):
        lm = _TPL * size + np.array([cx, cy])
        return np.concatenate([[cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, score], lm.reshape(-1)]).astype(np.float32)

    def batched_detect_faces(self, frames, conf_threshold=0.8, nms_threshold=0.4, use_origin_size=True, pre=None,
                             keep_empty=False):
        H, W = self.H, self.W
        return [np.stack([self.face(0.3 * W + 3 * k, 0.5 * H - 2 * k, 0.55 * H, 0.99),
                          self.face(0.93 * W - 2 * k, 0.4 * H + k, 0.3 * H, 0.9)]) for k in range(frames.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degraded", default="192x320", help="size of the degraded frames, HxW")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    import scipy.io
    from PIL import Image
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.codeformer import CodeFormer
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    from flair_amd.guided_diffusion.unet_new import UNetModel
    h, w = (int(v) for v in a.degraded.lower().split("x"))
    work = a.workdir or tempfile.mkdtemp(prefix="flair_rect_")
    wdir, frames, out = (os.path.join(work, n) for n in ("weights", "frames", "out"))
    os.makedirs(wdir, exist_ok=True)
    os.makedirs(frames, exist_ok=True)
    torch.manual_seed(0)
    m = UNetModel(**pl.model_config("gaussian", (4 * h, 4 * w)))
    wl.randomize_zero_modules(m)
    torch.save(m.state_dict(), os.path.join(wdir, "flair_gaussian.pt"))
    del m
    gan = CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9, connect_list=["32", "64", "128", "256"])
    torch.save({"params_ema": gan.state_dict()}, os.path.join(wdir, pl.CODEFORMER_FILE))
    torch.save(RetinaFace("resnet50", device="cpu").state_dict(), os.path.join(wdir, "detection_Resnet50_Final.pth"))
    torch.save(ParseNet(in_size=512, out_size=512, parsing_ch=19).state_dict(), os.path.join(wdir, pl.PARSER_FILE))
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(os.path.join(work, "kernels_12.mat"), {"kernels": kernels})
    rng = np.random.default_rng(2)
    base = rng.integers(0, 256, size=(h // 8, w // 8, 3), dtype=np.uint8)
    for i in range(a.frames):
        img = np.asarray(Image.fromarray(np.roll(base, i, axis=1), mode="RGB").resize((w, h), Image.BICUBIC))
        Image.fromarray(img, mode="RGB").save(os.path.join(frames, f"{i}.png"))
    argv = ["restore", "gaussian", frames, out, "--frame-size", "auto", "--faces", "all", "--steps", str(a.steps), "--tau", "0",
            "--weights", wdir, "--kernels", os.path.join(work, "kernels_12.mat"), "--seed", "1"]
    from flair_amd import __main__ as cli
    H, W = 4 * h, 4 * w
    pasted = []
    build = pl.build_pipeline

    def build_with_fixed_faces(*args, **kw):
        p = build(*args, **kw)
        p.face_helper.face_det = FixedFaces(H, W)
        paste = p.face_helper.paste_faces

        def spy(x0, restored, mats, face_frames):
            pasted.append((tuple(restored.shape), len(face_frames)))
            return paste(x0, restored, mats, face_frames)
        p.face_helper.paste_faces = spy
        return p
    pl.build_pipeline = build_with_fixed_faces
    t0 = time.perf_counter()
    try:
        rc = cli.main(argv)
    finally:
        pl.build_pipeline = build
    if rc != 0:
        print(f"exit status {rc}")
        return 1
    assert pasted and all(shape[1:] == (3, 512, 512) and shape[0] == n and n % 2 == 0 for shape, n in pasted), pasted[:4]
    names = sorted(os.listdir(out))
    assert names == [f"{i:04d}.png" for i in range(a.frames)], names
    shape = np.asarray(Image.open(os.path.join(out, names[0]))).shape
    assert shape == (4 * h, 4 * w, 3), shape
    print(f"ok: {a.frames} frames of {H}x{W} restored; CodeFormer ran on 512x512 crops of 2 faces per frame in {len(pasted)} "
          f"steps ({max(n for _, n in pasted)} crops in the largest window), {a.steps} steps a window, "
          f"{time.perf_counter() - t0:.1f} s including start-up")
    return 0


if __name__ == "__main__":
    sys.exit(main())
