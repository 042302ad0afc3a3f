"""Cost per sampler step of the unaligned prior branch (gaussian_diffusion.py:476-493) at 512 x 512, random weights.

The branch crops the faces out of x0 and x_t, runs CodeFormer on the crops, parses the restored faces (ParseNet),
blurs the parsing mask and pastes the faces back; the aligned branch runs CodeFormer on the whole frames.  Both are timed
here on a window of --frames frames, with a full-size CodeFormer and ParseNet (random weights) and one face per frame.

    python tools/bench_unaligned.py --frames 10      # one JSON line: ms per step of each part and of both branches
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from flair_amd import ops
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.codeformer import CodeFormer
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    T, S = a.frames, 512
    torch.manual_seed(0)
    gan = CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                     connect_list=["32", "64", "128", "256"]).to(dev).eval()
    parser = ParseNet(in_size=512, out_size=512, parsing_ch=19).to(dev).eval()
    helper = FaceRestoreHelper(face_size=S, device=dev, face_parse=parser)
    tpl = helper.face_template
    # one face per frame, 70 % of the template's size, drifting across the window
    mats = [estimate_affine_partial(tpl * 0.7 + np.array([60.0 + 4 * k, 90.0 - 2 * k]), tpl) for k in range(T)]
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.rand(T, 3, S, S, device=dev, generator=g) * 2 - 1
    xt = torch.randn(T, 3, S, S, device=dev, generator=g)
    aux = wl.codeformer_aux(gan)
    parts = {}

    def timed(name, fn, *args):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = fn(*args)
        ev1.record()
        parts.setdefault(name, []).append((ev0, ev1))
        return out

    def unaligned():
        f = timed("crop x0", helper.get_crop_face_from_affine_matrices, x0, mats)
        ft = timed("crop xt", helper.get_crop_face_from_affine_matrices, xt, mats)
        f = timed("codeformer", aux, f, None, ft)
        inv_face, inv_mask = timed("parse + mask blur + inverse warps", helper.inverse_faces, f, mats)
        return timed("blend", ops.face_blend, x0, inv_face.float().contiguous(), inv_mask.float().contiguous())

    def aligned():
        return aux(x0, None, xt)

    res = {}
    for name, fn in (("unaligned_branch", unaligned), ("aligned_branch", aligned)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        parts.clear()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.iters):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        res[name + "_ms"] = ev0.elapsed_time(ev1) / a.iters
        for part, evs in parts.items():
            res[part + "_ms"] = sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs)
    res.update(frames=T, size=S, iters=a.iters, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
