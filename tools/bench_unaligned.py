"""Cost per sampler step of the unaligned prior branch (gaussian_diffusion.py:476-493) at 512 x 512, random weights.

The branch crops the faces out of x0 and x_t, runs CodeFormer on the crops, parses the restored faces (ParseNet or
BiSeNet), blurs the parsing mask and pastes the faces back; the aligned branch runs CodeFormer on the whole frames.  Both
are timed here on a window of --frames frames, with a full-size CodeFormer and parser (random weights) and one face per
frame.

    python tools/bench_unaligned.py --frames 10      # one JSON line: ms per step of each part and of both branches
    python tools/bench_unaligned.py --parser both    # one line per parser, same process, plus the BiSeNet tail and the
                                                     # small-kernel timings (fused vs unfused arg-max, pool / gate launches)
    python tools/bench_unaligned.py --faces-per-frame 1 2   # one more line per count: the branch with that many faces in
                                                     # every frame (face_frames path) and the fused paste against the
                                                     # warp + warp + blend launches on the same data
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
    ap.add_argument("--parser", choices=("parsenet", "bisenet", "both"), default="parsenet")
    ap.add_argument("--faces-per-frame", type=int, nargs="*", default=[], metavar="F",
                    help="also time the several-faces path with F faces in every frame (one JSON line per F)")
    a = ap.parse_args()
    from flair_amd.guided_diffusion.codeformer import CodeFormer
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gan = CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9,
                     connect_list=["32", "64", "128", "256"]).to(dev).eval()
    for k, name in enumerate(("parsenet", "bisenet") if a.parser == "both" else (a.parser,)):
        run(a, dev, gan, name, with_aligned=k == 0)
        for F in a.faces_per_frame:
            run_faces(a, dev, gan, name, F)


def make_parser(name, dev):
    if name == "bisenet":
        from flair_amd.guided_diffusion.bisenet import BiSeNet
        return BiSeNet(num_class=19).to(dev).eval()
    from flair_amd.guided_diffusion.parsenet import ParseNet
    return ParseNet(in_size=512, out_size=512, parsing_ch=19).to(dev).eval()


def replay_us(fn, iters=20, warmup=3):
    """Microseconds per call of ``fn`` (device events around ``iters`` back-to-back calls, after ``warmup``)."""
    for _ in range(warmup):
        fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / iters


def bisenet_kernels(T, S, dev):
    """The fused arg-max tail against the unfused composition of launches (bilinear align_corners=True resize to full size,
    then flair_argmax_codebook), and the pool / gate launches at BiSeNet's four shapes: microseconds per launch."""
    from flair_amd import ops
    g = torch.Generator(device=dev).manual_seed(2)
    logits = torch.randn(T, S // 8, S // 8, 20, device=dev, generator=g)
    zero = torch.zeros((19, 1), dtype=torch.float32, device=dev)
    big = torch.empty((T, S, S, 20), dtype=torch.float32, device=dev)
    code = torch.empty((T, S, S, 1), dtype=torch.float32, device=dev)

    def unfused():
        ops.resize(logits, (S, S), 1, channels=19, out=big)
        return ops.argmax_codebook(big, 19, zero, out=code)[1]
    out = {"tail_fused_us": replay_us(lambda: ops.upsample_argmax(logits, 19, (S, S))),
           "tail_unfused_us": replay_us(unfused)}
    same = (ops.upsample_argmax(logits, 19, (S, S))[0].reshape(-1) == unfused()).float().mean().item()
    out["tail_fused_equals_unfused_share"] = same
    for C, s in ((512, S // 32), (128, S // 32), (128, S // 16), (256, S // 8)):
        x = torch.randn(T, s, s, C, device=dev, generator=g)
        gate = torch.randn(T, C, device=dev, generator=g)
        out[f"pool_c{C}_{s}x{s}_us"] = replay_us(lambda: ops.global_avgpool(x))
        out[f"gate_c{C}_{s}x{s}_us"] = replay_us(lambda: ops.channel_gate(x, gate, logit=True, add=x, out=x))
    return out


def run(a, dev, gan, parser_name, with_aligned=True):
    from flair_amd import ops
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    T, S = a.frames, 512
    parser = make_parser(parser_name, dev)
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
    for name, fn in (("unaligned_branch", unaligned), ("aligned_branch", aligned))[:2 if with_aligned else 1]:
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
    faces = helper.get_crop_face_from_affine_matrices(x0, mats)
    res["parser_forward_ms"] = replay_us(lambda: parser.parse_indices(faces), a.iters, a.warmup) / 1e3
    if parser_name == "bisenet":
        res.update(bisenet_kernels(T, S, dev))
    res.update(parser=parser_name, frames=T, size=S, iters=a.iters, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


def run_faces(a, dev, gan, parser_name, F):
    """The branch with F faces in every frame (sampler's face_frames path: indexed crops, the prior on T * F crops, parsing,
    mask blur, one flair_face_paste), and the paste alone against what it replaces: per layer of faces a warp of the faces,
    a warp of the masks and a blend over the window (3 F launches)."""
    from flair_amd import ops
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    T, S = a.frames, 512
    if F < 1:
        raise SystemExit("--faces-per-frame needs counts >= 1")
    helper = FaceRestoreHelper(face_size=S, device=dev, face_parse=make_parser(parser_name, dev))
    tpl = helper.face_template
    # face j of frame k: 70 % / (1 + j / 2) of the template's size, drifting across the window, neighbours overlapping
    mats = [estimate_affine_partial(tpl * (0.7 / (1 + 0.5 * j)) + np.array([60.0 + 4 * k + 110.0 * j, 90.0 - 2 * k + 40.0 * j]), tpl)
            for k in range(T) for j in range(F)]
    face_frames = [k for k in range(T) for _ in range(F)]
    g = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.rand(T, 3, S, S, device=dev, generator=g) * 2 - 1
    xt = torch.randn(T, 3, S, S, device=dev, generator=g)
    aux = wl.codeformer_aux(gan)

    def branch():
        f = helper.get_crop_face_from_affine_matrices(x0, mats, face_frames)
        ft = helper.get_crop_face_from_affine_matrices(xt, mats, face_frames)
        return helper.paste_faces(x0, aux(f, None, ft), mats, face_frames)
    res = {"unaligned_branch_ms": replay_us(branch, a.iters, a.warmup) / 1e3}
    # the paste alone, on the faces and masks of this window
    faces = aux(helper.get_crop_face_from_affine_matrices(x0, mats, face_frames), None, None).float().contiguous()
    lut, kern = helper._consts(dev)
    masks = ops.face_mask_blur(helper.face_parse.parse_indices(faces).reshape(-1), T * F, S, S, lut, kern)
    minv = helper._minv(mats, dev, twice=True)
    starts = helper.frame_starts(face_frames, T)
    starts_dev = helper._index(starts, dev)
    layers = [(faces[j::F].contiguous(), masks[j::F].contiguous(), minv[j::F].contiguous()) for j in range(F)]

    def three_launches():
        v = x0
        for f, m, mi in layers:
            v = ops.face_blend(v, ops.warp_affine_cubic(f, mi, (S, S), pre=True, post=True), ops.warp_affine_cubic(m, mi, (S, S)))
        return v
    res["paste_fused_us"] = replay_us(lambda: ops.face_paste(x0, faces, masks, minv, starts_dev, starts))
    res["paste_three_launches_us"] = replay_us(three_launches)
    res["paste_fused_equals_three_launches"] = bool(torch.equal(ops.face_paste(x0, faces, masks, minv, starts_dev, starts),
                                                                three_launches()))
    res.update(parser=parser_name, frames=T, faces_per_frame=F, size=S, iters=a.iters, device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
