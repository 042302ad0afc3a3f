"""Generate tests/golden/g15_bisenet.npz: the BiSeNet face parser, end to end, from the reference's own modules.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_bisenet.py

facelib/parsing/bisenet.py and resnet.py import torch only; they are loaded BY PATH (the package's __init__ pulls the
download helper and cv2) and run unmodified, eval mode, 8 intra-op threads (tests/util.FIXTURE_THREADS).  Inputs
(tests/bisenet_cpu.py): seeded uint8 blocks, (u8 - 128) / 128, enlarged bilinearly -- one 136 x 168 pair (odd feature
sizes at every level) and one 512 x 512 pair.

Weights: name-seeded (tests/golden/weights.py), which alone gives a degenerate parse (one class wins 74 % of the pixels
or more, the paste-mask colormap is 255 on > 99.8 % of them: a mask test would pass with a constant).  So the main head's
bias-free 1x1 (``conv_out.conv_out.weight``, 19 x 256) is refitted by least squares so that its logits on the two inputs
follow a seeded 6 x 6 normal field per class and frame, enlarged bicubically to the 1/8 grid.  The refit is a host
computation: the refitted weight is stored in the fixture.  Asserted below on the reference's own output, for both
inputs: 10 % .. 90 % of the pixels map to 255 under the colormap, at least 5 classes hold more than 1 % each, and class
2 holds between 2 % and 98 % (the face_weight test exchanges rows 0 and 2 of the head, which permutes the logits exactly
and makes that the class-0 share).

Stored per case: the 1/8-resolution logits of the three heads (forward hooks on the 1x1 convolutions; the 512 x 512
case at every second position -- every fourth for conv_out16 -- to keep the file under 1 MiB), the arg-max map in full
(uint8), the top-2 margin of every pixel as a quantised lower bound (``margin_q``: floor(4 log2(margin / max|logit|)) +
160, clipped to 0 .. 255, so margin >= max|logit| * 2 ** ((q - 160) / 4)), and the full-size logits and ``return_feat``
maps at 24 seeded pixels per frame.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import save  # noqa: E402
from tests import bisenet_cpu as bc  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402

MASK_COLORMAP = [0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 0, 0, 0, 0]
TARGET_SEED = 1520      # of the seeds tried upwards from 1500, the first whose parse meets every condition asserted below
SUB = {"small": (1, 1, 1), "big": (2, 4, 2)}            # stride of the stored 1/8-resolution logits per head


def load_reference_bisenet():
    """The reference's facelib/parsing/bisenet.py (+ resnet.py, its relative import) without the package __init__."""
    import importlib
    import refimport
    pkg = types.ModuleType("ref_parsing")
    pkg.__path__ = [os.path.join(refimport.REFERENCE_ROOT, "guided_diffusion", "facelib", "parsing")]
    sys.modules["ref_parsing"] = pkg
    sys.dont_write_bytecode = True
    return importlib.import_module("ref_parsing.bisenet")


def refit_head(m, xs):
    """Least-squares refit of the main head's 1x1 against a seeded smooth target on the 1/8 grids of the inputs ``xs``
    (all of them in one system, so that the parse is varied on each)."""
    feats = []
    h = m.conv_out.conv.register_forward_hook(lambda mod, inp, out: feats.append(out.detach().clone()))
    for x in xs:
        m(x)
    h.remove()
    g = torch.Generator().manual_seed(TARGET_SEED)
    X, T = [], []
    for feat in feats:                                                  # (B, 256, h, w)
        B, C, hh, ww = feat.shape
        target = F.interpolate(torch.randn(B, 19, 6, 6, generator=g), size=(hh, ww), mode="bicubic", align_corners=False)
        X.append(feat.permute(0, 2, 3, 1).reshape(-1, C).double())
        T.append(target.permute(0, 2, 3, 1).reshape(-1, 19).double())
    W = torch.linalg.lstsq(torch.cat(X), torch.cat(T)).solution         # (256, 19)
    return W.t().float().reshape(19, -1, 1, 1).contiguous()


def quantise_margin(margin, scale):
    q = torch.floor(4.0 * torch.log2((margin / scale).clamp_min(1e-30))) + 160
    return q.clamp(0, 255).to(torch.uint8)


def g15_bisenet():
    ref = load_reference_bisenet()
    m = ref.BiSeNet(num_class=19)
    name_seeded_weights(m)
    m.eval()
    xs = {case: bc.bisenet_input(bc.input_u8(case), case) for case in bc.SIZES}
    head = refit_head(m, [xs["big"], xs["small"]])
    with torch.no_grad():
        m.conv_out.conv_out.weight.copy_(head)
    sd = m.state_dict()
    arrays = dict(head=head.reshape(19, -1), param_names=np.array(list(sd.keys())),
                  param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
                  n_params=np.array(sum(p.numel() for p in m.parameters())))
    cmap = torch.tensor(MASK_COLORMAP)
    for case, x in xs.items():
        low = {}
        hooks = [getattr(m, n).conv_out.register_forward_hook(lambda mod, inp, out, n=n: low.__setitem__(n, out.detach().clone()))
                 for n in ("conv_out", "conv_out16", "conv_out32")]
        outs = m(x, return_feat=True)
        for h in hooks:
            h.remove()
        out = outs[0]
        am = out.argmax(1)
        share = torch.bincount(am.reshape(-1), minlength=19).float() / am.numel()
        white = (cmap[am] == 255).float().mean().item()
        print(case, "share mapped to 255:", round(white, 3), "classes above 1 %:", int((share > 0.01).sum()),
              "class shares:", [round(v, 3) for v in share.tolist()])
        assert 0.10 < white < 0.90, white
        assert int((share > 0.01).sum()) >= 5, share
        # the face_weight test exchanges rows 0 and 2 of the head (class 0 need not win on its own): class 2 must hold a real share
        assert 0.02 < share[2].item() < 0.98, share
        top2 = out.topk(2, dim=1)[0]
        margin = top2[:, 0] - top2[:, 1]
        scale = out.abs().max().item()
        for t in (1e-3, 3e-4, 1e-4):
            print("   margin below", t, "x max|logit|:", round((margin < t * scale).float().mean().item(), 4))
        pix = bc.sample_pixels(case)
        arrays.update({
            f"{case}_u8": bc.input_u8(case),
            f"{case}_argmax": am.to(torch.uint8), f"{case}_margin_q": quantise_margin(margin, scale),
            f"{case}_logit_max": np.array(scale, dtype=np.float32), f"{case}_pix": pix.int()})
        for n, s in zip(("conv_out", "conv_out16", "conv_out32"), SUB[case]):
            arrays[f"{case}_low_{n}"] = low[n][:, :, ::s, ::s].contiguous()
        for n, t in zip(("out", "out16", "out32", "feat", "feat16", "feat32"), outs):
            arrays[f"{case}_pix_{n}"] = bc.gather_pixels(t, pix)
    save("g15_bisenet", **arrays)
    size = os.path.getsize(os.path.join(HERE, "g15_bisenet.npz"))
    print("g15_bisenet.npz:", size, "bytes")
    assert size < 1 << 20, size


def main():
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g15_bisenet()


if __name__ == "__main__":
    main()
