"""Generate tests/golden/g14_vqfr.npz: the VQFR v2 prior (VQFRv2 in the VQFR project's v2 release configuration, and a
small "Nearest"-mode network), end to end, from the reference's own module.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_vqfr.py

vqfr.py runs unmodified.  What it imports and this environment lacks is stubbed: ``timm.models.layers.trunc_normal_``
(nn.init.trunc_normal_) and ``torchvision`` (``__version__`` 0.15.2, so DCNv2Pack takes its torchvision branch, and
``ops.deform_conv2d`` = oracle.thirdparty.deform_conv2d); the reference's ``guided_diffusion.dcn`` imports without its
compiled extension.  Weights: tests/vqfr_cpu.vqfr_seeded_weights (name-seeded, conv_offset x 4 so that the offsets are
several pixels long and samples leave the frame); eval mode, 8 intra-op threads.  Inputs are 4 x 4 blocks of seeded
128 x 128 uint8 images, x = (u8 - 128) / 128.  To stay under 1 MiB the large tensors are stored in part:

  * release network (G = 4, two faces): the code indices and the top-2 logit margins in full; the output and offset of
    the level-1 TextureWarpingModule (64 channels, 512^2) at 512 seeded pixels per face; main_dec at 4096 pixels;
  * "Nearest" network (G = 8, one face): the code indices, the top-2 distance margins, main_dec at 2048 pixels.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _load_ref_file, save  # noqa: E402
from tests.vqfr_cpu import RELEASE, SMALL_NEAREST, pixels, take, vqfr_input, vqfr_seeded_weights  # noqa: E402

TWM_PIXELS, DEC_PIXELS, SMALL_DEC_PIXELS = 512, 4096, 2048


def input_u8(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, 128, 128), generator=g, dtype=torch.uint8)


def _stubs():
    import torch.nn as nn
    from oracle import thirdparty as tp

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("timm")
    mod("timm.models")
    mod("timm.models.layers", trunc_normal_=nn.init.trunc_normal_)
    tv = sys.modules["torchvision"]
    tv.__version__ = "0.15.2"
    tv.ops.deform_conv2d = tp.deform_conv2d


def _margin(score):
    top2 = score.topk(2, dim=1)[0]
    return top2[:, 0] - top2[:, 1]


def run(vq, cfg, u8):
    m = vq.VQFRv2(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()})
    vqfr_seeded_weights(m)
    m.eval()
    twm = {}
    m.main_branch.align_func_dict["Level_1"].register_forward_hook(lambda mod, inp, out: twm.update(out=out))
    res = m(vqfr_input(u8))
    if cfg["code_selection_mode"] == "Predict":
        score = res["quant_logit"].reshape(-1, 1024)
    else:
        z = res["enc_feat"].permute(0, 2, 3, 1).reshape(-1, 256)
        e = m.quantizer.embedding.weight
        score = -(torch.sum(z ** 2, dim=1, keepdim=True) + torch.sum(e ** 2, dim=1) - 2 * z @ e.t())
    return m, res, score, twm["out"]


def g14_vqfr():
    vq = _load_ref_file("ref_vqfr", "vqfr.py")
    u8 = input_u8(2, 14)
    m, res, score, (warp, offset) = run(vq, RELEASE, u8)
    B = u8.shape[0]
    tpix, dpix = pixels(B, TWM_PIXELS, 141), pixels(B, DEC_PIXELS, 142)
    sd = m.state_dict()
    arrays = dict(x_u8=u8, param_names=np.array(list(sd.keys())),
                  param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
                  idx=score.argmax(1).reshape(B, -1).int(), margin=_margin(score).reshape(B, -1),
                  twm1_pix=tpix.int(), twm1_out=take(warp, tpix), twm1_offset=take(offset, tpix),
                  dec_pix=dpix.int(), dec_sub=take(res["main_dec"], dpix))
    u8s = input_u8(1, 15)
    ms, rs, ss, _ = run(vq, SMALL_NEAREST, u8s)
    spix = pixels(1, SMALL_DEC_PIXELS, 143)
    sds = ms.state_dict()
    arrays.update(n_x_u8=u8s, n_param_names=np.array(list(sds.keys())), n_idx=ss.argmax(1).reshape(1, -1).int(),
                  n_margin=_margin(ss).reshape(1, -1), n_dec_pix=spix.int(), n_dec_sub=take(rs["main_dec"], spix))
    save("g14_vqfr", **arrays)


def main():
    import refimport
    refimport.install_stubs()
    _stubs()
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g14_vqfr()


if __name__ == "__main__":
    main()
