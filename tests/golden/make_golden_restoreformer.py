"""Generate tests/golden/g13_restoreformer.npz: the RestoreFormer prior (VQVAEGANMultiHeadTransformer with its default
arguments), end to end, from the reference's own module.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_restoreformer.py

restoreformer.py imports torch and numpy only, so the reference's classes run unmodified here.  Weights are name-seeded
(tests/golden/weights.py), eval mode, 8 intra-op threads (tests/util.FIXTURE_THREADS).  The two 512 x 512 faces are
4 x 4 blocks of a 128 x 128 uint8 image each, x = (u8 - 128) / 128 (exact in fp16).  To keep the file under 1 MiB the
larger tensors are stored in part: ``mid_atten`` at every 4th channel, ``dec`` at 4096 seeded pixel positions per face
(``dec_pix``, flat indices into the 512 x 512 grid); z, the code indices and the top-2 distance margins in full.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _load_ref_file, save  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402

DEC_PIXELS = 4096


def restoreformer_input(x_u8):
    """(B, 3, 128, 128) uint8 -> (B, 3, 512, 512) f32 in [-1, 1): each pixel a 4 x 4 block."""
    x = (torch.as_tensor(np.asarray(x_u8)).float() - 128.0) / 128.0
    return x.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3).contiguous()


def input_u8(seed=13):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (2, 3, 128, 128), generator=g, dtype=torch.uint8)


def dec_pixels(seed=131):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(512 * 512, generator=g)[:DEC_PIXELS].sort()[0] for _ in range(2)]).int()


def g13_restoreformer():
    rf = _load_ref_file("ref_restoreformer", "restoreformer.py")
    m = rf.VQVAEGANMultiHeadTransformer()
    name_seeded_weights(m)
    m.eval()
    zs = []
    m.quant_conv.register_forward_hook(lambda mod, inp, out: zs.append(out.detach().clone()))
    u8 = input_u8()
    x = restoreformer_input(u8)
    dec, _, info, hs = m(x)
    z = zs[0]
    d = info[3]
    top2 = d.topk(2, dim=1, largest=False)[0]
    idx = info[2].reshape(2, -1)
    pix = dec_pixels()
    dec_sub = torch.stack([dec[b].reshape(3, -1)[:, pix[b].long()] for b in range(2)])
    sd = m.state_dict()
    save("g13_restoreformer", x_u8=u8, param_names=np.array(list(sd.keys())),
         param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
         z=z, idx=idx.int(), margin=(top2[:, 1] - top2[:, 0]).reshape(2, -1),
         mid_atten_c4=hs["mid_atten"][:, ::4].contiguous(), dec_pix=pix, dec_sub=dec_sub)


def main():
    import refimport
    refimport.install_stubs()
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g13_restoreformer()


if __name__ == "__main__":
    main()
