"""Generate tests/golden/g12_retinaface_mobile.npz: the RetinaFace MobileNet-0.25 detector, end to end, from the reference's
own modules.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_mobile.py

retinaface_net.py imports torch only, so MobileNetV1 (the body), FPN, SSH and the heads all run unmodified here, wired as
RetinaFace.__init__ / forward wire them for cfg_mnet (retinaface.py:31-49, 95-156).  retinaface.py itself needs cv2, so the
wiring and IntermediateLayerGetter (stage1 -> stage2 -> stage3, keeping the three outputs) are restated below.  Weights are
name-seeded under the names the full model gives them, in eval mode.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _load_ref_file, save  # noqa: E402
from tests.golden.weights import name_seeded_weights  # noqa: E402

H, W = 136, 168                 # not multiples of 32: the stride-2 blocks see odd sizes (68 x 84 -> ... -> 5 x 6)
MEAN = (104.0, 117.0, 123.0)


def mobile_input(seed=12):
    """Two mean-subtracted frames in [0, 255] - mean, fp16-exact so that the fixture stores them as halves."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(2, 3, H, W, generator=g) * 255.0 - torch.tensor(MEAN).view(1, 3, 1, 1)
    return x.half().float()


def g12_retinaface_mobile():
    net = _load_ref_file("ref_retinaface_net", "facelib", "detection", "retinaface", "retinaface_net.py")
    utl = _load_ref_file("ref_retinaface_utils", "facelib", "detection", "retinaface", "retinaface_utils.py")

    class Body(nn.Module):
        """IntermediateLayerGetter(MobileNetV1(), {'stage1': 1, 'stage2': 2, 'stage3': 3}): the modules up to stage3."""

        def __init__(self):
            super().__init__()
            full = net.MobileNetV1()
            self.stage1, self.stage2, self.stage3 = full.stage1, full.stage2, full.stage3

        def forward(self, x):
            o1 = self.stage1(x)
            o2 = self.stage2(o1)
            return [o1, o2, self.stage3(o2)]

    class Detector(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = Body()
            self.fpn = net.FPN([64, 128, 256], 64)
            self.ssh1, self.ssh2, self.ssh3 = net.SSH(64, 64), net.SSH(64, 64), net.SSH(64, 64)
            self.ClassHead = net.make_class_head(fpn_num=3, inchannels=64)
            self.BboxHead = net.make_bbox_head(fpn_num=3, inchannels=64)
            self.LandmarkHead = net.make_landmark_head(fpn_num=3, inchannels=64)

        def forward(self, x):
            out = self.body(x)
            fpn = self.fpn(out)
            features = [self.ssh1(fpn[0]), self.ssh2(fpn[1]), self.ssh3(fpn[2])]
            bbox = torch.cat([self.BboxHead[i](f) for i, f in enumerate(features)], dim=1)
            cls = torch.cat([self.ClassHead[i](f) for i, f in enumerate(features)], dim=1)
            ldm = torch.cat([self.LandmarkHead[i](f) for i, f in enumerate(features)], dim=1)
            return out, bbox, F.softmax(cls, dim=-1), ldm

    m = Detector()
    name_seeded_weights(m)
    m.eval()
    x = mobile_input()
    feats, bbox, conf, ldm = m(x)
    cfg = {"min_sizes": [[16, 32], [64, 128], [256, 512]], "steps": [8, 16, 32], "variance": [0.1, 0.2], "clip": False}
    priors = utl.PriorBox(cfg, image_size=(H, W)).forward()
    boxes = utl.decode(bbox[0].clone(), priors, cfg["variance"])
    lms = utl.decode_landm(ldm[0].clone(), priors, cfg["variance"])
    sd = m.state_dict()
    save("g12_retinaface_mobile", x=x.half(), body0=feats[0], body1=feats[1], body2=feats[2], bbox=bbox, conf=conf, ldm=ldm,
         priors=priors, boxes=boxes, landmarks=lms,
         param_names=np.array(list(sd.keys())), param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]))


def main():
    import refimport
    refimport.install_stubs()
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g12_retinaface_mobile()


if __name__ == "__main__":
    main()
