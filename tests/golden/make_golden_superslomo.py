"""Generate tests/golden/g17_superslomo.npz: SuperSloMo frame interpolation, end to end, from the reference's own module.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_superslomo.py

guided_diffusion/superslomo.py imports torch, numpy and ``torchvision.transforms.functional.normalize``; it is loaded BY
PATH with a three-line stand-in for that one function and runs unmodified, eval mode, 8 intra-op threads
(tests/util.FIXTURE_THREADS).

Weights: name-seeded (tests/golden/weights.py), regenerated in the tests and never stored.  On their own they give flows of
0.01 px, with which a test would pass with the flows ignored, so ``flow_estimator.conv3`` is scaled by S1 and
``interp.conv3`` by S2 (tests/superslomo_cpu.py; both factors are stored).  Inputs: seeded smooth frames, frame1 a shifted,
noised copy of frame0, stored as uint8.  Asserted below on the reference's own output, per case and timestep, over the
samples of the two final back-warps together: the mean |final flow| lies between 1 and 10 px and 5 % .. 40 % of the samples
have a corner outside the frame (and neither warp alone falls below 1 px or 5 %); the visibility map has a standard
deviation >= 0.1, a minimum below 0.1 and a maximum above 0.9; the output differs from the plain blend
(1 - t) frame0 + t frame1 by more than 100 x the stored deviation of the output.  (conv3 ends in a LeakyReLU: a visibility
logit below -2.2 needs a pre-activation below -22, and the same scale makes the positive flow components of that UNet
large, so S2 cannot be chosen freely; of the pairs tried on these inputs S1 = 85, S2 = 40 meets every condition with the
widest margins.)

Stored per case: f01, f10 and the output frames (case "small" in full; case "big" on every second row and column plus 64
seeded pixels per frame of the batch), the reference's parameter names and shapes, and per quantity THE REFERENCE'S OWN
f32-vs-float64 DEVIATION: the largest absolute difference between the module run in f32 and a ``.double()`` copy of it on
the same inputs.  The tests' bounds are multiples of that.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import save  # noqa: E402
from tests import superslomo_cpu as sc  # noqa: E402


def load_reference_superslomo():
    """The reference's guided_diffusion/superslomo.py without its package and without torchvision."""
    import refimport

    def normalize(tensor, mean, std, inplace=False):
        mean, std = (torch.as_tensor(v, dtype=tensor.dtype).view(-1, 1, 1) for v in (mean, std))
        return tensor.sub_(mean).div_(std) if inplace else (tensor - mean) / std
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision.transforms.functional"].normalize = normalize
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(
        "ref_superslomo", os.path.join(refimport.REFERENCE_ROOT, "guided_diffusion", "superslomo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def corner_outside(flow):
    """Share of the samples of back_warp(., flow) that touch a corner outside the frame."""
    H, W = flow.shape[2:]
    ix = torch.arange(W).view(1, 1, W) + flow[:, 0] - 0.5
    iy = torch.arange(H).view(1, H, 1) + flow[:, 1] - 0.5
    x0, y0 = ix.floor(), iy.floor()
    return ((x0 < 0) | (x0 + 1 > W - 1) | (y0 < 0) | (y0 + 1 > H - 1)).float().mean().item()


def g17_superslomo():
    ref = load_reference_superslomo()
    m = ref.SuperSloMo().eval()
    sd = sc.seeded_state_dict(m)
    m.load_state_dict(sd)
    m64 = ref.SuperSloMo().eval()
    m64.load_state_dict(sd)
    m64 = m64.double()
    print("parameters:", sum(p.numel() for p in m.parameters()))
    arrays = dict(s1=np.array(sc.S1), s2=np.array(sc.S2), param_names=np.array(list(sd.keys())),
                  param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
                  n_params=np.array(sum(p.numel() for p in m.parameters())))
    for case, c in sc.CASES.items():
        u8 = sc.input_u8(case)
        f0, f1 = sc.frames(u8)
        out, f01, f10 = m(f0.clone(), f1.clone(), c["factor"], return_flow=True)
        out64, f01_64, f10_64 = m64(f0.double(), f1.double(), c["factor"], return_flow=True)
        dev = {n: (a.double() - b).abs().max().item() for n, a, b in (("f01", f01, f01_64), ("f10", f10, f10_64), ("out", out, out64))}
        print(case, "f32-vs-f64 deviation:", {k: f"{v:.2e}" for k, v in dev.items()})
        # the restatement reproduces the reference on this host (tests/test_superslomo_cpu.py repeats it from the fixture)
        detail = []
        r_out, r_f01, r_f10 = sc.superslomo_forward(sd, f0, f1, c["factor"], detail=detail)
        print(case, "restatement vs reference:", (r_out - out).abs().max().item(), (r_f01 - f01).abs().max().item())
        for k, d in enumerate(detail, start=1):
            t = k / c["factor"]
            mag = [fl.pow(2).sum(1).sqrt().mean().item() for fl in (d["ft0f"], d["ft1f"])]
            outside = [corner_outside(fl) for fl in (d["ft0f"], d["ft1f"])]
            v = d["v0"]
            plain = (1 - t) * f0 + t * f1
            diff = (out[:, k - 1] - plain).abs().max().item()
            print(f"  {case} t={t:.2f}: mean |flow| {mag[0]:.2f} {mag[1]:.2f} px, outside share {outside[0]:.3f} {outside[1]:.3f}, "
                  f"visibility std {v.std().item():.3f} min {v.min().item():.4f} max {v.max().item():.4f}, "
                  f"max |out - plain blend| {diff:.3f}")
            assert 1.0 <= sum(mag) / 2 <= 10.0 and min(mag) >= 1.0, mag
            assert 0.05 <= sum(outside) / 2 <= 0.40 and min(outside) >= 0.05, outside
            assert v.std().item() >= 0.1 and v.min().item() < 0.1 and v.max().item() > 0.9
            assert diff > 100 * dev["out"], (diff, dev["out"])
        pix = sc.sample_pixels(case)
        arrays[f"{case}_u8"] = u8
        for n, t in (("f01", f01), ("f10", f10), ("out", out)):
            arrays[f"{case}_{n}"] = sc.stored(case, t)
            arrays[f"{case}_dev_{n}"] = np.array(dev[n])
            if case != "small":
                arrays[f"{case}_pix_{n}"] = sc.gather_pixels(t, pix)
        if case != "small":
            arrays[f"{case}_pix"] = pix.int()
    save("g17_superslomo", **arrays)
    size = os.path.getsize(os.path.join(HERE, "g17_superslomo.npz"))
    print("g17_superslomo.npz:", size, "bytes")
    assert size < 1 << 20, size


def main():
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g17_superslomo()


if __name__ == "__main__":
    main()
