"""GPU: flair_amd.degrade applies the very operator the data-consistency step assumes, and the degrade / evaluate command
lines run end to end on frame files."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

T = 3
SIZES = {"gaussian": (64, 128), "jpeg": (64, 128), "x8_bicubic": (128, 144), "x16_bicubic": (128, 144)}
TASKS = list(SIZES)


@functools.lru_cache(maxsize=None)
def smooth_frames(H, W, seed=11):
    """T seeded random smooth frames (T, 3, H, W) in [0, 1]: an 8 x 8 random field enlarged bilinearly, plus a little noise."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(T, 3, 8, 8, generator=g)
    return (F.interpolate(base, (H, W), mode="bilinear", align_corners=False)
            + 0.05 * torch.randn(T, 3, H, W, generator=g)).clamp(0, 1)


def kernel_of(task):
    from flair_amd import workload as wl
    return wl.synthetic_blur_kernel() if "bicubic" not in task else None


def degrader(task, dev, **kw):
    from flair_amd import degrade
    return degrade.Degrader(task, SIZES[task], dev, kernel=kernel_of(task), **kw)


def direct(task, x_n, dev, qf=60):
    """The operator calls A_pinv / bicubic_restore apply to the running estimate, on operators built from their classes."""
    from flair_amd import workload as wl
    H, W = x_n.shape[-2:]
    if "bicubic" in task:
        from flair_amd.guided_diffusion.restore_util import SRConv
        f = wl.TASKS[task]["factor"]
        A = SRConv(wl.bicubic_taps(f), 3, (H, W), dev, stride=f)
        return A.A(x_n.reshape(T, -1)).reshape(T, 3, H // f, W // f)
    from flair_amd.guided_diffusion import pseudoSR as psr
    from flair_amd.guided_diffusion.jpeg import jpeg_decode, jpeg_encode
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(), kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    y = A.DownscaleOP(x_n)
    return jpeg_decode(jpeg_encode(y, qf), qf) if task == "jpeg" else y


@pytest.mark.parametrize("task", TASKS)
def test_degrader_is_the_direct_composition(dev, task):
    from flair_amd import workload as wl
    H, W = SIZES[task]
    f = wl.TASKS[task]["factor"]
    clean = smooth_frames(H, W).to(dev)
    y_n, y_u8 = degrader(task, dev)(clean)
    assert y_n.shape == (T, 3, H // f, W // f) and y_n.dtype == torch.float32
    assert y_u8.shape == (T, H // f, W // f, 3) and y_u8.dtype == torch.uint8 and y_u8.is_contiguous()
    ref = direct(task, clean * 2 - 1, dev)
    assert torch.equal(y_n.view(torch.int32), ref.view(torch.int32))
    if task == "jpeg":                                    # another quality factor is another measurement
        y35 = degrader(task, dev, jpeg_qf=35)(clean)[0]
        assert torch.equal(y35.view(torch.int32), direct(task, clean * 2 - 1, dev, qf=35).view(torch.int32))
        assert not torch.equal(y35, y_n)


def test_against_the_cpu_oracle(dev):
    """gaussian at 64 x 64 against oracle.degrade.BlurOperator.down and x8 at 128 x 128 against oracle.degrade.SeparableSR.A,
    at the tolerance of test_blur_operator_vs_oracle."""
    from flair_amd import degrade, workload as wl
    from oracle import degrade as odeg
    clean = smooth_frames(64, 64)
    y_n, _ = degrade.Degrader("gaussian", (64, 64), dev, kernel=wl.synthetic_blur_kernel())(clean.to(dev))
    ref = odeg.BlurOperator(wl.synthetic_blur_kernel(), 4).down(clean * 2 - 1)
    err = (y_n.cpu() - ref).abs().max().item()
    print(f"degrade gaussian 64x64 vs oracle: {err:.3e}")
    assert y_n.shape == ref.shape and err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    clean = smooth_frames(128, 128)
    y_n, _ = degrade.Degrader("x8_bicubic", (128, 128), dev)(clean.to(dev))
    ref = odeg.SeparableSR(wl.bicubic_taps(8), 3, 128, 8).A((clean * 2 - 1).reshape(T, -1)).reshape(T, 3, 16, 16)
    err = (y_n.cpu() - ref).abs().max().item()
    print(f"degrade x8_bicubic 128x128 vs oracle: {err:.3e}")
    assert y_n.shape == ref.shape and err <= 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("task", TASKS)
def test_consistent_with_the_sampler(dev, task):
    """With y_n as the window's measurement, the data-consistency term of the clean frames (the Pipeline's restore_fn, built
    directly from the operator, no network) is exactly zero: the operator is deterministic, so the difference inside it
    is 0 bit for bit."""
    from flair_amd import pipeline as pl
    H, W = SIZES[task]
    clean = smooth_frames(H, W).to(dev)
    d = degrader(task, dev)
    y_n, _ = d(clean)
    A = pl.build_operator(task, (H, W), dev, kernel_of(task))
    p = pl.Pipeline(task, None, None, A, None, None, None, (H, W), dev)
    x_n = clean * 2 - 1
    term = p.restore_fn_for(d.jpeg_qf if task == "jpeg" else -1)(y_n[None])(x_n)
    assert term.shape == x_n.shape and torch.count_nonzero(term).item() == 0
    # a measurement that is off by one grey level somewhere is not consistent
    y_off = y_n.clone()
    y_off[0, 0, 1, 1] += 2.0 / 255
    assert torch.count_nonzero(p.restore_fn_for(d.jpeg_qf if task == "jpeg" else -1)(y_off[None])(x_n)).item() > 0


@pytest.mark.parametrize("task", TASKS)
def test_quantisation_is_rounding_to_nearest(dev, task):
    """|normalise(y_u8 / 255) - clamp(y_n, -1, 1)| <= 1/255 + 1e-6: half a grey level in the [-1, 1] domain."""
    H, W = SIZES[task]
    y_n, y_u8 = degrader(task, dev)(smooth_frames(H, W).to(dev))
    back = y_u8.permute(0, 3, 1, 2).float() / 255 * 2 - 1
    assert (back - y_n.clamp(-1, 1)).abs().max().item() <= 1 / 255 + 1e-6
    want = torch.from_numpy(np.rint(((y_n.double().cpu().numpy() + 1) / 2).clip(0, 1) * 255)).to(torch.uint8)
    assert (y_u8.cpu().permute(0, 3, 1, 2).int() - want.int()).abs().max().item() <= 1      # f32 against f64 at a tie
    assert (y_u8.cpu().permute(0, 3, 1, 2) != want).float().mean().item() < 1e-3


def test_noise(dev):
    """Seeded noise repeats bit for bit, another seed differs, and sigma is on the 0..255 scale of a [-1, 1] signal."""
    H, W = 128, 256                                       # 3 x 3 x 32 x 64 = 18 432 values
    from flair_amd import degrade, workload as wl
    d = degrade.Degrader("gaussian", (H, W), dev, kernel=wl.synthetic_blur_kernel())
    clean = smooth_frames(H, W).to(dev)
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)                                  # noqa: E731
    y0, _ = d(clean)
    a, a8 = d(clean, noise_sigma=5, generator=gen(3))
    b, b8 = d(clean, noise_sigma=5, generator=gen(3))
    c, _ = d(clean, noise_sigma=5, generator=gen(4))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a8, b8) and not torch.equal(a, c)
    diff = (a - y0).double()
    n = diff.numel()
    assert n >= 18000
    std = diff.std().item()
    print(f"noise: sample std {std:.5f} over {n} values, expected {10 / 255:.5f}")
    assert abs(std - 10 / 255) <= 0.05 * 10 / 255
    assert abs(diff.mean().item()) <= 4 * (10 / 255) / math.sqrt(n)


def test_degrade_and_evaluate_on_files(dev, tmp_path, capsys, monkeypatch):
    """Four clean 64 x 128 PNGs -> degrade gaussian -> four 16 x 32 PNGs with the bytes of y_u8; evaluate of a directory
    against itself reports inf and 1.0000, and against a copy with one changed pixel the PSNR computed by hand."""
    import json
    from flair_amd import io as fio, pipeline as pl, workload as wl
    from flair_amd.__main__ import main
    clean_dir, out_dir, copy_dir = tmp_path / "clean", tmp_path / "lr", tmp_path / "copy"
    clean_dir.mkdir()
    copy_dir.mkdir()
    g = torch.Generator().manual_seed(5)
    base = torch.rand(4, 3, 8, 8, generator=g)
    frames = (F.interpolate(base, (64, 128), mode="bilinear", align_corners=False) * 255).round().to(torch.uint8)
    hwc = frames.permute(0, 2, 3, 1).contiguous().numpy()
    for i in range(4):
        fio.write_frame(str(clean_dir / f"{i:04d}.png"), hwc[i])
        changed = hwc[i].copy()
        if i == 2:
            changed[7, 9, 1] = (int(changed[7, 9, 1]) + 40) % 256
        fio.write_frame(str(copy_dir / f"{i:04d}.png"), changed)
    monkeypatch.setattr(pl, "load_blur_kernel", lambda path: wl.synthetic_blur_kernel())
    try:
        assert main(["degrade", "gaussian", str(clean_dir), str(out_dir)]) == 0
        from flair_amd import degrade
        _, y_u8 = degrade.Degrader("gaussian", (64, 128), dev, kernel=wl.synthetic_blur_kernel())(frames.float().to(dev) / 255.0)
        paths = fio.list_frames(str(out_dir))
        assert [os.path.basename(p) for p in paths] == [f"{i:04d}.png" for i in range(4)]
        for i, p in enumerate(paths):
            got = fio.decode_frame(p).transpose(1, 2, 0)
            assert got.shape == (16, 32, 3) and np.array_equal(got, y_u8[i].cpu().numpy())
        capsys.readouterr()
        assert main(["evaluate", str(clean_dir), str(clean_dir)]) == 0
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 5 and all("psnr inf" in ln and "ssim 1.0000" in ln for ln in lines), lines
        report = tmp_path / "m.json"
        assert main(["evaluate", str(copy_dir), str(clean_dir), "--json", str(report)]) == 0
        lines = capsys.readouterr().out.strip().splitlines()
        d = int(hwc[2][7, 9, 1]) - (int(hwc[2][7, 9, 1]) + 40) % 256
        psnr = 10 * math.log10(255.0 ** 2 * 3 * 64 * 128 / d ** 2)
        assert f"0002.png  psnr {psnr:.4f}" in lines[2] and "psnr inf" in lines[0] and "psnr inf" in lines[4]
        got = json.load(open(report))
        assert got["count"] == 4 and abs(got["frames"][2]["psnr"] - psnr) < 1e-9 and got["frames"][2]["ssim"] < 1
        assert got["frames"][0]["psnr"] == math.inf and got["mean"]["psnr"] == math.inf
    finally:
        torch.set_grad_enabled(True)
