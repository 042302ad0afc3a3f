"""Make a task's degraded frames from clean ones with the exact measurement model the data-consistency step assumes.

``restore`` solves ``y = A(x)`` for one operator per task (pipeline.build_operator): frames degraded any other way -- an
image editor's bicubic, a real JPEG encoder -- silently break that equation.  ``Degrader`` applies the very calls
``A_pinv`` / ``bicubic_restore`` apply to the running estimate, on the same HIP kernels:

  * gaussian:  ``A.DownscaleOP(x)`` (the 9 x 9 anti-aliasing blur, every 4th sample from phase ``pre_stride``);
  * jpeg:      the same followed by the 4:2:0 codec at ``jpeg_qf`` (``jpeg_decode(jpeg_encode(., qf), qf)``);
  * x8 / x16:  ``SRConv.A`` (the 32 / 64-tap bicubic kernel, reflect padding).

The reference ships 25 pre-degraded frames per task and no tool to make more.
"""
import torch

from . import io as fio
from . import pipeline as pl
from . import workload as wl


class Degrader:
    """``Degrader(task, (H, W), device, kernel=None, jpeg_qf=None)``: (H, W) must pass pipeline.check_frame_size;
    ``kernel``: the 25 x 25 blur array of the gaussian and jpeg tasks (pipeline.load_blur_kernel); ``jpeg_qf``: the
    codec's quality factor, jpeg only (default: the demo's, workload.TASKS["jpeg"]["jpeg_qf"])."""

    def __init__(self, task, size, device, kernel=None, jpeg_qf=None):
        self.hw = pl.check_frame_size(task, size)
        if jpeg_qf is not None and task != "jpeg":
            raise ValueError(f"{task}: jpeg_qf belongs to the jpeg task")
        self.task, self.device = task, torch.device(device)
        self.factor = wl.TASKS[task]["factor"]
        self.jpeg_qf = None
        if task == "jpeg":
            self.jpeg_qf = int(wl.TASKS["jpeg"]["jpeg_qf"] if jpeg_qf is None else jpeg_qf)
            if not 1 <= self.jpeg_qf <= 100:
                raise ValueError(f"jpeg: jpeg_qf={jpeg_qf!r} is not a quality factor in 1..100")
        self.A = pl.build_operator(task, self.hw, self.device, kernel)

    def operator(self, x_n):
        """y_n = A(x_n) for (T, 3, H, W) f32 frames in [-1, 1] on the device."""
        T, C, H, W = x_n.shape
        if (H, W) != self.hw or C != 3:
            raise ValueError(f"{self.task}: frames of {tuple(x_n.shape)}, built for (T, 3, {self.hw[0]}, {self.hw[1]})")
        x_n = x_n.float().contiguous()
        if "bicubic" in self.task:
            f = self.factor
            return self.A.A(x_n.reshape(T, -1)).reshape(T, 3, H // f, W // f)
        y = self.A.DownscaleOP(x_n)
        if self.task == "jpeg":
            from .guided_diffusion.jpeg import jpeg_decode, jpeg_encode
            y = jpeg_decode(jpeg_encode(y, self.jpeg_qf), self.jpeg_qf)
        return y

    def __call__(self, clean01, noise_sigma=0.0, generator=None):
        """clean01: (T, 3, H, W) in [0, 1] -> (y_n, y_u8): the normalised measurement (T, 3, h, w) f32 in [-1, 1] (before
        quantisation) and the frames to write, (T, h, w, 3) uint8, rounded to nearest (half to even) after clamping.
        ``noise_sigma`` > 0 adds white Gaussian noise of that standard deviation on the 0..255 scale, drawn from
        ``generator`` (a generator of the operator's device)."""
        if noise_sigma < 0:
            raise ValueError(f"noise_sigma={noise_sigma!r} must not be negative")
        x_n = clean01.to(self.device).float() * 2 - 1
        y_n = self.operator(x_n)
        if noise_sigma > 0:
            y_n = y_n + (2.0 * noise_sigma / 255.0) * torch.randn(y_n.shape, generator=generator, device=y_n.device,
                                                                  dtype=y_n.dtype)
        y_u8 = (((y_n + 1) / 2).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return y_n, y_u8


def degrade_video_files(task, clean_dir, out_dir, *, device, kernel=None, jpeg_qf=None, noise_sigma=0.0, seed=None, batch=8):
    """Clean frame files of ``clean_dir`` (one size, valid for the task: check_frame_size's own refusal otherwise) ->
    ``out_dir/{i:04d}.png`` degraded frames, decoded, uploaded, degraded and encoded in overlapping stages (the reader
    and writer threads of flair_amd.io).  ``seed`` seeds the noise.  Returns the number of frames written."""
    paths = fio.list_frames(clean_dir)
    if not paths:
        raise ValueError(f"degrade: no frame files in {clean_dir}")
    sizes = [fio.frame_size(p) for p in paths]
    for p, s in zip(paths, sizes):
        if s != sizes[0]:
            raise ValueError(f"degrade: {p} is {s[0]}x{s[1]} and {paths[0]} is {sizes[0][0]}x{sizes[0][1]}; "
                             "the frames of a video must share one size")
    deg = Degrader(task, sizes[0], device, kernel=kernel, jpeg_qf=jpeg_qf)
    gen = None
    if noise_sigma > 0:
        gen = torch.Generator(device=deg.device)
        gen.manual_seed(0 if seed is None else int(seed))
    batch = max(1, int(batch))
    groups = [(i, min(batch, len(paths) - i)) for i in range(0, len(paths), batch)]
    writer = fio._Writer(out_dir, y4m=fio.y4m.output_params(fio.y4m.stream_of(paths)))
    written = 0
    try:
        for first, (u8,) in fio.iter_frame_batches([paths], groups, deg.device):
            clean01 = u8.permute(0, 3, 1, 2).float() / 255.0
            _, y_u8 = deg(clean01, noise_sigma=noise_sigma, generator=gen)
            writer.submit_bytes(first, y_u8)
            written += y_u8.shape[0]
    finally:
        writer.close()
    return written
