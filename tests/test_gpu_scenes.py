"""GPU: scene cuts.  flair_block_luma_sums (csrc/scenes.hip) against the int64 numpy values of tests/scenes_ref.py, exactly;
detection on written frames; restoration per shot (toy network of tests/test_video_windows.py); interpolation that does not
cross a cut (SuperSloMo with name-seeded weights, as tests/test_gpu_superslomo.py builds it).

Every launch of the kernel runs on frames and an output that sit inside larger allocations whose guard values must come back
unchanged.  The frames start 0 .. 3 bytes past a dword; rows (3 W bytes) and frames (H W 3 bytes) of these shapes are no
multiples of 4 either, so heads and tails of every length occur."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import scenes_ref as R
from tests import util

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (2, 13, 29), (3, 45, 70), (2, 85, 143), (1, 96, 1283)]
CONTENTS = ["random", "white", "black", "red", "green", "blue", "mixed"]
SENTINEL = -0x0123456789ABCDEF


def content(name, n, H, W):
    """Frame n of a content as (H, W, 3) uint8."""
    if name == "mixed":                                  # another content per frame: a mix-up between frames shows
        return content(CONTENTS[(n + 3) % 6], n + 1, H, W)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    if name == "random":
        out = np.random.default_rng(100 * n + H + 7 * W).integers(0, 256, (H, W, 3)).astype(np.uint8)
    elif name == "white":
        out[:] = 255
    elif name in ("red", "green", "blue"):
        out[..., ("red", "green", "blue").index(name)] = 255
    return out


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """The frames of one (content, shape) and their int64 block sums, computed once and shared (read-only)."""
    N, H, W = shape
    frames = np.stack([content(name, n, H, W) for n in range(N)])
    ref = R.block_sums(frames)
    frames.setflags(write=False)
    ref.setflags(write=False)
    return frames, ref


def run_guarded(frames, dev, shift=0):
    """One call of the entry through ctypes on guarded buffers, the frames ``shift`` bytes past a 16-byte boundary
    -> the (N, 64) int64 rows on the host."""
    from flair_amd import _lib
    N, H, W, _ = frames.shape
    fbuf, fv, f0 = util.flat_guarded(frames.shape, torch.uint8, dev, 0x5A, src=torch.tensor(frames), pad=64 + shift)
    assert fv.data_ptr() % 4 == shift % 4 and fv.is_contiguous()
    obuf, ov, o0 = util.flat_guarded((N, 64), torch.int64, dev, SENTINEL)
    rc = _lib.lib().flair_block_luma_sums(_lib.ptr(fv), N, H, W, _lib.ptr(ov), _lib.stream())
    _lib.check(rc, "flair_block_luma_sums")
    torch.cuda.synchronize()
    util.assert_flat_untouched(fbuf, f0, what="frames")
    util.assert_flat_untouched(obuf, o0, view=ov, what="out")
    return ov.cpu().numpy().copy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", CONTENTS)
def test_block_sums_are_exact(dev, name, shape):
    frames, ref = case(name, shape)
    N, H, W = shape
    for shift in range(4):
        got = run_guarded(frames, dev, shift)
        assert got.dtype == np.int64 and np.array_equal(got, ref), (name, shape, shift, np.argwhere(got != ref)[:4])
    cnt = R.block_counts(H, W)
    per_pixel = dict(white=255, black=0, red=77, green=149, blue=29)
    if name in per_pixel:                                 # pins the weights and the block edges without the restatement
        assert np.array_equal(ref, np.broadcast_to(per_pixel[name] * cnt, (N, 64)))


@pytest.mark.parametrize("shape", [(3, 45, 70), (2, 85, 143)], ids=["3x45x70", "2x85x143"])
def test_rows_do_not_depend_on_the_batch(dev, shape):
    """ops.block_luma_sums: a frame's row is the same alone, at another position and in a longer batch; two runs are equal."""
    from flair_amd import ops
    frames, ref = case("random", shape)
    x = torch.tensor(frames).to(dev)
    first = ops.block_luma_sums(x).clone()
    again = ops.block_luma_sums(x)
    assert first.dtype == torch.int64 and tuple(first.shape) == (shape[0], 64)
    assert torch.equal(first, again) and np.array_equal(first.cpu().numpy(), ref)
    for n in range(shape[0]):
        assert torch.equal(ops.block_luma_sums(x[n:n + 1].contiguous())[0], first[n])
    rev = ops.block_luma_sums(x.flip(0).contiguous())
    assert torch.equal(rev.flip(0), first)
    twice = ops.block_luma_sums(torch.cat([x, x, x[:1]]))
    assert torch.equal(twice, torch.cat([first, first, first[:1]]))
    out = torch.full((shape[0], 64), 7, dtype=torch.int64, device=dev)           # a used output: the entry zeroes it itself
    assert ops.block_luma_sums(x, out=out) is out and torch.equal(out, first)


def test_refusals_launch_nothing(dev):
    from flair_amd import _lib, ops
    lib = _lib.lib()
    frames = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    obuf, ov, o0 = util.flat_guarded((2, 64), torch.int64, dev, SENTINEL)
    for f, N, H, W, o, what in ((None, 2, 16, 16, ov, "null pointer"), (frames, 2, 16, 16, None, "null pointer"),
                                (frames, 0, 16, 16, ov, "N = 0"), (frames, -1, 16, 16, ov, "N = -1"),
                                (frames, 2, 7, 16, ov, "7x16"), (frames, 2, 16, 7, ov, "16x7")):
        rc = lib.flair_block_luma_sums(_lib.ptr(f), N, H, W, _lib.ptr(o), _lib.stream())
        msg = lib.flair_last_error().decode()
        assert rc == -1 and "flair_block_luma_sums" in msg and what in msg, (rc, msg)
    odd = ctypes.c_void_p(ov.data_ptr() + 4)
    assert lib.flair_block_luma_sums(_lib.ptr(frames), 2, 16, 16, odd, _lib.stream()) == -1
    assert "8-byte aligned" in lib.flair_last_error().decode()
    with pytest.raises(_lib.FlairHipError, match="flair_block_luma_sums.*smaller than the 8x8 grid"):
        ops.block_luma_sums(torch.zeros(1, 7, 16, 3, dtype=torch.uint8, device=dev), out=ov[:1])
    with pytest.raises(_lib.FlairHipError, match="no CPU path"):
        ops.block_luma_sums(frames.cpu(), out=ov)
    with pytest.raises(ValueError, match="uint8"):
        ops.block_luma_sums(frames.float(), out=ov)
    with pytest.raises(ValueError, match="contiguous"):
        ops.block_luma_sums(frames.permute(0, 2, 1, 3)[:, ::2], out=ov)
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\)"):
        ops.block_luma_sums(torch.zeros(2, 16, 16, 4, dtype=torch.uint8, device=dev), out=ov)
    with pytest.raises(ValueError, match="out is a dense"):
        ops.block_luma_sums(frames, out=ov.to(torch.int32))
    torch.cuda.synchronize()
    util.assert_flat_untouched(obuf, o0, what="out")                             # nothing ran: not even the zeroing


# ------------------------------------------------------------------------------------------------------ detection on files
def test_detect_cuts_files_on_the_fixture(dev, tmp_path):
    from flair_amd import __main__ as cli
    from flair_amd import io as fio
    from flair_amd import scenes
    H, W = 45, 70
    seq = R.cut_sequence(H, W)
    for i, frame in enumerate(seq):
        fio.write_frame(str(tmp_path / f"f_{i}.png"), frame)                     # natural order: f_2 before f_10
    paths = fio.list_frames(tmp_path)
    want = R.pair_distances(R.block_sums(seq), H, W)
    for batch in (8, 5):
        got = scenes.detect_cuts_files(paths, dev, batch=batch)
        assert got["cuts"] == [7, 13] and got["shots"] == [(0, 7), (7, 13), (13, 19)] and got["frames"] == 19
        assert got["distances"] == want                                          # the same float64 operations on the same integers
    assert scenes.detect_cuts_files(paths, dev, min_shot=1)["cuts"] == [7, 13, 14]
    assert scenes.detect_cuts_files(paths[:1], dev) == dict(cuts=[], distances=[], shots=[(0, 1)], frames=1)
    js = tmp_path / "cuts.json"
    with torch.enable_grad():                                                    # main() turns autograd off for the process
        assert cli.main(["scenes", str(tmp_path), "--json", str(js), "--device", str(dev)]) == 0
    assert scenes.read_cuts(str(js), 19) == [7, 13]


# ------------------------------------------------------------------------------------------------------ restoration per shot
def test_restoration_per_shot(dev, tmp_path):
    """9 frames with a cut at 4: restore_video(cuts=[4]) is the concatenation of restore_video on frames 0..3 and on 4..8 (the
    second with its noise functions shifted by the windows of the first shot), differs from the run without cuts from frame 4
    on, and the file driver gives the same bytes."""
    from PIL import Image
    from flair_amd import io as fio
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    from tests.test_video_windows import _toy_model, _write_pngs
    N, s, S, L, OV, steps, cuts = 9, 8, 32, 4, 1, 4, [4]
    _write_pngs(tmp_path, N, s)
    paths = fio.list_frames(tmp_path)
    degraded = fio.read_frames(paths).to(dev)
    plan = video.window_plan(N, cuts, L, OV)
    assert [idx for idx, _ in plan] == [[0, 1, 2, 3], [4, 5, 6, 7], [7, 8]] and [st for _, st in plan] == [True, True, False]
    g = torch.Generator().manual_seed(9)
    tapes = [[torch.randn(L, 3, S, S, generator=g).to(dev) for _ in range(steps)] for _ in range(3)]
    qnoise = [torch.randn(L, 3, S, S, generator=g).to(dev) for _ in range(3)]
    seen = []

    def noise_fn(wi, it, like, shift=0):
        return tapes[wi + shift][it][:like.shape[0]].contiguous()

    def q_noise_fn(wi, like, shift=0):
        seen.append((wi + shift, like.shape[0]))
        return qnoise[wi + shift][:like.shape[0]].contiguous()
    diffusion = wl.diffusion_for(steps)
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(),
                     kernel_indx=10).WrapArchitecture_PyTorch().to(dev)

    class M:
        def parameters(self):
            return iter([degraded])

        def __call__(self, x, t, **kw):
            return _toy_model(x, t, **kw)
    rf = lambda d_n: (lambda x0: A.A_pinv(d_n[0].contiguous(), x0))      # noqa: E731
    common = dict(size=S, tau=1, length=L, overlap=OV)
    run = lambda frames, shift=0, **kw: video.restore_video(              # noqa: E731
        "gaussian", frames, M(), diffusion, rf, noise_fn=functools.partial(noise_fn, shift=shift),
        q_noise_fn=functools.partial(q_noise_fn, shift=shift), **common, **kw)
    got = run(degraded, cuts=cuts)
    assert seen == [(0, 4), (1, 4), (2, 2)]                               # window_index counts over the whole video
    first = run(degraded[:, :4].contiguous())
    second = run(degraded[:, 4:].contiguous(), shift=1)
    assert got.shape == (N, 3, S, S) and torch.equal(got, torch.cat([first, second]))
    plain = run(degraded)
    assert torch.equal(run(degraded, cuts=[]), plain)
    assert torch.equal(plain[:4], got[:4])                                # the first window is the same window
    assert all(not torch.equal(plain[i], got[i]) for i in range(4, N))
    n = fio.restore_video_files("gaussian", tmp_path, tmp_path / "out", M(), diffusion, rf, device=dev, cuts=cuts,
                                noise_fn=noise_fn, q_noise_fn=q_noise_fn, **common)
    assert n == N
    want = fio.to_bytes(got).cpu().numpy()
    for i in range(N):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{i:04d}.png")), want[i]), i


# ------------------------------------------------------------------------------------------------------ interpolation
@pytest.mark.parametrize("factor", [2, 3])
def test_interpolation_does_not_cross_a_cut(dev, tmp_path, factor):
    """Six 32 x 32 frames, two shots of three: the files between frames 2 and 3 are byte-identical to the source frame the 0.5
    rule names, every other file is identical to a run without cuts."""
    from flair_amd import interpolate as fi
    from flair_amd import io as fio
    from tests.test_gpu_superslomo import _net
    T, cuts = 6, [3]
    seq = np.concatenate([R.shot(1, 32, 32, 3), R.shot(2, 32, 32, 3)])
    src = tmp_path / "src"
    src.mkdir()
    for i, frame in enumerate(seq):
        fio.write_frame(str(src / f"{i:03d}.png"), frame)
    net = _net(dev)
    assert fi.interpolate_video_files(str(src), str(tmp_path / "plain"), factor, net=net, device=dev) == factor * (T - 1) + 1
    assert fi.interpolate_video_files(str(src), str(tmp_path / "cut"), factor, net=net, device=dev, cuts=cuts) == factor * (T - 1) + 1
    names = [f"{i:04d}.png" for i in range(factor * (T - 1) + 1)]
    assert sorted(os.listdir(tmp_path / "cut")) == names
    plain = [fio.decode_frame_hwc(str(tmp_path / "plain" / n)) for n in names]
    got = [fio.decode_frame_hwc(str(tmp_path / "cut" / n)) for n in names]
    crossed = 0
    for i, (kind, p, *k) in enumerate(fi.interleave_index(T, factor)):
        if kind == "mid" and p + 1 in cuts:
            src_frame = p if (k[0] + 1) / factor < 0.5 else p + 1
            assert np.array_equal(got[i], seq[src_frame]), (i, p, k)
            assert not np.array_equal(plain[i], got[i])                   # the network did synthesise something there
            crossed += 1
        else:
            assert np.array_equal(got[i], plain[i]), (i, kind, p)
    assert crossed == factor - 1
    frames01 = torch.tensor(seq).to(dev).permute(0, 3, 1, 2).float() / 255.0
    mem = fio.to_bytes(fi.interpolate_frames(net, frames01, factor, cuts=cuts)).cpu().numpy()
    assert np.array_equal(mem, np.stack(got))
