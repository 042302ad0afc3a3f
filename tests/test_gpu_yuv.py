"""GPU: flair_yuv_to_rgb_u8 and flair_rgb_to_yuv_u8 bit for bit against the integer definition (tests/yuv_ref.py) in every
format, matrix, range and layout on guarded buffers at odd addresses; their refusals; and the seam in flair_amd.io: .y4m
streams through the readers, the writer, evaluate, scenes and restore_video_files."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import yuv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
COMBOS = [(m, r) for m in R.MATRICES for r in R.RANGES]


def guarded(dev, nbytes, pad):
    """A sentinel-filled device buffer and the view of ``nbytes`` bytes that starts ``pad`` bytes into it."""
    buf = torch.full((pad + nbytes + 29,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[pad:pad + nbytes]


def untouched(buf, nbytes, pad):
    host = buf.cpu().numpy()
    return (host[:pad] == SENTINEL).all() and (host[pad + nbytes:] == SENTINEL).all()


def at_odd_offset(dev, array):
    """The bytes of ``array`` on the device, starting one byte into a larger buffer."""
    flat = np.ascontiguousarray(array).reshape(-1)
    buf = torch.zeros(flat.size + 8, dtype=torch.uint8, device=dev)
    buf[1:1 + flat.size] = torch.from_numpy(flat.copy()).to(dev)
    assert buf.data_ptr() % 2 == 0
    return buf[1:1 + flat.size].view(array.shape)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_decode_is_the_definition_bit_for_bit(dev, fmt):
    from flair_amd import ops
    ran = 0
    for N, H, W in R.all_cases():
        host = R.payload_case(fmt, N, H, W)
        payload = at_odd_offset(dev, host)
        for matrix, range_ in COMBOS:
            for planar in (False, True):
                shape = (N, 3, H, W) if planar else (N, H, W, 3)
                pad = 13 if N == 1 else 16                       # unaligned and aligned outputs
                buf, view = guarded(dev, N * H * W * 3, pad)
                out = ops.yuv_to_rgb_u8(payload, (H, W), fmt, matrix, range_, planar=planar, out=view.view(shape))
                want = R.decode(host, H, W, fmt, matrix, range_, planar=planar)
                assert np.array_equal(out.cpu().numpy(), want), (fmt, N, H, W, matrix, range_, planar)
                assert untouched(buf, N * H * W * 3, pad), (fmt, N, H, W, matrix, range_, planar)
                ran += 1
    assert ran == len(R.SHAPES) * len(R.COUNTS) * 4 * 2


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_encode_is_the_definition_bit_for_bit(dev, fmt):
    from flair_amd import ops
    for N, H, W in R.all_cases():
        host = R.rgb_case(N, H, W)
        for shift, rgb in ((0, torch.from_numpy(host.copy()).to(dev)), (1, at_odd_offset(dev, host))):
            if shift and N == 3:
                continue                                        # the odd input address once per shape
            P = R.payload_bytes(fmt, H, W)
            for matrix, range_ in COMBOS:
                pad = 13 if N == 1 else 16
                buf, view = guarded(dev, N * P, pad)
                out = ops.rgb_to_yuv_u8(rgb, fmt, matrix, range_, out=view.view(N, P))
                want = R.encode(host, fmt, matrix, range_)
                assert np.array_equal(out.cpu().numpy(), want), (fmt, N, H, W, matrix, range_, shift)
                assert untouched(buf, N * P, pad), (fmt, N, H, W, matrix, range_, shift)


def test_the_wrappers_allocate_what_they_return(dev):
    from flair_amd import ops
    host = R.payload_case("420jpeg", 3, 6, 8)
    out = ops.yuv_to_rgb_u8(torch.from_numpy(host.copy()).to(dev), (6, 8), "420jpeg", "bt709", "full")
    assert out.shape == (3, 6, 8, 3) and np.array_equal(out.cpu().numpy(), R.decode(host, 6, 8, "420jpeg", "bt709", "full"))
    back = ops.rgb_to_yuv_u8(out, "422", "bt601", "limited")
    assert back.shape == (3, 6 * 8 * 2) and np.array_equal(back.cpu().numpy(), R.encode(out.cpu().numpy(), "422", "bt601", "limited"))
    with pytest.raises(ValueError, match=r"yuv_to_rgb_u8: payload is a dense \(N, 72\) uint8 tensor for 420jpeg frames of 6x8"):
        ops.yuv_to_rgb_u8(torch.zeros(1, 71, dtype=torch.uint8, device=dev), (6, 8), "420jpeg", "bt601", "limited")
    with pytest.raises(ValueError, match="format '411'"):
        ops.yuv_to_rgb_u8(torch.zeros(1, 72, dtype=torch.uint8, device=dev), (6, 8), "411", "bt601", "limited")
    with pytest.raises(ValueError, match="matrix 'bt2020'"):
        ops.rgb_to_yuv_u8(out, "444", "bt2020", "limited")


def test_every_refusal_leaves_the_buffers_alone(dev):
    """Status -1 and the entry's message for every refusal of the header, nothing enqueued: the guarded outputs keep their
    sentinel.  N = 0 is a no-op that looks at no pointer."""
    from flair_amd import _lib
    lib = _lib.lib()
    H, W = 6, 8
    P = R.payload_bytes("420jpeg", H, W)
    pbuf, payload = guarded(dev, 2 * P, 16)
    obuf, rgb = guarded(dev, 2 * H * W * 3, 16)
    torch.cuda.synchronize()
    pp, op = payload.data_ptr(), rgb.data_ptr()
    for case in R.entry_refusals(pp, op, H, W):
        R.assert_refused(lib, *case)
    for name, args in R.entry_noops(pp, op, H, W):
        assert getattr(lib, name)(*args, None) == 0, (name, args)
    torch.cuda.synchronize()
    assert (pbuf.cpu().numpy() == SENTINEL).all() and (obuf.cpu().numpy() == SENTINEL).all()
    with pytest.raises(_lib.FlairHipError, match=r"flair_yuv_to_rgb_u8 failed \(status -1\): flair_yuv_to_rgb_u8: out overlaps payload"):
        _lib.call.flair_yuv_to_rgb_u8(payload, 1, H, W, 0, 0, 0, 0, payload)


# ------------------------------------------------------------------------------------------- the seam
def _stream_file(tmp_path, name, n, H, W, fmt="420jpeg", seed=0, **kw):
    payloads = R.random_bytes(n * R.payload_bytes(fmt, H, W), 900 + seed).reshape(n, -1)
    return R.write_y4m(tmp_path / name, payloads, W, H, fmt, **kw), payloads


def test_the_readers_yield_the_reference_rgb(dev, tmp_path):
    from flair_amd import io as fio
    from flair_amd.video import window_indices
    path, payloads = _stream_file(tmp_path, "clip.y4m", 9, 6, 10)
    want = R.decode(payloads, 6, 10, "420jpeg", "bt601", "limited")
    refs = fio.list_frames(path)
    assert len(refs) == 9 and fio.frame_size(refs[4]) == (6, 10)
    groups = [(0, 4), (4, 4), (8, 1)]
    got = list(fio.iter_frame_batches([refs], groups, dev))
    assert [f for f, _ in got] == [0, 4, 8]
    for (first, n), (_, (u8,)) in zip(groups, got):
        assert u8.dtype == torch.uint8 and u8.shape == (n, 6, 10, 3) and u8.device == dev
        assert np.array_equal(u8.cpu().numpy(), want[first:first + n])
    wins = list(fio.iter_windows(refs, dev, length=4, overlap=1))
    assert [idx for idx, _ in wins] == window_indices(9, 4, 1)
    for idx, x in wins:
        assert x.dtype == torch.float32 and x.shape == (1, len(idx), 3, 6, 10)
        planar = torch.from_numpy(want[idx[0]:idx[-1] + 1]).permute(0, 3, 1, 2).contiguous()
        assert x.device == dev and torch.equal((x[0] * 255.0).round().to(torch.uint8).cpu(), planar)       # the reference's bytes
        assert torch.equal(x[0], planar.to(dev).float() / 255.0)        # ... scaled as for a directory: the device's own division
    assert np.array_equal(fio.decode_frame_hwc(refs[8]), want[8])
    assert torch.equal(fio.read_frames(refs[:2])[0], torch.from_numpy(want[:2]).permute(0, 3, 1, 2).float() / 255.0)


def test_a_stream_and_a_directory_side_by_side(dev, tmp_path):
    """Lists are handled one by one: one list a stream, the other frame files."""
    from flair_amd import io as fio
    path, payloads = _stream_file(tmp_path, "a.y4m", 3, 5, 7, fmt="422", tags="Ip XCOLORRANGE=FULL")
    want = R.decode(payloads, 5, 7, "422", "bt601", "full")
    os.makedirs(tmp_path / "png")
    for i, f in enumerate(want[::-1]):
        fio.write_frame(str(tmp_path / "png" / f"{i}.png"), f)
    (first, (a, b)), = list(fio.iter_frame_batches([fio.list_frames(path), fio.list_frames(tmp_path / "png")], [(0, 3)], dev))
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want[::-1])


def test_the_writer_writes_the_reference_payloads(dev, tmp_path):
    from flair_amd import io as fio
    from flair_amd import y4m
    rgb = R.rgb_case(3, 17, 130)
    params = dict(y4m.output_params(), fps=(30000, 1001), format="422", range="full", aspect="1:1")
    w = fio._Writer(tmp_path / "sub" / "out.Y4M", y4m=params)
    w.submit_bytes(0, torch.from_numpy(rgb[:2].copy()).to(dev))
    w.submit_bytes(2, torch.from_numpy(rgb[2:].copy()))             # a host tensor is uploaded first
    w.close()
    line, P, frames = R.read_y4m(tmp_path / "sub" / "out.Y4M")
    assert line == "YUV4MPEG2 W130 H17 F30000:1001 Ip A1:1 C422 XCOLORRANGE=FULL"
    want = R.encode(rgb, "422", "bt601", "full")
    assert P == want.shape[1] and len(frames) == 3
    assert all(frames[i] == want[i].tobytes() for i in range(3))
    back = y4m.Y4MStream(tmp_path / "sub" / "out.Y4M")
    assert (back.frame_count, back.fps, back.format, back.range, back.aspect) == (3, (30000, 1001), "422", "full", "1:1")
    # the defaults: 420jpeg at 25:1, limited, and submit() through to_bytes
    w = fio._Writer(tmp_path / "plain.y4m")
    x = torch.from_numpy(rgb[:1].copy()).to(dev).permute(0, 3, 1, 2).float() / 255.0
    w.submit(0, x)
    w.close()
    line, _, frames = R.read_y4m(tmp_path / "plain.y4m")
    assert line == "YUV4MPEG2 W130 H17 F25:1 Ip C420jpeg XCOLORRANGE=LIMITED"
    assert frames[0] == R.encode(fio.to_bytes(x).cpu().numpy(), "420jpeg", "bt601", "limited")[0].tobytes()
    w = fio._Writer(tmp_path / "bad.y4m")
    w.submit_bytes(0, torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="frames of 4x6 in a stream of 4x4"):
        w.submit_bytes(1, torch.zeros(1, 4, 6, 3, dtype=torch.uint8, device=dev))
    w.close()


def _png_dir(tmp_path, name, frames):
    from flair_amd import io as fio
    os.makedirs(tmp_path / name)
    for i, f in enumerate(frames):
        fio.write_frame(str(tmp_path / name / f"{i:04d}.png"), f)
    return str(tmp_path / name)


def _without_names(result):
    return dict(result, frames=[{k: v for k, v in f.items() if k != "name"} for f in result["frames"]])


def test_evaluate_agrees_with_the_png_path(dev, tmp_path):
    """The smallest frames evaluate accepts (SSIM's window: 11 a side)."""
    from flair_amd import metrics as fm
    a, pa = _stream_file(tmp_path, "restored.y4m", 3, 11, 13, seed=1)
    b, pb = _stream_file(tmp_path, "truth.y4m", 3, 11, 13, fmt="444", seed=2)
    da = _png_dir(tmp_path, "restored", R.decode(pa, 11, 13, "420jpeg", "bt601", "limited"))
    db = _png_dir(tmp_path, "truth", R.decode(pb, 11, 13, "444", "bt601", "limited"))
    want = fm.evaluate_dirs(da, db, dev, batch=2)
    assert want["count"] == 3 and all(np.isfinite(f["psnr"]) for f in want["frames"])
    for x, y in ((a, b), (a, db), (da, b)):
        got = fm.evaluate_dirs(x, y, dev, batch=2)
        assert _without_names(got) == _without_names(want)
    assert [f["name"] for f in fm.evaluate_dirs(a, db, dev)["frames"]] == ["restored.y4m#0000", "restored.y4m#0001", "restored.y4m#0002"]


def test_scenes_agree_with_the_png_path(dev, tmp_path):
    """One hard cut, at the smallest size the block grid accepts (8 a side)."""
    from flair_amd import io as fio
    from flair_amd import scenes
    rng = np.random.default_rng(11)
    rgb = np.concatenate([rng.integers(40, 60, size=(6, 8, 9, 3)), rng.integers(180, 200, size=(6, 8, 9, 3))]).astype(np.uint8)
    payloads = R.encode(rgb, "420jpeg", "bt601", "limited")
    path = R.write_y4m(tmp_path / "cut.y4m", payloads, 9, 8)
    d = _png_dir(tmp_path, "cut", R.decode(payloads, 8, 9, "420jpeg", "bt601", "limited"))
    want = scenes.detect_cuts_files(fio.list_frames(d), dev, batch=5)
    got = scenes.detect_cuts_files(fio.list_frames(path), dev, batch=5)
    assert want["cuts"] == [6] and got == want


def test_restore_video_files_from_stream_to_stream(dev, tmp_path):
    """Y4M in and Y4M out == the in-memory loop on the reference-decoded frames, encoded by the reference (toy network,
    4-step chain, as tests/test_video_windows.py)."""
    from flair_amd import io as fio
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    from tests.test_video_windows import _toy_model
    N, s, S, L, OV, steps = 7, 8, 32, 4, 1, 4
    path, payloads = _stream_file(tmp_path, "lr.y4m", N, s, s, fps=(24, 1), seed=3)
    frames = R.decode(payloads, s, s, "420jpeg", "bt601", "limited")
    # scaled on the device like iter_windows' frames (its division by 255 need not round as the host's does)
    degraded = (torch.from_numpy(frames).permute(0, 3, 1, 2).contiguous().to(dev).float() / 255.0).unsqueeze(0)
    g = torch.Generator().manual_seed(3)
    wins = video.window_indices(N, L, OV)
    tapes = [[torch.randn(len(w), 3, S, S, generator=g).to(dev) for _ in range(steps)] for w in wins]
    qnoise = [torch.randn(len(w), 3, S, S, generator=g).to(dev) for w in wins]
    diffusion = wl.diffusion_for(steps)
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(),
                     kernel_indx=10).WrapArchitecture_PyTorch().to(dev)

    class M:
        def parameters(self):
            return iter([degraded])

        def __call__(self, x, t, **kw):
            return _toy_model(x, t, **kw)
    common = dict(size=S, tau=1, length=L, overlap=OV, noise_fn=lambda wi, it, like: tapes[wi][it],
                  q_noise_fn=lambda wi, like: qnoise[wi])
    rf = lambda d_n: (lambda x0: A.A_pinv(d_n[0].contiguous(), x0))      # noqa: E731
    ref = video.restore_video("gaussian", degraded, M(), diffusion, rf, **common)
    n = fio.restore_video_files("gaussian", path, tmp_path / "out.y4m", M(), diffusion, rf, device=dev, **common)
    assert n == N
    want = R.encode(fio.to_bytes(ref).cpu().numpy(), "420jpeg", "bt601", "limited")
    line, P, got = R.read_y4m(tmp_path / "out.y4m")
    assert line == f"YUV4MPEG2 W{S} H{S} F24:1 Ip C420jpeg XCOLORRANGE=LIMITED"
    assert len(got) == N and all(got[i] == want[i].tobytes() for i in range(N))
