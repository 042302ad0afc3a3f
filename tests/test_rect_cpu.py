"""Rectangular frames, host side: size parsing and the frame multiple, every refusal of the pair mode, the command
line's --frame-size, the layout rule of model_config, SRConv's per-axis matrices and the new C entry's presence."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_multiple_and_size_parsing():
    from flair_amd import pipeline as pl
    assert pl.frame_multiple("gaussian") == pl.frame_multiple("jpeg") == 64        # 2^6 levels, factor 4, 16-pixel MCU x 4
    assert pl.frame_multiple("x8_bicubic") == pl.frame_multiple("x16_bicubic") == 16   # 2^4 levels, factors 8 / 16
    assert pl.frame_minimum("gaussian") == 64 and pl.frame_minimum("x8_bicubic") == 128
    assert pl.parse_frame_size("768x1280") == (768, 1280) and pl.parse_frame_size(" 64X128 ") == (64, 128)
    assert pl.parse_frame_size("512,768") == (512, 768) and pl.parse_frame_size("auto") == "auto"
    for bad in ("768", "768x", "0x64", "axb", "64x64x64", "-64x64"):
        with pytest.raises(ValueError, match="HxW"):
            pl.parse_frame_size(bad)
    with pytest.raises(ValueError, match="unknown task"):
        pl.frame_multiple("deblur")
    assert pl.check_frame_size("gaussian", (768, 1280), frames=10) == (768, 1280)
    assert pl.check_frame_size("x16_bicubic", (128, 144)) == (128, 144)


def test_size_that_is_no_multiple_names_the_nearest_valid_sizes():
    from flair_amd import pipeline as pl
    with pytest.raises(ValueError, match=r"700x1300.*multiples of 64.*640x1280 and 704x1344"):
        pl.check_frame_size("gaussian", (700, 1300))
    with pytest.raises(ValueError, match=r"multiples of 16 and at least 128.*128x256 and 128x256"):
        pl.check_frame_size("x8_bicubic", (64, 256))
    with pytest.raises(ValueError, match=r"bisenet.*multiples of 32"):
        pl.check_frame_size("x8_bicubic", (144, 256), parser="bisenet")
    assert pl.check_frame_size("x8_bicubic", (144, 256), parser="parsenet") == (144, 256)
    with pytest.raises(ValueError, match=r"multiples of 64"):                     # refused before any file is looked for
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=(100, 128), prior=False)
    with pytest.raises(ValueError, match="int or a pair"):
        pl.check_frame_size("gaussian", (64, 64, 64))


def test_clip_beyond_the_index_limit_is_refused():
    from flair_amd import pipeline as pl
    from flair_amd import video
    # one frame of the 432 offset / mask channels below the convolution entry's 1 GiB, per dtype
    assert video.max_frame_pixels(torch.bfloat16) == (2 ** 30 - 1) // (432 * 2) == 1242756
    assert video.max_frame_pixels(torch.float32) == (2 ** 30 - 1) // (432 * 4) == 621378
    assert video.max_clip_pixels() == (2 ** 31 - 1) // 16
    video.check_clip_elements(10, 768, 1280)
    video.check_clip_elements(10, 960, 1280)
    with pytest.raises(ValueError, match=r"1024x2048.*bf16.*1242756"):
        video.check_clip_elements(10, 1024, 2048)
    with pytest.raises(ValueError, match=r"768x1280.*f32.*621378"):
        video.check_clip_elements(10, 768, 1280, torch.float32)
    with pytest.raises(ValueError, match=r"200 frames.*shorter windows"):
        video.check_clip_elements(200, 768, 1280)
    with pytest.raises(ValueError, match=r"1024x2048"):
        pl.check_frame_size("gaussian", (1024, 2048), frames=10)
    with pytest.raises(ValueError, match=r"f32"):
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=(768, 1280), dtype="fp32", prior=False)

    # the per-frame limit follows the network's own alignment modules (27 * deform_groups channels)
    from flair_amd.guided_diffusion.unet_new import BasicVSRPP
    assert video.offset_channels(BasicVSRPP(mid_channels=64)) == 432 and video.offset_channels(object()) == 432
    assert video.max_frame_pixels(torch.bfloat16, 27 * 8) == (2 ** 30 - 1) // (216 * 2)
    video.check_clip_elements(10, 1024, 2048, channels=27 * 8)

    class Never:
        dtype = torch.bfloat16

        def __call__(self, *a, **k):
            raise AssertionError("the network ran")
    with pytest.raises(ValueError, match=r"1024x2048"):                           # restore_window refuses on shapes alone
        video.restore_window("gaussian", torch.zeros(1, 2, 3, 256, 512, device="meta"), Never(), None, None, size=(1024, 2048))


def test_degraded_size_mismatch_is_refused_before_any_launch():
    from flair_amd import video
    video.check_degraded("gaussian", (16, 24), (64, 96))
    video.check_degraded("x8_bicubic", (16, 24), (128, 192))
    with pytest.raises(ValueError, match=r"64x96.*16x24.*got 24x16.*size=\(96, 64\)"):
        video.check_degraded("gaussian", (24, 16), (64, 96))
    with pytest.raises(ValueError, match=r"128x192.*8x12 \(factor 16\).*16x24"):
        video.check_degraded("x16_bicubic", (16, 24), (128, 192))
    for fn in (video.restore_window, video.restore_video):                        # meta tensors: nothing can launch
        with pytest.raises(ValueError, match=r"got 32x32"):
            fn("gaussian", torch.zeros(1, 2, 3, 32, 32, device="meta"), None, None, None, size=(64, 128))
    assert video.frame_hw(48) == (48, 48) and video.frame_hw((32, 48)) == (32, 48) and video.frame_hw([32, 48]) == (32, 48)
    assert video.is_pair((64, 64)) and not video.is_pair(64)
    assert not video.is_pair(np.int64(64)) and video.frame_hw(np.int32(48)) == (48, 48)     # any integral type is the int mode


def test_aligned_with_a_prior_needs_whole_512_frames():
    from flair_amd import pipeline as pl
    mk = lambda size, prior: pl.Pipeline("gaussian", None, None, None, None, None, None, size, "cpu", prior=prior)   # noqa: E731
    with pytest.raises(ValueError, match=r"aligned=True.*CodeFormer.*512x512.*768x1280"):
        mk((768, 1280), "codeformer").restore_video_files("in", "out", aligned=True)
    with pytest.raises(ValueError, match=r"VQFR"):
        mk((512, 768), "vqfrv2").check_aligned(True)
    mk((768, 1280), "codeformer").check_aligned(False)                            # un-aligned: any frame size
    mk((768, 1280), None).check_aligned(True)                                     # no prior: nothing needs 512
    mk((512, 512), "codeformer").check_aligned(True)
    mk(512, "codeformer").check_aligned(True)
    # the int mode keeps its own rule and message
    with pytest.raises(ValueError, match=r"size=64 needs prior=False"):
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=64)


def test_model_config_pair_is_the_checkpoint_layout_and_int_is_untouched():
    from flair_amd import pipeline as pl
    for task in pl.TASK_NAMES:
        for size in ((64, 128), (512, 512), (768, 1280)):
            assert pl.model_config(task, size) == pl.MODEL_CONFIG[task]
        assert pl.model_config(task, 512) == pl.MODEL_CONFIG[task]
    g = pl.model_config("gaussian", 64)
    assert g["image_size"] == 64 and g["attention_resolutions"] == (2, 4, 8) and g["rnn_resolutions"] == (1, 2)
    b = pl.model_config("x8_bicubic", 64)
    assert b["image_size"] == 64 and b["attn_res"] == (8, 4) and b["vsrpp_res"] == (64, 32)


def test_frame_size_on_the_command_line(tmp_path):
    from PIL import Image
    from flair_amd import __main__ as cli
    from flair_amd import pipeline as pl
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(2):
        Image.fromarray(np.zeros((192, 320, 3), dtype=np.uint8), mode="RGB").save(frames / f"{i}.png")
    ap = cli.make_parser()
    base = ["restore", "gaussian", str(frames), str(tmp_path / "out")]
    args = ap.parse_args(base)
    assert args.frame_size is None and cli.size_of(args, "gaussian", [(str(frames), "o")]) == 512
    args = ap.parse_args(base + ["--size", "256"])
    assert cli.size_of(args, "gaussian", [(str(frames), "o")]) == 256                     # --size as it was: an int
    args = ap.parse_args(base + ["--frame-size", "768x1280", "--faces", "all"])
    assert cli.size_of(args, "gaussian", [(str(frames), "o")]) == (768, 1280)
    args = ap.parse_args(base + ["--frame-size", "auto"])
    assert cli.size_of(args, "gaussian", [(str(frames), "o")]) == (768, 1280)             # first frame 192 x 320, factor 4
    assert pl.auto_frame_size("x8_bicubic", frames) == (1536, 2560)
    with pytest.raises(SystemExit, match="exclude each other"):
        cli.size_of(ap.parse_args(base + ["--frame-size", "auto", "--size", "256"]), "gaussian", [(str(frames), "o")])
    with pytest.raises(SystemExit, match="multiples of 64"):
        cli.size_of(ap.parse_args(base + ["--frame-size", "700x1280"]), "gaussian", [(str(frames), "o")])
    with pytest.raises(SystemExit, match="HxW"):
        cli.size_of(ap.parse_args(base + ["--frame-size", "big"]), "gaussian", [(str(frames), "o")])
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(SystemExit, match="no frame files"):
        cli.size_of(ap.parse_args(base + ["--frame-size", "auto"]), "gaussian", [(str(empty), "o")])
    demo = ap.parse_args(["jpeg-demo", "--frame-size", "128x192"])                       # the demos take it too
    assert cli.size_of(demo, "jpeg", [("x", "o")]) == (128, 192)


def test_srconv_pair_matrices_are_two_oracle_operators():
    """SRConv((H, W)) holds one 1-D operator per axis: its host-built matrices equal those of two
    oracle.degrade.SeparableSR (f64 SVD here, f32 there: 2e-5), its spectrum their outer product; an int builds
    today's object."""
    from flair_amd.guided_diffusion.restore_util import SRConv
    from oracle import degrade as odeg
    f, H, W = 8, 32, 64
    taps = torch.from_numpy(odeg.bicubic_taps(f)).float()
    k = taps / taps.sum()
    sr = SRConv(k, 3, (H, W), "cpu", stride=f)
    oh, ow = odeg.SeparableSR(k, 3, H, f), odeg.SeparableSR(k, 3, W, f)
    fwd = lambda o: o.U @ torch.diag(o.sv) @ o.V[:, :o.s].t()                                        # noqa: E731
    pinv = lambda o: o.V[:, :o.s] @ torch.diag(torch.where(o.sv > 0, 1.0 / o.sv, torch.zeros_like(o.sv))) @ o.U.t()  # noqa: E731
    assert sr._fwd.shape == (H // f, H) and sr._fwd_t.shape == (W, W // f)
    assert sr._pinv.shape == (H, H // f) and sr._pinv_t.shape == (W // f, W)
    for got, ref in ((sr._fwd, fwd(oh)), (sr._fwd_t, fwd(ow).t()), (sr._pinv, pinv(oh)), (sr._pinv_t, pinv(ow).t())):
        assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    assert (sr.singulars() - torch.outer(oh.sv, ow.sv).reshape(-1).repeat_interleave(3)).abs().max().item() <= 1e-6
    assert sr.img_dim == (H, W) and sr.y_dim == (H // f, W // f)
    sq, sq2 = SRConv(k, 3, 64, "cpu", stride=f), SRConv(k, 3, (64, 64), "cpu", stride=f)
    assert sq.img_dim == 64 and sq.y_dim == 8 and torch.equal(sq._fwd_t, sq._fwd.t()) and torch.equal(sq._fwd, sq2._fwd)
    assert torch.equal(sq.singulars(), sq2.singulars())
    with pytest.raises(ValueError, match="multiple of the stride"):
        SRConv(k, 3, (36, 64), "cpu", stride=f)


def test_abi_14_and_the_new_entry_everywhere():
    from flair_amd import _lib
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 14
    assert hasattr(lib, "flair_jpeg_roundtrip_hw") and hasattr(lib, "flair_jpeg_roundtrip")
    header = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    assert re.search(r"int flair_jpeg_roundtrip_hw\(const float\* x, int N, int H, int W,", header)
    assert "int flair_jpeg_roundtrip(const float* x, int N, int S," in header
    ops_src = open(os.path.join(ROOT, "flair_amd", "ops.py")).read()
    assert "flair_jpeg_roundtrip_hw(" in ops_src and "flair_jpeg_roundtrip(" in ops_src


def test_jpeg_wrapper_refuses_partial_mcus():
    from flair_amd import ops
    with pytest.raises(ValueError, match="16x16 MCUs"):
        ops.jpeg_roundtrip(torch.zeros(1, 3, 24, 32), [1.0] * 64, [1.0] * 64, [0.0] * 64)
    with pytest.raises(ValueError, match="square entry"):
        ops.jpeg_roundtrip(torch.zeros(1, 3, 16, 32), [1.0] * 64, [1.0] * 64, [0.0] * 64, entry="square")
