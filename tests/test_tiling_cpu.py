"""Tiled denoising without a GPU: the planner's properties, the weights' definition (tests/tile_ref.py) and its mutants against the
bound tests/test_gpu_tile.py asserts, the eighth header's binding and refusals, the tiled frame's refusals and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("t,p,g", [(64, 16, 4), (64, 8, 8), (32, 8, 4), (48, 16, 16)])
def test_plan_axis_properties_over_a_sweep_of_lengths(t, p, g):
    """L = 64 .. 300 step 4 (lengths the grid divides): every pixel covered, the last origin L - t, origins multiples of g in
    ascending order, consecutive overlaps at least the minimum; and the planner equals the reference's restatement."""
    from flair_amd import tiling
    for L in range(64, 301, 4):
        if L % g:
            with pytest.raises(ValueError, match="multiples of"):
                tiling.plan_axis(L, t, p, g)
            continue
        o = tiling.plan_axis(L, t, p, g)
        assert o == R.plan_axis(L, t, p, g), (L, o)
        assert o[0] == 0 and o[-1] == L - t and all(v % g == 0 for v in o) and o == sorted(set(o)), (L, o)
        cover = np.zeros(L, dtype=int)
        for v in o:
            cover[v:v + t] += 1
        assert cover.min() >= 1, (L, o)
        assert all(a + t - b >= p for a, b in zip(o, o[1:])), (L, o)
        if L == t:
            assert o == [0]
        else:
            assert len(o) == max(2, -(-(L - p) // (t - p)))


def test_plan_axis_triple_cover_and_refusals():
    from flair_amd import tiling
    o = tiling.plan_axis(116, 64, 16, 4)
    assert o == [0, 24, 52]
    cover = np.zeros(116, dtype=int)
    for v in o:
        cover[v:v + 64] += 1
    assert cover.max() == 3 and set(np.nonzero(cover == 3)[0]) == set(range(52, 64))
    assert tiling.plan_axis(60, 32, 8, 4) == [0, 12, 28] and tiling.plan_axis(44, 32, 8, 4) == [0, 12]       # the GPU tests' plan
    assert tiling.plan_axis(1080, 512, 64, 4) == [0, 284, 568] and len(tiling.plan_axis(1920, 512, 64, 4)) == 5
    for bad, msg in (((32, 64, 8, 4), "1 <= t <= L"), ((64, 32, 32, 4), "below the tile side"), ((64, 32, 6, 4), "multiple of 4"),
                     ((64, 30, 8, 4), "multiples of 4")):
        with pytest.raises(ValueError, match=msg):
            tiling.plan_axis(*bad)
    plan = tiling.make_plan((44, 60), (32, 32), 8, 4)
    assert (plan.rows, plan.cols, plan.n_tiles) == (2, 3, 6) and plan.origins()[4] == (12, 12)
    assert tiling.tile_side(1080, 512, 64) == 512 and tiling.tile_side(300, 512, 64) == 256 and tiling.tile_side(40, 512, 64) == 0
    with pytest.raises(ValueError, match="at least 1 pixel"):
        tiling.make_plan((44, 60), (32, 32), 0, 4)


# ------------------------------------------------------------------------------------------------ the weights
PLANS = [(44, 60, 32, 32, 8, 4), (116, 116, 64, 64, 16, 4), (40, 116, 32, 64, 16, 4), (32, 48, 32, 48, 8, 4), (48, 48, 32, 32, 8, 8)]


@pytest.mark.parametrize("H,W,th,tw,p,g", PLANS)
def test_normalised_weights_sum_to_one_and_are_positive(H, W, th, tw, p, g):
    oy, ox = R.plan_axis(H, th, p, g), R.plan_axis(W, tw, p, g)
    w, cover = R.weights(H, W, th, tw, oy, ox, p)
    wn, _ = R.normalised(H, W, th, tw, oy, ox, p)
    assert w.sum(0).min() >= 1.0 - 1e-12                                  # the denominator never drops below one
    assert np.abs(wn.sum(0) - 1.0).max() <= 1e-15
    k = 0
    for a in oy:
        for b in ox:
            inside = np.zeros((H, W), dtype=bool)
            inside[a:a + th, b:b + tw] = True
            assert (wn[k][inside] > 0).all() and (wn[k][~inside] == 0).all()
            k += 1
    assert (wn.max(0)[cover == 1] == 1.0).all()                           # a pixel under one tile takes that tile's value


def test_the_gpu_blend_cases_cover_the_triple_cover_plans():
    """The plans tests/test_gpu_tile.py blends: three tiles on a pixel along W (times two along H) in the first, three along
    both axes in the second."""
    from tests.test_gpu_tile import BLENDS
    cover = {}
    for H, W, th, tw, p, g in BLENDS:
        oy, ox = R.plan_axis(H, th, p, g), R.plan_axis(W, tw, p, g)
        cover[(H, W)] = (oy, ox, R.weights(H, W, th, tw, oy, ox, p)[1])
    oy, ox, c = cover[(44, 60)]
    assert (oy, ox) == ([0, 12], [0, 12, 28]) and c.max() == 6 and c[0].max() == 3 and c[:, 0].max() == 2
    assert cover[(116, 116)][0] == [0, 24, 52] and cover[(116, 116)][2].max() == 9 and cover[(45, 61)][2].max() == 6


def test_weights_by_hand():
    """L = 44, t = 32, ramp 8, origins 0 and 12: tile 0 falls over its last 8 pixels, tile 1 rises over its first 8."""
    w = R.axis_weights(44, 32, [0, 12], 8)
    assert (w[0, :24] == 1).all() and list(w[0, 24:32]) == [(31.5 - p) / 8 for p in range(24, 32)] and (w[0, 32:] == 0).all()
    assert (w[1, :12] == 0).all() and list(w[1, 12:20]) == [(p - 11.5) / 8 for p in range(12, 20)] and (w[1, 20:] == 1).all()


def _data(H, W, th, tw, p, g, N=2, C=3, seed=0):
    oy, ox = R.plan_axis(H, th, p, g), R.plan_axis(W, tw, p, g)
    rng = np.random.default_rng(seed)
    tiles = rng.standard_normal((len(oy) * len(ox) * N, C, th, tw)).astype(np.float32)
    return oy, ox, tiles


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_breaks_the_blend_bound(mutant):
    """What the GPU test's per-element bound (k + 2) 2^-24 sum w^ |v| is worth: a blend with the ramp one pixel longer, without
    the half-pixel centre, with a ramp at a frame border or with the two axes' weights exchanged misses it by orders of
    magnitude -- while float32 rounding of the true weights and sums stays inside it."""
    # a border ramp shows only where a second tile reaches into it (elsewhere the normalisation divides it out): 36 = 32 + 4
    H, W, th, tw, p, g = {"swapped_axes": (48, 48, 32, 32, 8, 8), "border_ramped": (36, 60, 32, 32, 8, 4)}.get(mutant, (44, 60, 32, 32, 8, 4))
    oy, ox, tiles = _data(H, W, th, tw, p, g)
    ref, mag, cover = R.blend(tiles, H, W, oy, ox, p)
    bad, _, _ = R.blend(tiles, H, W, oy, ox, p, mutant)
    ratio = np.abs(bad - ref) / R.bound(mag, cover)
    print(f"{mutant}: worst |error| / bound = {ratio.max():.3g}")
    assert ratio.max() > 1e3
    # float32 arithmetic in the kernel's order stays inside: w^ rounded once, products fused into the sums
    wn, _ = R.normalised(H, W, th, tw, oy, ox, p)
    N = tiles.shape[0] // len(wn)
    acc = np.zeros(ref.shape, dtype=np.float32)
    for k, (a, b) in enumerate((a, b) for a in oy for b in ox):
        w32 = wn[k, a:a + th, b:b + tw].astype(np.float32)
        exact = w32.astype(np.float64) * tiles[k * N:(k + 1) * N] + acc[:, :, a:a + th, b:b + tw]
        acc[:, :, a:a + th, b:b + tw] = exact.astype(np.float32)           # one rounding per fused multiply-add
    assert (np.abs(acc - ref) <= R.bound(mag, cover)).all()


def test_reference_blend_of_gathered_tiles_is_the_frame():
    H, W, th, tw, p, g = 40, 116, 32, 64, 16, 4
    oy, ox = R.plan_axis(H, th, p, g), R.plan_axis(W, tw, p, g)
    frame = np.random.default_rng(3).standard_normal((2, 3, H, W))
    out, _, cover = R.blend(R.gather(frame, oy, ox, th, tw), H, W, oy, ox, p)
    assert (len(oy), len(ox), cover.max()) == (2, 3, 6) and np.abs(out - frame).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ the eighth header
def tile_declared():
    text = open(os.path.join(ROOT, "include", "flair_tile.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_tile_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib
    assert tile_declared() == sorted(_header.TILE_PROTOS) == ["flair_tile_blend_f32", "flair_tile_gather_f32"]
    others = (set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS) | set(_header.IDENT_PROTOS)
              | set(_header.TEMPORAL_PROTOS) | set(_header.FACESCORE_PROTOS) | set(_header.YUV_PROTOS))
    assert not set(_header.TILE_PROTOS) & others and not set(_header.TILE_PROTOS) & set(_lib.ALL_PROTOS)
    assert _header.parse(open(_header.TILE_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 24
    i, v = ctypes.c_int, ctypes.c_void_p
    plan = [("N", i, None), ("C", i, None), ("H", i, None), ("W", i, None), ("oy", v, "int"), ("rows", i, None), ("ox", v, "int"),
            ("cols", i, None), ("th", i, None), ("tw", i, None)]
    want = {"flair_tile_gather_f32": [("frame", v, "float")] + plan + [("tiles", v, "float"), ("stream", v, None)],
            "flair_tile_blend_f32": [("tiles", v, "float")] + plan + [("ramp", i, None), ("out", v, "float"), ("stream", v, None)]}
    for name, params in want.items():
        restype, got = _header.TILE_PROTOS[name]
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and [tuple(p) for p in got] == params
        assert list(f.argtypes) == [p.ctype for p in got]
    header = open(_header.TILE_HEADER_PATH).read()
    code = re.sub(r"//.*", "", open(os.path.join(ROOT, "flair_amd", "csrc", "tile.hip")).read())
    assert "flair_abi_version() is 24 from this header on" in " ".join(header.replace("\n *", " ").split())
    assert "atomic" not in code and "__shared__" not in code and "asm" not in code
    assert "flair_tile.h" in open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read()


def _refused(lib, name, args, piece):
    assert getattr(lib, name)(*args, None) == -1, (name, piece)
    msg = lib.flair_last_error().decode()
    assert msg.startswith(name + ":") and piece in msg, (name, piece, msg)


def test_the_entries_refuse_before_any_launch():
    """Every refusal the header lists, on a machine without a GPU: status -1 and the entry's message."""
    from flair_amd import _lib
    lib = _lib.lib()
    F, T, OY, OX = 1 << 20, 1 << 28, 1 << 12, 1 << 13                      # addresses that are never read
    good = dict(N=2, C=3, H=44, W=60, oy=OY, rows=2, ox=OX, cols=3, th=32, tw=32)

    def args(entry, **kw):
        a = dict(good, **kw)
        plan = [a[k] for k in ("N", "C", "H", "W", "oy", "rows", "ox", "cols", "th", "tw")]
        if entry == "flair_tile_gather_f32":
            return [kw.get("frame", F)] + plan + [kw.get("tiles", T)]
        return [kw.get("tiles", T)] + plan + [kw.get("ramp", 8), kw.get("out", F)]
    for entry, frame in (("flair_tile_gather_f32", "frame"), ("flair_tile_blend_f32", "out")):
        for kw, piece in (({frame: None}, "null pointer"), ({"tiles": None}, "null pointer"), ({"oy": None}, "null pointer"),
                          ({"ox": None}, "null pointer"), ({"N": 0}, "must be positive"), ({"C": 0}, "must be positive"),
                          ({"rows": 0}, "must be positive"), ({"cols": -1}, "must be positive"), ({"th": 0}, "fit the 44 x 60 frame"),
                          ({"th": 45}, "fit the 44 x 60 frame"), ({"tw": 61}, "fit the 44 x 60 frame"),
                          ({"tiles": F + 64}, "overlaps tiles"),
                          ({"N": 1 << 30, "C": 1 << 30, "rows": 1 << 30, "cols": 1 << 30}, "64-bit offsets")):
            _refused(lib, entry, args(entry, **kw), piece)
    _refused(lib, "flair_tile_blend_f32", args("flair_tile_blend_f32", ramp=0), "ramp = 0")
    big = dict(N=1 << 20, H=1 << 12, W=1 << 12, th=32, tw=32, tiles=1 << 60)
    _refused(lib, "flair_tile_blend_f32", args("flair_tile_blend_f32", **big), "2^31 - 1 workgroups")
    _refused(lib, "flair_tile_gather_f32", args("flair_tile_gather_f32", N=1 << 20, C=1 << 10, rows=64, cols=64, H=4096, W=4096, tiles=1 << 60),
             "2^31 - 1 workgroups")


def test_the_wrappers_refuse_wrong_tensors_and_plans():
    from flair_amd import _lib, ops
    frame = torch.zeros(2, 3, 44, 60)
    with pytest.raises(ValueError, match=r"tile_gather: frame is a dense \(N, C, H, W\) float32 tensor"):
        ops.tile_gather(frame.double(), [0, 12], [0, 12, 28], (32, 32))
    with pytest.raises(ValueError, match="tile_gather: frame is a dense"):
        ops.tile_gather(frame.permute(0, 1, 3, 2), [0], [0], (32, 32))
    with pytest.raises(ValueError, match=r"tile_gather: oy = \[0, 13\]: every tile of 32 pixels must lie inside the axis of 44"):
        ops.tile_gather(frame, [0, 13], [0, 12, 28], (32, 32))
    with pytest.raises(ValueError, match=r"tile_gather: ox = \[-4, 28\]"):
        ops.tile_gather(frame, [0, 12], [-4, 28], (32, 32))
    with pytest.raises(ValueError, match="tile_gather: tiles of 45x32"):
        ops.tile_gather(frame, [0], [0], (45, 32))
    with pytest.raises(ValueError, match=r"tile_gather: out is a dense \(12, 3, 32, 32\) float32 tensor"):
        ops.tile_gather(frame, [0, 12], [0, 12, 28], (32, 32), out=torch.zeros(6, 3, 32, 32))
    tiles = torch.zeros(12, 3, 32, 32)
    with pytest.raises(ValueError, match=r"tile_blend: ox = \[0, 28\] with tiles of 32 pixels leaves pixel 60 of 64 uncovered"):
        ops.tile_blend(tiles[:8], [0, 12], [0, 28], (44, 64), 8)
    with pytest.raises(ValueError, match=r"tile_blend: ox = \[0, 28\] with tiles of 24 pixels leaves pixel 24 of 52 uncovered"):
        ops.tile_blend(torch.zeros(8, 3, 32, 24), [0, 12], [0, 28], (44, 52), 8)
    with pytest.raises(ValueError, match="tile_blend: 12 tile planes for a plan of 2x4 tiles"):
        ops.tile_blend(tiles, [0, 12], [0, 8, 16, 28], (44, 60), 8)
    with pytest.raises(ValueError, match="tile_blend: ramp = 0 pixels"):
        ops.tile_blend(tiles, [0, 12], [0, 12, 28], (44, 60), 0)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):          # every check passed: the launch is next
        ops.tile_gather(frame, [0, 12], [0, 12, 28], (32, 32))
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        ops.tile_blend(tiles, [0, 12], [0, 12, 28], (44, 60), 8)


# ------------------------------------------------------------------------------------------------ the tiled frame's refusals
def test_check_tiled_frame_size_chooses_the_tile_and_refuses_by_name():
    from flair_amd import pipeline as pl
    assert pl.check_tiled_frame_size("gaussian", (1080, 1920), (512, 512), 64, frames=10) == ((1080, 1920), (512, 512))
    assert pl.check_tiled_frame_size("gaussian", (720, 1280), (512, 512), 64, frames=10) == ((720, 1280), (512, 512))
    assert pl.check_tiled_frame_size("gaussian", (300, 1280), (512, 512), 64) == ((300, 1280), (256, 512))       # clipped to the frame
    assert pl.check_tiled_frame_size("x8_bicubic", (1080, 1920), (512, 512), 64, parser="bisenet") == ((1080, 1920), (512, 512))
    assert pl.check_tiled_frame_size("jpeg", (1088, 1920), (512, 512), 64) == ((1088, 1920), (512, 512))
    assert pl.tile_multiple("gaussian") == 64 and pl.tile_multiple("x8_bicubic", "bisenet") == 32 and pl.tile_multiple("x16_bicubic", "parsenet") == 16
    with pytest.raises(ValueError, match="gaussian: tiled frames of 1082x1920: H and W must be multiples of the factor 4"):
        pl.check_tiled_frame_size("gaussian", (1082, 1920), (512, 512))
    with pytest.raises(ValueError, match="jpeg: tiled frames of 1080x1920: H and W must stay multiples of 64, because the codec's 16x16 MCU grid"):
        pl.check_tiled_frame_size("jpeg", (1080, 1920), (512, 512))
    with pytest.raises(ValueError, match="gaussian: frames of 60x1920 with tiles of 512x512: a tile's sides are multiples of 64 and at least 64"):
        pl.check_tiled_frame_size("gaussian", (60, 1920), (512, 512))
    assert pl.frame_minimum("x8_bicubic") == 128
    with pytest.raises(ValueError, match="x8_bicubic: frames of 120x1920 with tiles of 512x512: .* at least 128"):
        pl.check_tiled_frame_size("x8_bicubic", (120, 1920), (512, 512), parser="parsenet")
    assert pl.check_tiled_frame_size("x8_bicubic", (136, 1920), (512, 512), parser="parsenet") == ((136, 1920), (128, 512))
    for bad in (0, 6, 512, -4):
        with pytest.raises(ValueError, match=f"gaussian: tile overlap {bad}: a positive multiple of the factor 4 below the tile's sides 512x512"):
            pl.check_tiled_frame_size("gaussian", (1080, 1920), (512, 512), bad)
    with pytest.raises(ValueError, match=r"frames of 1024x1536 are 1572864 pixels; the bf16 kernels address one frame"):      # the tile's own limit
        pl.check_tiled_frame_size("gaussian", (2160, 3840), (1024, 1536), 64, frames=10)
    assert pl.needs_tiling("gaussian", (1080, 1920), frames=10) and pl.needs_tiling("gaussian", (720, 1280), frames=10)
    assert not pl.needs_tiling("gaussian", (768, 1280), frames=10) and pl.needs_tiling("gaussian", (768, 1280), frames=10, dtype="fp32")
    assert pl.parse_tile("off") is None and pl.parse_tile("AUTO") == "auto" and pl.parse_tile("384x512") == (384, 512)
    with pytest.raises(ValueError, match="tile '5x': off, auto or HxW"):
        pl.parse_tile("5x")


def test_whole_frame_limits_are_refused_by_the_consumer_s_name():
    from flair_amd import video
    video.check_tiled_frame_elements("gaussian", 10, 2160, 3840)
    video.check_tiled_frame_elements("x8_bicubic", 10, 4320, 7680)
    with pytest.raises(ValueError, match="ops.resize and the face warps .* exact up to 8388607 pixels a side"):
        video.check_tiled_frame_elements("gaussian", 1, 4, 1 << 23)
    with pytest.raises(ValueError, match="one launch of flair_tile_blend_f32"):
        video.check_tiled_frame_elements("gaussian", 10, 1 << 20, 1 << 20)
    with pytest.raises(ValueError, match="the bicubic operator's flair_matmul_f32 takes at most 1048560 rows"):
        video.check_tiled_frame_elements("x8_bicubic", 10, 1048576, 64)
    video.check_tiled_frame_elements("gaussian", 10, 1048576, 64)
    from flair_amd import tiling
    plan = tiling.make_plan((1 << 18, 1 << 18), (64, 64), 32, 4)           # 8191 x 8191 tiles: the blend's launch fits, the gather's not
    video.check_tiled_frame_elements("gaussian", 3, 1 << 18, 1 << 18)
    with pytest.raises(ValueError, match="67092481 tiles of 64x64 exceeds one launch of flair_tile_gather_f32"):
        video.check_tiled_frame_elements("gaussian", 3, 1 << 18, 1 << 18, plan)


class _Stub:
    dtype = torch.bfloat16

    def parameters(self):
        return iter([torch.zeros(1)])


def test_restore_window_refuses_a_bad_tiled_frame_before_any_launch():
    """CPU tensors: a refusal reached here came before the first launch.  Without tile= the refusal of before."""
    from flair_amd import video
    deg = torch.zeros(1, 2, 3, 11, 15)
    kw = dict(size=(44, 60))
    with pytest.raises(ValueError, match="gaussian: frames of 44x60 are smaller than one tile of 64x32; frames are not padded"):
        video.restore_window("gaussian", deg, _Stub(), None, None, tile=(64, 32), tile_overlap=8, **kw)
    with pytest.raises(ValueError, match="gaussian: tiles of 32x32 with overlap 6 on frames of 44x60: .*multiple of 4"):
        video.restore_window("gaussian", deg, _Stub(), None, None, tile=(32, 32), tile_overlap=6, **kw)
    with pytest.raises(ValueError, match=r"tile=\(32, 32\) needs a size pair"):
        video.restore_window("gaussian", deg, _Stub(), None, None, size=64, tile=(32, 32))
    with pytest.raises(ValueError, match="gaussian restores 44x60 frames from degraded frames of 11x15"):
        video.restore_window("gaussian", deg[..., :10, :], _Stub(), None, None, tile=(32, 32), tile_overlap=8, **kw)
    m = video.tiled_model("gaussian", _Stub(), (44, 60), (32, 32), 8, 2)
    assert (m.plan.oy, m.plan.ox, m.dtype, m.takes_noise_level) == ([0, 12], [0, 12, 28], torch.bfloat16, False) and isinstance(m.model, _Stub)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_parses_tile_options_and_off_is_the_path_of_before(tmp_path, capsys):
    from flair_amd import __main__ as cli
    ap = cli.make_parser()
    a = ap.parse_args(["restore", "gaussian", "in", "out"])
    assert (a.tile, a.tile_overlap) == ("off", 64) and cli.tile_of(a, "gaussian", 512) == {}
    a = ap.parse_args(["restore", "gaussian", "in", "out", "--frame-size", "1080x1920", "--tile", "auto"])
    assert cli.size_of(a, "gaussian", [("in", "out")]) == (1080, 1920)
    assert cli.tile_of(a, "gaussian", (1080, 1920)) == dict(tile=(512, 512), tile_overlap=64)
    a = ap.parse_args(["restore", "gaussian", "in", "out", "--frame-size", "768x1280", "--tile", "auto"])
    assert cli.tile_of(a, "gaussian", (768, 1280)) == {}                               # restorable whole: not tiled
    a = ap.parse_args(["restore", "gaussian", "in", "out", "--frame-size", "768x1280", "--tile", "384x512", "--tile-overlap", "32"])
    assert cli.tile_of(a, "gaussian", (768, 1280)) == dict(tile=(384, 512), tile_overlap=32)
    a = ap.parse_args(["gaussian-demo", "--frame-size", "720x1280", "--tile", "512x512"])
    assert cli.tile_of(a, "gaussian", (720, 1280)) == dict(tile=(512, 512), tile_overlap=64)
    for argv, msg in ((["--tile", "512x512"], "restore: --tile needs --frame-size"),
                      (["--frame-size", "720x1280", "--tile", "huge"], "restore: tile 'huge': off, auto or HxW"),
                      (["--frame-size", "722x1280", "--tile", "auto"], "multiples of the factor 4"),
                      (["--frame-size", "720x1280", "--tile", "512x512", "--tile-overlap", "7"], "tile overlap 7")):
        a = ap.parse_args(["restore", "gaussian", "in", "out"] + argv)
        with pytest.raises(SystemExit, match=msg):
            cli.tile_of(a, "gaussian", cli.size_of(a, "gaussian", [("in", "out")]) if "--frame-size" in argv else 512)
    # --tile off (and no --tile at all) reaches check_frame_size with its present message
    for extra in ([], ["--tile", "off"]):
        a = ap.parse_args(["restore", "gaussian", "in", "out", "--frame-size", "720x1280"] + extra)
        with pytest.raises(SystemExit, match=r"restore: gaussian: frame size 720x1280 is not valid: H and W must be multiples of 64 and at least 64; "
                                             r"the nearest valid sizes are 704x1280 and 768x1280 \(frames are not padded or cropped for you\)"):
            cli.size_of(a, "gaussian", [("in", "out")])
    help_text = ap._subparsers._group_actions[0].choices["restore"].format_help()
    assert "NOT been validated on real footage" in " ".join(help_text.split()) and "--tile-overlap" in help_text


def test_build_pipeline_refuses_a_tile_without_a_pair_before_reading_any_file():
    from flair_amd import pipeline as pl
    with pytest.raises(ValueError, match=r"tile=\(512, 512\) needs a size pair"):
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=512, tile=(512, 512))
    with pytest.raises(ValueError, match="jpeg: tiled frames of 1080x1920"):
        pl.build_pipeline("jpeg", "/nonexistent", device="cpu", size=(1080, 1920), tile=(512, 512))
    with pytest.raises(ValueError, match="frame size 1080x1920 is not valid"):            # tile=None: the refusal of before
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=(1080, 1920))
    with pytest.raises(FileNotFoundError):                                                # the tiled frame passed every check
        pl.build_pipeline("gaussian", "/nonexistent", device="cpu", size=(1080, 1920), tile=(512, 512), kernels_path="/nonexistent.mat")
