"""CPU: YUV4MPEG2 streams without a GPU: the header parser and its refusals, the frame refs of flair_amd.io, the coefficient
table of include/flair_yuv.h and csrc/yuv.hip against the one tests/yuv_ref.py derives, properties and mutants of that
reference, the seventh header's binding and refusals, and the command line."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import yuv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _process_defaults():
    from flair_amd import y4m
    yield
    y4m.set_defaults("bt601", "limited")
    y4m.set_output(None, None)


def _file(tmp_path, name="clip.y4m", n=3, H=4, W=6, fmt="420jpeg", **kw):
    P = R.payload_bytes(fmt or "420jpeg", H, W)
    payloads = R.random_bytes(n * P, 77).reshape(n, P)
    return R.write_y4m(tmp_path / name, payloads, W, H, fmt, **kw), payloads


# ------------------------------------------------------------------------------------------- the header
def test_every_tag_is_read(tmp_path):
    from flair_amd import y4m
    path, payloads = _file(tmp_path, fmt="422", fps=(30000, 1001), tags="Ip A4:3 XYSCSS=422 XCOLORRANGE=FULL XFOO=1")
    s = y4m.Y4MStream(path)
    assert (s.width, s.height, s.fps, s.aspect, s.format, s.range, s.matrix) == (6, 4, (30000, 1001), "4:3", "422", "full", "bt601")
    assert s.extra == ["XYSCSS=422", "XFOO=1"] and s.header_range == "full"
    assert s.frame_count == len(s) == 3 and s.payload_bytes == 4 * 6 * 2
    assert s.header_bytes == len("YUV4MPEG2 W6 H4 F30000:1001 Ip A4:3 XYSCSS=422 XCOLORRANGE=FULL XFOO=1 C422\n")
    buf = np.zeros(s.payload_bytes, dtype=np.uint8)
    for k in (2, 0, 1):                                           # random access
        s.read_into(k, buf)
        assert np.array_equal(buf, payloads[k])
    with pytest.raises(IndexError, match="frame 3 of 3"):
        s.read_into(3, buf)
    with pytest.raises(ValueError, match="a buffer of 5 bytes for a payload of 48"):
        s.read_into(0, np.zeros(5, dtype=np.uint8))
    s.close()


def test_defaults_fill_what_the_header_leaves_open(tmp_path):
    from flair_amd import y4m
    path, _ = _file(tmp_path, fmt=None, tags="")                  # no C, no I, no X
    s = y4m.Y4MStream(path)
    assert (s.format, s.range, s.matrix, s.aspect, s.fps, s.header_range) == ("420jpeg", "limited", "bt601", None, (25, 1), None)
    bare, _ = _file(tmp_path, "bare.y4m", fmt="420")
    assert y4m.Y4MStream(bare).format == "420jpeg"
    for fmt in R.FORMATS:
        p, _ = _file(tmp_path, f"{fmt}.y4m", fmt=fmt, H=3, W=5)    # odd sizes: (W + 1) / 2 and (H + 1) / 2
        s = y4m.Y4MStream(p)
        assert (s.format, s.frame_count, s.payload_bytes) == (fmt, 3, R.payload_bytes(fmt, 3, 5))
    assert [R.payload_bytes(f, 3, 5) for f in R.FORMATS] == [15 + 12, 15 + 12, 15 + 18, 45, 15]
    y4m.set_defaults("bt709", "full")
    s = y4m.Y4MStream(path)
    assert (s.matrix, s.range) == ("bt709", "full")
    tagged, _ = _file(tmp_path, "tagged.y4m", tags="Ip XCOLORRANGE=LIMITED")
    assert y4m.Y4MStream(tagged).range == "limited"               # the header wins over the default range
    y4m.set_defaults(range="limited")
    assert y4m.defaults() == dict(matrix="bt709", range="limited")
    with pytest.raises(ValueError, match="y4m: matrix 'bt2020', one of bt601, bt709"):
        y4m.set_defaults(matrix="bt2020")
    with pytest.raises(ValueError, match="y4m: range 'tv', one of limited, full"):
        y4m.set_defaults(range="tv")


@pytest.mark.parametrize("header,message", [
    ("YUV4MPEG2 H4 F25:1", r"the header has no W tag \(the frame's width\)"),
    ("YUV4MPEG2 W6 F25:1", r"the header has no H tag \(the frame's height\)"),
    ("YUV4MPEG2 W6 H4 It", r"interlaced stream \(It\); only progressive streams \(Ip\) are read"),
    ("YUV4MPEG2 W6 H4 Ib", r"interlaced stream \(Ib\)"),
    ("YUV4MPEG2 W6 H4 Im", r"interlaced stream \(Im\)"),
    ("YUV4MPEG2 W6 H4 C420paldv", r"chroma format C420paldv is not supported \(8-bit 420jpeg, 420mpeg2, 422, 444, mono and the bare 420\)"),
    ("YUV4MPEG2 W6 H4 C411", "chroma format C411 is not supported"),
    ("YUV4MPEG2 W6 H4 C420p10", "chroma format C420p10 is not supported"),
    ("YUV4MPEG2 W6 H4 C444alpha", "chroma format C444alpha is not supported"),
    ("YUV4MPEG2 W0 H4", "header tag 'W0' is not a positive size"),
    ("YUV4MPEG2 W6 H4 F0:1", "frame rate '0:1' is not N or N:D"),
    ("YUV4MPEG2 W6 H4 XCOLORRANGE=WIDE", "header tag 'XCOLORRANGE=WIDE' is neither FULL nor LIMITED"),
    ("YUV4MPEG2 W6 H4 Q7", "unknown header tag 'Q7'"),
    ("YUV4MPEG3 W6 H4", "not a YUV4MPEG2 stream"),
])
def test_the_header_refuses_by_name(tmp_path, header, message):
    from flair_amd import y4m
    path = R.write_y4m(tmp_path / "bad.y4m", [], 6, 4, header=header)
    with pytest.raises(ValueError, match=re.escape(str(path)) + ": " + message):
        y4m.Y4MStream(path)


def test_the_frame_count_comes_from_the_file_size_alone(tmp_path):
    from flair_amd import y4m
    path, payloads = _file(tmp_path, n=4, H=3, W=5)                # odd W and H: 15 + 2 * 2 * 3 bytes a frame
    assert y4m.Y4MStream(path).frame_count == 4 and y4m.Y4MStream(path).payload_bytes == 27
    data = open(path, "rb").read()
    cut = tmp_path / "cut.y4m"
    cut.write_bytes(data[:-5])
    with pytest.raises(ValueError, match=r"cut.y4m: \d+ bytes after the header are not whole frames of 6 \+ 27 bytes \(420jpeg, 5x3\): a truncated file"):
        y4m.Y4MStream(cut)
    params = R.write_y4m(tmp_path / "params.y4m", payloads, 5, 3, frame_line=b"FRAME Ip\n")
    with pytest.raises(ValueError, match="a truncated file, or frames with parameters"):
        y4m.Y4MStream(params)
    wrong = R.write_y4m(tmp_path / "wrong.y4m", payloads, 5, 3, frame_line=b"FRAMX\n")     # the size fits, the six bytes do not
    s = y4m.Y4MStream(wrong)
    with pytest.raises(ValueError, match=r"frame 1 does not start with 'FRAME\\n' \(got b'FRAMX\\n'\); per-frame parameters are not supported"):
        s.read_into(1, np.zeros(27, dtype=np.uint8))
    empty = R.write_y4m(tmp_path / "empty.y4m", [], 5, 3)
    assert y4m.Y4MStream(empty).frame_count == 0
    (tmp_path / "text.y4m").write_bytes(b"hello")
    with pytest.raises(ValueError, match="not a YUV4MPEG2 stream"):
        y4m.Y4MStream(tmp_path / "text.y4m")


def test_header_line_and_output_params(tmp_path):
    from flair_amd import y4m
    assert y4m.header_line(130, 17, (30000, 1001), "422", "full", "1:1", ["XFOO=1"]) == b"YUV4MPEG2 W130 H17 F30000:1001 Ip A1:1 C422 XCOLORRANGE=FULL XFOO=1\n"
    assert y4m.header_line(8, 8, (25, 1), "420jpeg", "limited") == b"YUV4MPEG2 W8 H8 F25:1 Ip C420jpeg XCOLORRANGE=LIMITED\n"
    assert y4m.output_params() == dict(fps=(25, 1), aspect=None, format="420jpeg", matrix="bt601", range="limited", extra=[])
    path, _ = _file(tmp_path, fmt="444", fps=(24, 1), tags="Ip A1:1 XCOLORRANGE=FULL XFOO=1")
    src = y4m.Y4MStream(path)
    assert y4m.output_params(src, rate=2) == dict(fps=(48, 1), aspect="1:1", format="444", matrix="bt601", range="full", extra=["XFOO=1"])
    y4m.set_output("420mpeg2", "30000:1001")
    assert y4m.output_params(src, rate=3)["fps"] == (90000, 1001) and y4m.output_params(src)["format"] == "420mpeg2"
    assert y4m.parse_fps("30") == (30, 1) and y4m.parse_fps((50, 2)) == (50, 2)
    for bad in ("0", "30:0", "x", "1:2:3", "-5"):
        with pytest.raises(ValueError, match="is not N or N:D with positive integers"):
            y4m.parse_fps(bad)
    with pytest.raises(ValueError, match="chroma format '411'"):
        y4m.set_output("411")


# ------------------------------------------------------------------------------------------- frame refs
def test_list_frames_and_frame_size(tmp_path):
    from flair_amd import io as fio
    from flair_amd.y4m import Y4MFrame
    path, _ = _file(tmp_path, "Clip.Y4M", n=12, H=4, W=6)          # any case
    refs = fio.list_frames(path)
    assert len(refs) == 12 and all(isinstance(r, Y4MFrame) and isinstance(r, str) for r in refs)
    assert refs[7] == f"{path}#0007" and os.path.basename(refs[7]) == "Clip.Y4M#0007"
    assert (refs[7].index, refs[7].stream.path) == (7, path) and refs[0].stream is refs[11].stream
    assert [fio.frame_size(r) for r in refs[:2]] == [(4, 6), (4, 6)]
    assert sorted(reversed(refs), key=fio.natural_key) == refs and sorted(reversed(refs)) == refs
    # a directory that holds both lists its frame files, in natural order; the stream is not one of them
    for i in (10, 2, 1):
        fio.write_frame(str(tmp_path / f"frame_{i}.png"), np.zeros((4, 6, 3), dtype=np.uint8))
    assert [os.path.basename(p) for p in fio.list_frames(tmp_path)] == ["frame_1.png", "frame_2.png", "frame_10.png"]
    assert fio.frame_size(fio.list_frames(tmp_path)[0]) == (4, 6)


def test_a_stream_on_a_cpu_device_is_refused_by_name(tmp_path, monkeypatch):
    from flair_amd import io as fio
    path, _ = _file(tmp_path)
    refs = fio.list_frames(path)
    with pytest.raises(ValueError, match=r"clip.y4m#0000: the frames of a \.y4m stream become RGB in flair_yuv_to_rgb_u8 on the GPU; there is no CPU colour path \(device cpu\)"):
        next(fio.iter_windows(refs, "cpu"))
    with pytest.raises(ValueError, match="there is no CPU colour path"):
        next(fio.iter_frame_batches([refs], [(0, 1)], "cpu"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="there is no CPU colour path"):
        fio.decode_frame_hwc(refs[0])
    w = fio._Writer(tmp_path / "out.y4m")
    with pytest.raises(ValueError, match=r"out.y4m: the frames of a \.y4m stream are made in flair_rgb_to_yuv_u8 on the GPU; there is no CPU colour path"):
        w.submit_bytes(0, torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"frames are \(n, H, W, 3\) uint8"):
        w.submit_bytes(0, torch.zeros(1, 4, 4, 3))
    w.close()
    assert os.path.getsize(tmp_path / "out.y4m") == 0              # no frame, no header


# ------------------------------------------------------------------------------------------- the table and the definition
def _header_table():
    text = open(os.path.join(ROOT, "include", "flair_yuv.h")).read()
    rows = re.findall(r"coefficients (bt\d+) (limited|full)\s*: cy (-?\d+) crv (-?\d+) cgu (-?\d+) cgv (-?\d+) cbu (-?\d+) "
                      r"ey (-?\d+) (-?\d+) (-?\d+) eu (-?\d+) (-?\d+) (-?\d+) ev (-?\d+) (-?\d+) (-?\d+)", text)
    return {(m, r): tuple(int(v) for v in vals) for m, r, *vals in rows}


def test_the_tables_are_the_derived_coefficients():
    table = _header_table()
    assert sorted(table) == sorted((m, r) for m in R.MATRICES for r in R.RANGES)
    for key, row in table.items():
        assert row == R.coefficients(*key), key
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "yuv.hip")).read()
    body = re.search(r"YUV_TAB\[4\]\[14\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [tuple(int(v) for v in row.split(",")) for row in re.findall(r"\{([^{}]*)\}", body)]
    assert rows == [R.coefficients(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]      # index matrix * 2 + range
    assert R.coefficients("bt601", "limited") == (76309, 104597, 25675, 53279, 132201, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681)
    assert min(R.tie_margin(m, r) for m in R.MATRICES for r in R.RANGES) > 0.003       # no product near a rounding tie
    for m in R.MATRICES:
        for r in R.RANGES:
            k = R.coefficients(m, r)
            assert sum(k[8:11]) in (-1, 0, 1) and sum(k[11:14]) in (-1, 0, 1)            # grey has (almost) no chroma


def test_the_python_ids_are_the_headers():
    from flair_amd import ops, y4m
    text = open(os.path.join(ROOT, "include", "flair_yuv.h")).read()
    ids = {n: int(v) for n, v in re.findall(r"#define FLAIR_YUV_(\w+) (\d+)", text)}
    assert ids == {"420JPEG": 0, "420MPEG2": 1, "422": 2, "444": 3, "MONO": 4, "BT601": 0, "BT709": 1, "LIMITED": 0, "FULL": 1}
    assert all(ids[k.upper()] == v for d in (ops.YUV_FORMATS, ops.YUV_MATRICES, ops.YUV_RANGES) for k, v in d.items())
    assert tuple(ops.YUV_FORMATS) == y4m.FORMATS == R.FORMATS and tuple(ops.YUV_MATRICES) == y4m.MATRICES and tuple(ops.YUV_RANGES) == y4m.RANGES
    for fmt in R.FORMATS:
        for H, W in R.SHAPES:
            assert y4m.payload_bytes(fmt, H, W) == R.payload_bytes(fmt, H, W) and y4m.chroma_size(fmt, H, W) == R.chroma_size(fmt, H, W)


@pytest.mark.parametrize("matrix", sorted(R.MATRICES))
def test_grey_stays_grey_and_the_range_maps_to_the_ends(matrix):
    Y = np.arange(256, dtype=np.uint8)
    for range_ in R.RANGES:
        payload = np.concatenate([Y, np.full(512, 128, np.uint8)])[None]          # 444, 1 x 256: U = V = 128
        rgb = R.decode(payload, 1, 256, "444", matrix, range_)[0, 0]
        assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all()
        mono = R.decode(Y[None], 1, 256, "mono", matrix, range_)[0, 0]
        assert np.array_equal(mono, rgb)
        if range_ == "limited":
            assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and rgb[:16].max() == 0 and rgb[235:].min() == 255
            assert rgb[126, 0] == 128                                              # (126 - 16) 255 / 219 = 128.08
        else:
            assert np.array_equal(rgb[:, 0], Y)
        white, black = np.full((1, 2, 2, 3), 255, np.uint8), np.zeros((1, 2, 2, 3), np.uint8)
        hi, lo = (235, 16) if range_ == "limited" else (255, 0)
        for fmt in R.FORMATS:
            n = R.payload_bytes(fmt, 2, 2) - 4
            assert R.encode(white, fmt, matrix, range_).tolist() == [[hi] * 4 + [128] * n]
            assert R.encode(black, fmt, matrix, range_).tolist() == [[lo] * 4 + [128] * n]


@pytest.mark.parametrize("fmt", R.FORMATS[:4])
def test_constant_chroma_upsamples_to_a_constant(fmt):
    H, W = 5, 7
    hc, wc = R.chroma_size(fmt, H, W)
    for u, v in ((128, 128), (0, 255), (90, 240), (255, 17)):
        payload = np.concatenate([np.full(H * W, 120, np.uint8), np.full(hc * wc, u, np.uint8), np.full(hc * wc, v, np.uint8)])[None]
        got = R.decode(payload, H, W, fmt, "bt709", "full")
        want = R.decode(np.array([[120, u, v]], dtype=np.uint8), 1, 1, "444", "bt709", "full")
        assert (got == want[0, 0, 0]).all(), (fmt, u, v)
    for mode, n in (("full", 7), ("centred", 4), ("cosited", 4)):                  # the weights are quarters that sum to 4
        i0, w0, i1, w1 = R.decode_taps(mode, 7, n)
        assert ((w0 + w1) == 4).all() and i0.min() >= 0 and max(i0.max(), i1.max()) <= n - 1 and i1.min() >= 0


def test_the_444_round_trip_over_the_colour_lattice():
    lat = np.unique(np.append(np.arange(0, 256, 5), 255))
    rgb = np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), -1).reshape(1, -1, 1, 3).astype(np.uint8)
    for matrix in R.MATRICES:
        for range_, bound in (("limited", 2), ("full", 1)):
            back = R.decode(R.encode(rgb, "444", matrix, range_), rgb.shape[1], 1, "444", matrix, range_)
            worst = int(np.abs(back.astype(int) - rgb.astype(int)).max())
            print(f"{matrix} {range_}: 444 round trip differs by at most {worst}")
            assert worst <= bound


def test_footprints_replicate_the_edge():
    """3 x 5: the last chroma column averages luma column 4 with itself, the last chroma row luma row 2 with itself."""
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=(1, 3, 5, 3), dtype=np.uint8)
    padded = np.concatenate([rgb, rgb[:, -1:]], axis=1)
    padded = np.concatenate([padded, padded[:, :, -1:]], axis=2)                 # 4 x 6 with the edge repeated
    for fmt in ("420jpeg", "420mpeg2", "422"):
        a, b = R.encode(rgb, fmt, "bt601", "full"), R.encode(padded, fmt, "bt601", "full")
        hc, wc = R.chroma_size(fmt, 3, 5)
        hp, wp = R.chroma_size(fmt, padded.shape[1], 6)
        assert (hp, wp) == ((hc, wc) if fmt != "422" else (4, 3))
        ua, ub = a[0, 15:15 + hc * wc].reshape(hc, wc), b[0, padded.shape[1] * 6:padded.shape[1] * 6 + hp * wp].reshape(hp, wp)
        assert np.array_equal(ua, ub[:hc, :wc]), fmt


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_the_reference_on_the_gpu_inputs(mutant):
    """Equality with the reference on the GPU tests' inputs means something: each mutant changes its output there."""
    combos = [("bt601", "limited"), ("bt709", "full")]
    decode = encode = 0
    for fmt in R.FORMATS:
        for N, H, W in R.all_cases():
            if N != 1:
                continue
            pl, rgb = R.payload_case(fmt, N, H, W), R.rgb_case(N, H, W)
            for m, r in combos:
                decode += not np.array_equal(R.decode(pl, H, W, fmt, m, r), R.decode(pl, H, W, fmt, m, r, mutant=mutant))
                encode += not np.array_equal(R.encode(rgb, fmt, m, r), R.encode(rgb, fmt, m, r, mutant=mutant))
    print(f"{mutant}: changes {decode} decodes and {encode} encodes")
    if mutant.startswith("coef"):
        assert (decode if int(mutant[4:]) < 5 else encode) > 0
    else:
        assert decode > 0 and encode > 0


# ------------------------------------------------------------------------------------------- the seventh header
def yuv_declared():
    text = open(os.path.join(ROOT, "include", "flair_yuv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_yuv_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib
    assert yuv_declared() == sorted(_header.YUV_PROTOS) == ["flair_rgb_to_yuv_u8", "flair_yuv_to_rgb_u8"]
    others = (set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS) | set(_header.IDENT_PROTOS)
              | set(_header.TEMPORAL_PROTOS) | set(_header.FACESCORE_PROTOS))
    assert not set(_header.YUV_PROTOS) & others and not set(_header.YUV_PROTOS) & set(_lib.ALL_PROTOS)
    assert len(_header.STRUCTS) == 7 and _header.parse(open(_header.YUV_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 23
    i, v = ctypes.c_int, ctypes.c_void_p
    want = {"flair_yuv_to_rgb_u8": [("payload", v, "uint8_t"), ("N", i, None), ("H", i, None), ("W", i, None), ("format", i, None), ("matrix", i, None),
                                    ("range", i, None), ("planar", i, None), ("out", v, "uint8_t"), ("stream", v, None)],
            "flair_rgb_to_yuv_u8": [("rgb", v, "uint8_t"), ("N", i, None), ("H", i, None), ("W", i, None), ("format", i, None), ("matrix", i, None),
                                    ("range", i, None), ("payload_out", v, "uint8_t"), ("stream", v, None)]}
    for name, params in want.items():
        restype, got = _header.YUV_PROTOS[name]
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and [tuple(p) for p in got] == params
        assert list(f.argtypes) == [p.ctype for p in got]
    header = open(_header.YUV_HEADER_PATH).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "yuv.hip")).read()
    assert "is 23 from this header on" in header and "NOT swscale's path" in header and "no counterpart in the reference" in header
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code and "__shared__" not in code and "asm" not in code
    kernels = code[:code.index("bool overlaps(")]
    assert not re.search(r"\b(float|double|__half)\b", kernels)                                    # integers throughout the device code
    assert not re.search(r"size_t\s+flair_", re.sub(r"/\*.*?\*/", "", header, flags=re.S))         # nothing allocated, no workspace
    assert "flair_yuv.h" in open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read()


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entries():
    from flair_amd import _lib
    call = _lib.call
    u8, f32 = _device_tensor(torch.uint8), _device_tensor(torch.float32)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_yuv_to_rgb_u8(torch.zeros(2, dtype=torch.uint8), 1, 1, 1, 0, 0, 0, 0, u8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_yuv_to_rgb_u8: payload must be uint8, got float32$"):
        call.flair_yuv_to_rgb_u8(f32, 1, 1, 1, 0, 0, 0, 0, u8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_rgb_to_yuv_u8: payload_out must be uint8, got float32$"):
        call.flair_rgb_to_yuv_u8(u8, 1, 1, 1, 0, 0, 0, f32)
    with pytest.raises(TypeError, match="flair_rgb_to_yuv_u8 takes 8 arguments"):
        call.flair_rgb_to_yuv_u8(u8, 1)
    with pytest.raises(AttributeError, match="flair_yuv_workspace is not an entry"):
        call.flair_yuv_workspace


def test_the_entries_refuse_before_any_launch(monkeypatch):
    """Every refusal the header lists: status -1 and the entry's message, on a machine without a GPU; N = 0 enqueues nothing."""
    from flair_amd import _lib
    lib = _lib.lib()
    cases = R.entry_refusals(1 << 20, 1 << 24, 6, 8)
    assert {n for n, _, _ in cases} == {"flair_yuv_to_rgb_u8", "flair_rgb_to_yuv_u8"} and len(cases) >= 30
    for case in cases:
        R.assert_refused(lib, *case)
    for name, args in R.entry_noops(1 << 20, 1 << 24, 6, 8):
        assert getattr(lib, name)(*args, None) == 0
    monkeypatch.setattr(_lib, "stream", lambda: None)
    u8 = _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_rgb_to_yuv_u8 failed \(status -1\): flair_rgb_to_yuv_u8: payload_out overlaps rgb"):
        _lib.call.flair_rgb_to_yuv_u8(u8, 1, 4, 4, 0, 0, 0, u8)


def test_the_wrappers_refuse_wrong_tensors():
    from flair_amd import _lib, ops
    rgb = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"rgb_to_yuv_u8: rgb is a dense \(N, H, W, 3\) uint8 tensor, got \(2, 6, 8, 3\) torch.float32"):
        ops.rgb_to_yuv_u8(rgb.float(), "444", "bt601", "full")
    with pytest.raises(ValueError, match="rgb_to_yuv_u8: rgb is a dense"):
        ops.rgb_to_yuv_u8(rgb.permute(0, 2, 1, 3), "444", "bt601", "full")
    with pytest.raises(ValueError, match=r"rgb_to_yuv_u8: out is a dense \(2, 72\) uint8 tensor, got \(2, 71\)"):
        ops.rgb_to_yuv_u8(rgb, "420jpeg", "bt601", "full", out=torch.zeros(2, 71, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rgb_to_yuv_u8: range 'tv', one of limited, full"):
        ops.rgb_to_yuv_u8(rgb, "444", "bt601", "tv")
    payload = torch.zeros(2, 72, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"yuv_to_rgb_u8: payload is a dense \(N, 96\) uint8 tensor for 422 frames of 6x8, got \(2, 72\)"):
        ops.yuv_to_rgb_u8(payload, (6, 8), "422", "bt601", "full")
    with pytest.raises(ValueError, match=r"yuv_to_rgb_u8: out is a dense \(2, 3, 6, 8\) uint8 tensor, got \(2, 6, 8, 3\)"):
        ops.yuv_to_rgb_u8(payload, (6, 8), "420jpeg", "bt601", "full", planar=True, out=rgb)
    with pytest.raises(ValueError, match="yuv_to_rgb_u8: frames of 0x8 pixels"):
        ops.yuv_to_rgb_u8(payload, (0, 8), "420jpeg", "bt601", "full")
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):          # every check passed: the launch is next
        ops.yuv_to_rgb_u8(payload, (6, 8), "420jpeg", "bt601", "full")
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        ops.rgb_to_yuv_u8(rgb, "mono", "bt709", "limited")
    assert ops.yuv_to_rgb_u8(payload[:0], (6, 8), "420jpeg", "bt601", "full").shape == (0, 6, 8, 3)      # N = 0 launches nothing, on any device
    assert ops.rgb_to_yuv_u8(rgb[:0], "422", "bt601", "full").shape == (0, 96)


# ------------------------------------------------------------------------------------------- the command line
def test_every_command_takes_streams_and_the_new_options():
    from flair_amd.__main__ import make_parser
    ap = make_parser()
    yuv = ["--yuv-matrix", "bt709", "--yuv-range", "full"]
    out = ["--y4m-chroma", "422", "--fps", "30000:1001"]
    a = ap.parse_args(["restore", "gaussian", "lr.y4m", "out.y4m", "--ground-truth", "clean.y4m", "--frame-size", "auto"] + yuv + out)
    assert (a.paths, a.ground_truth, a.yuv_matrix, a.yuv_range, a.y4m_chroma, a.fps) == (["lr.y4m", "out.y4m"], "clean.y4m", "bt709", "full", "422", "30000:1001")
    a = ap.parse_args(["restore", "gaussian", "a.y4m", "b.y4m", "--output-root", "o"])
    assert (a.yuv_matrix, a.yuv_range, a.y4m_chroma, a.fps) == (None, None, None, None)
    a = ap.parse_args(["degrade", "gaussian", "clean.y4m", "lr.y4m"] + yuv + out)
    assert (a.clean_dir, a.out_dir, a.y4m_chroma, a.fps, a.yuv_matrix) == ("clean.y4m", "lr.y4m", "422", "30000:1001", "bt709")
    a = ap.parse_args(["interpolate", "out.y4m", "out_x2.y4m", "--factor", "2"] + yuv + out)
    assert (a.src_dir, a.out_dir, a.y4m_chroma, a.yuv_range) == ("out.y4m", "out_x2.y4m", "422", "full")
    for argv, attr in ((["evaluate", "restored.y4m", "clean_pngs"], "restored_dir"), (["niqe", "a.y4m"], "frames_dir"), (["warp-error", "a.y4m"], "frames_dir"),
                       (["scenes", "a.y4m"], "src_dir")):
        a = ap.parse_args(argv + yuv)
        assert getattr(a, attr).endswith(".y4m") and (a.yuv_matrix, a.yuv_range) == ("bt709", "full")
        assert not hasattr(a, "y4m_chroma") and not hasattr(a, "fps")                  # the reading commands write no stream
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--y4m-chroma", "444"])
    for bad in (["--yuv-matrix", "bt2020"], ["--yuv-range", "tv"], ["--y4m-chroma", "mono"], ["--y4m-chroma", "411"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["degrade", "gaussian", "a.y4m", "b.y4m"] + bad)
    assert "not passed through byte for byte" in " ".join(ap._subparsers._group_actions[0].choices["interpolate"].format_help().split())


def test_the_command_line_sets_the_process_defaults_and_refuses_early(tmp_path):
    from flair_amd import y4m
    from flair_amd.__main__ import frames_exist, main, metrics_path
    missing = str(tmp_path / "none.y4m")
    for argv, message in ((["scenes", missing], f"scenes: {missing} is not a directory"), (["niqe", missing, "--params", __file__], f"niqe: {missing} is not a directory"),
                          (["degrade", "gaussian", missing, str(tmp_path / "o.y4m")], f"degrade: {missing} is not a directory"),
                          (["restore", "gaussian", missing, str(tmp_path / "o.y4m")], f"restore: {missing} is not a directory"),
                          (["interpolate", missing, str(tmp_path / "o.y4m"), "--factor", "2"], f"interpolate: {missing} is not a file")):
        with pytest.raises(SystemExit, match=re.escape(message)):
            main(argv + ["--yuv-matrix", "bt709", "--yuv-range", "full"])
    assert y4m.defaults() == dict(matrix="bt709", range="full")
    with pytest.raises(SystemExit):
        main(["scenes", missing])
    assert y4m.defaults() == dict(matrix="bt601", range="limited")                    # a command line is complete
    with pytest.raises(SystemExit, match="degrade: y4m: frame rate '0' is not N or N:D"):
        main(["degrade", "gaussian", missing, "o.y4m", "--fps", "0"])
    bad = R.write_y4m(tmp_path / "bad.y4m", [], 6, 4, header="YUV4MPEG2 W6 H4 It")
    with pytest.raises(SystemExit, match=r"restore: .*bad.y4m: interlaced stream \(It\)"):
        main(["restore", "gaussian", bad, str(tmp_path / "o.y4m")])
    with pytest.raises(SystemExit, match=r"scenes: .*bad.y4m: interlaced stream \(It\)"):
        main(["scenes", bad])
    with pytest.raises(SystemExit, match=r"interpolate: .*bad.y4m: interlaced stream \(It\)"):
        main(["interpolate", bad, str(tmp_path / "o.y4m"), "--factor", "2"])
    ok, _ = _file(tmp_path, "ok.y4m")
    assert frames_exist(ok) and frames_exist(str(tmp_path)) and not frames_exist(missing) and not frames_exist(str(tmp_path / "nodir"))
    assert metrics_path("out/clip.y4m") == "out/clip.y4m.metrics.json" and metrics_path("out/clip") == os.path.join("out/clip", "metrics.json")


def test_auto_frame_size_reads_the_stream_header(tmp_path):
    from flair_amd import pipeline as pl
    path, _ = _file(tmp_path, "lr.y4m", n=2, H=16, W=24)
    assert pl.auto_frame_size("gaussian", path) == (64, 96)
