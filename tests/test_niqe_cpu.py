"""CPU: NIQE's definition (tests/niqe_ref.py) on hand cases and against six misreadings, the host statistics of
flair_amd/niqe.py against it, the third header, the two entries' and the loader's refusals, the command line and the report."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import niqe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = R.synthetic_params()
SCORE_BOUND = 1e-9                       # relative, what tests/test_gpu_niqe.py grants the kernels on the whole score


def png(path, h, w, value=0):
    from flair_amd import io as fio
    fio.write_frame(str(path), np.full((h, w, 3), value, dtype=np.uint8))


def write_params(path, mu=None, cov=None, window=None, **extra):
    np.savez(path, mu_pris_param=PARAMS[0].reshape(1, 36) if mu is None else mu, cov_pris_param=PARAMS[1] if cov is None else cov,
             gaussian_window=PARAMS[2] if window is None else window, **extra)
    return str(path)


# ------------------------------------------------------------------------------------------- hand cases
def test_luma_is_the_exact_rounded_quotient():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    px = np.concatenate([rng.integers(0, 256, (200, 3)), R.tie_triples()[::7].astype(np.int64), [[0, 0, 0], [255, 255, 255]]]).astype(np.uint8)
    got = R.luma(px[None])[0]
    for (r, g, b), y in zip(px.tolist(), got.tolist()):
        assert y == round(Fraction(65481 * r + 128553 * g + 24966 * b, 255000)) + 16        # Fraction rounds half to even
    assert got[-2] == 16 and got[-1] == 235
    ties = R.tie_triples().astype(np.int64)
    exact = (65481 * ties[:, 0] + 128553 * ties[:, 1] + 24966 * ties[:, 2]) % 255000 == 127500
    assert exact.sum() == 194 and len(ties) == 580


def test_half_scale_weights_and_reflection():
    assert R.HALF_TAPS.sum() == 256 and list(R.HALF_TAPS) == list(R.HALF_TAPS[::-1])
    # MATLAB's antialiased cubic at a factor of 1/2: cubic(x / 2) / 2 at x = -3.5 .. 3.5
    x = np.abs(np.arange(-3.5, 4.0, 1.0) / 2)
    cubic = np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2)
    assert np.array_equal(cubic / 2 * 256, R.HALF_TAPS)
    y = np.full((96, 96), 100, dtype=np.int64)
    assert np.all(R.half_scale(y) == 100 * 65536)
    ramp = np.tile(np.arange(96, dtype=np.int64), (96, 1))
    h = R.half_scale(ramp)
    assert np.all(h[:, 2:46] == (2 * np.arange(2, 46) + 0.5) * 65536)                     # a linear ramp is reproduced inside
    taps = [2, 1, 0, 0, 1, 2, 3, 4]                                                           # inputs -3 .. 4 of output 0: -3 -> 2, -2 -> 1, -1 -> 0
    assert h[0, 0] == 256 * int(np.dot(R.HALF_TAPS, taps))
    assert np.abs(R.half_scale(np.random.default_rng(0).integers(16, 236, (96, 192)))).max() < 2 ** 25


def test_a_constant_frame_has_zero_moments_and_no_score():
    from flair_amd import niqe as Q
    u8 = np.full((96, 192, 3), 77, dtype=np.uint8)
    got = R.analyse(u8, PARAMS, form="restatement")
    assert not got["moments"].any() and np.isnan(got["features"]).all() and math.isnan(got["score"])
    noisy = R.analyse(u8, PARAMS, form="definition")              # the unshifted sums leave rounding noise on every pixel
    assert (noisy["mscn"][0] != 0).sum() == 96 * 192 and np.abs(noisy["mscn"][0]).max() < 1e-12
    f = Q.features(np.zeros((2, 5, 5)), 96 * 96)
    assert f.shape == (2, 18) and np.isnan(f).all() and math.isnan(Q.score(np.full((2, 36), np.nan), PARAMS[0], PARAMS[1]))
    one_good = np.vstack([np.ones((1, 36)), np.full((3, 36), np.nan)])
    assert math.isnan(Q.score(one_good, PARAMS[0], PARAMS[1])) and math.isnan(R.score_of(one_good, PARAMS[0], PARAMS[1]))


def test_block_order_is_column_major():
    m = np.zeros((192, 288))
    for i in range(2):
        for j in range(3):
            m[96 * i:96 * i + 96, 96 * j:96 * j + 96] = 10 * i + j
    assert [int(b[0, 0]) for b in R.blocks_of(m, 96)] == [0, 10, 1, 11, 2, 12]             # index j nh + i
    assert [int(b[0, 0]) for b in R.blocks_of(m, 96, order="row")] == [0, 1, 2, 10, 11, 12]


def test_the_roll_wraps_inside_the_block():
    m = np.arange(96 * 192, dtype=np.float64).reshape(96, 192) + 1
    maps = R.maps_of(m, 96)
    b1 = m[:, 96:]
    assert maps.shape == (2, 5, 96, 96) and np.array_equal(maps[1, 0], b1)
    assert maps[1, 1, 5, 0] == b1[5, 0] * b1[5, 95]              # (0, 1): the left neighbour of column 0 is the BLOCK's last column
    assert maps[1, 1, 5, 0] != m[5, 96] * m[5, 95]               # ... not the plane's column 95
    assert maps[1, 2, 0, 7] == b1[0, 7] * b1[95, 7]              # (1, 0)
    assert maps[1, 3, 0, 0] == b1[0, 0] * b1[95, 95]             # (1, 1)
    assert maps[1, 4, 0, 95] == b1[0, 95] * b1[95, 0]            # (1, -1): the right neighbour of column 95 is the block's column 0
    assert maps[0, 4, 3, 4] == m[3, 4] * m[2, 5]


def test_moments_leave_zeros_out():
    x = np.array([[-2.0, 0.0, 3.0, 0.0], [1.0, -1.0, 0.0, 0.5]])
    assert R.moments_of(x).tolist() == [2.0, 3.0, 5.0, 10.25, 7.5]
    assert R.moments_of(x, zeros_positive=True).tolist() == [2.0, 6.0, 5.0, 10.25, 7.5]


# ------------------------------------------------------------------------------------------- host statistics
def test_host_statistics_are_the_references():
    from flair_amd import niqe as Q
    for got in R.case_reference(3, 200, 301):
        f = np.concatenate([Q.features(got["moments"][:, 0], 96 * 96), Q.features(got["moments"][:, 1], 48 * 48)], axis=1)
        assert np.array_equal(f, got["features"]) and not np.isnan(f).any()
        assert Q.score(f, PARAMS[0], PARAMS[1]) == got["score"]
    x = np.random.default_rng(0).uniform(-0.1, 1.0, 4000)
    x[:4] = [0.0, 1.0, R.R_GAM[0], R.R_GAM[-1]]
    x[4:104] = R.R_GAM[100:200]
    x[104:204] = (R.R_GAM[100:200] + R.R_GAM[101:201]) / 2                                   # grid points and midpoints
    assert np.array_equal(Q.nearest_alpha(x), [np.argmin((R.R_GAM - v) ** 2) for v in x])
    assert np.array_equal(Q.ALPHAS, R.ALPHAS) and np.array_equal(Q.R_GAM, R.R_GAM) and len(Q.ALPHAS) == 9801
    # a map with one empty side has no fit: every feature of it is NaN, in both
    mom = got["moments"][:1, 0].copy()
    mom[0, 2, 0] = mom[0, 2, 2] = 0.0
    f, r = Q.features(mom, 96 * 96), R.features_of(mom, 96 * 96)
    assert np.isnan(f[0, 6:10]).all() and not np.isnan(np.delete(f[0], range(6, 10))).any() and np.array_equal(f, r, equal_nan=True)


def test_restatement_agrees_with_the_definition():
    for got, again in zip(R.case_reference(3, 200, 301), R.case_reference(3, 200, 301, "restatement")):
        assert max(np.abs(a - b).max() for a, b in zip(got["mscn"], again["mscn"])) < 1e-11
        assert np.array_equal(got["moments"][..., :2], again["moments"][..., :2])
        assert abs(got["score"] - again["score"]) < 1e-12 * got["score"]


# ------------------------------------------------------------------------------------------- misreadings
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_misreadings_move_the_result(mutant):
    u8 = R.frame(192, 288, 40.0, 5)
    if mutant == "zeros_positive":
        u8[:, :112] = 90                  # exact zeros in M: the blocks of column 0 are flat, those of column 1 partly
    form = "restatement" if mutant == "zeros_positive" else "definition"
    base, bent = R.analyse(u8, PARAMS, form=form), R.analyse(u8, PARAMS, form=form, mutant=mutant)
    if mutant == "row_major":             # the same blocks in another order: mean and covariance do not see it
        assert np.abs(bent["features"] - base["features"]).max() > 0.1
        assert np.array_equal(bent["features"][[0, 3, 1, 4, 2, 5]], base["features"])
    else:
        assert abs(bent["score"] - base["score"]) > 10 * SCORE_BOUND * base["score"], (base["score"], bent["score"])


def test_one_alpha_cell_is_visible_on_the_gpu_tests_inputs():
    """The bound of tests/test_gpu_niqe.py on the whole score, 1e-9 relative, lies between float64 order noise (the two
    forms of the MSCN map differ by less than 1e-14 in the score) and the smallest real fault on those very inputs: one
    alpha one grid cell off in one block moves the score by more than ten times the bound, whichever block and alpha."""
    for shape in [(1, 96, 192), (3, 200, 301), (2, 192, 96)]:
        for n, (got, again) in enumerate(zip(R.case_reference(*shape), R.case_reference(*shape, "restatement"))):
            faults = R.alpha_cell_faults(got["features"], PARAMS[0], PARAMS[1])
            noise = abs(again["score"] - got["score"]) / got["score"]
            print(f"niqe bound   {'x'.join(map(str, shape))} frame {n}: form noise {noise:.3e}, one alpha cell moves the score by "
                  f"{faults.min():.3e} (min) / {np.median(faults):.3e} (median) / {faults.max():.3e} (max)")
            assert noise < 1e-14 < SCORE_BOUND and faults.min() > 10 * SCORE_BOUND


# ------------------------------------------------------------------------------------------- the third header
def noref_declared():
    text = open(os.path.join(ROOT, "include", "flair_noref.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_the_noref_header_is_parsed_typed_and_exported():
    from flair_amd import _header, _lib
    assert noref_declared() == sorted(_header.NOREF_PROTOS) == ["flair_niqe_luma", "flair_niqe_moments"]
    assert not set(_header.NOREF_PROTOS) & (set(_header.PROTOS) | set(_header.EVAL_PROTOS))
    assert set(_lib.ALL_PROTOS) == set(_header.PROTOS) | set(_header.EVAL_PROTOS) | set(_header.NOREF_PROTOS)
    assert len(_header.STRUCTS) == 7 and _header.parse(open(_header.NOREF_HEADER_PATH).read())[0] == {}
    lib = _lib.lib()
    assert lib.flair_abi_version() >= 19
    for name, (restype, params) in _header.NOREF_PROTOS.items():
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and restype is ctypes.c_int and params[-1].name == "stream", name
        assert list(f.argtypes) == [p.ctype for p in params], name
    i, d, v = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    assert [tuple(p) for p in _header.NOREF_PROTOS["flair_niqe_luma"][1]] == [
        ("u8", v, "uint8_t"), ("N", i, None), ("H", i, None), ("W", i, None), ("y1", v, "int"), ("y2", v, "int"), ("stream", v, None)]
    assert [tuple(p) for p in _header.NOREF_PROTOS["flair_niqe_moments"][1]] == [
        ("y", v, "int"), ("N", i, None), ("Hc", i, None), ("Wc", i, None), ("block", i, None), ("inv_scale", d, None),
        ("window", v, "double"), ("out", v, "double"), ("mscn", v, "double"), ("stream", v, None)]
    header = open(_header.NOREF_HEADER_PATH).read()
    src = open(os.path.join(ROOT, "flair_amd", "csrc", "niqe.hip")).read()
    from flair_amd import ops
    assert int(re.search(r"#define FLAIR_NIQE_BLOCK (\d+)", header).group(1)) == ops.NIQE_BLOCK == R.BLOCK
    assert "atomic" not in src and "float " not in re.sub(r"//.*", "", src)               # float64 and integers only
    assert re.search(r"(?m)^niqe\.o: CXXFLAGS \+= -ffp-contract=off$", open(os.path.join(ROOT, "flair_amd", "csrc", "Makefile")).read())


def _device_tensor(dtype):
    import types
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_types_the_new_entries():
    from flair_amd import _lib
    call = _lib.call
    i32, f64, u8 = _device_tensor(torch.int32), _device_tensor(torch.float64), _device_tensor(torch.uint8)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_niqe_luma(torch.zeros(3, dtype=torch.uint8), 1, 96, 192, i32, i32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_niqe_luma: y2 must be int32, got float64$"):
        call.flair_niqe_luma(u8, 1, 96, 192, i32, f64)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_niqe_moments: window must be float64, got int32$"):
        call.flair_niqe_moments(i32, 1, 96, 192, 96, 1.0, i32, f64, None)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_niqe_moments: mscn must be float64, got uint8$"):
        call.flair_niqe_moments(i32, 1, 96, 192, 96, 1.0, f64, f64, u8)
    with pytest.raises(TypeError, match="flair_niqe_moments takes 9 arguments"):
        call.flair_niqe_moments(i32, 1)


def test_entries_refuse_before_any_launch(monkeypatch):
    """Every refusal of the two entries: status -1 and the entry's message, on a machine without a GPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    P, odd4, odd2 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4), ctypes.c_void_p((1 << 20) + 2)

    def refused(name, args, what):
        rc = getattr(lib, name)(*args, None)
        msg = lib.flair_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)

    luma = lambda **k: tuple({**dict(u8=P, N=1, H=96, W=192, y1=P, y2=P), **k}.values())  # noqa: E731
    for k, what in [(dict(u8=None), "null pointer"), (dict(y1=None), "null pointer"), (dict(y2=None), "null pointer"), (dict(N=0), "N = 0"),
                    (dict(H=0), "H = 0"), (dict(W=-3), "W = -3"), (dict(H=95), "frames of 95x192 hold no 96x96 block"),
                    (dict(W=64), "hold no 96x96 block"), (dict(y1=odd2), "4-byte aligned"), (dict(y2=odd2), "4-byte aligned"),
                    (dict(N=1 << 30, H=960, W=960), "exceed one launch")]:
        refused("flair_niqe_luma", luma(**k), what)
    mom = lambda **k: tuple({**dict(y=P, N=1, Hc=96, Wc=192, block=96, inv_scale=ctypes.c_double(1.0), window=P, out=P, mscn=None), **k}.values())  # noqa: E731
    for k, what in [(dict(y=None), "null pointer"), (dict(window=None), "null pointer"), (dict(out=None), "null pointer"), (dict(N=0), "N = 0"),
                    (dict(Hc=0), "Hc = 0"), (dict(Wc=0), "Wc = 0"), (dict(block=32), "block = 32"), (dict(block=0), "block = 0"),
                    (dict(Hc=100), "the plane of 100x192 is not made of 96x96 blocks"), (dict(block=48, Wc=200), "is not made of 48x48 blocks"),
                    (dict(inv_scale=ctypes.c_double(0.5)), "inv_scale = 0.5"), (dict(y=odd2), "y = "), (dict(window=odd4), "8-byte aligned"),
                    (dict(out=odd4), "8-byte aligned"), (dict(mscn=odd4), "8-byte aligned"),
                    (dict(N=1 << 30, Hc=960, Wc=960, block=48), "exceed one launch")]:
        refused("flair_niqe_moments", mom(**k), what)
    monkeypatch.setattr(_lib, "stream", lambda: None)
    i32, f64 = _device_tensor(torch.int32), _device_tensor(torch.float64)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_niqe_moments failed \(status -1\): flair_niqe_moments: block = 64"):
        _lib.call.flair_niqe_moments(i32, 1, 192, 192, 64, 1.0, f64, f64, None)


def test_ops_wrappers_refuse_wrong_tensors():
    from flair_amd import ops
    u8 = torch.zeros(1, 96, 192, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\(N, H, W, 3\) frames"):
        ops.niqe_luma(u8[..., :2])
    with pytest.raises(ValueError, match="uint8 frames"):
        ops.niqe_luma(u8.float())
    with pytest.raises(ValueError, match="dense"):
        ops.niqe_luma(u8.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match="frames of 95x192 hold no 96x96 block"):
        ops.niqe_luma(u8[:, :95].contiguous())
    with pytest.raises(ValueError, match=r"y2 is a dense \(1, 48, 96\) int32 tensor"):
        ops.niqe_luma(u8, y2=torch.zeros(1, 48, 95, dtype=torch.int32))
    y, win = torch.zeros(1, 96, 192, dtype=torch.int32), torch.zeros(7, 7, dtype=torch.float64)
    with pytest.raises(ValueError, match="y is a dense"):
        ops.niqe_moments(y.double(), 96, 1.0, win)
    with pytest.raises(ValueError, match="block = 32"):
        ops.niqe_moments(y, 32, 1.0, win)
    with pytest.raises(ValueError, match="not made of 96x96 blocks"):
        ops.niqe_moments(y[:, :, :100].contiguous(), 96, 1.0, win)
    with pytest.raises(ValueError, match=r"window is a dense \(7, 7\) float64"):
        ops.niqe_moments(y, 96, 1.0, win.float())
    with pytest.raises(ValueError, match=r"out is a dense \(1, 2, 5, 5\)"):
        ops.niqe_moments(y, 96, 1.0, win, out=torch.zeros(1, 2, 25, dtype=torch.float64))
    with pytest.raises(ValueError, match="mscn is a dense"):
        ops.niqe_moments(y, 96, 1.0, win, mscn=torch.zeros(1, 96, 192))


# ------------------------------------------------------------------------------------------- the loader
def test_loader_reads_and_refuses(tmp_path):
    from flair_amd import niqe as Q
    m = Q.load_niqe(write_params(tmp_path / "ok.npz"), "cpu")
    assert np.array_equal(m.mu, PARAMS[0]) and np.array_equal(m.cov, PARAMS[1]) and np.array_equal(m.window_host, PARAMS[2])
    assert m.window.dtype == torch.float64 and tuple(m.window.shape) == (7, 7)
    with pytest.raises(FileNotFoundError, match="nope.npz not found"):
        Q.load_niqe(str(tmp_path / "nope.npz"), "cpu")
    np.savez(tmp_path / "short.npz", mu_pris_param=PARAMS[0], gaussian_window=PARAMS[2])
    with pytest.raises(ValueError, match=r"missing keys: cov_pris_param \(holds mu_pris_param, gaussian_window\)"):
        Q.load_niqe(str(tmp_path / "short.npz"), "cpu")
    with pytest.raises(ValueError, match=r"mu_pris_param has shape \(1, 35\), not \(36,\)"):
        Q.load_niqe(write_params(tmp_path / "a.npz", mu=np.zeros((1, 35))), "cpu")
    with pytest.raises(ValueError, match=r"cov_pris_param has shape \(36, 35\)"):
        Q.load_niqe(write_params(tmp_path / "b.npz", cov=np.zeros((36, 35))), "cpu")
    with pytest.raises(ValueError, match=r"gaussian_window has shape \(5, 5\)"):
        Q.load_niqe(write_params(tmp_path / "c.npz", window=np.full((5, 5), 0.04)), "cpu")
    skew = PARAMS[2].copy()
    skew[0, 1] += 1e-9
    skew[3, 3] -= 1e-9
    with pytest.raises(ValueError, match="not symmetric under both flips and transposition"):
        Q.load_niqe(write_params(tmp_path / "d.npz", window=skew), "cpu")
    with pytest.raises(ValueError, match="not to 1 within 1e-12"):
        Q.load_niqe(write_params(tmp_path / "e.npz", window=PARAMS[2] * (1 + 1e-11)), "cpu")
    with pytest.raises(ValueError, match="finite"):
        Q.load_niqe(write_params(tmp_path / "f.npz", cov=np.full((36, 36), np.nan)), "cpu")
    (tmp_path / "g.npz").write_bytes(b"not a zip")
    with pytest.raises(ValueError, match="not an .npz file"):
        Q.load_niqe(str(tmp_path / "g.npz"), "cpu")
    Q.check_size(96, 192)
    Q.check_size(200, 100)
    with pytest.raises(ValueError, match=r"frames are 191x191, which holds 1 blocks of 96x96; the score needs at least two"):
        Q.check_size(191, 191)
    with pytest.raises(ValueError, match="holds 0 blocks"):
        m(torch.zeros(1, 64, 512, 3, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------- command line
def test_command_line_parses_and_refuses(tmp_path):
    from flair_amd.__main__ import lpips_of, main, make_parser, niqe_of
    ap = make_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["evaluate", "only_one"])
    e = ap.parse_args(["evaluate", "out", "truth"])
    assert e.niqe is None and niqe_of(e, "evaluate") is None
    assert ap.parse_args(["evaluate", "out", "truth", "--niqe", "p.npz"]).niqe == "p.npz"
    assert ap.parse_args(["interpolate", "in", "out", "--factor", "2", "--niqe", "p.npz", "--json", "j"]).niqe == "p.npz"
    assert not hasattr(ap.parse_args(["jpeg-demo"]), "niqe")
    q = ap.parse_args(["niqe", "frames", "--params", "p.npz", "--json", "j.json", "--device", "cuda:1"])
    assert (q.frames_dir, q.params, q.json, q.device) == ("frames", "p.npz", "j.json", "cuda:1")
    (tmp_path / "in").mkdir()
    with pytest.raises(SystemExit, match="niqe: --params FILE is required"):
        main(["niqe", str(tmp_path / "in")])
    with pytest.raises(SystemExit, match=r"niqe: --params .*nope\.npz is not a file"):
        main(["niqe", str(tmp_path / "in"), "--params", str(tmp_path / "nope.npz")])
    params = write_params(tmp_path / "p.npz")
    with pytest.raises(SystemExit, match="niqe: .*missing is not a directory"):
        main(["niqe", str(tmp_path / "missing"), "--params", params])
    with pytest.raises(SystemExit, match=r"evaluate: --niqe .*nope\.npz is not a file"):
        main(["evaluate", "out", "truth", "--niqe", str(tmp_path / "nope.npz")])
    # restore --niqe stands without --ground-truth: the option is accepted, and its only refusal is about its own file
    r = ap.parse_args(["restore", "gaussian", str(tmp_path / "in"), str(tmp_path / "out"), "--niqe", params])
    assert r.ground_truth is None and lpips_of(r, "restore") is None and niqe_of(r, "restore") == params
    with pytest.raises(SystemExit, match=r"restore: --niqe .*nope\.npz is not a file"):
        main(["restore", "gaussian", str(tmp_path / "in"), str(tmp_path / "out"), "--niqe", str(tmp_path / "nope.npz")])
    for i in range(2):
        png(tmp_path / "in" / f"{i}.png", 32, 32)
    from flair_amd.__main__ import interpolate_of
    with pytest.raises(SystemExit, match="interpolate: --json writes the scores of --ground-truth DIR"):
        interpolate_of(ap.parse_args(["interpolate", str(tmp_path / "in"), "o", "--factor", "2", "--json", "j"]))
    assert len(interpolate_of(ap.parse_args(["interpolate", str(tmp_path / "in"), "o", "--factor", "2", "--json", "j", "--niqe", params]))) == 2
    from flair_amd.__main__ import load_niqe_of
    assert load_niqe_of(None, "cpu", "niqe") is None and load_niqe_of(params, "cpu", "niqe").mu.shape == (36,)
    with pytest.raises(SystemExit, match=r"niqe: .*short\.npz: missing keys: cov_pris_param, gaussian_window"):
        np.savez(tmp_path / "short.npz", mu_pris_param=PARAMS[0])
        load_niqe_of(str(tmp_path / "short.npz"), "cpu", "niqe")


# ------------------------------------------------------------------------------------------- reports
class Scorer:
    """Stands in for NIQE: the second frame of every call has no score."""

    def __call__(self, u8):
        return [4.25 + 0.5 * i if i != 1 else math.nan for i in range(u8.shape[0])]


def _dirs(tmp_path, n=3, h=96, w=192):
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        for i in range(n):
            png(tmp_path / d / f"{i:04d}.png", h, w, value=i)


def test_evaluate_report_with_and_without_a_scorer(tmp_path, monkeypatch):
    from flair_amd import metrics
    rows = dict(psnr=[30.0, 31.0, 32.0], ssim=[0.5, 0.75, 1.0], sse=[3, 2, 1])
    monkeypatch.setattr(metrics, "psnr_ssim", lambda a, b: rows)
    _dirs(tmp_path)
    plain = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu")
    assert plain["mean"] == dict(psnr=31.0, ssim=0.75) and set(plain["frames"][0]) == {"name", "psnr", "ssim"}
    assert metrics.format_report(plain)[-1] == "mean of 3 frames  psnr 31.0000  ssim 0.7500"
    res = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", niqe=Scorer())
    assert [f["niqe"] for f in res["frames"]] == [4.25, None, 5.25]
    assert res["mean"] == dict(psnr=31.0, ssim=0.75, niqe=4.75, niqe_frames=2) and res["count"] == 3
    assert metrics.format_report(res) == ["0000.png  psnr 30.0000  ssim 0.5000  niqe 4.2500", "0001.png  psnr 31.0000  ssim 0.7500  niqe n/a",
                                          "0002.png  psnr 32.0000  ssim 1.0000  niqe 5.2500", "mean of 3 frames  psnr 31.0000  ssim 0.7500  niqe 4.7500"]
    text = json.dumps(res)
    assert '"niqe": null' in text and "NaN" not in text and json.loads(text) == res

    class Lpips:
        net = "vgg"

        def __call__(self, a, b):
            return [0.25] * a.shape[0]
    both = metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", lpips=Lpips(), niqe=Scorer())
    assert metrics.format_report(both)[0] == "0000.png  psnr 30.0000  ssim 0.5000  lpips 0.2500  niqe 4.2500"
    assert list(both["mean"]) == ["psnr", "ssim", "lpips", "niqe", "niqe_frames"]
    # too small for two blocks: refused on the file headers, nothing decoded
    png(tmp_path / "a" / "0001.png", 96, 191)
    png(tmp_path / "b" / "0001.png", 96, 191)
    monkeypatch.setattr(metrics.fio, "iter_frame_batches", lambda *a, **k: pytest.fail("decoded before the refusal"))
    with pytest.raises(ValueError, match=r"niqe: evaluate: .*0001\.png are 96x191, which holds 1 blocks"):
        metrics.evaluate_dirs(str(tmp_path / "a"), str(tmp_path / "b"), "cpu", niqe=Scorer())


def test_niqe_command_report_and_json(tmp_path, monkeypatch, capsys):
    from flair_amd import __main__ as cli
    from flair_amd import niqe as Q
    _dirs(tmp_path)
    res = Q.niqe_dir(str(tmp_path / "a"), "cpu", Scorer(), batch=2)            # batches of 2 and 1: the stub's NaN is frame 1 only
    assert res == dict(frames=[dict(name="0000.png", niqe=4.25), dict(name="0001.png", niqe=None), dict(name="0002.png", niqe=4.25)],
                       mean=dict(niqe=4.25, niqe_frames=2), count=3)
    assert Q.format_report(res) == ["0000.png  niqe 4.2500", "0001.png  niqe n/a", "0002.png  niqe 4.2500", "mean of 2 of 3 frames  niqe 4.2500"]
    none = dict(frames=[dict(name="x.png", niqe=None)], mean=Q.mean_of([None]), count=1)
    assert none["mean"] == dict(niqe=None, niqe_frames=0) and Q.format_report(none)[-1] == "mean of 0 of 1 frames  niqe n/a"
    with pytest.raises(ValueError, match="niqe: no frame files in"):
        (tmp_path / "empty").mkdir()
        Q.niqe_dir(str(tmp_path / "empty"), "cpu", Scorer())
    monkeypatch.setattr(cli, "load_niqe_of", lambda path, device, command: Scorer())
    out = tmp_path / "scores.json"
    with torch.enable_grad():                     # main() turns autograd off for the process; keep it to this test
        assert cli.main(["niqe", str(tmp_path / "a"), "--params", write_params(tmp_path / "p.npz"), "--json", str(out), "--device", "cpu"]) == 0
    assert capsys.readouterr().out.splitlines() == ["0000.png  niqe 4.2500", "0001.png  niqe n/a", "0002.png  niqe 5.2500",
                                                    "mean of 2 of 3 frames  niqe 4.7500"]
    assert json.loads(out.read_text()) == dict(frames=[dict(name="0000.png", niqe=4.25), dict(name="0001.png", niqe=None),
                                                       dict(name="0002.png", niqe=5.25)], mean=dict(niqe=4.75, niqe_frames=2), count=3)
    assert '"niqe": null' in out.read_text()
    png(tmp_path / "a" / "0002.png", 100, 100)
    with torch.enable_grad(), pytest.raises(SystemExit, match=r"^niqe: .*0002\.png are 100x100, which holds 1 blocks"):
        cli.main(["niqe", str(tmp_path / "a"), "--params", str(tmp_path / "p.npz"), "--device", "cpu"])
    assert torch.is_grad_enabled()
