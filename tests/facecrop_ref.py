"""The face score's crop of include/flair_facescore.h in numpy int64 on the CPU, written from the header's definition with the
geometry and the weight table of tests/face_ref.py (tap_geometry, cubic_table), the cases the CPU and the GPU tests share, the
mutants that the cases must tell apart, and the entry's refusals.

    position  X = (rint((M1 y + M2) 2^10) + 16 + rint(M0 x 2^10)) >> 5, first tap (X >> 5) - 1, weight row X & 31
    value     S = sum over 4 x 4 taps of s num_x num_y (s = the source byte, or border[c] outside), byte = clamp((S + 2^33) >> 34)
"""
import functools

import numpy as np

from tests import face_ref as F

BORDER = (135, 133, 132)
ONE = 1 << (2 * F.TAB_BITS)                                     # 2^34
MUTANTS = ("swap_xy", "half_away", "floor", "no_clamp", "no_half", "border_zero")
HS, WS = 37, 70                                                 # the source frames of most cases


def crop(src, minv, out_hw, border=BORDER, mutant=None):
    """src (Hs, Ws, 3) uint8 -> dict: value (Hd, Wd, 3) uint8, raw (Hd, Wd, 3) int64 the rounded value before the clamp, S the
    int64 sums, cls the window classes of face_ref.classify, sx, sy, fx, fy."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    Hs, Ws, _ = src.shape
    Hd, Wd = out_hw
    rule = mutant if mutant in ("half_away", "floor") else "half_even"
    sx, sy, fx, fy = F.tap_geometry(minv, Hd, Wd, rule)
    _, num = F.cubic_table()
    wx, wy = (num[fy], num[fx]) if mutant == "swap_xy" else (num[fx], num[fy])          # (Hd, Wd, 4) each
    cv = np.zeros(3, dtype=np.int64) if mutant == "border_zero" else np.array([int(v) for v in border], dtype=np.int64)
    s64 = src.astype(np.int64)
    S = np.zeros((Hd, Wd, 3), dtype=np.int64)
    for r in range(4):
        for c in range(4):
            yi, xi = sy + r, sx + c
            ok = (yi >= 0) & (yi < Hs) & (xi >= 0) & (xi < Ws)
            s = np.where(ok[..., None], s64[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)], cv)
            S += s * (wx[..., c] * wy[..., r])[..., None]
    assert np.abs(S).max() <= 255 * 121 * ONE // 64                               # 255 (11/8)^2 2^34
    raw = (S + (0 if mutant == "no_half" else ONE // 2)) >> (2 * F.TAB_BITS)       # numpy's >> on int64 is the floor shift
    value = (raw & 255 if mutant == "no_clamp" else np.clip(raw, 0, 255)).astype(np.uint8)
    return dict(value=value, raw=raw, S=S, cls=F.classify(sx, sy, Hs, Ws), sx=sx, sy=sy, fx=fx, fy=fy)


def crop_float64(src, minv, out_hw, border=BORDER):
    """floor(v + 0.5), clamped, of the FLOAT64 sum v = sum s w_x w_y with w = num / 2^17: every term is a multiple of 2^-34
    below 2^9 in magnitude, so the sum is exact in float64 in any order -> (Hd, Wd, 3) uint8."""
    src = np.asarray(src)
    Hs, Ws, _ = src.shape
    Hd, Wd = out_hw
    sx, sy, fx, fy = F.tap_geometry(minv, Hd, Wd)
    _, num = F.cubic_table()
    w = num.astype(np.float64) / float(1 << F.TAB_BITS)
    wx, wy = w[fx], w[fy]
    cv = np.array(border, dtype=np.float64)
    v = np.zeros((Hd, Wd, 3), dtype=np.float64)
    for r in range(4):
        for c in range(4):
            yi, xi = sy + r, sx + c
            ok = (yi >= 0) & (yi < Hs) & (xi >= 0) & (xi < Ws)
            s = np.where(ok[..., None], src[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)].astype(np.float64), cv)
            v += s * (wx[..., c] * wy[..., r])[..., None]
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def crop_batch(frames, minv, src_index, out_hw, border=BORDER):
    """frames (N, Hs, Ws, 3) uint8, minv (K, 6), src_index K ints -> (K, Hd, Wd, 3) uint8."""
    minv = np.asarray(minv, dtype=np.float64).reshape(-1, 6)
    out = np.empty((len(minv),) + tuple(out_hw) + (3,), dtype=np.uint8)
    for k, (m, i) in enumerate(zip(minv, src_index)):
        out[k] = crop(frames[int(i)], m, out_hw, border)["value"]
    return out


def corners_outside(minv, out_hw, Hs, Ws):
    """The `clipped` flag of the face score: a corner of the crop maps outside [0, Ws - 1] x [0, Hs - 1]."""
    m = np.asarray(minv, dtype=np.float64).reshape(6)
    Hd, Wd = out_hw
    for x in (0, Wd - 1):
        for y in (0, Hd - 1):
            px, py = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
            if not (0 <= px <= Ws - 1 and 0 <= py <= Hs - 1):
                return True
    return False


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def frames(N=2, Hs=HS, Ws=WS, seed=11):
    """Random bytes (N, Hs, Ws, 3), read-only; frames(...)[0] of the default is the source of the single-frame cases."""
    a = np.random.default_rng(seed).integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def step_source():
    """A vertical 0 | 255 step between columns 34 and 35 of a 37 x 70 frame."""
    s = np.zeros((HS, WS, 3), dtype=np.uint8)
    s[:, 35:] = 255
    s.setflags(write=False)
    return s


def rotation(theta=0.3, scale=1.7, tx=-6.3, ty=-9.1):
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([c, -s, tx, s, c, ty], dtype=np.float64)


def _src(name):
    if name == "step":
        return step_source()
    if name.startswith("tiny"):
        h, w = {"tiny1x1": (1, 1), "tiny3x5": (3, 5)}[name]
        return frames(1, h, w, seed=5)[0]
    if name == "7x9":
        return frames(1, 7, 9, seed=3)[0]
    return frames()[0]


# name -> (source name, (Hd, Wd), dst -> src matrix)
CASES = {
    "copy": ("random", (16, 24), np.array([1, 0, 5, 0, 1, 3], dtype=np.float64)),
    "quarter-x": ("random", (16, 24), np.array([1, 0, 5.25, 0, 1, 3], dtype=np.float64)),
    "quarter-y": ("random", (16, 24), np.array([1, 0, 5, 0, 1, 3.75], dtype=np.float64)),
    "quarter-xy": ("random", (16, 24), np.array([1, 0, -1.25, 0, 1, 30.5], dtype=np.float64)),
    "step": ("step", (16, 24), np.array([1, 0, 20.5, 0, 1, 3], dtype=np.float64)),
    "rotation": ("random", (40, 24), rotation()),               # 40 rows of 24: a non-square destination, half a wave wide
    "outside": ("random", (9, 13), np.array([1, 0, 200, 0, 1, -300], dtype=np.float64)),
    "src1x1": ("tiny1x1", (6, 7), np.array([0.5, 0, -1.25, 0, 0.5, -1.5], dtype=np.float64)),
    "src3x5": ("tiny3x5", (12, 16), np.array([0.5, 0, -1.25, 0, 0.25, -0.5], dtype=np.float64)),
    "dst1x1": ("random", (1, 1), np.array([1, 0, 7.5, 0, 1, 9.25], dtype=np.float64)),
}
# the rounding-rule cases of face_ref (ties in the position) on a 7 x 9 source of random bytes
for _name, (_hw, _out, _m, _) in F.ROUNDING_CASES.items():
    assert _hw == (7, 9)
    CASES[_name] = ("7x9", _out, np.asarray(_m, dtype=np.float64).reshape(6))
ROTATION_CLASSES = (566, 307, 87)                               # outside, inner, partial windows of "rotation"
STEP_RANGE = (-24, 279)                                         # the unclamped values of "step"


@functools.lru_cache(maxsize=None)
def case(name, mutant=None):
    """The reference crop of a named case (of a mutant of the definition), computed once and read-only."""
    got = crop(case_source(name), CASES[name][2], CASES[name][1], BORDER, mutant)
    for v in got.values():
        v.setflags(write=False)
    return got


def case_source(name):
    return _src(CASES[name][0])


# four faces from two frames through src_index: three from frame 1, one from frame 0
MULTI_MINV = np.stack([rotation(0.2, 1.1, 3.0, -2.0), np.array([1, 0, 5.25, 0, 1, 3.5]), rotation(-0.4, 0.8, 20.0, 9.0),
                       np.array([0.75, 0, -3.0, 0, 0.75, 2.0])])
MULTI_INDEX = (1, 1, 0, 1)
MULTI_HW = (21, 70)                                             # two column groups of 64, a ragged last group of rows


# ------------------------------------------------------------------------------------------- the entry's refusals
def entry_refusals():
    """[(entry, argument tuple without the stream, text the message must hold)]: every refusal include/flair_facescore.h
    lists, on pointers that are never dereferenced (a refusal comes before any launch; border is a real host array)."""
    import ctypes
    P, Q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    odd4 = ctypes.c_void_p((1 << 20) + 4)
    odd2 = ctypes.c_void_p((1 << 20) + 2)
    bd = (ctypes.c_uint8 * 3)(*BORDER)
    base = dict(a=P, b=None, Nsrc=2, Hs=37, Ws=70, minv=P, src_index=P, K=3, Hd=16, Wd=24, border=bd, out_a=Q, out_b=None)
    arg = lambda **k: tuple({**base, **k}.values())  # noqa: E731
    inside = ctypes.c_void_p((1 << 20) + 2 * 37 * 70 * 3 - 1)                       # the last byte of a
    before = ctypes.c_void_p((1 << 20) - 3 * 16 * 24 * 3 + 1)                       # out's last byte is a's first
    R = ctypes.c_void_p(1 << 29)
    cases = [(dict(a=None), "null pointer"), (dict(border=None), "null pointer"), (dict(minv=None), "null pointer"),
             (dict(src_index=None), "null pointer"), (dict(out_a=None), "null pointer"),
             (dict(b=R), "come together or not at all"), (dict(out_b=R), "come together or not at all"),
             (dict(Nsrc=0), "Nsrc = 0"), (dict(Hs=0), "Hs = 0"), (dict(Ws=-2), "Ws = -2"), (dict(Hd=0), "Hd = 0"), (dict(Wd=0), "Wd = 0"),
             (dict(K=-1), "K = -1"), (dict(minv=odd4), "8-byte aligned"), (dict(src_index=odd2), "4-byte aligned"),
             (dict(K=1 << 30, Hd=64), "exceed one launch"), (dict(K=0x7fffffff, Hd=0x7fffffff, Wd=0x7fffffff), "exceed one launch"),
             (dict(Nsrc=0x7fffffff, Hs=0x7fffffff, Ws=0x7fffffff), "exceed 64-bit offsets"),
             (dict(out_a=P), "out overlaps a source"), (dict(out_a=inside), "out overlaps a source"), (dict(out_a=before), "out overlaps a source"),
             (dict(b=R, out_b=R), "out overlaps a source"), (dict(b=R, out_b=inside), "out overlaps a source"),
             (dict(b=R, out_b=Q, out_a=R), "out overlaps a source")]
    return [("flair_face_crop_u8", arg(**k), what) for k, what in cases]


def entry_accepts_without_launch():
    """Argument tuples the entry takes without enqueueing anything: K = 0, with or without the pointers K > 0 needs."""
    import ctypes
    P = ctypes.c_void_p(1 << 20)
    bd = (ctypes.c_uint8 * 3)(*BORDER)
    return [(P, None, 2, 37, 70, None, None, 0, 16, 24, bd, None, None), (P, None, 2, 37, 70, P, P, 0, 16, 24, bd, P, None)]


def assert_refused(lib, name, args, what):
    rc = getattr(lib, name)(*args, None)
    msg = lib.flair_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)
