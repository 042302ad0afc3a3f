"""References for the kernels of csrc/face.hip, written from the definition that face.hip's comments state (OpenCV's
warpAffine(INTER_CUBIC, BORDER_CONSTANT) and separable reflect-101 blur), not from oracle/facewarp.py: nothing here
imports the oracle, so a misreading shared by kernel and oracle shows as a disagreement with this file
(tests/test_face_exact_cpu.py compares the two; tests/test_gpu_face_exact.py compares the kernels with this file).

Warp.  A destination pixel (x, y) under the dst -> src matrix M = (M0 .. M5) has the fixed-point source position

    X = (rint((M1 y + M2) 2^10) + 16 + rint(M0 x 2^10)) >> 5         (floor shift; Y likewise with M3, M4, M5)

in 1/32 pixel: (X >> 5) - 1 is the first of four taps, X & 31 the row of the weight table.  rint rounds half to even
and rounds the two parts separately; `rule` swaps in three other rules, which exist only so that the CPU tests can show
that the exact cases tell them apart.  The three classes of a window: OUTSIDE (no tap in the image: the border value),
INNER (all 16 in: sum S w), PARTIAL (cv + sum over the taps inside of (S - cv) w).  The 1-D weights are the a = -0.75
cubic evaluated in f32, the 2-D weight is their f32 product; both roundings belong to the specification.  All 128 table
entries are dyadic rationals (multiples of 2^-17) that f32 holds exactly, which cubic_table() asserts.

Blur.  lut[clamp(label)] -> `repeats` separable passes with reflect-101 indexing -> the `edge` outermost pixels zeroed
-> / div.  blur_fsum sums every pass with math.fsum; blur_numpy is the float64 restatement in the order face.hip
documents; blur_exact evaluates dyadic kernels on integers in integer arithmetic.
"""
import functools
import math
from fractions import Fraction

import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53
OUTSIDE, INNER, PARTIAL = 0, 1, 2
CLASS_NAMES = ("outside", "inner", "partial")
RULES = ("half_even", "half_away", "floor", "sum")
TAB_BITS = 17                                                     # every table entry is a multiple of 2^-17


# ------------------------------------------------------------------------------------------------------------ weights
@functools.lru_cache(maxsize=None)
def cubic_table():
    """-> (tab32 (32, 4) float32, num (32, 4) int64 with tab32 = num / 2^17).  The exact rational value of every entry
    of the a = -0.75 table is a multiple of 2^-17, equals its f32 value and equals the step-by-step f32 evaluation."""
    A = Fraction(-3, 4)
    exact = []
    for i in range(32):
        x = Fraction(i, 32)
        c0 = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A
        c1 = ((A + 2) * x - (A + 3)) * x * x + 1
        c2 = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1
        exact.append([c0, c1, c2, 1 - c0 - c1 - c2])
    f = np.float32
    x = np.arange(32, dtype=np.float32) * f(1.0 / 32)
    a = f(-0.75)
    s0 = ((a * (x + f(1)) - f(5) * a) * (x + f(1)) + f(8) * a) * (x + f(1)) - f(4) * a
    s1 = ((a + f(2)) * x - (a + f(3))) * x * x + f(1)
    s2 = ((a + f(2)) * (f(1) - x) - (a + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
    step = np.stack([s0, s1, s2, f(1) - s0 - s1 - s2], axis=1)
    assert step.dtype == np.float32
    # every intermediate of the three polynomials is exact in f32 (at most 17 significant bits), so an evaluation that
    # fuses a product into the following sum gives the same table
    for i in range(32):
        t = Fraction(i, 32)
        for u, first in ((t + 1, A * (t + 1) - 5 * A), (t, (A + 2) * t - (A + 3)), (1 - t, (A + 2) * (1 - t) - (A + 3))):
            steps = [u, A * u, (A + 2) * u, first, first * u, first * u + 8 * A, (first * u + 8 * A) * u, first * u * u]
            assert all(Fraction(float(np.float32(float(v)))) == v for v in steps), (i, steps)
    num = np.empty((32, 4), dtype=np.int64)
    for i in range(32):
        for k in range(4):
            n = exact[i][k] * (1 << TAB_BITS)
            assert n.denominator == 1 and abs(n.numerator) <= 1 << TAB_BITS, (i, k, exact[i][k])
            assert Fraction(float(np.float32(float(exact[i][k])))) == exact[i][k], (i, k)
            assert Fraction(float(step[i, k])) == exact[i][k], (i, k, step[i, k], exact[i][k])
            num[i, k] = n.numerator
    tab32 = (num.astype(np.float64) / (1 << TAB_BITS)).astype(np.float32)
    assert max(sum(abs(v) for v in row) for row in exact) == Fraction(11, 8)          # the largest absolute row sum
    return tab32, num


# ----------------------------------------------------------------------------------------------------------- geometry
def _round(v, rule):
    if rule in ("half_even", "sum"):
        r = np.rint(v)
    elif rule == "half_away":
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    elif rule == "floor":
        r = np.floor(v)
    else:
        raise ValueError(rule)
    return r.astype(np.int64)


def tap_geometry(minv, Hd, Wd, rule="half_even"):
    """-> sx, sy (first tap), fx, fy (row of the weight table), each (Hd, Wd) int64.  The products and the one sum are
    float64 operations (as written above, two roundings in (M1 y + M2)); everything after the rounding is integer."""
    M = [float(v) for v in np.asarray(minv, dtype=np.float64).reshape(6)]
    xs = np.arange(Wd, dtype=np.float64)[None, :]
    ys = np.arange(Hd, dtype=np.float64)[:, None]
    out = []
    for m0, m1, m2 in ((M[0], M[1], M[2]), (M[3], M[4], M[5])):
        a = (m0 * xs) * 1024.0
        b = (m1 * ys + m2) * 1024.0
        if rule == "sum":
            v = _round(a + b, rule) + 16
        else:
            v = _round(b, rule) + 16 + _round(a, rule)
        v = v >> 5                                                # numpy's >> on int64 is the arithmetic (floor) shift
        first = (v >> 5) - 1
        assert np.abs(first).max() < 32000                        # the 16-bit saturation is out of reach (and out of scope)
        out += [np.broadcast_to(first, (Hd, Wd)), np.broadcast_to(v & 31, (Hd, Wd))]
    return out[0], out[2], out[1], out[3]


def classify(sx, sy, Hs, Ws):
    outside = (sx >= Ws) | (sx + 4 <= 0) | (sy >= Hs) | (sy + 4 <= 0)
    inner = (sx >= 0) & (sx + 3 < Ws) & (sy >= 0) & (sy + 3 < Hs)
    assert not (outside & inner).any()
    return np.where(outside, OUTSIDE, np.where(inner, INNER, PARTIAL))


def class_counts(cls):
    return tuple(int((cls == c).sum()) for c in (OUTSIDE, INNER, PARTIAL))


def partial_sides(cls, sx, sy, Hs, Ws):
    """Counts of partial windows that hang over the left, right, top, bottom edge and over a corner (two edges that meet)."""
    p = cls == PARTIAL
    lr, tb = (sx < 0) | (sx + 4 > Ws), (sy < 0) | (sy + 4 > Hs)
    return dict(left=int((p & (sx < 0)).sum()), right=int((p & (sx + 4 > Ws)).sum()), top=int((p & (sy < 0)).sum()),
                bottom=int((p & (sy + 4 > Hs)).sum()), corner=int((p & lr & tb).sum()))


def _gather(src, sx, sy):
    """src (C, Hs, Ws) -> taps (C, 4, 4, Hd, Wd) (clamped reads) and ok (4, 4, Hd, Wd): the tap lies in the image."""
    C, Hs, Ws = src.shape
    taps = np.empty((C, 4, 4) + sx.shape, dtype=src.dtype)
    ok = np.empty((4, 4) + sx.shape, dtype=bool)
    for r in range(4):
        for c in range(4):
            yi, xi = sy + r, sx + c
            ok[r, c] = (yi >= 0) & (yi < Hs) & (xi >= 0) & (xi < Ws)
            taps[:, r, c] = src[:, np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)]
    return taps, ok


# ------------------------------------------------------------------------------------------------------- sample value
def pre32(v):
    """The input transform of `pre`: clamp((v + 1) / 2, 0, 1) * 255, each step rounded to f32."""
    v = np.asarray(v, dtype=np.float32)
    return (np.clip((v + np.float32(1)) / np.float32(2), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.float32)


def post64(o):
    return np.clip((np.asarray(o, dtype=np.float64) / 255.0 - 0.5) / 0.5, -1.0, 1.0)


def warp_ref64(src, minv, out_hw, border, rule="half_even", pre=False):
    """src (C, Hs, Ws) float32 or float64 -> dict: value (C, Hd, Wd) float64 before `post`, S the magnitude sum
    |cv| + sum |w| |S - cv| (partial), sum |w| |S| (inner), |cv| (outside), cls, sx, sy, fx, fy."""
    src = np.asarray(src)
    if pre:
        src = pre32(src)
    C, Hs, Ws = src.shape
    Hd, Wd = out_hw
    sx, sy, fx, fy = tap_geometry(minv, Hd, Wd, rule)
    cls = classify(sx, sy, Hs, Ws)
    tab32, _ = cubic_table()
    w = (tab32[fy][..., :, None] * tab32[fx][..., None, :])                      # (Hd, Wd, 4, 4), the f32 product
    assert w.dtype == np.float32
    w = np.moveaxis(w, (2, 3), (0, 1)).astype(np.float64)                       # (4, 4, Hd, Wd)
    taps, ok = _gather(src.astype(np.float64), sx, sy)
    cv = np.array([np.float32(border[k]) if k < len(border) else 0.0 for k in range(C)], dtype=np.float64)[:, None, None]
    d = (taps - cv[:, None, None]) * ok
    part = cv + (d * w).sum((1, 2))
    part_S = np.abs(cv) + (np.abs(d) * np.abs(w)).sum((1, 2))
    inn = (taps * w).sum((1, 2))
    inn_S = (np.abs(taps) * np.abs(w)).sum((1, 2))
    full = np.broadcast_to(cv, part.shape)
    value = np.where(cls == OUTSIDE, full, np.where(cls == INNER, inn, part))
    S = np.where(cls == OUTSIDE, np.abs(full), np.where(cls == INNER, inn_S, part_S))
    return dict(value=value, S=S, cls=cls, sx=sx, sy=sy, fx=fx, fy=fy)


def warp_exact(src, minv, out_hw, border, rule="half_even"):
    """The same on integer data in integer arithmetic: src (C, Hs, Ws) integers, border integers.  The 2-D weight is the
    integer product of the table numerators over 2^34.  Asserts what makes the one correct f32 (and f64) answer the
    exact value in ANY summation order: the f32 product of the two weights is exact, and every partial sum -- bounded
    by |cv| + sum |w| |term| -- is a multiple of a power of two that f32 holds.  -> the dict of warp_ref64, value exact."""
    src = np.asarray(src)
    assert np.array_equal(src, np.round(src)) and all(float(b) == int(b) for b in border)
    src = src.astype(np.int64)
    C, Hs, Ws = src.shape
    Hd, Wd = out_hw
    sx, sy, fx, fy = tap_geometry(minv, Hd, Wd, rule)
    cls = classify(sx, sy, Hs, Ws)
    tab32, num = cubic_table()
    wn = num[fy][..., :, None] * num[fx][..., None, :]                           # numerators over 2^34
    w32 = tab32[fy][..., :, None] * tab32[fx][..., None, :]
    assert np.array_equal(w32.astype(np.float64) * 2.0 ** (2 * TAB_BITS), wn.astype(np.float64)), "an f32 weight product rounds"
    wn = np.moveaxis(wn, (2, 3), (0, 1))
    taps, ok = _gather(src, sx, sy)
    cv = np.array([int(border[k]) if k < len(border) else 0 for k in range(C)], dtype=np.int64)[:, None, None]
    d = (taps - cv[:, None, None]) * ok
    one = 1 << (2 * TAB_BITS)
    part = cv * one + (d * wn).sum((1, 2))
    inn = (taps * wn).sum((1, 2))
    full = np.broadcast_to(cv * one, part.shape)
    n = np.where(cls == OUTSIDE, full, np.where(cls == INNER, inn, part))
    mag = np.where(cls == OUTSIDE, np.abs(full), np.where(cls == INNER, (np.abs(taps) * np.abs(wn)).sum((1, 2)),
                                                          np.abs(cv) * one + (np.abs(d) * np.abs(wn)).sum((1, 2))))
    # every term and partial sum is a multiple of g = 2^tz / 2^34 (tz: the trailing zeros shared by the pixel's 16
    # weight numerators) and at most mag in magnitude: exact in f32 when mag / g < 2^24
    g = np.bitwise_or.reduce(np.bitwise_or.reduce(np.abs(wn), axis=0), axis=0)
    g = np.where(g == 0, one, g & -g)
    need = np.where(cls == OUTSIDE, 0, mag // g)
    assert need.max() < 1 << 24, f"partial sums need {int(need.max()).bit_length()} bits: not exact in f32"
    value = n.astype(np.float64) / one
    assert np.array_equal(value.astype(np.float32).astype(np.float64), value)    # representable in f32, hence in f64
    return dict(value=value, S=mag.astype(np.float64) / one, cls=cls, sx=sx, sy=sy, fx=fx, fy=fy)


def describe(ref, idx):
    """The class and tap position of output element idx = (..., y, x), for a failure message."""
    y, x = idx[-2], idx[-1]
    return (f"{CLASS_NAMES[int(ref['cls'][y, x])]} window, first tap (x {int(ref['sx'][y, x])}, y {int(ref['sy'][y, x])}), "
            f"fraction (x {int(ref['fx'][y, x])}/32, y {int(ref['fy'][y, x])}/32)")


# --------------------------------------------------------------------------------------------------------- warp cases
def _m(*v):
    return np.array(v, dtype=np.float64).reshape(2, 3)


QUARTER = {"scale": _m(0.25, 0, -1.75, 0, 0.5, -2.25), "turn": _m(0, -0.25, 7.5, 0.5, 0, -3), "shift": _m(1, 0, -2.5, 0, 1, 1.25)}
ALL3 = (OUTSIDE, INNER, PARTIAL)
EDGE = (OUTSIDE, PARTIAL)
# name -> (Hs, Ws), (Hd, Wd), dst -> src matrix, the classes the case reaches with at least 20 pixels
EXACT_CASES = {
    "7x9-scale": ((7, 9), (40, 48), QUARTER["scale"], ALL3),
    "7x9-turn": ((7, 9), (40, 48), QUARTER["turn"], ALL3),
    "7x9-shift": ((7, 9), (40, 48), QUARTER["shift"], ALL3),
    "1x9-scale": ((1, 9), (40, 48), QUARTER["scale"], EDGE),
    "9x2-turn": ((9, 2), (40, 48), QUARTER["turn"], EDGE),
    "3x3-scale": ((3, 3), (40, 48), QUARTER["scale"], EDGE),
    "4x4-scale": ((4, 4), (40, 48), QUARTER["scale"], EDGE),     # 4 x 4 is the smallest source with an inner window: 8 here
}


def _tie(n):
    return (2 * n + 1) / 2048.0                                  # times 2^10: n + 0.5


# Rounding-rule cases: one coordinate sits on an integer pixel (its weights are 0, 1, 0, 0), the other carries scaled
# entries that land on n + 0.5.  With one weight vector in {0, 1} the products are exact at every fraction.
#   n = -17: -16.5 -> -16 (half-even), -17 (half-away and floor);  -16 + 16 = 0 -> pixel 0, -17 + 16 = -1 -> pixel -1/32
#   n = 15:   15.5 ->  16 (half-even and half-away), 15 (floor);    16 + 16 = 32 -> 1/32, 15 + 16 = 31 -> 0
#   M0 = 1 + 2^-11 makes M0 x 2^10 = 1024 x + x / 2, a tie at odd x; with M2 2^10 = m + 0.5 and (x - 1) / 2 and m both
#   odd, rint(a) + rint(b) = a + b + 1; (x - 1) / 2 + m = 14 mod 32 puts that step across a 1/32-pixel boundary (x = 3)
ROUNDING_CASES = {
    "tie-x-neg": ((7, 9), (12, 16), _m(1, 0, _tie(-17), 0, 1, 0), EDGE),
    "tie-x-pos": ((7, 9), (12, 16), _m(1, 0, _tie(15), 0, 1, -1), EDGE),
    "tie-y-neg": ((7, 9), (12, 16), _m(1, 0, -1, 0, 1, _tie(-17)), EDGE),
    "tie-y-pos": ((7, 9), (12, 16), _m(1, 0, -2, 0, 1, _tie(15)), EDGE),
    "parts-x-pos": ((7, 9), (12, 16), _m(1 + 2.0 ** -11, 0, _tie(13), 0, 1, 0), EDGE),
    "parts-x-neg": ((7, 9), (12, 16), _m(1 + 2.0 ** -11, 0, _tie(-19), 0, 1, -1), EDGE),
    "parts-y-pos": ((7, 9), (12, 16), _m(1, 0, 0, 1 + 2.0 ** -11, 1, _tie(13)), EDGE),
}
WARP_CASES = dict(EXACT_CASES, **ROUNDING_CASES)
# 7x9-shift moves the source down by 1.25 pixels: no window hangs over its top edge (the other cases cover that edge)
SIDES_NOT_REACHED = {"7x9-shift": ("top",)}
BORDER = (37, 41, 43, 47)                                       # distinct integers, none of them a pixel value


def int_source(n, C, Hs, Ws, seed):
    """(n, C, Hs, Ws) integers in [0, 31] as int64; the four corners of every plane hold 0, 31, 31, 0."""
    s = np.random.default_rng(seed).integers(0, 32, (n, C, Hs, Ws))
    s[..., 0, 0] = 0
    s[..., 0, -1] = 31
    s[..., -1, 0] = 31
    s[..., -1, -1] = 0
    return s.astype(np.int64)


def similarity(scale, theta, tx, ty):
    c, s = scale * math.cos(theta), scale * math.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


# src -> dst similarity transforms of a 23 x 37 source into a 45 x 61 output (inverted by the caller); the last one
# leaves the face partly outside the source
RANDOM_SRC, RANDOM_DST = (23, 37), (45, 61)
RANDOM_MATS = [similarity(1.45, 0.08, 3.7, 5.2), similarity(2.1, -0.21, -9.3, 6.4), similarity(0.93, 0.3, 14.0, -3.5),
               similarity(1.3, -0.5, -22.6, 18.1)]


def invert(M):
    """The dst -> src matrix of a src -> dst one, in float64 (host glue of the tests; the kernels take the result)."""
    M = np.asarray(M, dtype=np.float64)
    D = 1.0 / (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
    a11, a22, a12, a21 = M[1, 1] * D, M[0, 0] * D, -M[0, 1] * D, -M[1, 0] * D
    return np.array([[a11, a12, -a11 * M[0, 2] - a12 * M[1, 2]], [a21, a22, -a21 * M[0, 2] - a22 * M[1, 2]]])


# --------------------------------------------------------------------------------------------------------------- blur
def reflect101(i, n):
    """-> (index, number of reflections): reflect without repeating the edge pixel, as often as needed."""
    k = 0
    if n == 1:
        return 0, 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
        k += 1
    return i, k


def reflect_table(n, r):
    """idx (n + 2 r,) the source index of positions -r .. n + r - 1, and the largest number of reflections."""
    t = [reflect101(i, n) for i in range(-r, n + r)]
    return np.array([a for a, _ in t], dtype=np.int64), max(b for _, b in t)


def lut_lookup(labels, lut):
    lut = np.asarray(lut)
    return lut[np.clip(np.asarray(labels, dtype=np.int64), 0, len(lut) - 1)]


def _zero_edge(a, edge):
    if edge > 0:
        a[..., :edge, :] = 0
        a[..., -edge:, :] = 0
        a[..., :, :edge] = 0
        a[..., :, -edge:] = 0
    return a


def blur_numpy(labels, lut, kern, repeats, edge, div):
    """Float64 restatement in the order face.hip documents: rows sum_k k[k] S[i + k] in ascending k, columns
    k[r] S[c] + sum_{j >= 1} k[r + j] (S[c + j] + S[c - j]).  labels (N, H, W) -> (N, H, W) float64."""
    v = lut_lookup(labels, np.asarray(lut, dtype=np.float64)).astype(np.float64)
    N, H, W = v.shape
    k = np.asarray(kern, dtype=np.float64)
    r = len(k) // 2
    ix, _ = reflect_table(W, r)
    iy, _ = reflect_table(H, r)
    for _ in range(repeats):
        P = v[:, :, ix]
        acc = k[0] * P[:, :, 0:W]
        for j in range(1, len(k)):
            acc = acc + k[j] * P[:, :, j:j + W]
        Q = acc[:, iy, :]
        v = k[r] * Q[:, r:r + H]
        for j in range(1, r + 1):
            v = v + k[r + j] * (Q[:, r + j:r + j + H] + Q[:, r - j:r - j + H])
    return _zero_edge(v.copy(), edge) / div


@functools.lru_cache(maxsize=None)
def _blur_fsum(labels_key, shape, lut, kern, repeats, edge, div):
    labels = np.frombuffer(labels_key, dtype=np.int64).reshape(shape)
    v = lut_lookup(labels, np.asarray(lut, dtype=np.float64)).astype(np.float64)
    mag = np.abs(v)
    N, H, W = shape
    r = len(kern) // 2
    ak = [abs(t) for t in kern]

    def line_pass(a, n):
        """a: list of n floats -> the filtered list, fsum per element."""
        idx, _ = reflect_table(n, r)
        ext = [a[i] for i in idx]
        return [math.fsum(kern[j] * ext[i + j] for j in range(len(kern))) for i in range(n)]

    def mag_pass(a, n):
        idx, _ = reflect_table(n, r)
        ext = [a[i] for i in idx]
        return [math.fsum(ak[j] * ext[i + j] for j in range(len(kern))) for i in range(n)]
    for _ in range(repeats):
        for n_ in range(N):
            for y in range(H):
                v[n_, y] = line_pass(v[n_, y].tolist(), W)
                mag[n_, y] = mag_pass(mag[n_, y].tolist(), W)
            for x in range(W):
                v[n_, :, x] = line_pass(v[n_, :, x].tolist(), H)
                mag[n_, :, x] = mag_pass(mag[n_, :, x].tolist(), H)
    v, mag = _zero_edge(v, edge) / div, _zero_edge(mag, edge) / abs(div)
    v.setflags(write=False)
    mag.setflags(write=False)
    return v, mag


def blur_fsum(labels, lut, kern, repeats, edge, div):
    """Every 1-D pass summed with math.fsum (one rounding per output of a pass, on products rounded once) -> (value, mag):
    mag carries sum |k| |v| through the passes the same way, which is what the roundings of all passes act on.
    Cached per argument set: the CPU and the GPU tests share one evaluation."""
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    return _blur_fsum(labels.tobytes(), labels.shape, tuple(float(t) for t in lut), tuple(float(t) for t in kern),
                      int(repeats), int(edge), float(div))


def blur_exact(labels, lut_int, kern_int, kern_shift, repeats, edge, div_shift):
    """Integer LUT, kernel kern_int / 2^kern_shift, div = 2^div_shift, in integer arithmetic -> float64, exact.  Asserts
    that every intermediate fits the 53 bits of a float64, so that the kernel's sums are exact in any order."""
    v = lut_lookup(labels, np.asarray(lut_int, dtype=np.int64)).astype(np.int64)
    N, H, W = v.shape
    k = [int(t) for t in kern_int]
    assert sum(k) == 1 << kern_shift and k == k[::-1]
    r = len(k) // 2
    ix, _ = reflect_table(W, r)
    iy, _ = reflect_table(H, r)
    for _ in range(repeats):
        P = v[:, :, ix]
        v = sum(k[j] * P[:, :, j:j + W] for j in range(len(k)))
        Q = v[:, iy, :]
        v = sum(k[j] * Q[:, j:j + H] for j in range(len(k)))
        assert np.abs(v).max() < 1 << 53                          # non-negative terms: no partial sum is larger
    v = _zero_edge(v, edge)
    return v.astype(np.float64) / 2.0 ** (2 * kern_shift * repeats + div_shift)


def gaussian_kernel(ksize, sigma):
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return k * (1.0 / k.sum())


BINOMIAL = {5: ([1, 4, 6, 4, 1], 4), 9: ([1, 8, 28, 56, 70, 56, 28, 8, 1], 8)}
EXACT_LUT = [0, 3, 7, 15, 1, 12]                                  # <= 15: 4 bits + 48 fraction bits after three 9-tap repeats
# (N, H, W, ksize), reflects twice
EXACT_BLUR = [((2, 3, 5, 9), True), ((2, 5, 2, 5), True), ((1, 17, 33, 9), False)]
# (ksize, H, W, repeats) with N = 2; 101 taps on 20 x 28 is a shape the entry refuses (50 >= 2 * 20 - 1)
GAUSS_BLUR = [(9, 20, 28, 1), (9, 20, 28, 3), (9, 64, 64, 2), (101, 64, 64, 2)]
GAUSS_LUT = [0.0] + [255.0] * 13 + [0.0] * 5                      # the mask colour map of the paste


def exact_labels(N, H, W, seed):
    """Labels in [-2, nlut + 2): some below 0 and some >= nlut, pinned at the first two pixels of every image."""
    lab = np.random.default_rng(seed).integers(-2, len(EXACT_LUT) + 2, (N, H, W))
    lab[:, 0, 0] = -2
    lab[:, 0, 1] = len(EXACT_LUT) + 1
    return lab.astype(np.int64)


def blob_labels(N, H, W, seed):
    """A blocky label map over all 19 classes (6 x 6 pixel blocks of random labels)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 19, (N, (H + 5) // 6, (W + 5) // 6))
    return np.repeat(np.repeat(small, 6, axis=1), 6, axis=2)[:, :H, :W].astype(np.int64)
