"""The flow-warping error of include/flair_temporal.h in numpy float64 on the CPU, with the header's operation order (numpy
rounds every product and every sum on its own, as the kernels do), the deliberately wrong variants the CPU tests must tell
apart from it, and the cases the CPU and the GPU tests share.  S is ``math.fsum`` of the per-pixel errors: the exact sum,
rounded once."""
import functools
import math

import numpy as np

MUTANTS = ("dropped_half", "swapped_flows", "backward_differences", "inside_off_by_one", "mask_ignored_in_n")


def _taps(f, mutant=None):
    """Steps 1 and 2 up to the weights for one pair: f (H, W, 2) f32 -> dict(inside, x0, x1, y0, y1, l0x, l1x, l0y, l1y)."""
    H, W, _ = f.shape
    f = f.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    qx, qy = xs + f[..., 0], ys + f[..., 1]
    hi_x, hi_y = (W, H) if mutant == "inside_off_by_one" else (W - 1, H - 1)
    with np.errstate(invalid="ignore"):
        inside = (qx >= 0) & (qx <= hi_x) & (qy >= 0) & (qy <= hi_y)
    qx, qy = np.where(inside, qx, 0.0), np.where(inside, qy, 0.0)
    x0, y0 = np.minimum(np.floor(qx).astype(np.int64), W - 1), np.minimum(np.floor(qy).astype(np.int64), H - 1)
    l1x, l1y = qx - x0, qy - y0
    return dict(inside=inside, x0=x0, x1=np.minimum(x0 + 1, W - 1), y0=y0, y1=np.minimum(y0 + 1, H - 1),
                l0x=1.0 - l1x, l1x=l1x, l0y=1.0 - l1y, l1y=l1y)


def _bilinear(v, t):
    """v (H, W) float64 gathered at the taps: l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11)."""
    v00, v01, v10, v11 = v[t["y0"], t["x0"]], v[t["y0"], t["x1"]], v[t["y1"], t["x0"]], v[t["y1"], t["x1"]]
    return t["l0y"] * (t["l0x"] * v00 + t["l1x"] * v01) + t["l1y"] * (t["l0x"] * v10 + t["l1x"] * v11)


def occlusion(f, g, mutant=None):
    """Steps 1 to 5 for one pair: f, g (H, W, 2) f32 -> dict(mask (H, W) uint8, margin (H, W) float64, and the boolean maps
    inside, occluded, boundary).  ``margin`` is the smaller relative distance |lhs - rhs| / max(|lhs|, |rhs|) of the two sides
    of tests 3 and 4 (inf outside): where it is tiny, arithmetic in another order may decide the pixel the other way."""
    if mutant == "swapped_flows":
        f, g = g, f
    t = _taps(f, mutant)
    f64, g64 = f.astype(np.float64), g.astype(np.float64)
    fx, fy = f64[..., 0], f64[..., 1]
    gx, gy = _bilinear(g64[..., 0], t), _bilinear(g64[..., 1], t)
    sx, sy = fx + gx, fy + gy
    ff, gg = fx * fx + fy * fy, gx * gx + gy * gy
    lhs3 = sx * sx + sy * sy
    rhs3 = 0.01 * (ff + gg) if mutant == "dropped_half" else 0.01 * (ff + gg) + 0.5
    dx, dy = np.zeros_like(f64), np.zeros_like(f64)
    if mutant == "backward_differences":
        dx[:, 1:] = f64[:, 1:] - f64[:, :-1]
        dy[1:] = f64[1:] - f64[:-1]
    else:
        dx[:, :-1] = f64[:, 1:] - f64[:, :-1]
        dy[:-1] = f64[1:] - f64[:-1]
    lhs4 = (dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + (dy[..., 0] * dy[..., 0] + dy[..., 1] * dy[..., 1])
    rhs4 = 0.01 * ff + 0.002
    mask = t["inside"] & ~(lhs3 > rhs3) & ~(lhs4 > rhs4)
    with np.errstate(invalid="ignore", divide="ignore"):
        m3 = np.abs(lhs3 - rhs3) / np.maximum(np.abs(lhs3), np.abs(rhs3))
        m4 = np.abs(lhs4 - rhs4) / np.maximum(np.abs(lhs4), np.abs(rhs4))
    return dict(mask=mask.astype(np.uint8), margin=np.where(t["inside"], np.minimum(m3, m4), np.inf), inside=t["inside"],
                occluded=t["inside"] & (lhs3 > rhs3), boundary=t["inside"] & (lhs4 > rhs4))


def sums(a, b, f, mask, mutant=None):
    """Steps 6 and 7 for one pair: a, b (H, W, 3) uint8, f (H, W, 2) f32, mask (H, W) -> (S, N), S = fsum of M e.  A pixel
    whose mask is set but whose q is outside is left out, as the kernel leaves it out."""
    t = _taps(f, mutant)
    keep = (np.asarray(mask) != 0) & t["inside"]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    e = None
    for c in range(3):
        d = a64[..., c] - _bilinear(b64[..., c], t)
        e = d * d if e is None else e + d * d
    n = a.shape[0] * a.shape[1] if mutant == "mask_ignored_in_n" else int(keep.sum())
    return math.fsum(e[keep].tolist()), n


def pair(a, b, f, g, mutant=None):
    """-> (mask, S, N) of one pair, every step by the same variant."""
    if mutant == "swapped_flows":
        f, g = g, f
    mask = occlusion(f, g, None if mutant == "swapped_flows" else mutant)["mask"]
    return (mask,) + sums(a, b, f, mask, mutant)


def warp_err(S, N):
    return None if N == 0 else S / (255.0 ** 2 * N)


def batch(frames, f, g, frames2=None):
    """frames (P + 1, H, W, 3) uint8, f, g (P, H, W, 2) f32 -> (mask (P, H, W) uint8, out (sets, P, 2) float64) as the two
    entries define them."""
    P = f.shape[0]
    masks = np.stack([occlusion(f[i], g[i])["mask"] for i in range(P)])
    sets = [frames] if frames2 is None else [frames, frames2]
    out = np.array([[sums(s[i], s[i + 1], f[i], masks[i]) for i in range(P)] for s in sets], dtype=np.float64)
    return masks, out


# ------------------------------------------------------------------------------------------- known answers
def _shift_case(H, W, dx, dy, seed):
    """b is a shifted by the integer vector (dx, dy): b(p + (dx, dy)) = a(p); f = (dx, dy) everywhere, g = -f.  The mask is
    1 exactly where p + f is inside and S = 0.  A second set differs from the first in ONE unmasked byte of frame 0, by k = 7:
    its S is exactly 49."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs + dx >= 0) & (xs + dx <= W - 1) & (ys + dy >= 0) & (ys + dy <= H - 1)
    b[(ys + dy)[inside], (xs + dx)[inside]] = a[inside]
    f = np.empty((H, W, 2), dtype=np.float32)
    f[..., 0], f[..., 1] = dx, dy
    a2 = a.copy()
    y, x = np.argwhere(inside)[len(np.argwhere(inside)) // 2]
    a2[y, x, 1] = a2[y, x, 1] + 7 if a2[y, x, 1] < 200 else a2[y, x, 1] - 7
    n = int(inside.sum())
    return dict(name=f"shift {H}x{W} by ({dx}, {dy})", frames=np.stack([a, b]), frames2=np.stack([a2, b]), f=f[None], g=-f[None],
                mask=inside.astype(np.uint8)[None], S=[0.0, 49.0], N=n)


def _half_pixel_case(H=37, W=70):
    """f = (0.5, 0), g = 0: |f + g|^2 = 0.25 is under 0.01 * 0.25 + 0.5, so nothing is occluded (without the + 0.5 everything
    would be); the last column lands on W - 0.5, outside.  a = 10 everywhere, b(x) = 2 x in every channel: b~ = 2 x + 1 exactly
    and S = 3 * sum over the inside pixels of (10 - 2 x - 1)^2, an integer."""
    a = np.full((H, W, 3), 10, dtype=np.uint8)
    b = np.broadcast_to((2 * np.arange(W, dtype=np.uint8))[None, :, None], (H, W, 3)).copy()
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[..., 0] = 0.5
    mask = np.ones((H, W), dtype=np.uint8)
    mask[:, W - 1] = 0
    S = 3 * H * sum((10 - 2 * x - 1) ** 2 for x in range(W - 1))
    return dict(name="half pixel", frames=np.stack([a, b]), frames2=None, f=f[None], g=np.zeros_like(f)[None], mask=mask[None],
                S=[float(S)], N=H * (W - 1))


def _step_case(H=37, W=70, at=20):
    """f.x = 0 left of column ``at`` and 1 from it on, g = -f: consistent everywhere (g~ at q is -f), so nothing is occluded;
    the forward difference is 1 in column at - 1 alone (|f|^2 = 0 there: 1 > 0.002), the last column is outside.  Flat frames."""
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[:, at:, 0] = 1.0
    mask = np.ones((H, W), dtype=np.uint8)
    mask[:, at - 1] = 0
    mask[:, W - 1] = 0
    frames = np.full((2, H, W, 3), 99, dtype=np.uint8)
    return dict(name="flow step", frames=frames, frames2=None, f=f[None], g=-f[None], mask=mask[None], S=[0.0], N=H * (W - 2))


@functools.lru_cache(maxsize=None)
def known_answers():
    """The hand cases: dict(name, frames (2, H, W, 3), frames2 or None, f, g (1, H, W, 2), mask (1, H, W), S per set, N).
    37 x 70: H is no multiple of the 32-row tile and W is one 64-column tile and a part; column W - 4 lands on W - 1 (inside)
    and column W - 3 on W (outside).  1 x 40 and 40 x 1: a size-1 axis, whose differences are zero.  Read-only."""
    return (_shift_case(37, 70, 3, -2, 1), _shift_case(1, 40, 3, 0, 2), _shift_case(40, 1, 0, -2, 3), _half_pixel_case(), _step_case())


def check_known_answer(case, mask, out):
    """The failures of (mask (1, H, W), out (sets, 1, 2)) against a case's exact answers, as a list of strings."""
    bad = []
    if not np.array_equal(np.asarray(mask), case["mask"]):
        bad.append(f"{case['name']}: mask differs on {int((np.asarray(mask) != case['mask']).sum())} pixels")
    for s, want in enumerate(case["S"]):
        if out[s][0][0] != want or out[s][0][1] != case["N"]:
            bad.append(f"{case['name']}: set {s} gives (S, N) = ({out[s][0][0]!r}, {out[s][0][1]!r}), not ({want!r}, {case['N']!r})")
    return bad


def run_known_answer(case, mutant=None):
    """The reference (or a mutant of it) on a case -> (mask (1, H, W), out (sets, 1, 2))."""
    sets = [case["frames"]] if case["frames2"] is None else [case["frames"], case["frames2"]]
    got = [pair(s[0], s[1], case["f"][0], case["g"][0], mutant) for s in sets]
    return got[0][0][None], np.array([[[S, N]] for _, S, N in got], dtype=np.float64)


# ------------------------------------------------------------------------------------------- generated data
def smooth_flow(rng, P, H, W, amplitude, cells=6):
    """A smooth random flow: a coarse grid of vectors, bilinearly enlarged -> (P, H, W, 2) float64 within +- amplitude."""
    coarse = rng.uniform(-amplitude, amplitude, (P, cells, cells, 2))
    yy, xx = np.linspace(0, cells - 1, H), np.linspace(0, cells - 1, W)
    y0, x0 = np.minimum(yy.astype(int), cells - 2), np.minimum(xx.astype(int), cells - 2)
    wy, wx = (yy - y0)[None, :, None, None], (xx - x0)[None, None, :, None]
    c = lambda dy, dx: coarse[:, y0 + dy][:, :, x0 + dx]                 # noqa: E731
    return (1 - wy) * ((1 - wx) * c(0, 0) + wx * c(0, 1)) + wy * ((1 - wx) * c(1, 0) + wx * c(1, 1))


DYADIC_MOTION = ((2.25, -1.5), (-7.0, 6.5), (0.75, 3.0))


@functools.lru_cache(maxsize=None)
def dyadic_case(P, H=37, W=70, seed=5):
    """Flows on a 1/4 grid with |f| <= 8 and random bytes: every bilinear weight is a multiple of 1/4, every bilinear value of
    a byte a multiple of 1/16 and every squared error of 1/256, so S is exact in double in ANY order, and both sides of the
    mask's tests are sums of exactly representable numbers and one product with 0.01.  Pair i moves by DYADIC_MOTION[i] plus
    -1/4, 0 or 1/4 per 9 x 11 block (motion boundaries at block edges); g is -f plus up to 3/4 per pixel (occluded or not).
    -> dict(frames, frames2, f, g).  Read-only."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(-1, 2, (P, -(-H // 9), -(-W // 11), 2)) / 4.0
    f = np.repeat(np.repeat(blocks, 9, axis=1), 11, axis=2)[:, :H, :W] + np.array(DYADIC_MOTION[:P])[:, None, None, :]
    g = -f + rng.integers(-3, 4, f.shape) / 4.0
    assert np.abs(f).max() <= 8 and np.abs(g).max() <= 8
    return dict(frames=rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8), frames2=rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8),
                f=f.astype(np.float32), g=g.astype(np.float32))


RANDOM_SEED = 7                                 # chosen on the CPU: tests/test_temporal_cpu.py asserts what it must give


@functools.lru_cache(maxsize=None)
def random_case(P=2, H=37, W=70, seed=RANDOM_SEED):
    """Arbitrary f32 flows (a common motion + a smooth field + noise; g roughly -f) and random bytes -> dict(frames, frames2,
    f, g).  Read-only."""
    rng = np.random.default_rng(seed)
    f = np.array([1.3, -0.6]) + smooth_flow(rng, P, H, W, 1.5, cells=4) + 0.02 * rng.standard_normal((P, H, W, 2))
    g = -f + smooth_flow(rng, P, H, W, 0.8, cells=4) + 0.02 * rng.standard_normal((P, H, W, 2))
    return dict(frames=rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8), frames2=rng.integers(0, 256, (P + 1, H, W, 3), dtype=np.uint8),
                f=f.astype(np.float32), g=g.astype(np.float32))


# ------------------------------------------------------------------------------------------- the entries' refusals
def entry_refusals():
    """[(entry, argument tuple without the stream, text the message must hold)]: every refusal include/flair_temporal.h lists,
    on pointers that are never dereferenced (a refusal comes before any launch)."""
    import ctypes
    P, odd4 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    Z = ctypes.c_size_t
    out = []
    occ = lambda **k: tuple({**dict(f=P, g=P, P=1, H=64, W=64, mask=P), **k}.values())  # noqa: E731
    for k, what in [(dict(f=None), "null pointer"), (dict(g=None), "null pointer"), (dict(mask=None), "null pointer"), (dict(P=0), "P = 0"),
                    (dict(H=0), "H = 0"), (dict(W=-3), "W = -3"), (dict(f=odd4), "8-byte aligned"), (dict(g=odd4), "8-byte aligned"),
                    (dict(P=1 << 30), "exceed one launch"), (dict(P=0x7fffffff, H=0x7fffffff, W=0x7fffffff), "exceed one launch")]:
        out.append(("flair_flow_occlusion", occ(**k), what))
    err = lambda **k: tuple({**dict(a=P, a2=None, f=P, mask=P, P=2, H=64, W=128, out=P, ws=P, ws_bytes=Z(128)), **k}.values())  # noqa: E731
    for k, what in [(dict(a=None), "null pointer"), (dict(f=None), "null pointer"), (dict(mask=None), "null pointer"), (dict(out=None), "null pointer"),
                    (dict(ws=None), "null pointer"), (dict(P=0), "P = 0"), (dict(H=-1), "H = -1"), (dict(W=0), "W = 0"),
                    (dict(f=odd4), "f = "), (dict(out=odd4), "out = "), (dict(ws=odd4), "ws = "),
                    (dict(ws_bytes=Z(127)), "ws_bytes = 127, sets * P * ceil(H / FLAIR_WARP_TILE_H) * ceil(W / FLAIR_WARP_TILE_W) * 16 = 128"),
                    (dict(a2=P, ws_bytes=Z(255)), "= 256"), (dict(H=65, ws_bytes=Z(128)), "= 192"), (dict(W=129, ws_bytes=Z(128)), "= 192"),
                    (dict(P=1 << 30, ws_bytes=Z(1 << 40)), "exceed one launch"),
                    (dict(P=0x7fffffff, H=0x7fffffff, W=0x7fffffff, ws_bytes=Z((1 << 64) - 1)), "ws_bytes")]:
        out.append(("flair_warp_error", err(**k), what))
    return out


def assert_refused(lib, name, args, what):
    rc = getattr(lib, name)(*args, None)
    msg = lib.flair_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)
