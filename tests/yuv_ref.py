"""The definition of include/flair_yuv.h restated in numpy int64, its mutants, the inputs the GPU tests use, and a plain-Python
YUV4MPEG2 writer and reader for fixtures.  The coefficients are derived here from Kr and Kb; nothing is copied from the header."""
import functools

import numpy as np

FORMATS = ("420jpeg", "420mpeg2", "422", "444", "mono")
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")
# (horizontal, vertical) sampling of the chroma planes
AXES = {"420jpeg": ("centred", "centred"), "420mpeg2": ("cosited", "centred"), "422": ("cosited", "full"), "444": ("full", "full")}
MUTANTS = ("swap_uv", "swap_siting", "no_clamp", "other_matrix", "other_range") + tuple(f"coef{i}" for i in range(14))
SHAPES = ((1, 1), (2, 2), (3, 5), (6, 8), (17, 130), (37, 131))          # (H, W)
COUNTS = (1, 3)


def _round16(x):
    return int(np.floor(x * 65536.0 + 0.5))


@functools.lru_cache(None)
def coefficients(matrix, range_):
    """-> (cy, crv, cgu, cgv, cbu, ey[3], eu[3], ev[3]) as 14 integers, round(x 65536) of the float64 values."""
    Kr, Kb = MATRICES[matrix]
    Kg = 1.0 - Kr - Kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (1.0, 1.0)
    dec = [sy, 2 * (1 - Kr) * sc, 2 * Kb * (1 - Kb) / Kg * sc, 2 * Kr * (1 - Kr) / Kg * sc, 2 * (1 - Kb) * sc]
    ey = [Kr / sy, Kg / sy, Kb / sy]
    eu = [v / (2 * (1 - Kb)) / sc for v in (-Kr, -Kg, 1 - Kb)]
    ev = [v / (2 * (1 - Kr)) / sc for v in (1 - Kr, -Kg, -Kb)]
    return tuple(_round16(v) for v in dec + ey + eu + ev)


def tie_margin(matrix, range_):
    """How near any coefficient's product with 65536 comes to a rounding tie."""
    Kr, Kb = MATRICES[matrix]
    Kg = 1.0 - Kr - Kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (1.0, 1.0)
    vals = [sy, 2 * (1 - Kr) * sc, 2 * Kb * (1 - Kb) / Kg * sc, 2 * Kr * (1 - Kr) / Kg * sc, 2 * (1 - Kb) * sc, Kr / sy, Kg / sy, Kb / sy]
    vals += [v / (2 * (1 - Kb)) / sc for v in (-Kr, -Kg)] + [v / (2 * (1 - Kr)) / sc for v in (-Kg, -Kb)]
    return min(abs((v * 65536.0) % 1.0 - 0.5) for v in vals)


def limits(range_):
    """(y0, lo, hiY, hiC)"""
    return (16, 16, 235, 240) if range_ == "limited" else (0, 0, 255, 255)


def chroma_size(fmt, H, W):
    if fmt == "mono":
        return 0, 0
    return ((H + 1) // 2 if fmt.startswith("420") else H), (W if fmt == "444" else (W + 1) // 2)


def payload_bytes(fmt, H, W):
    hc, wc = chroma_size(fmt, H, W)
    return H * W + 2 * hc * wc


def _setup(fmt, matrix, range_, mutant):
    if mutant == "other_matrix":
        matrix = "bt709" if matrix == "bt601" else "bt601"
    if mutant == "other_range":
        range_ = "full" if range_ == "limited" else "limited"
    k = list(coefficients(matrix, range_))
    if mutant and mutant.startswith("coef"):
        k[int(mutant[4:])] += 1
    axes = AXES.get(fmt)
    if mutant == "swap_siting" and axes:
        swap = {"centred": "cosited", "cosited": "centred", "full": "full"}
        axes = (swap[axes[0]], swap[axes[1]])
    return k, limits(range_), axes


def _fix(idx, n, mutant):
    return idx % n if mutant == "no_clamp" else np.clip(idx, 0, n - 1)


def decode_taps(mode, length, n, mutant=None):
    """Per luma index i of an axis: two (chroma index, weight) taps, weights in quarters -> (i0, w0, i1, w1) int64 arrays."""
    i = np.arange(length, dtype=np.int64)
    c, odd = i >> 1, (i & 1) == 1
    if mode == "full":
        return i, np.full(length, 4, np.int64), i, np.zeros(length, np.int64)
    if mode == "centred":
        return c, np.full(length, 3, np.int64), _fix(np.where(odd, c + 1, c - 1), n, mutant), np.ones(length, np.int64)
    assert mode == "cosited"
    return c, np.where(odd, 2, 4).astype(np.int64), _fix(np.where(odd, c + 1, c), n, mutant), np.where(odd, 2, 0).astype(np.int64)


def decode(payload, H, W, fmt, matrix, range_, planar=False, mutant=None):
    """payload (N, P) uint8 -> (N, H, W, 3) uint8, or (N, 3, H, W) with planar."""
    payload = np.asarray(payload, dtype=np.uint8)
    N = payload.shape[0]
    assert payload.shape == (N, payload_bytes(fmt, H, W))
    k, (y0, _, _, _), axes = _setup(fmt, matrix, range_, mutant)
    cy, crv, cgu, cgv, cbu = k[:5]
    p = payload.astype(np.int64)
    Y = p[:, :H * W].reshape(N, H, W)
    if fmt == "mono":
        U16 = V16 = np.full((N, H, W), 2048, np.int64)
    else:
        hc, wc = chroma_size(fmt, H, W)
        U = p[:, H * W:H * W + hc * wc].reshape(N, hc, wc)
        V = p[:, H * W + hc * wc:].reshape(N, hc, wc)
        if mutant == "swap_uv":
            U, V = V, U
        x0, wx0, x1, wx1 = decode_taps(axes[0], W, wc, mutant)
        r0, wy0, r1, wy1 = decode_taps(axes[1], H, hc, mutant)

        def up(C):
            rows = C[:, :, x0] * wx0 + C[:, :, x1] * wx1                                  # (N, hc, W), in quarters
            return rows[:, r0, :] * wy0[:, None] + rows[:, r1, :] * wy1[:, None]          # (N, H, W), in sixteenths
        U16, V16 = up(U), up(V)
    yy, u, v = cy * 16 * (Y - y0), U16 - 2048, V16 - 2048
    assert max(np.abs(yy).max(), np.abs(crv * v).max(), np.abs(cbu * u).max()) < 6e8 / 2
    R = np.clip((yy + crv * v + (1 << 19)) >> 20, 0, 255)
    G = np.clip((yy - cgu * u - cgv * v + (1 << 19)) >> 20, 0, 255)
    B = np.clip((yy + cbu * u + (1 << 19)) >> 20, 0, 255)
    out = np.stack([R, G, B], axis=1 if planar else 3).astype(np.uint8)
    return np.ascontiguousarray(out)


def _footprint(x, axis, mode, mutant):
    """The weighted sums of x over the footprints of one axis -> (array with the axis subsampled, k of the weight 2^k)."""
    n = x.shape[axis]
    if mode == "full":
        return x, 0
    c = np.arange((n + 1) // 2, dtype=np.int64)
    if mode == "centred":
        taps = ((2 * c, 1), (2 * c + 1, 1))
    else:
        taps = ((2 * c - 1, 1), (2 * c, 2), (2 * c + 1, 1))
    return sum(np.take(x, _fix(i, n, mutant), axis=axis) * w for i, w in taps), (1 if mode == "centred" else 2)


def encode(rgb, fmt, matrix, range_, mutant=None):
    """rgb (N, H, W, 3) uint8 -> (N, P) uint8 payloads Y | U | V."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    N, H, W, _ = rgb.shape
    k, (y0, lo, hiY, hiC), axes = _setup(fmt, matrix, range_, mutant)
    ey, eu, ev = (np.array(k[5 + 3 * i:8 + 3 * i], dtype=np.int64) for i in range(3))
    p = rgb.astype(np.int64)
    Y = np.clip((((p * ey).sum(axis=3) + (1 << 15)) >> 16) + y0, lo, hiY)
    planes = [Y.reshape(N, -1)]
    if fmt != "mono":
        chroma = []
        for e in (eu, ev):
            c = (p * e).sum(axis=3)                                                       # unrounded, at scale 2^16
            c, kx = _footprint(c, 2, axes[0], mutant)
            c, ky = _footprint(c, 1, axes[1], mutant)
            kk = kx + ky
            chroma.append(np.clip(((c + (1 << (15 + kk))) >> (16 + kk)) + 128, lo, hiC).reshape(N, -1))
        if mutant == "swap_uv":
            chroma.reverse()
        planes += chroma
    out = np.concatenate(planes, axis=1).astype(np.uint8)
    assert out.shape == (N, payload_bytes(fmt, H, W))
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------- the GPU tests' inputs
@functools.lru_cache(None)
def random_bytes(n, seed):
    """n random bytes with 0 and 255 forced in (anywhere in 0..255: Y and chroma outside the nominal range too)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=n, dtype=np.uint8)
    first = int(rng.integers(0, n))
    b[first] = 0
    if n > 1:
        b[(first + 1 + int(rng.integers(0, n - 1))) % n] = 255
    b.setflags(write=False)
    return b


def payload_case(fmt, N, H, W):
    P = payload_bytes(fmt, H, W)
    return random_bytes(N * P, 1000 + 7 * H + W).reshape(N, P)


def rgb_case(N, H, W):
    return random_bytes(N * H * W * 3, 5000 + 7 * H + W).reshape(N, H, W, 3)


def all_cases():
    return [(N, H, W) for (H, W) in SHAPES for N in COUNTS]


# ------------------------------------------------------------------------------------------- fixtures: a plain Y4M writer and reader
def write_y4m(path, payloads, W, H, fmt="420jpeg", fps=(25, 1), tags="Ip", header=None, frame_line=b"FRAME\n"):
    """payloads: rows of bytes.  ``tags``: the header's other tags as text ('Ip A1:1 XCOLORRANGE=FULL'); ``fmt`` None leaves
    the C tag out; ``header`` replaces the whole line (without newline)."""
    if header is None:
        parts = ["YUV4MPEG2", f"W{W}", f"H{H}", f"F{fps[0]}:{fps[1]}"] + ([tags] if tags else []) + ([f"C{fmt}"] if fmt else [])
        header = " ".join(parts)
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + b"\n")
        for p in payloads:
            f.write(frame_line)
            f.write(bytes(np.asarray(p, dtype=np.uint8).tobytes()))
    return str(path)


def read_y4m(path):
    """-> (header line as text, payload size inferred from the text's W, H and C, [payload bytes])."""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    line = data[:end].decode("ascii")
    tags = {t[0]: t[1:] for t in line.split(" ")[1:] if t[0] != "X"}
    fmt = tags.get("C", "420jpeg")
    P = payload_bytes("420jpeg" if fmt == "420" else fmt, int(tags["H"]), int(tags["W"]))
    body, frames = data[end + 1:], []
    assert len(body) % (6 + P) == 0
    for o in range(0, len(body), 6 + P):
        assert body[o:o + 6] == b"FRAME\n"
        frames.append(body[o + 6:o + 6 + P])
    return line, P, frames


# ------------------------------------------------------------------------------------------- the entries' refusals
def entry_refusals(payload, rgb, H, W):
    """(entry, arguments without the stream, a piece of the message) for every refusal of include/flair_yuv.h.  ``payload`` and
    ``rgb``: addresses of two buffers of at least two frames (420jpeg) each; on a machine without a GPU any two numbers that
    do not overlap, since nothing is enqueued."""
    d, e = "flair_yuv_to_rgb_u8", "flair_rgb_to_yuv_u8"
    cases = [(d, (None, 1, H, W, 0, 0, 0, 0, rgb), "null pointer"), (d, (payload, 1, H, W, 0, 0, 0, 0, None), "null pointer"),
             (e, (None, 1, H, W, 0, 0, 0, payload), "null pointer"), (e, (rgb, 1, H, W, 0, 0, 0, None), "null pointer"),
             (d, (payload, 1, H, W, 0, 0, 0, 2, rgb), "planar = 2"), (d, (payload, 1, H, W, 0, 0, 0, -1, rgb), "planar = -1"),
             (d, (payload, 1, H, W, 0, 0, 0, 0, payload), "out overlaps payload"), (d, (payload, 2, H, W, 0, 0, 0, 0, payload + H * W), "out overlaps payload"),
             (e, (rgb, 1, H, W, 0, 0, 0, rgb), "payload_out overlaps rgb"), (e, (rgb, 2, H, W, 3, 0, 0, rgb + 3 * H * W), "payload_out overlaps rgb")]
    for name, head, tail in ((d, (payload,), (0, rgb)), (e, (rgb,), (payload,))):
        cases += [(name, head + (1, 0, W, 0, 0, 0) + tail, f"H = 0, W = {W} must be positive"),
                  (name, head + (1, H, -3, 0, 0, 0) + tail, f"H = {H}, W = -3 must be positive"),
                  (name, head + (-1, H, W, 0, 0, 0) + tail, "N = -1 frames must not be negative"),
                  (name, head + (1, H, W, 5, 0, 0) + tail, "unknown format = 5"), (name, head + (1, H, W, -1, 0, 0) + tail, "unknown format = -1"),
                  (name, head + (1, H, W, 0, 2, 0) + tail, "unknown matrix = 2"), (name, head + (1, H, W, 0, -1, 0) + tail, "unknown matrix = -1"),
                  (name, head + (1, H, W, 0, 0, 2) + tail, "unknown range = 2"), (name, head + (1, H, W, 0, 0, -1) + tail, "unknown range = -1"),
                  (name, head + (1 << 30, 17, 129, 0, 0, 0) + tail, "exceed one launch of 2^31 - 1 workgroups"),
                  (name, head + (0, H, W, 7, 0, 0) + tail, "unknown format = 7")]          # N = 0 does not excuse a bad id
    return cases


def entry_noops(payload, rgb, H, W):
    """N = 0: status 0, no pointer looked at."""
    return [("flair_yuv_to_rgb_u8", (None, 0, H, W, 0, 0, 0, 0, None)), ("flair_yuv_to_rgb_u8", (payload, 0, H, W, 4, 1, 1, 1, payload)),
            ("flair_rgb_to_yuv_u8", (None, 0, H, W, 0, 0, 0, None)), ("flair_rgb_to_yuv_u8", (rgb, 0, H, W, 2, 1, 0, rgb))]


def assert_refused(lib, name, args, what):
    rc = getattr(lib, name)(*args, None)
    msg = lib.flair_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)
