"""NIQE in numpy float64: the definition of include/flair_noref.h, step by step, for tests/test_niqe_cpu.py and
tests/test_gpu_niqe.py.

Two forms of the MSCN map: ``mscn_definition`` (scipy.ndimage.convolve with mode='nearest', the text of step 3) and
``mscn_restatement`` (the shifted form of difference D2, tap by tap in the kernel's order).  Everything downstream takes the
map as an argument, so either form, or a kernel's output, can be followed to the score.  ``MUTANTS`` names the misreadings
the CPU tests show to move the result.
"""
import functools
import math

import numpy as np
from scipy.ndimage import convolve
from scipy.special import gamma

BLOCK = 96
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.int64)        # / 256, on inputs 2i - 3 .. 2i + 4
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
ALPHAS = np.arange(0.2, 10.001, 0.001)
R_GAM = gamma(2.0 / ALPHAS) ** 2 / (gamma(1.0 / ALPHAS) * gamma(3.0 / ALPHAS))


# ------------------------------------------------------------------------------------------------ synthetic parameters
def gaussian_window():
    """fspecial('gaussian', 7, 7/6) in closed form."""
    x = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def synthetic_params(seed=0):
    """(mu_p (36,), cov_p (36, 36), window (7, 7)): a seeded pristine model with cov_p = A A^T + 0.01 I."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((36, 36)) * 0.2
    return rng.standard_normal(36) * 0.5 + 1.0, a @ a.T + 0.01 * np.eye(36), gaussian_window()


def frame(h, w, sigma, seed):
    """A smooth field plus Gaussian noise of ``sigma`` grey levels, (h, w, 3) uint8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 60 * np.sin(yy / 23.0 + seed) * np.cos(xx / 31.0) + 30 * np.sin((xx + 2 * yy) / 57.0)
    img = base[:, :, None] + np.array([10.0, -5.0, 3.0]) + sigma * rng.standard_normal((h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ steps 1 and 2
def luma(u8):
    """(H, W, 3) uint8 -> (H, W) int64: round_half_even((65481 R + 128553 G + 24966 B) / 255000) + 16."""
    p = u8.astype(np.int64)
    num = 65481 * p[..., 0] + 128553 * p[..., 1] + 24966 * p[..., 2]
    q, rem = np.divmod(num, 255000)
    return q + ((2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1))) + 16


def crop(y):
    return y[:y.shape[0] // BLOCK * BLOCK, :y.shape[1] // BLOCK * BLOCK]


def _half_axis(a, axis, phase=0):
    n = a.shape[axis]
    idx = 2 * np.arange(n // 2)[:, None] + np.arange(-3, 5)[None, :] + phase
    idx = np.where(idx < 0, -1 - idx, np.where(idx >= n, 2 * n - 1 - idx, idx))       # symmetric reflection
    taken = np.take(a, idx, axis=axis)                                                # axis -> (n / 2, 8)
    return np.tensordot(taken, HALF_TAPS, axes=([axis + 1], [0]))


def half_scale(y, phase=0):
    """(H, W) int64, even sizes -> (H / 2, W / 2) int64 = 65536 x MATLAB imresize(y, 0.5), exactly."""
    return _half_axis(_half_axis(y, 0, phase), 1, phase)


def tie_triples():
    """Every (R, G, B) whose luma quotient sits exactly on .5 and those one numerator step from it, as an (n, 3) uint8 array."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    gb, found = 128553 * g + 24966 * b, []
    for r in range(256):
        near = np.abs(2 * ((65481 * r + gb) % 255000) - 255000) <= 2 * 3
        found.append(np.stack([np.full(int(near.sum()), r, dtype=np.int64), g[near], b[near]], axis=1))
    return np.concatenate(found).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ step 3
def mscn_definition(y, window, pad_mode="nearest", plus=1.0):
    """The text of step 3 on a float64 plane."""
    mu = convolve(y, window, mode=pad_mode)
    sigma = np.sqrt(np.abs(convolve(y * y, window, mode=pad_mode) - mu * mu))
    return (y - mu) / (sigma + plus)


def mscn_restatement(y, window):
    """Difference D2: d = Y_tap - Y_centre, M = -sum g d / (sqrt(|sum g d^2 - (sum g d)^2|) + 1), taps in row-major order,
    tap (dy, dx) weighing window[3 - dy][3 - dx] (a convolution)."""
    h, w = y.shape
    p = np.pad(y, 3, mode="edge")
    s1, s2 = np.zeros_like(y), np.zeros_like(y)
    for ky in range(7):
        for kx in range(7):
            d = p[ky:ky + h, kx:kx + w] - y
            gd = window[6 - ky, 6 - kx] * d
            s1 = s1 + gd
            s2 = s2 + gd * d
    return -s1 / (np.sqrt(np.abs(s2 - s1 * s1)) + 1.0)


# ------------------------------------------------------------------------------------------------ step 4
def blocks_of(m, block, order="column"):
    """(Hc, Wc) -> (blocks, block, block) with block index j nh + i."""
    nh, nw = m.shape[0] // block, m.shape[1] // block
    t = m.reshape(nh, block, nw, block)
    t = t.transpose(2, 0, 1, 3) if order == "column" else t.transpose(0, 2, 1, 3)
    return t.reshape(nh * nw, block, block)


def maps_of(m, block, roll="block", order="column"):
    """The five maps of every block, (blocks, 5, block, block)."""
    b = blocks_of(m, block, order)
    if roll == "block":
        prods = [b * np.roll(b, s, axis=(1, 2)) for s in SHIFTS]
    else:                                                                              # the mutant: wrap around the plane
        prods = [blocks_of(m * np.roll(m, s, axis=(0, 1)), block, order) for s in SHIFTS]
    return np.stack([b] + prods, axis=1)


def moments_of(maps, zeros_positive=False):
    """(..., block, block) maps -> (..., 5): c-, c+, s-, s+, a; and the sums of |terms| that bound the order of summation."""
    neg = maps < 0
    pos = maps >= 0 if zeros_positive else maps > 0
    sq = maps * maps
    return np.stack([neg.sum((-2, -1)).astype(np.float64), pos.sum((-2, -1)).astype(np.float64), np.where(neg, sq, 0).sum((-2, -1)),
                     np.where(pos, sq, 0).sum((-2, -1)), np.abs(maps).sum((-2, -1))], axis=-1)


# ------------------------------------------------------------------------------------------------ steps 5 and 6
def aggd(mom, n):
    """(5,) moments of one map -> (alpha, beta_l, beta_r), one map at a time with the full arg-min over the grid."""
    cn, cp, sn, sp, a = (float(v) for v in mom)
    with np.errstate(divide="ignore", invalid="ignore"):
        left, right = np.sqrt(np.float64(sn) / cn), np.sqrt(np.float64(sp) / cp)
        g = left / right
        rho = (np.float64(a) / n) ** 2 / ((np.float64(sn) + sp) / n)
        rhon = rho * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
        alpha = ALPHAS[np.argmin((R_GAM - rhon) ** 2)] if not np.isnan(rhon) else np.nan     # no fit without both sides
        scale = np.sqrt(gamma(1.0 / alpha) / gamma(3.0 / alpha))
    return alpha, left * scale, right * scale


def features_of(moments, n):
    """(blocks, 5, 5) moments of one scale -> (blocks, 18)."""
    rows = []
    for blk in moments:
        alpha, bl, br = aggd(blk[0], n)
        row = [alpha, (bl + br) / 2]
        for k in range(1, 5):
            alpha, bl, br = aggd(blk[k], n)
            row += [alpha, (br - bl) * (gamma(2.0 / alpha) / gamma(1.0 / alpha)), bl, br]
        rows.append(row)
    return np.array(rows, dtype=np.float64)


def score_of(feats, mu_p, cov_p):
    good = ~np.isnan(feats).any(axis=1)
    if good.sum() < 2:
        return math.nan
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mu_d = np.nanmean(feats, axis=0)
    cov_d = np.cov(feats[good], rowvar=False)
    d = (mu_p - mu_d).reshape(1, 36)
    return float(np.sqrt(d @ np.linalg.pinv((cov_p + cov_d) / 2) @ d.T).item())


ALPHA_COLUMNS = (0, 2, 6, 10, 14, 18, 20, 24, 28, 32)       # where the ten alphas sit among a block's 36 features


def alpha_cell_faults(feats, mu_p, cov_p):
    """The smallest real fault: one alpha of one block lands one grid cell (0.001) off.  -> the relative change of the score
    for every (block, alpha, direction), as a flat array."""
    base = score_of(feats, mu_p, cov_p)
    moved = []
    for b in range(feats.shape[0]):
        for a in ALPHA_COLUMNS:
            for step in (0.001, -0.001):
                bent = feats.copy()
                bent[b, a] += step
                moved.append(abs(score_of(bent, mu_p, cov_p) - base) / base)
    return np.array(moved)


# ------------------------------------------------------------------------------------------------ the whole thing
MUTANTS = ("zero_pad", "sigma_plus_0", "roll_plane", "row_major", "half_phase", "zeros_positive")


def planes(u8, mutant=None):
    """(H, W, 3) uint8 -> [(plane float64, block)] of the two scales."""
    y1 = crop(luma(u8))
    y2 = half_scale(y1, phase=1 if mutant == "half_phase" else 0)
    return [(y1.astype(np.float64), BLOCK), (y2.astype(np.float64) / 65536.0, BLOCK // 2)]


def analyse(u8, params, form="definition", mutant=None, mscn=None):
    """One frame -> dict(mscn=[2 maps], moments=(blocks, 2, 5, 5), features=(blocks, 36), score).  ``form``: "definition" or
    "restatement"; ``mscn``: two given maps (a kernel's) instead of either; ``mutant``: one of MUTANTS."""
    mu_p, cov_p, window = params
    assert mutant is None or mutant in MUTANTS
    out_m, out_mom, out_f = [], [], []
    for s, (y, block) in enumerate(planes(u8, mutant)):
        if mscn is not None:
            m = mscn[s]
        elif form == "restatement":
            m = mscn_restatement(y, window)
        else:
            m = mscn_definition(y, window, pad_mode="constant" if mutant == "zero_pad" else "nearest",
                                plus=0.0 if mutant == "sigma_plus_0" else 1.0)
        maps = maps_of(m, block, roll="plane" if mutant == "roll_plane" else "block", order="row" if mutant == "row_major" else "column")
        mom = moments_of(maps, zeros_positive=mutant == "zeros_positive")
        out_m.append(m)
        out_mom.append(mom)
        out_f.append(features_of(mom, block * block))
    feats = np.concatenate(out_f, axis=1)
    return dict(mscn=out_m, moments=np.stack(out_mom, axis=1), features=feats, score=score_of(feats, mu_p, cov_p))


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """The frames of a GPU test shape: noise of 12, 40 and 80 grey levels in turn, (n, h, w, 3) uint8."""
    return np.stack([frame(h, w, (12.0, 40.0, 80.0)[i % 3], 100 * h + w + i) for i in range(n)])


@functools.lru_cache(maxsize=None)
def case_reference(n, h, w, form="definition"):
    """analyse() of every frame of case(n, h, w) with synthetic_params(), computed once per session."""
    return [analyse(f, synthetic_params(), form=form) for f in case(n, h, w)]
