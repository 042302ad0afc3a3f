"""numpy restatement of scene-cut detection (flair_amd/scenes.py, csrc/scenes.hip) and the fixture sequences of its tests.

Restated from the definitions alone: the integer luma, the 8 x 8 block sums as int64, the distances in float64 (divisions of
the integers by the block counts, the 64 absolute differences summed with correct rounding, so that the order of the blocks
cannot matter) and the rule with its greedy acceptance.
"""
import math

import numpy as np

GRID = 8


def luma(u8):
    """(..., 3) uint8 -> (...) int64: (77 R + 150 G + 29 B + 128) >> 8."""
    p = np.asarray(u8).astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def edges(n):
    return [(k * n) // GRID for k in range(GRID + 1)]


def block_sums(u8):
    """(N, H, W, 3) uint8 -> (N, 64) int64."""
    y = luma(u8)
    N, H, W = y.shape
    ys, xs = edges(H), edges(W)
    out = np.zeros((N, GRID * GRID), dtype=np.int64)
    for a in range(GRID):
        for b in range(GRID):
            out[:, GRID * a + b] = y[:, ys[a]:ys[a + 1], xs[b]:xs[b + 1]].sum(axis=(1, 2), dtype=np.int64)
    return out


def block_counts(H, W):
    ys, xs = edges(H), edges(W)
    return np.array([(ys[a + 1] - ys[a]) * (xs[b + 1] - xs[b]) for a in range(GRID) for b in range(GRID)], dtype=np.int64)


def pair_distances(sums, H, W):
    means = np.asarray(sums).astype(np.float64) / block_counts(H, W).astype(np.float64)
    return [math.fsum(np.abs(means[i] - means[i + 1]).tolist()) / 64.0 for i in range(len(means) - 1)]


def local_median(dist, i, radius):
    near = [dist[j] for j in range(len(dist)) if j != i and abs(j - i) <= radius]
    return float(np.median(near)) if near else 0.0


def candidates(dist, threshold=6.0, ratio=3.0, radius=4):
    return [i + 1 for i, d in enumerate(dist) if d >= threshold and d >= ratio * local_median(dist, i, radius)]


def find_cuts(dist, threshold=6.0, ratio=3.0, radius=4, min_shot=4):
    n, cuts, prev = len(dist) + 1, [], 0
    for k in candidates(dist, threshold, ratio, radius):
        if k - prev >= min_shot and n - k >= min_shot:
            cuts.append(k)
            prev = k
    return cuts


def margins(dist, true_cuts, threshold=6.0, ratio=3.0, radius=4):
    """The margins of the restatement alone, asserted before any cut list: every true cut has
    d >= 2 max(threshold, ratio * local median); every other pair has d <= (2/3) ratio * local median or d < threshold."""
    for i, d in enumerate(dist):
        med = local_median(dist, i, radius)
        if i + 1 in true_cuts:
            assert d >= 2 * max(threshold, ratio * med), (i, d, med)
        else:
            assert d <= (2.0 / 3.0) * ratio * med or d < threshold, (i, d, med)


# --------------------------------------------------------------------------------------------------- fixture sequences
def shot(seed, H, W, frames, speed=1.0, start=0):
    """(frames, H, W, 3) uint8: per channel the mean of six sinusoids with spatial frequencies drawn from default_rng(seed) in
    +-0.03 cycles / px, scaled to clip((0.5 + 0.9 mean) 255), translated by ``speed`` px per frame along x; ``start``: the
    index of the first frame (a shot continued after another)."""
    rng = np.random.default_rng(seed)
    fy = rng.uniform(-0.03, 0.03, size=(3, 6))
    fx = rng.uniform(-0.03, 0.03, size=(3, 6))
    ph = rng.uniform(0, 2 * np.pi, size=(3, 6))
    y = np.arange(H, dtype=np.float64)[:, None, None, None]
    x = np.arange(W, dtype=np.float64)[None, :, None, None]
    out = np.empty((frames, H, W, 3), dtype=np.uint8)
    for t in range(frames):
        s = speed * (start + t)
        v = np.sin(2 * np.pi * (fy * y + fx * (x - s)) + ph).mean(axis=3)              # (H, W, 3)
        out[t] = np.clip(np.rint((0.5 + 0.9 * v) * 255), 0, 255).astype(np.uint8)
    return out


def cut_sequence(H, W):
    """Shots of 7, 6, 1 and 5 frames (seeds 1, 2, 3, and 2 continued) moving at 1 px per frame: candidates 7, 13 and 14, of
    which min_shot = 4 keeps 7 and 13 (the flash frame 13 joins the last shot)."""
    return np.concatenate([shot(1, H, W, 7), shot(2, H, W, 6), shot(3, H, W, 1), shot(2, H, W, 5, start=7)])


def fast_pan(H, W):
    return shot(4, H, W, 10, speed=9.0)


def fade(H, W):
    base = shot(5, H, W, 10).astype(np.float64)
    gain = (1.0 - 0.09 * np.arange(10))[:, None, None, None]
    return np.clip(np.rint(base * gain), 0, 255).astype(np.uint8)


def noisy(H, W):
    base = shot(6, H, W, 10).astype(np.int64)
    noise = np.random.default_rng(60).integers(-25, 26, size=base.shape)
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def still(H, W):
    return np.repeat(shot(7, H, W, 1), 6, axis=0)


SIZES = ((40, 72), (45, 70), (96, 160))
