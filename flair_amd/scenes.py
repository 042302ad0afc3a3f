"""Scene cuts of a video: ``python -m flair_amd scenes SRC_DIR``, ``restore --scene-cuts``, ``interpolate --scene-cuts``.

The reference restores one continuous 25-frame clip and has nothing of this; real footage has cuts, across which neither the
window chain of ``restore`` (``prev_recon``, the recurrence, the temporal attention) nor a flow-based interpolator should
reach.  A cut at ``k`` means that frame ``k`` starts a new shot.

Detection compares the mean brightness of an 8 x 8 grid of blocks between neighbouring frames.  The GPU supplies the exact
integer luma sums of the blocks (``ops.block_luma_sums``, csrc/scenes.hip); everything here is host arithmetic in float64 on
those integers:

  d_i = mean over the 64 blocks of |S_i / cnt - S_{i+1} / cnt|        (0..255 scale)

and pair ``i`` is a cut candidate when ``d_i >= threshold`` and ``d_i >= ratio * median(d_j, 0 < |j - i| <= radius)``: a jump
that is large in absolute terms AND against its neighbourhood, so that fast motion, noise and fades (which raise every ``d``
of the neighbourhood alike) are not cuts.  Fades and dissolves are deliberately NOT detected.

The defaults (threshold 6, ratio 3, radius 4, min_shot 4) are heuristics chosen on synthetic sequences.  They have NOT been
validated on real footage: every one of them is an option, and a cuts file (``write_cuts`` / ``read_cuts``) replaces detection.
"""
import json
import math
import numbers
import os

GRID = 8
RULE_DEFAULTS = dict(threshold=6.0, ratio=3.0, radius=4, min_shot=4)       # min_shot = video.OVERLAP + 1


def block_counts(H, W):
    """The 64 pixel counts of the blocks, entry 8 a + b = rows (a H) // 8 .. ((a + 1) H) // 8 times the columns of b."""
    H, W = int(H), int(W)
    if H < GRID or W < GRID:
        raise ValueError(f"frames of {H}x{W} have fewer than {GRID} pixels a side: no {GRID}x{GRID} grid of blocks")
    rows = [((a + 1) * H) // GRID - (a * H) // GRID for a in range(GRID)]
    cols = [((b + 1) * W) // GRID - (b * W) // GRID for b in range(GRID)]
    return [r * c for r in rows for c in cols]


def pair_distances(sums, H, W):
    """(T, 64) exact integer block sums (a tensor, an array or nested lists) -> the T - 1 distances d_i as Python floats:
    float64 divisions of the integers by the counts, the 64 absolute differences summed with correct rounding
    (math.fsum: the result does not depend on the order of the blocks), divided by 64."""
    rows = sums.tolist() if hasattr(sums, "tolist") else [list(r) for r in sums]
    cnt = block_counts(H, W)
    if any(len(r) != GRID * GRID for r in rows):
        raise ValueError(f"pair_distances: rows of {GRID * GRID} block sums")
    means = [[int(s) / c for s, c in zip(r, cnt)] for r in rows]
    return [math.fsum(abs(x - y) for x, y in zip(means[i], means[i + 1])) / (GRID * GRID) for i in range(len(means) - 1)]


def _median(values):
    v = sorted(values)
    if not v:
        return 0.0
    m = len(v) // 2
    return v[m] if len(v) % 2 else (v[m - 1] + v[m]) / 2


def local_median(dist, i, radius):
    """Median of d_j for 0 < |j - i| <= radius, j in range; 0 for an empty neighbourhood."""
    return _median([dist[j] for j in range(max(0, i - radius), min(len(dist), i + radius + 1)) if j != i])


def check_rule(threshold, ratio, radius, min_shot):
    if not threshold >= 0 or not ratio >= 0:
        raise ValueError(f"threshold={threshold!r}, ratio={ratio!r}: neither may be negative")
    if isinstance(radius, bool) or int(radius) != radius or radius < 1:
        raise ValueError(f"radius={radius!r}: an integer >= 1")
    if isinstance(min_shot, bool) or int(min_shot) != min_shot or min_shot < 1:
        raise ValueError(f"min_shot={min_shot!r}: an integer >= 1")


def candidates(dist, threshold=6.0, ratio=3.0, radius=4):
    """Pairs i with d_i >= threshold and d_i >= ratio * local median, as the cuts k = i + 1 they stand for."""
    return [i + 1 for i, d in enumerate(dist) if d >= threshold and d >= ratio * local_median(dist, i, int(radius))]


def find_cuts(dist, threshold=6.0, ratio=3.0, radius=4, min_shot=4):
    """The T - 1 distances of a video of T frames -> sorted cuts.  Candidates are accepted greedily from left to right: a cut
    needs ``min_shot`` frames between it and the previous accepted cut (or frame 0) and ``min_shot`` frames after it, which
    folds flash frames into a neighbouring shot."""
    check_rule(threshold, ratio, radius, min_shot)
    dist = [float(d) for d in dist]
    n_frames = len(dist) + 1
    cuts, prev = [], 0
    for k in candidates(dist, threshold, ratio, radius):
        if k - prev >= min_shot and n_frames - k >= min_shot:
            cuts.append(k)
            prev = k
    return cuts


def check_cuts(cuts, n_frames):
    """Cuts are strictly increasing integers in 1 .. n_frames - 1; a ValueError names the first that is not.  -> list of int."""
    out, prev = [], 0
    for k in cuts:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise ValueError(f"cut {k!r} is not an integer")
        if not 1 <= k <= n_frames - 1:
            raise ValueError(f"cut {k} is outside 1..{n_frames - 1} (a cut at k means that frame k of the {n_frames} starts a shot)")
        if k <= prev:
            raise ValueError(f"cut {k} does not follow cut {prev}: cuts are strictly increasing")
        out.append(int(k))
        prev = int(k)
    return out


def shots(n_frames, cuts):
    """[(start, stop)] of the shots, stop exclusive."""
    edges = [0] + check_cuts(cuts or [], n_frames) + [int(n_frames)]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)] if n_frames > 0 else []


def check_frames(paths):
    """The refusals of detection on the file headers, before anything is decoded -> (h, w)."""
    from . import io as fio
    if not paths:
        raise ValueError("no frame files")
    sizes = [fio.frame_size(p) for p in paths]
    for p, s in zip(paths, sizes):
        if s != sizes[0]:
            raise ValueError(f"{p} is {s[0]}x{s[1]} and {paths[0]} is {sizes[0][0]}x{sizes[0][1]}; the frames of a video "
                             "must share one size")
    block_counts(*sizes[0])
    return sizes[0]


def detect_cuts_files(paths, device, batch=8, **rule):
    """Frame files -> dict(cuts, distances, shots, frames).  The frames go through io.iter_frame_batches ``batch`` at a time
    and ops.block_luma_sums; only the (T, 64) integers come back to the host.  ``rule``: find_cuts' keywords."""
    import torch
    from . import io as fio
    from . import ops
    rule = dict(RULE_DEFAULTS, **rule)
    check_rule(**rule)
    paths = list(paths)
    h, w = check_frames(paths)
    T = len(paths)
    if T == 1:
        return dict(cuts=[], distances=[], shots=[(0, 1)], frames=1)
    batch = max(1, int(batch))
    sums = torch.empty((T, GRID * GRID), dtype=torch.int64, device=device)
    for first, (u8,) in fio.iter_frame_batches([paths], [(p, min(batch, T - p)) for p in range(0, T, batch)], device):
        ops.block_luma_sums(u8, out=sums[first:first + u8.shape[0]])
    dist = pair_distances(sums.cpu(), h, w)
    cuts = find_cuts(dist, **rule)
    return dict(cuts=cuts, distances=dist, shots=shots(T, cuts), frames=T)


def describe(result):
    """One line per shot: ``shot 2: frames 13..17 (5), opened by d = 48.21``."""
    lines = []
    for s, (a, b) in enumerate(result["shots"]):
        how = f", opened by d = {result['distances'][a - 1]:.2f}" if a > 0 and len(result["distances"]) >= a else ""
        lines.append(f"shot {s}: frames {a}..{b - 1} ({b - a}){how}")
    return lines


def write_cuts(path, result):
    """``{"cuts": [...], "distances": [...], "frames": n}`` as JSON."""
    frames = result["frames"] if "frames" in result else len(result["distances"]) + 1
    with open(path, "w") as f:
        json.dump(dict(cuts=[int(k) for k in result["cuts"]], distances=[float(d) for d in result["distances"]],
                       frames=int(frames)), f, indent=1)
        f.write("\n")


def read_cuts(path, n_frames):
    """The cuts of a cuts file written for a video of ``n_frames`` frames; a ValueError for anything else."""
    if not os.path.isfile(path):
        raise ValueError(f"cuts file {path} not found")
    try:
        with open(path) as f:
            obj = json.load(f)
    except (OSError, ValueError) as exc:
        raise ValueError(f"cuts file {path} is not JSON: {exc}")
    if not isinstance(obj, dict) or not isinstance(obj.get("cuts"), list) or "frames" not in obj:
        raise ValueError(f'cuts file {path}: expected {{"cuts": [...], "distances": [...], "frames": n}}')
    if obj["frames"] != n_frames:
        raise ValueError(f"cuts file {path} was written for {obj['frames']} frames; the video has {n_frames}")
    try:
        return check_cuts(obj["cuts"], n_frames)
    except ValueError as exc:
        raise ValueError(f"cuts file {path}: {exc}")


def resolve(scene_cuts, paths, device, **rule):
    """The ``scene_cuts`` argument of the drivers -> (cuts or None, detection result or None): "off" / None -> no cuts;
    "auto" -> detect_cuts_files on ``paths``; a list is checked; anything else is the path of a cuts file."""
    if scene_cuts is None or (isinstance(scene_cuts, str) and scene_cuts == "off"):
        return None, None
    if isinstance(scene_cuts, str) and scene_cuts == "auto":
        result = detect_cuts_files(paths, device, **rule)
        return result["cuts"], result
    if isinstance(scene_cuts, (list, tuple)):
        return check_cuts(scene_cuts, len(paths)), None
    return read_cuts(os.fspath(scene_cuts), len(paths)), None
