"""Tiled denoising restated in numpy float64: the planner, the weights and the blend of include/flair_tile.h, written from the
definition and not from flair_amd/tiling.py or csrc/tile.hip, with the mutants tests/test_tiling_cpu.py proves the bounds of
tests/test_gpu_tile.py against.  A plain-Python module (no test in it): the CPU and the GPU tests share it."""
import numpy as np

MUTANTS = ("ramp_off_by_one", "missing_half", "border_ramped", "swapped_axes")
U = 2.0 ** -24                      # unit roundoff of float32


def plan_axis(L, t, min_overlap, g):
    """Origins along one axis: [0] for L == t, else n = max(2, ceil((L - p) / (t - p))) tiles at floor(i (L - t) / (n - 1) / g) g."""
    if L == t:
        return [0]
    n = max(2, int(np.ceil((L - min_overlap) / (t - min_overlap))))
    return [int(np.floor(i * (L - t) / (n - 1) / g)) * g for i in range(n)]


def axis_weights(L, t, origins, ramp, mutant=None):
    """(len(origins), L): w of every tile at every pixel of the axis, 0 outside the tile."""
    out = np.zeros((len(origins), L))
    r = ramp + 1 if mutant == "ramp_off_by_one" else ramp
    half = 0.0 if mutant == "missing_half" else 0.5
    for i, o in enumerate(origins):
        for p in range(o, o + t):
            dl, dr = p - o + half, o + t - p - half
            wl = 1.0 if o == 0 and mutant != "border_ramped" else min(1.0, dl / r)
            wr = 1.0 if o + t == L and mutant != "border_ramped" else min(1.0, dr / r)
            out[i, p] = min(wl, wr)
    return out


def weights(H, W, th, tw, oy, ox, ramp, mutant=None):
    """(K, H, W) raw weights wy wx in plan order (tile k = r len(ox) + c) and the (H, W) number of covering tiles."""
    wy, wx = axis_weights(H, th, oy, ramp, mutant), axis_weights(W, tw, ox, ramp, mutant)
    if mutant == "swapped_axes":                    # tile (r, c) weighted as tile (c, r): needs a plan that is the same on both axes
        assert (H, th, list(oy)) == (W, tw, list(ox))
        w = np.stack([np.outer(wy[c], wx[r]) for r in range(len(oy)) for c in range(len(ox))])
    else:
        w = np.stack([np.outer(wy[r], wx[c]) for r in range(len(oy)) for c in range(len(ox))])
    cover = np.zeros((H, W), dtype=np.int64)
    for r, a in enumerate(oy):
        for c, b in enumerate(ox):
            cover[a:a + th, b:b + tw] += 1
    return w, cover


def normalised(H, W, th, tw, oy, ox, ramp, mutant=None):
    """(K, H, W) w^_k = w_k / sum_j w_j, and the cover count."""
    w, cover = weights(H, W, th, tw, oy, ox, ramp, mutant)
    return w / w.sum(0, keepdims=True), cover


def gather(frame, oy, ox, th, tw):
    """(N, C, H, W) -> (K N, C, th, tw) by slicing, the tile index major."""
    return np.concatenate([frame[:, :, a:a + th, b:b + tw] for a in oy for b in ox], 0)


def blend(tiles, H, W, oy, ox, ramp, mutant=None):
    """tiles (K N, C, th, tw) -> (out (N, C, H, W) float64, sum of w^ |v| per element, cover count (H, W))."""
    tiles = np.asarray(tiles, dtype=np.float64)
    K = len(oy) * len(ox)
    N, (C, th, tw) = tiles.shape[0] // K, tiles.shape[1:]
    wn, cover = normalised(H, W, th, tw, oy, ox, ramp, mutant)
    out, mag = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    k = 0
    for a in oy:
        for b in ox:
            v = tiles[k * N:(k + 1) * N]
            w = wn[k, a:a + th, b:b + tw]
            out[:, :, a:a + th, b:b + tw] += w * v
            mag[:, :, a:a + th, b:b + tw] += w * np.abs(v)
            k += 1
    return out, mag, cover


def bound(mag, cover):
    """The per-element bound of the f32 blend: (k + 2) 2^-24 sum w^ |v| for k covering tiles -- one rounding of w^, one of each
    product and of each of the k - 1 sums (k + 1 with the products fused into the sums), and one to spare."""
    return (cover + 2) * U * mag


def tiled(model, H, W, th, tw, oy, ox, ramp):
    """A whole-frame model made of ``model`` on every torch-sliced tile, blended here: the reference of TiledModel and of the
    tiled window loop.  ``model(x, t, **kw)`` with kw's low_res_input / rnn_input (1, T, 3, H, W) cut like x."""
    import torch

    def whole(x, t, **kw):
        outs = []
        for a in oy:
            for b in ox:
                kk = dict(kw)
                for name in ("low_res_input", "rnn_input"):
                    if kk.get(name) is not None:
                        kk[name] = kk[name][..., a:a + th, b:b + tw].contiguous()
                outs.append(model(x[..., a:a + th, b:b + tw].contiguous(), t, **kk).double().numpy())
        out, _, _ = blend(np.concatenate(outs, 0), H, W, oy, ox, ramp)
        return torch.from_numpy(out).to(x.dtype)
    return whole
