"""NIQE (Mittal et al. 2013), a score for written frames that needs no ground truth, on the GPU:
``python -m flair_amd niqe FRAMES_DIR --params FILE`` and ``--niqe FILE`` of evaluate / restore / interpolate.

The reference ships no scoring tool and BasicSR is not a dependency; the definition is restated in include/flair_noref.h
(BasicSR's ``calculate_niqe`` on the Y channel without border crop, with two named differences: exact-integer luma, and the
MSCN map in a shifted form that is exactly zero on flat regions).  Per batch three launches, ``flair_niqe_luma`` (bytes -> the
cropped luma plane and its bicubic half scale, exact integers) and ``flair_niqe_moments`` once per scale (MSCN map and 25
moments per block, float64, deterministic); 50 doubles per block come back, and the AGGD fits, the 36 features per block and
the distance to the pristine model are numpy float64 here, vectorised over all blocks of the batch.  Lower is better.

The parameters are the user's: BasicSR's ``niqe_pris_params.npz`` (keys ``mu_pris_param`` (1, 36), ``cov_pris_param`` (36, 36),
``gaussian_window`` (7, 7)).  Nothing is downloaded or shipped.
"""
import math
import os
import warnings

import numpy as np
import torch
from scipy.special import gamma

from . import io as fio
from . import ops

BLOCK = ops.NIQE_BLOCK
FEATURES = 36                                   # 18 per scale: [alpha, mean beta] of M and [alpha, eta, beta_l, beta_r] of four products
KEYS = {"mu_pris_param": 36, "cov_pris_param": 36 * 36, "gaussian_window": 49}

# the AGGD shape grid and r(alpha) = Gamma(2/alpha)^2 / (Gamma(1/alpha) Gamma(3/alpha)), which rises strictly with alpha
ALPHAS = np.arange(0.2, 10.001, 0.001)
R_GAM = gamma(2.0 / ALPHAS) ** 2 / (gamma(1.0 / ALPHAS) * gamma(3.0 / ALPHAS))
assert np.all(np.diff(R_GAM) > 0)


def check_size(h, w, what="frames"):
    """ValueError where a frame holds fewer than two 96 x 96 blocks (the covariance over the blocks needs two)."""
    if (h // BLOCK) * (w // BLOCK) < 2:
        raise ValueError(f"niqe: {what} are {h}x{w}, which holds {(h // BLOCK) * (w // BLOCK)} blocks of {BLOCK}x{BLOCK}; the score "
                         "needs at least two")


def nearest_alpha(x):
    """Index into ALPHAS of the first minimum of (R_GAM - x)^2, i.e. ``np.argmin((R_GAM - x) ** 2)`` for every entry of ``x``
    without the (entries, 9801) table: R_GAM is sorted, so the minimum lies next to where x would be inserted.  NaN -> 0
    (the caller gives such an entry no alpha at all)."""
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(-1)
    k = np.searchsorted(R_GAM, flat)
    cand = np.clip(k[:, None] + np.arange(-2, 2)[None, :], 0, len(R_GAM) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        pick = np.argmin((R_GAM[cand] - flat[:, None]) ** 2, axis=1)
    idx = cand[np.arange(flat.size), pick]
    return np.where(np.isnan(flat), 0, idx).reshape(x.shape)


def features(moments, pixels):
    """Step 5: moments (..., 5 maps, 5) of blocks of ``pixels`` pixels -> (..., 18) features in float64.  A map without a
    negative or without a positive value has no fit: 0 / 0 makes rho' NaN, nothing minimises the distance to it, and all
    of its features are NaN (numpy's argmin would answer alpha = 0.2 there, which nanmean would then count)."""
    m = np.asarray(moments, dtype=np.float64)
    cn, cp, sn, sp, a = (m[..., i] for i in range(5))
    n = float(pixels)
    with np.errstate(divide="ignore", invalid="ignore"):
        left, right = np.sqrt(sn / cn), np.sqrt(sp / cp)
        g = left / right
        rho = (a / n) ** 2 / ((sn + sp) / n)
        rhon = rho * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
        alpha = np.where(np.isnan(rhon), np.nan, ALPHAS[nearest_alpha(rhon)])
        g1, g2, g3 = gamma(1.0 / alpha), gamma(2.0 / alpha), gamma(3.0 / alpha)
        bl, br = left * np.sqrt(g1 / g3), right * np.sqrt(g1 / g3)
        first = np.stack([alpha[..., 0], (bl[..., 0] + br[..., 0]) / 2], axis=-1)
        rest = np.stack([alpha[..., 1:], (br[..., 1:] - bl[..., 1:]) * (g2[..., 1:] / g1[..., 1:]), bl[..., 1:], br[..., 1:]], axis=-1)
    return np.concatenate([first, rest.reshape(rest.shape[:-2] + (16,))], axis=-1)


def score(feats, mu_p, cov_p):
    """Step 6: (blocks, 36) features of one frame -> the distance to the pristine model; NaN with fewer than two NaN-free blocks."""
    feats = np.asarray(feats, dtype=np.float64)
    good = ~np.isnan(feats).any(axis=1)
    if good.sum() < 2:
        return math.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mu_d = np.nanmean(feats, axis=0)
    cov_d = np.cov(feats[good], rowvar=False)
    d = mu_p.reshape(1, FEATURES) - mu_d.reshape(1, FEATURES)
    return float(np.sqrt(d @ np.linalg.pinv((cov_p + cov_d) / 2) @ d.T).item())


class NIQE:
    """``NIQE(mu, cov, window, device)``: the pristine model (36,), (36, 36) and the (7, 7) MSCN window as float64 arrays.
    ``model(u8)``: (N, H, W, 3) uint8 frames on the device -> N Python floats (NaN where no score exists)."""

    def __init__(self, mu, cov, window, device):
        self.mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(FEATURES)
        self.cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(FEATURES, FEATURES)
        self.window_host = np.ascontiguousarray(window, dtype=np.float64).reshape(7, 7)
        self.device = torch.device(device)
        self.window = torch.from_numpy(self.window_host).to(self.device)

    def moments(self, u8):
        """(N, H, W, 3) uint8 -> device tensor (2 scales, N, blocks, 5 maps, 5 moments) float64: the three launches."""
        if u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError(f"niqe: (N, H, W, 3) frames, got {tuple(u8.shape)}")
        check_size(u8.shape[1], u8.shape[2])
        y1, y2 = ops.niqe_luma(u8.contiguous())
        blocks = (y1.shape[1] // BLOCK) * (y1.shape[2] // BLOCK)
        out = torch.empty((2, u8.shape[0], blocks, 5, 5), dtype=torch.float64, device=u8.device)     # one copy to the host
        ops.niqe_moments(y1, BLOCK, 1.0, self.window, out=out[0])
        ops.niqe_moments(y2, BLOCK // 2, ops.NIQE_HALF_UNIT, self.window, out=out[1])
        return out

    def features(self, u8):
        """(N, H, W, 3) uint8 -> (N, blocks, 36) float64 features on the host, scale 1 first."""
        m = self.moments(u8).cpu().numpy()
        f = np.stack([features(m[0], BLOCK * BLOCK), features(m[1], BLOCK * BLOCK // 4)], axis=2)
        return f.reshape(f.shape[0], f.shape[1], FEATURES)

    def __call__(self, u8):
        return [score(f, self.mu, self.cov) for f in self.features(u8)]


def check_params(mu, cov, window, what="parameters"):
    """The loader's refusals on the three arrays -> them as float64 (36,), (36, 36), (7, 7)."""
    out = []
    for name, arr, shape in (("mu_pris_param", mu, (FEATURES,)), ("cov_pris_param", cov, (FEATURES, FEATURES)), ("gaussian_window", window, (7, 7))):
        arr = np.asarray(arr)
        if arr.size != KEYS[name] or not (arr.shape == shape or (name == "mu_pris_param" and arr.shape == (1, FEATURES))):
            raise ValueError(f"{what}: {name} has shape {tuple(arr.shape)}, not {shape}")
        if not np.issubdtype(arr.dtype, np.floating) or not np.isfinite(arr).all():
            raise ValueError(f"{what}: {name} must hold finite floating-point numbers")
        out.append(arr.astype(np.float64).reshape(shape))
    w = out[2]
    if not (np.array_equal(w, w[::-1]) and np.array_equal(w, w[:, ::-1]) and np.array_equal(w, w.T)):
        raise ValueError(f"{what}: gaussian_window is not symmetric under both flips and transposition")
    if abs(float(w.sum()) - 1.0) > 1e-12:
        raise ValueError(f"{what}: gaussian_window sums to {float(w.sum())!r}, not to 1 within 1e-12")
    return out


def load_niqe(path, device):
    """``NIQE`` on ``device`` from an ``.npz`` with mu_pris_param, cov_pris_param and gaussian_window (BasicSR's
    niqe_pris_params.npz).  FileNotFoundError, or ValueError for a missing key, a wrong shape, or a window that is not
    symmetric or does not sum to 1."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found")
    try:
        z = np.load(path, allow_pickle=False)
    except (OSError, EOFError, ValueError) as exc:
        raise ValueError(f"{path}: not an .npz file ({exc})")
    if not isinstance(z, np.lib.npyio.NpzFile):
        raise ValueError(f"{path}: not an .npz file (a single array)")
    with z:
        missing = [k for k in KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: missing keys: {', '.join(missing)} (holds {', '.join(z.files) or 'nothing'})")
        arrays = [z[k] for k in KEYS]
    return NIQE(*check_params(*arrays, what=str(path)), device)


def mean_of(values):
    """{niqe, niqe_frames} of per-frame values (None for a frame without a score): the mean over the frames that have one."""
    have = [v for v in values if v is not None]
    return dict(niqe=sum(have) / len(have) if have else None, niqe_frames=len(have))


def _jsonable(values):
    return [None if math.isnan(v) else v for v in values]


def score_paths(paths, sizes, device, model, batch=8):
    """Per-frame values (None where the score is NaN) of frame files whose sizes were checked, batched like evaluate."""
    from .metrics import _groups
    values = []
    for _first, (u8,) in fio.iter_frame_batches([paths], _groups(sizes, max(1, int(batch))), device):
        values += _jsonable(model(u8))
    return values


def niqe_dir(frames_dir, device, model, batch=8):
    """Score the frames of ``frames_dir`` in ``io.list_frames`` order: ``dict(frames=[{name, niqe}], mean={niqe, niqe_frames},
    count)``; ``niqe`` is None for a frame without a score (JSON null), which the mean leaves out.  ValueError for an empty
    directory or a frame with fewer than two blocks, checked on the file headers before anything is decoded."""
    paths = fio.list_frames(frames_dir)
    if not paths:
        raise ValueError(f"niqe: no frame files in {frames_dir}")
    sizes = [fio.frame_size(p) for p in paths]
    for p, (h, w) in zip(paths, sizes):
        check_size(h, w, what=f"{p}")
    values = score_paths(paths, sizes, device, model, batch)
    return dict(frames=[dict(name=os.path.basename(p), niqe=v) for p, v in zip(paths, values)], mean=mean_of(values), count=len(paths))


def format_value(v):
    """``  niqe 4.1234`` or ``  niqe n/a``: the piece every report line ends with."""
    return "  niqe n/a" if v is None else f"  niqe {v:.4f}"


def format_report(result):
    """One line per frame and the mean of the frames that have a score."""
    lines = [f["name"] + format_value(f["niqe"]) for f in result["frames"]]
    lines.append(f"mean of {result['mean']['niqe_frames']} of {result['count']} frames" + format_value(result["mean"]["niqe"]))
    return lines
