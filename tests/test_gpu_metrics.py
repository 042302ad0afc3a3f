"""GPU: flair_image_metrics (csrc/metrics.hip) against the float64 numpy reference of tests/metrics_ref.py.

The squared error must be the exact integer.  Per-frame SSIM must be within 1e-4 of the reference: a float32 emulation of
the algorithm over these input families at sizes 11..70 is off by at most 1.0e-5 per frame (the near-flat family is the
worst), and the reports print four decimals, so 1e-4 is the condition.  Every launch runs on inputs, outputs and a
workspace that sit inside larger allocations whose guard values must come back unchanged."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr
from tests import util

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-4


def shapes():
    """(N, H, W): one SSIM sample; a map narrower than a tile; a map wider than a tile in one direction only; and, derived
    from the kernel's tile (flair_amd.metrics.TILE_H x TILE_W map pixels per workgroup), a map of two whole tiles plus a
    part of a third in both directions, neither a multiple of the tile: H = 2 TILE_H + 11 + 10, W = 2 TILE_W + 5 + 10."""
    from flair_amd.metrics import TILE_H, TILE_W
    return [(1, 11, 11), (2, 12, 43), (3, 45, 70), (2, 2 * TILE_H + 21, 2 * TILE_W + 15)]


SHAPE_IDS = ["one_sample", "12x43", "45x70", "three_tiles_each_way"]
FAMILIES = ["noisy_copy", "near_flat", "black_vs_rows", "inverse", "mixed"]


def family(name, n, H, W):
    """Frame n of an input family as two (H, W, 3) uint8 arrays; every frame of a call differs from the others."""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + 17 * n + H + 7 * W)
    if name == "mixed":                                  # another family per frame: a mix-up between frames shows
        return family(FAMILIES[(n + 1) % 4], n + 5, H, W)
    if name == "noisy_copy":
        a = rng.integers(0, 256, (H, W, 3))
        b = np.clip(a + np.rint(rng.normal(0, 6 + 10 * n, (H, W, 3))), 0, 255)
    elif name == "near_flat":
        a, b = rng.integers(127, 129, (H, W, 3)), rng.integers(127, 129, (H, W, 3))
    elif name == "black_vs_rows":
        a = np.zeros((H, W, 3))
        b = np.zeros((H, W, 3))
        b[(1 + n) % 2::2] = 255
    else:
        a = rng.integers(0, 256, (H, W, 3))
        b = 255 - a
    return a.astype(np.uint8), b.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """The frames of one (family, shape) and their reference, computed once and shared (read-only) by the tests."""
    N, H, W = shape
    pairs = [family(name, n, H, W) for n in range(N)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for arr in (a, b):
        arr.setflags(write=False)
    return a, b, mr.reference(a, b)


def run_guarded(a, b, dev):
    """One call of the entry through its ctypes binding on guarded buffers -> the (N, 4) float64 rows on the host."""
    from flair_amd import _lib
    N, H, W, _ = a.shape
    abuf, av, a0 = util.flat_guarded(a.shape, torch.uint8, dev, 0x5A, src=torch.tensor(a))
    bbuf, bv, b0 = util.flat_guarded(b.shape, torch.uint8, dev, 0xA5, src=torch.tensor(b))
    obuf, ov, o0 = util.flat_guarded((N, 4), torch.float64, dev, util.OUT_FILL)
    nbytes = _lib.image_metrics_workspace(N, H, W)
    assert nbytes > 0 and nbytes % 8 == 0
    wbuf, wv, w0 = util.flat_guarded((nbytes // 8,), torch.float64, dev, util.OUT_FILL)
    rc = _lib.image_metrics(_lib.ptr(av), _lib.ptr(bv), N, H, W, _lib.ptr(ov), _lib.ptr(wv), nbytes)
    _lib.check(rc, "flair_image_metrics")
    torch.cuda.synchronize()
    util.assert_flat_untouched(abuf, a0, what="a")
    util.assert_flat_untouched(bbuf, b0, what="b")
    util.assert_flat_untouched(obuf, o0, view=ov, what="out")
    util.assert_flat_untouched(wbuf, w0, view=wv, what="workspace")
    return ov.cpu().numpy().copy()


WORST = {}


@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
@pytest.mark.parametrize("name", FAMILIES)
def test_sse_exact_and_ssim_within_1e4(dev, name, shape):
    a, b, (sse, sums, ssim, psnr) = case(name, shape)
    N, H, W = shape
    rows = run_guarded(a, b, dev)
    got_ssim = rows[:, 1:].sum(1) / (3.0 * (H - 10) * (W - 10))
    err = np.abs(got_ssim - ssim)
    err_ch = np.abs(rows[:, 1:] - sums).max() / ((H - 10) * (W - 10))
    WORST[(name, shape)] = err.max()
    print(f"image_metrics {name} {N}x{H}x{W}: max per-frame |ssim - ref| = {err.max():.3e} (per channel {err_ch:.3e}), "
          f"worst so far {max(WORST.values()):.3e}")
    assert rows[:, 0].astype(np.int64).tolist() == sse.tolist() and (rows[:, 0] == np.floor(rows[:, 0])).all()
    assert err.max() <= SSIM_TOL, (name, shape, err.tolist())
    assert np.isfinite(rows).all()


@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
def test_psnr_ssim_of_the_wrapper(dev, shape):
    """metrics.psnr_ssim (ops.image_metrics, the library's own workspace) gives the reference's PSNR, SSIM and integers."""
    from flair_amd import metrics
    a, b, (sse, sums, ssim, psnr) = case("noisy_copy", shape)
    got = metrics.psnr_ssim(torch.tensor(a).to(dev), torch.tensor(b).to(dev))
    assert got["sse"] == sse.tolist()
    assert np.abs(np.array(got["psnr"]) - psnr).max() <= 1e-9
    assert np.abs(np.array(got["ssim"]) - ssim).max() <= SSIM_TOL


@pytest.mark.parametrize("shape", shapes(), ids=SHAPE_IDS)
def test_identical_inputs(dev, shape):
    from flair_amd import metrics
    for name in ("noisy_copy", "near_flat", "black_vs_rows"):
        a = torch.tensor(case(name, shape)[1]).to(dev)
        got = metrics.psnr_ssim(a, a.clone())
        assert got["sse"] == [0] * shape[0] and all(p == math.inf for p in got["psnr"])
        assert min(got["ssim"]) >= 1 - 1e-6 and max(got["ssim"]) <= 1 + 1e-6, got["ssim"]


@pytest.mark.parametrize("name", ["noisy_copy", "mixed"])
def test_same_bits_every_run_and_for_every_batch(dev, name):
    """No floating-point atomics: two calls agree bit for bit, and frame n of a call with N = 3 carries the bits of a call
    on frame n alone (at the three-frame shape and at the shape of several tiles per frame)."""
    from flair_amd import ops
    from flair_amd.metrics import TILE_H, TILE_W
    for shape in [(3, 45, 70), (3, 2 * TILE_H + 21, 2 * TILE_W + 15)]:
        a, b, _ = case(name, shape)
        a, b = torch.tensor(a).to(dev), torch.tensor(b).to(dev)
        first = ops.image_metrics(a, b).clone()
        again = ops.image_metrics(a, b)
        assert torch.equal(util.bits(first), util.bits(again))
        for n in range(3):
            one = ops.image_metrics(a[n:n + 1].contiguous(), b[n:n + 1].contiguous())
            assert torch.equal(util.bits(one[0]), util.bits(first[n])), (shape, n)


def test_wrapper_refusals_reach_the_entry(dev):
    from flair_amd import _lib, ops
    a = torch.zeros(1, 10, 32, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FlairHipError, match="flair_image_metrics.*smaller than the 11x11"):
        ops.image_metrics(a, a)
