"""Float64 numpy reference of the image metrics (flair_amd.metrics, csrc/metrics.hip): the squared error in int64 and
SSIM as the restoration literature computes it on RGB (Wang et al. 2004; BasicSR's calculate_ssim): 11 x 11 Gaussian
window of sigma 1.5 normalised to sum 1, applied separably to the valid region only, on the 0..255 scale."""
import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian_window(size=11, sigma=1.5):
    d = np.arange(size, dtype=np.float64) - (size - 1) / 2
    g = np.exp(-d * d / (2 * sigma * sigma))
    return g / g.sum()


def valid_filter(img, g=None):
    """Separable valid correlation of an (..., H, W) float64 array -> (..., H - 10, W - 10)."""
    g = gaussian_window() if g is None else g
    k = len(g)
    H, W = img.shape[-2:]
    rows = sum(g[i] * img[..., :, i:i + W - k + 1] for i in range(k))
    return sum(g[i] * rows[..., i:i + H - k + 1, :] for i in range(k))


def ssim_map(x, y):
    """x, y: (..., H, W) arrays on the 0..255 scale -> the SSIM map (..., H - 10, W - 10) in float64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = valid_filter(x), valid_filter(y)
    vx, vy, cxy = valid_filter(x * x) - mx * mx, valid_filter(y * y) - my * my, valid_filter(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def reference(a, b):
    """a, b: (N, H, W, 3) uint8 arrays -> (sse int64 [N], channel SSIM sums float64 [N, 3], ssim float64 [N], psnr [N])."""
    a, b = np.asarray(a), np.asarray(b)
    N, H, W, _ = a.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    sse = (d * d).reshape(N, -1).sum(1)
    m = ssim_map(a.transpose(0, 3, 1, 2), b.transpose(0, 3, 1, 2))          # (N, 3, H - 10, W - 10)
    sums = m.reshape(N, 3, -1).sum(2)
    ssim = sums.sum(1) / (3.0 * (H - 10) * (W - 10))
    with np.errstate(divide="ignore"):
        psnr = np.where(sse == 0, np.inf, 10 * np.log10(255.0 ** 2 * 3 * H * W / np.maximum(sse, 1)))
    return sse, sums, ssim, psnr
