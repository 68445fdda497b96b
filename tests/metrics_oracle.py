"""numpy restatement of the frame-metric definition (include/emavfi.h, "FRAME METRIC DEFINITION"), written from the formulas - the oracle of
tests/test_metrics_cpu.py, tests/test_gpu_metrics.py and tests/test_gpu_evaluate.py: int64 moments, the float64 tail in the stated operation
order, the quantised sum; beside it a plain real-valued-Gaussian SSIM.  Nothing here looks at the kernels."""
import math

import numpy as np

WIN = 11
SIGMA = 1.5
MAX_DIM = 16384
Q = 2 ** 32
C1 = 6.5025                  # (0.01 * 255)^2 and (0.03 * 255)^2 as decimal literals: the doubles nearest them, not the rounded products
C2 = 58.5225
G = (67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67)


def gaussian():
    """the normalised real-valued per-axis weights"""
    g = np.exp(-((np.arange(WIN) - WIN // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def weights_by_rule():
    """floor(g_real 65536 + 0.5), the centre raised by what is missing to 65536"""
    w = np.floor(gaussian() * 65536.0 + 0.5).astype(np.int64)
    w[WIN // 2] += 65536 - w.sum()
    return tuple(int(v) for v in w)


def windows(H, W):
    return max(H - WIN + 1, 0) * max(W - WIN + 1, 0)


def _filter(img, g):
    """valid separable 11 x 11 filtering of [..., H, W] along the last two axes, in img's dtype"""
    H, W = img.shape[-2:]
    rows = sum(g[j] * img[..., :, j:j + W - WIN + 1] for j in range(WIN))
    return sum(g[i] * rows[..., i:i + H - WIN + 1, :] for i in range(WIN))


def sse(a, b):
    """uint8 [..., H, W, C] -> int64 [..., C]"""
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).sum((-3, -2))


def moments(a, b):
    """uint8 [..., H, W] planes -> the five int64 moment maps [..., H - 10, W - 10], each below 65025 * 2^32"""
    g = np.array(G, dtype=np.int64)
    a, b = a.astype(np.int64), b.astype(np.int64)
    out = tuple(_filter(v, g) for v in (a, b, a * a, b * b, a * b))
    for m in out:
        assert m.size == 0 or (m.min() >= 0 and m.max() <= 65025 * Q)
    return out


def tail(A, B, Axx, Ayy, Axy):
    """the float64 tail in the definition's operation order -> int64 q per window"""
    s = 1.0 / Q
    a, b, axx, ayy, axy = (np.asarray(v, dtype=np.int64).astype(np.float64) * s for v in (A, B, Axx, Ayy, Axy))
    aa, bb, ab = a * a, b * b, a * b
    sx, sy, sxy = axx - aa, ayy - bb, axy - ab
    num = (2.0 * ab + C1) * (2.0 * sxy + C2)
    den = ((aa + bb) + C1) * ((sx + sy) + C2)
    m = num / den
    return np.floor(m * 4294967296.0).astype(np.int64)


def ssimq(a, b):
    """uint8 [..., H, W, C] -> int64 [..., C]: the sum of q over the windows, 0 where there is none"""
    H, W, C = a.shape[-3:]
    if H < WIN or W < WIN:
        return np.zeros((*a.shape[:-3], C), dtype=np.int64)
    pa, pb = np.moveaxis(a, -1, -3), np.moveaxis(b, -1, -3)           # [..., C, H, W]
    return tail(*moments(pa, pb)).sum((-2, -1))


def metrics(a, b):
    """uint8 [B, H, W, C] pairs -> int64 [B, C, 2] = {sse, ssimq}: what emavfi_frame_metrics_u8 writes"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8 and a.ndim == 4
    assert 1 <= a.shape[3] <= 4 and 1 <= min(a.shape[1:3]) and max(a.shape[1:3]) <= MAX_DIM
    return np.stack([sse(a, b), ssimq(a, b)], axis=-1)


def psnr(sse_, n):
    return math.inf if sse_ == 0 else 10.0 * math.log10(255.0 * 255.0 * n / sse_)


def ssim(ssimq_, H, W):
    n = windows(H, W)
    return math.nan if n == 0 else ssimq_ / (float(Q) * n)


def ssim_real(a, b):
    """the plain SSIM of Wang et al. with real-valued Gaussian weights, float64 throughout: uint8 [H, W] planes -> float"""
    g = gaussian()
    a, b = a.astype(np.float64), b.astype(np.float64)
    mu_a, mu_b = _filter(a, g), _filter(b, g)
    sx, sy, sxy = _filter(a * a, g) - mu_a * mu_a, _filter(b * b, g) - mu_b * mu_b, _filter(a * b, g) - mu_a * mu_b
    m = ((2.0 * mu_a * mu_b + C1) * (2.0 * sxy + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (sx + sy + C2))
    return float(m.mean())
