"""numpy int64 restatement of the scene-cut definition (include/emavfi.h, "SCENE CUT DEFINITION"), written from the formulas - the oracle of
tests/test_scene_cpu.py and tests/test_gpu_scene.py.  Nothing here looks at the kernels."""
import math

import numpy as np

GRID = 32
SIG_WORDS = GRID * GRID
MAX_DIM = 16384
MEAN_MAX = 16 * 255                      # a cell's mean in sixteenths of a count
LUMA = (313524, 615514, 119538)          # R, G, B: the BT.601 full-range encode row, sum 2^20


def bounds(n):
    """first index of cell 0..32 along an axis of n pixels: floor(i n / 32)"""
    return (np.arange(GRID + 1, dtype=np.int64) * n) // GRID


def cell_pixels(H, W):
    """[32, 32]: the number of pixels in each cell (0: an empty cell)"""
    return np.outer(np.diff(bounds(H)), np.diff(bounds(W)))


def cells(H, W):
    return min(H, GRID) * min(W, GRID)


def luma(img, order="bgr"):
    """uint8 [..., H, W, C], C = 1 or 3 -> int64 [..., H, W]"""
    p = img.astype(np.int64)
    if img.shape[-1] == 1:
        return p[..., 0]
    assert img.shape[-1] == 3 and order in ("bgr", "rgb")
    r, g, b = (p[..., 0], p[..., 1], p[..., 2]) if order == "rgb" else (p[..., 2], p[..., 1], p[..., 0])
    v = (LUMA[0] * r + LUMA[1] * g + LUMA[2] * b + 2 ** 19) >> 20
    assert v.min() >= 0 and v.max() <= 255
    return v


def signature(img, order="bgr"):
    """uint8 [..., H, W, C] -> int64 [..., 1024]: the luma sum of each cell, 0 for an empty cell"""
    y = luma(img, order)
    H, W = y.shape[-2:]
    assert 1 <= min(H, W) and max(H, W) <= MAX_DIM
    S = np.zeros((*y.shape[:-2], H + 1, W + 1), dtype=np.int64)          # integral image
    S[..., 1:, 1:] = y.cumsum(-2).cumsum(-1)
    yb, xb = bounds(H), bounds(W)
    sig = S[..., yb[1:], :][..., xb[1:]] - S[..., yb[:-1], :][..., xb[1:]] - S[..., yb[1:], :][..., xb[:-1]] + S[..., yb[:-1], :][..., xb[:-1]]
    return sig.reshape(*y.shape[:-2], SIG_WORDS)


def means(sig, H, W):
    """[..., 1024] sums -> the cells' means in sixteenths of a count, rounded; 0 for an empty cell"""
    n = cell_pixels(H, W).reshape(SIG_WORDS)
    num = 16 * np.asarray(sig, dtype=np.int64) + n // 2
    assert num.max() < 2 ** 31
    return np.where(n > 0, num // np.maximum(n, 1), 0)


def score(sig_a, sig_b, H, W):
    return np.abs(means(sig_a, H, W) - means(sig_b, H, W)).sum(-1)


def threshold_units(fraction, H, W):
    return int(math.ceil(fraction * (MEAN_MAX * cells(H, W))))
