"""numpy / Fraction restatement of the duplicate-frame definition (include/emavfi.h, "DUPLICATE FRAME DEFINITION"), written from the formulas -
the oracle of tests/test_dedup_cpu.py and tests/test_gpu_dedup.py: the cell measures, score and flag of an image pair in int64, the kept
frames by the rules as stated, and the schedule worked out on a brute-force timeline of exact rationals instead of the integer recurrences
the harness uses.  Nothing here imports the package or looks at the kernels; cells and 3-byte luma are the scene definition's
(tests/scene_oracle.py)."""
from fractions import Fraction
from math import floor

import numpy as np

import scene_oracle

CELLS = scene_oracle.SIG_WORDS
MAX_DEPTH = 5           # the deepest dyadic tree of the temporal resample definition


def threshold_units(fraction, depth=8):
    return floor(Fraction(fraction) * 16 * (2 ** depth - 1))


def luma(img, order="bgr", depth=8, shift=0):
    """uint8 [..., H, W, C] (C = 1 or 3) or uint16 [..., H, W] words -> int64 [..., H, W]"""
    if img.dtype == np.uint8:
        assert depth == 8 and shift == 0
        return scene_oracle.luma(img, order)
    assert img.dtype == np.uint16 and depth in (10, 12, 16) and 0 <= shift <= 16 - depth
    return (img.astype(np.int64) >> shift) & (2 ** depth - 1)


def cells(a, b, order="bgr", depth=8, shift=0):
    """-> int64 [..., 1024]: per cell the ceiling of the mean absolute luma difference in sixteenths of a count, 0 for an empty cell"""
    d = np.abs(luma(a, order, depth, shift) - luma(b, order, depth, shift))
    H, W = d.shape[-2:]
    assert 1 <= min(H, W) and max(H, W) <= scene_oracle.MAX_DIM
    S = np.zeros((*d.shape[:-2], H + 1, W + 1), dtype=np.int64)          # integral image
    S[..., 1:, 1:] = d.cumsum(-2).cumsum(-1)
    yb, xb = scene_oracle.bounds(H), scene_oracle.bounds(W)
    sad = S[..., yb[1:], :][..., xb[1:]] - S[..., yb[:-1], :][..., xb[1:]] - S[..., yb[1:], :][..., xb[:-1]] + S[..., yb[:-1], :][..., xb[:-1]]
    n = scene_oracle.cell_pixels(H, W)
    m = np.where(n > 0, (16 * sad + n - 1) // np.maximum(n, 1), 0)
    assert m.min() >= 0 and m.max() <= 16 * (2 ** depth - 1)
    return m.reshape(*d.shape[:-2], CELLS)


def score(c):
    return np.asarray(c).max(-1)


def flags(c, threshold):
    return (score(c) <= threshold).astype(np.int64)


# ---------------------------------------------------------------- the schedule
def kept(flagged, n, base=0, max_run=3, span=64):
    """local indices of the kept frames: a frame is dropped when its pair with the frame before it is flagged and no rule keeps it"""
    out, dropped = [], []                       # dropped: the frames dropped since the last kept one
    for t in range(n):
        rules = (t == 0, t == n - 1, (base + t) % span == 0, len(dropped) == max_run)
        if t > 0 and flagged[t - 1] and not any(rules):
            dropped.append(t)
        else:
            out.append(t)
            dropped = []
    return out


def log2_ceil(m):
    c = 0
    while 2 ** c < m:
        c += 1
    return c


def plan(kept_frames, rate_in, rate_out, depth, method, base=0, tail=True):
    """[(k, t_i, m, j0, j1, w)] with global indices: every output k >= 0 whose rational time k Fi / Fo falls into a gap of the kept frames, and
    (tail) the one that falls on the last kept frame; w = 256 normalised to node j0 + 1 alone"""
    step = Fraction(rate_in) / Fraction(rate_out)
    anchors = [base + t for t in kept_frames]
    out = []
    if not anchors:
        return out
    k = 0
    while k * step <= anchors[-1]:
        t = k * step
        k += 1
        if t < anchors[0]:
            continue
        if t == anchors[-1]:
            if tail:
                out.append((k - 1, anchors[-1], 1, 0, 0, 0))
            continue
        t0, t1 = next((a, b) for a, b in zip(anchors, anchors[1:]) if a <= t < b)
        m = t1 - t0
        G = 2 ** (depth + log2_ceil(m))
        pos = (t - t0) / m * G                  # the position in node units of the gap's tree, 0 <= pos < G
        if method == "nearest":
            j = floor(pos + Fraction(1, 2))     # a tie goes to the later node
            out.append((k - 1, t0, m, j, j, 0))
        else:
            j0 = floor(pos)
            w = floor(256 * (pos - j0) + Fraction(1, 2))
            out.append((k - 1, t0, m, j0 + 1, j0 + 1, 0) if w == 256 else (k - 1, t0, m, j0, j0, 0) if w == 0 else (k - 1, t0, m, j0, j0 + 1, w))
    return out


def parents(j):
    return j - (j & -j), j + (j & -j)


def needed(nodes, depth):
    """the smallest set that holds the inner nodes of `nodes` and is closed under parents"""
    G, need = 1 << depth, set()
    grow = {j for j in nodes if 0 < j < G}
    while grow:
        need |= grow
        grow = {p for j in grow for p in parents(j) if 0 < p < G} - need
    return need
