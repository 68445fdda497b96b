"""numpy restatement of the align definition of include/emavfi.h ("ALIGN DEFINITION"): the signature grid of a normalised fp32 batch, the
mean absolute difference of every candidate shift, the choice with its tie rule and acceptance, and the shift as a pure gather of 32-bit
words - the arrays are indexed through their uint32 view, so no bit pattern is touched.  Everything after the pixel's fp32 sum and its
product with 64 is integer arithmetic in Python ints or int64, written from the text of the definition and not from the kernels."""
import numpy as np

from ensemble_oracle import checksum, generated   # noqa: F401  (the generator and the checksum the host checks share)

CELL = 4
MAX_RADIUS = 32
MAX_RATIO = 1024
MAX_HALF = 16384


def quantise(x):
    """q of step 1 per pixel: float32 [..., 3, H, W] -> int64 [..., H, W]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.shape[-3] == 3
    with np.errstate(all="ignore"):
        l = (x[..., 0, :, :] + x[..., 1, :, :]) + x[..., 2, :, :]
        t = l * np.float32(64.0)
        assert l.dtype == np.float32 and t.dtype == np.float32
        mid = np.floor(np.where(np.isfinite(t), t, np.float32(0.0))).astype(np.int64) + 512
        return np.where(~(t >= np.float32(-512.0)), 0, np.where(t >= np.float32(512.0), 1023, mid))


def signature(x):
    """G of step 1: float32 [B, 3, H, W] -> uint16 [B, H // 4, W // 4]; the remainder rows and columns are not looked at"""
    q = quantise(x)
    B, H, W = q.shape
    Hc, Wc = H // CELL, W // CELL
    g = q[:, :Hc * CELL, :Wc * CELL].reshape(B, Hc, CELL, Wc, CELL).sum(axis=(2, 4))
    assert g.min() >= 0 and g.max() <= 16 * 1023
    return g.astype(np.uint16)


def scores(ga, gb, R):
    """m(d) of step 2 for one sample: two uint16 [Hc, Wc] grids -> {(dy, dx): m} over the (2R + 1)^2 candidates, Python ints"""
    ga, gb = np.asarray(ga).astype(np.int64), np.asarray(gb).astype(np.int64)
    Hc, Wc = ga.shape
    assert ga.shape == gb.shape and 1 <= R <= MAX_RADIUS and 2 * R <= min(Hc, Wc)
    m = {}
    for dy in range(-R, R + 1):
        ya, yb = slice(max(0, -dy), Hc - max(0, dy)), slice(max(0, dy), Hc - max(0, -dy))
        for dx in range(-R, R + 1):
            xa, xb = slice(max(0, -dx), Wc - max(0, dx)), slice(max(0, dx), Wc - max(0, -dx))
            sad = int(np.abs(ga[ya, xa] - gb[yb, xb]).sum())
            n = (Hc - abs(dy)) * (Wc - abs(dx))
            assert ga[ya, xa].size == n
            m[(dy, dx)] = sad * 256 // n
    return m


def choose(m, ratio):
    """steps 3's record {4 dy*, 4 dx*, m(d*), m(0)} from the scores of one sample"""
    assert 0 <= ratio <= MAX_RATIO
    least = min(m.values())
    left = [d for d, v in m.items() if v == least]
    l1 = min(abs(dy) + abs(dx) for dy, dx in left)
    left = [d for d in left if abs(d[0]) + abs(d[1]) == l1]
    ly = min(abs(dy) for dy, _ in left)
    left = [d for d in left if abs(d[0]) == ly]
    best = left[0] if len(left) == 1 else (0, 0)
    if best != (0, 0) and not m[best] * 1024 <= m[(0, 0)] * ratio:
        best = (0, 0)
    return [CELL * best[0], CELL * best[1], m[best], m[(0, 0)]]


def search(sig_a, sig_b, R, ratio):
    """the records of a batch: two uint16 [B, Hc, Wc] -> int32 [B, 4]"""
    return np.array([choose(scores(a, b, R), ratio) for a, b in zip(sig_a, sig_b)], dtype=np.int32)


def half(d_px):
    """the half-shift of a recorded word, whatever it holds: an arithmetic shift, clamped to +-16384"""
    return min(max(int(d_px) >> 1, -MAX_HALF), MAX_HALF)


def shift(x, shifts, sign):
    """step 4: out[b][c][y][x] = x[b][c][cy(y - sign hy)][cx(x - sign hx)] over a float32 [B, C, H, W] array, words 2 and 3 of a record
    not looked at"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and sign in (1, -1)
    B, C, H, W = x.shape
    words, out = x.view(np.uint32), np.empty(x.shape, np.uint32)
    for b in range(B):
        my, mx = sign * half(shifts[b][0]), sign * half(shifts[b][1])
        iy = np.clip(np.arange(H, dtype=np.int64) - my, 0, H - 1)
        ix = np.clip(np.arange(W, dtype=np.int64) - mx, 0, W - 1)
        out[b] = words[b][:, iy, :][:, :, ix]
    return out.view(np.float32)


def align_pair(a, b, R_px, ratio_units):
    """(a', b', records) of two float32 [B, 3, H, W] batches; the radius in pixels, the ratio in 1024ths"""
    rec = search(signature(a), signature(b), R_px // CELL, ratio_units)
    return shift(a, rec, 1), shift(b, rec, -1), rec


def interior(H, W, rec):
    """the slices of the positions of a' and b' whose source indices were not clamped, for one record"""
    hy, hx = abs(half(rec[0])), abs(half(rec[1]))
    return slice(hy, H - hy), slice(hx, W - hx)


def planted(frames, H, W, dy, dx, top=48, left=64):
    """a pair cut from one float32 [3, Hf, Wf] picture: a at (top, left), b the window whose content sits (dy, dx) pixels further - the
    content of a at (y, x) is b's at (y + dy, x + dx)"""
    a = frames[:, top:top + H, left:left + W]
    b = frames[:, top - dy:top - dy + H, left - dx:left - dx + W]
    return np.ascontiguousarray(a)[None], np.ascontiguousarray(b)[None]


def host_case():
    """the pair of tests/host/host_check_align.cpp: a = generated(0, 3 * 16 * 24) / 128 as [1, 3, 16, 24], b = a moved by (4, -4) pixels with
    replicated edges"""
    a = (generated(0, 3 * 16 * 24) / np.float32(128.0)).astype(np.float32).reshape(1, 3, 16, 24)
    b = shift(a, [[8, -8, 0, 0]], 1)
    return a, b
