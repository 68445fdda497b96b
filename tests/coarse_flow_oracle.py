"""numpy restatement of steps 1 and 3 of the coarse flow definition of include/emavfi.h ("COARSE FLOW DEFINITION"): the balanced quadtree
mean of s x s blocks of clamped leaves, and the bilinear flow upsample at half-pixel centres times s.  Every operation is one numpy
float32 operation on whole arrays - numpy never reassociates or contracts - in the definition's order; the weights are built from the
integer formulas.  Also the generated case of tests/host/host_check_coarse.cpp."""
import numpy as np

from ensemble_oracle import checksum, generated   # noqa: F401  (the generator and the checksum the host checks share)

SCALES = (2, 4, 8)


def coarse_size(H, W, s):
    assert s in SCALES and H >= 1 and W >= 1
    return (H + s - 1) // s, (W + s - 1) // s


def down(x, s):
    """down_s over the last two axes of a float32 array"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2 and s in SCALES
    H, W = x.shape[-2:]
    Hs, Ws = coarse_size(H, W, s)
    # the leaves, clamped once: L[..., i, r, j, c] = x[min(s i + r, H - 1)][min(s j + c, W - 1)]
    ys = np.minimum(np.arange(Hs * s), H - 1)
    xs = np.minimum(np.arange(Ws * s), W - 1)
    t = x[..., ys, :][..., :, xs]                       # [..., Hs * s, Ws * s]: T_1 of every block side by side
    quarter = np.float32(0.25)
    m = 1
    while m < s:
        # T_2m(r, c) = ((T_m(2r, 2c) + T_m(2r, 2c+1)) + (T_m(2r+1, 2c) + T_m(2r+1, 2c+1))) * 0.25f; the blocks' sides are even at every level,
        # so pairing rows and columns of the whole array never pairs across two blocks
        top = t[..., 0::2, 0::2] + t[..., 0::2, 1::2]
        bot = t[..., 1::2, 0::2] + t[..., 1::2, 1::2]
        t = (top + bot) * quarter
        assert t.dtype == np.float32
        m *= 2
    assert t.shape[-2:] == (Hs, Ws)
    return np.ascontiguousarray(t)


def tap(d, n, s):
    """(j0, j1, w) of one axis: destination index d, coarse length n"""
    num = 2 * d + 1 - s
    i0 = num // (2 * s)                                 # Python's // is the floor
    w = np.float32(num - 2 * s * i0) / np.float32(2 * s)
    return min(max(i0, 0), n - 1), min(max(i0 + 1, 0), n - 1), w


def taps(N, n, s):
    t = [tap(d, n, s) for d in range(N)]
    return (np.array([a for a, _, _ in t], np.int64), np.array([b for _, b, _ in t], np.int64), np.array([w for _, _, w in t], np.float32))


def up(p, size, s, rows=None):
    """step 3 over the last two axes of a float32 array [..., Hs, Ws] -> [..., H, W]; `rows`: only these destination rows, in this order
    (a sample of a large tensor)"""
    p = np.ascontiguousarray(p)
    H, W = size
    assert p.dtype == np.float32 and p.ndim >= 2 and s in SCALES and p.shape[-2:] == coarse_size(H, W, s)
    y0, y1, wy = taps(H, p.shape[-2], s)
    x0, x1, wx = taps(W, p.shape[-1], s)
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        y0, y1, wy, H = y0[rows], y1[rows], wy[rows], len(rows)
    one = np.float32(1.0)
    r0, r1 = p[..., y0, :], p[..., y1, :]
    top = (one - wx) * r0[..., :, x0] + wx * r0[..., :, x1]
    bot = (one - wx) * r1[..., :, x0] + wx * r1[..., :, x1]
    wy = wy[:, None]
    v = (one - wy) * top + wy * bot
    out = np.float32(s) * v
    assert out.dtype == np.float32 and out.shape[-2:] == (H, W)
    return np.ascontiguousarray(out)


def host_case():
    """the 2-plane 5 x 7 tensor of tests/host/host_check_coarse.cpp: generated(0, 70)"""
    return generated(0, 70).reshape(2, 5, 7)
