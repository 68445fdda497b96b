"""numpy restatement of the STATIC REGION DEFINITION (include/emavfi.h), written from its formulas: it looks at no kernel.

A frame is a flat array of samples (uint8, or uint16 words) in one of three dense layouts:
    "interleaved": [H][W][C];  "nv12": [H][W] Y, then [H/2][W/2] pairs {U, V};  "i420": Y, then U [H/2][W/2], then V [H/2][W/2].
A sample is the element itself (bytes), or (word >> shift) & (2^depth - 1).
"""
import numpy as np

LAYOUTS = {"interleaved": 0, "nv12": 1, "i420": 2}


def frame_samples(H, W, layout, C=1):
    """the number of samples of a dense frame"""
    return H * W * C if layout == "interleaved" else H * W * 3 // 2


def sample(x, depth=8, shift=0):
    return (np.asarray(x).astype(np.int64) >> shift) & ((1 << depth) - 1)


def planes(frame, H, W, layout, C=1):
    """views of the flat `frame`: interleaved -> ([H,W,C],); nv12 -> (Y [H,W], UV [H/2,W/2,2]); i420 -> (Y, U [H/2,W/2], V [H/2,W/2])"""
    f = np.asarray(frame).reshape(-1)
    assert f.size == frame_samples(H, W, layout, C), (f.size, H, W, layout, C)
    if layout == "interleaved":
        return (f.reshape(H, W, C),)
    assert H % 2 == 0 and W % 2 == 0
    y = f[:H * W].reshape(H, W)
    if layout == "nv12":
        return y, f[H * W:].reshape(H // 2, W // 2, 2)
    q = H * W // 4
    return y, f[H * W:H * W + q].reshape(H // 2, W // 2), f[H * W + q:].reshape(H // 2, W // 2)


def same_map(a, b, H, W, layout, C=1, depth=8, shift=0, tol=0):
    """bool [H, W]: same(y, x)"""
    pa, pb = planes(a, H, W, layout, C), planes(b, H, W, layout, C)
    ok = [np.abs(sample(x, depth, shift) - sample(y, depth, shift)) <= tol for x, y in zip(pa, pb)]
    if layout == "interleaved":
        return ok[0].all(axis=2)
    chroma = ok[1].all(axis=2) if layout == "nv12" else ok[1] & ok[2]
    return ok[0] & np.repeat(np.repeat(chroma, 2, axis=0), 2, axis=1)       # the chroma sample at (y >> 1, x >> 1)


def core_map(same, r):
    """bool [H, W]: every pixel of the window of radius r, clipped to the frame, is `same` - by an integral image of the differing pixels"""
    H, W = same.shape
    ii = np.zeros((H + 1, W + 1), dtype=np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(~same, axis=0, dtype=np.int64), axis=1)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r, H - 1) + 1
    x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r, W - 1) + 1
    bad = ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]
    return bad == 0


def chroma_core(core):
    """bool [H/2, W/2]: all four luma pixels (2 i + {0, 1}, 2 j + {0, 1}) are core"""
    return core[0::2, 0::2] & core[0::2, 1::2] & core[1::2, 0::2] & core[1::2, 1::2]


def apply(d, a, core, H, W, layout, C=1):
    """a copy of the flat frame `d` with a's elements (whole words) at the replaced positions"""
    out = np.array(d).reshape(-1).copy()
    po, pa = planes(out, H, W, layout, C), planes(a, H, W, layout, C)
    if layout == "interleaved":
        po[0][core] = pa[0][core]
        return out
    po[0][core] = pa[0][core]
    cc = chroma_core(core)
    for o, s in zip(po[1:], pa[1:]):
        o[cc] = s[cc]
    return out


def guard(d, a, b, H, W, layout, C=1, depth=8, shift=0, radius=0, tol=0):
    """(the guarded copy of d, the number of core pixels, core)"""
    core = core_map(same_map(a, b, H, W, layout, C, depth, shift, tol), radius)
    return apply(d, a, core, H, W, layout, C), int(core.sum()), core
