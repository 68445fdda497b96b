"""numpy int64 restatement of the resize definition (include/emavfi.h, "RESIZE DEFINITION"), written from the formulas - the oracle of
tests/test_resize_cpu.py and tests/test_gpu_resize.py.  Nothing here looks at the kernels."""
import numpy as np

MAX_DIM = 16384


def axis(nd, ns, align_corners=False):
    """(i0, i1, w) per destination index: source indices and the 11-bit weight of the second.  `align_corners=True` is NOT the definition:
    it is the deliberately wrong geometry (no half-pixel shift) the tests use to show that they can tell the two apart."""
    d = np.arange(nd, dtype=np.int64)
    if align_corners:
        den = max(nd - 1, 1)
        num = d * (ns - 1)                      # position d (ns - 1) / (nd - 1)
        i0 = num // den
        w = ((num - i0 * den) * 2048 + den // 2) // den
    else:
        num = np.clip((2 * d + 1) * ns - nd, 0, 2 * nd * (ns - 1))
        i0 = num // (2 * nd)
        fr = num - i0 * 2 * nd
        w = (fr * 2048 + nd) // (2 * nd)
    return i0, np.minimum(i0 + 1, ns - 1), w


def resize(img, size, align_corners=False):
    """uint8 [..., Hs, Ws, C] -> uint8 [..., Hd, Wd, C], every channel on its own"""
    Hd, Wd = size
    Hs, Ws = img.shape[-3:-1]
    assert 1 <= min(Hd, Wd, Hs, Ws) and max(Hd, Wd, Hs, Ws) <= MAX_DIM
    y0, y1, wy = axis(Hd, Hs, align_corners)
    x0, x1, wx = axis(Wd, Ws, align_corners)
    p = img.astype(np.int64)
    wx, wy = wx[:, None], wy[:, None, None]
    top = (2048 - wx) * p[..., y0, :, :][..., :, x0, :] + wx * p[..., y0, :, :][..., :, x1, :]
    bot = (2048 - wx) * p[..., y1, :, :][..., :, x0, :] + wx * p[..., y1, :, :][..., :, x1, :]
    v = ((2048 - wy) * top + wy * bot + 2 ** 21) >> 22
    assert v.min() >= 0 and v.max() <= 255 and ((2048 - wy) * top + wy * bot + 2 ** 21).max() < 2 ** 31
    return v.astype(np.uint8)


def resize_nv12(y, uv, size):
    """Y [..., Hs, Ws] as a 1-channel image to Hd x Wd, UV [..., ceil(Hs/2), ceil(Ws/2), 2] as a 2-channel image to ceil(Hd/2) x ceil(Wd/2)"""
    Hd, Wd = size
    return resize(y[..., None], (Hd, Wd))[..., 0], resize(uv, ((Hd + 1) // 2, (Wd + 1) // 2))


def real_bilinear(img, size):
    """the real-valued bilinear image the definition quantises: torch's float64 F.interpolate(mode="bilinear", align_corners=False)"""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(img)).to(torch.float64)
    lead = x.shape[:-3]
    x = x.reshape(-1, *x.shape[-3:]).permute(0, 3, 1, 2)
    out = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    return out.permute(0, 2, 3, 1).reshape(*lead, size[0], size[1], img.shape[-1]).numpy()
