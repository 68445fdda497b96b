"""numpy int64 restatement of the NV12 colour definition (include/emavfi.h, "NV12"), written from the formulas - the oracle of
tests/test_nv12_cpu.py and tests/test_gpu_nv12.py.  Nothing here looks at the kernels."""
import math

import numpy as np

STANDARDS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]   # EMAVFI_YUV_* codes 0..3, in order
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def q20(k):
    return math.floor(k * 2 ** 20 + 0.5)


def coefficients(standard, full_range):
    """(decode [CY, CVR, CUG, CVG, CUB], encode [YR, YG, YB, UR, UG, UB, VR, VG, VB]) as fixed-point integers"""
    kr, kb = K[standard]
    kg = 1 - kr - kb
    cy, s = (1.0, 1.0) if full_range else (255 / 219, 255 / 224)
    t, sp = (1.0, 1.0) if full_range else (219 / 255, 224 / 255)
    dec = [cy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s]
    enc = [kr * t, kg * t, kb * t,
           -kr / (2 * (1 - kb)) * sp, -kg / (2 * (1 - kb)) * sp, 0.5 * sp,
           0.5 * sp, -kg / (2 * (1 - kr)) * sp, -kb / (2 * (1 - kr)) * sp]
    return [q20(k) for k in dec], [q20(k) for k in enc]


def decode(y, uv, standard="bt601", full_range=False, order="bgr"):
    """y uint8 [..., H, W], uv uint8 [..., ceil(H/2), ceil(W/2), 2] -> uint8 [..., H, W, 3] with channel 0 = B ("bgr") or R ("rgb")"""
    (cy, cvr, cug, cvg, cub), _ = coefficients(standard, full_range)
    H, W = y.shape[-2:]
    up = np.repeat(np.repeat(uv.astype(np.int64), 2, axis=-3), 2, axis=-2)[..., :H, :W, :]   # nearest: pixel (y, x) <- pair (y >> 1, x >> 1)
    u, v = up[..., 0] - 128, up[..., 1] - 128
    l = y.astype(np.int64)
    if not full_range:
        l = np.maximum(l - 16, 0)
    r = np.clip((cy * l + cvr * v + 2 ** 19) >> 20, 0, 255)
    g = np.clip((cy * l + cug * u + cvg * v + 2 ** 19) >> 20, 0, 255)
    b = np.clip((cy * l + cub * u + 2 ** 19) >> 20, 0, 255)
    return np.stack((b, g, r) if order == "bgr" else (r, g, b), axis=-1).astype(np.uint8)


def encode(pix, standard="bt601", full_range=False, order="bgr"):
    """uint8 [..., H, W, 3] -> (y uint8 [..., H, W], uv uint8 [..., ceil(H/2), ceil(W/2), 2])"""
    _, (yr, yg, yb, ur, ug, ub, vr, vg, vb) = coefficients(standard, full_range)
    p = pix.astype(np.int64)
    r, g, b = (p[..., 2], p[..., 1], p[..., 0]) if order == "bgr" else (p[..., 0], p[..., 1], p[..., 2])
    yoff = 0 if full_range else 16
    y = np.clip(((yr * r + yg * g + yb * b + 2 ** 19) >> 20) + yoff, 0, 255)
    H, W = r.shape[-2:]
    ys = np.minimum(np.arange(0, H + (H & 1)), H - 1)      # past the last row / column: clamped
    xs = np.minimum(np.arange(0, W + (W & 1)), W - 1)

    def mean4(c):
        c = c[..., ys, :][..., :, xs]
        return (c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2] + 2) >> 2

    rm, gm, bm = mean4(r), mean4(g), mean4(b)
    u = np.clip(((ur * rm + ug * gm + ub * bm + 2 ** 19) >> 20) + 128, 0, 255)
    v = np.clip(((vr * rm + vg * gm + vb * bm + 2 ** 19) >> 20) + 128, 0, 255)
    return y.astype(np.uint8), np.stack((u, v), axis=-1).astype(np.uint8)
