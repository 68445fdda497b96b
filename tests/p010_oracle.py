"""numpy int64 / float64 restatement of the high-bit-depth colour definition (include/emavfi.h, "HIGH BIT DEPTH"), written from the
formulas - the oracle of tests/test_p010_cpu.py and tests/test_gpu_p010.py.  Nothing here looks at the kernels."""
import math

import numpy as np

STANDARDS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True), ("bt2020", False), ("bt2020", True)]   # codes 0..5, in order
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
DEPTHS = (10, 12, 16)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def q20(k):
    return math.floor(k * 2 ** 20 + 0.5)


def constants(depth, full_range):
    """(P, mid, yoff, Yr, Cr)"""
    P, s = 2 ** depth - 1, 2 ** (depth - 8)
    return (P, 2 ** (depth - 1), 0, P, P) if full_range else (P, 2 ** (depth - 1), 16 * s, 219 * s, 224 * s)


def coefficients(standard, full_range, depth):
    """(decode [CY, CVR, CUG, CVG, CUB], encode [YR, YG, YB, UR, UG, UB, VR, VG, VB]) as fixed-point integers; depth 8 is NV12's"""
    kr, kb = K[standard]
    kg = 1 - kr - kb
    P, _, _, Yr, Cr = constants(depth, full_range)
    cy, s, t, sp = P / Yr, P / Cr, Yr / P, Cr / P
    dec = [cy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s]
    enc = [kr * t, kg * t, kb * t,
           -kr / (2 * (1 - kb)) * sp, -kg / (2 * (1 - kb)) * sp, 0.5 * sp,
           0.5 * sp, -kg / (2 * (1 - kr)) * sp, -kb / (2 * (1 - kr)) * sp]
    return [q20(k) for k in dec], [q20(k) for k in enc]


def samples(words, depth):
    """16-bit words -> int64 samples: the top `depth` bits"""
    return words.astype(np.int64) >> (16 - depth)


def words(samp, depth):
    return (np.asarray(samp).astype(np.int64) << (16 - depth)).astype(np.uint16)


def decode(y, uv, depth=10, standard="bt601", full_range=False, order="bgr"):
    """y uint16 words [..., H, W], uv uint16 words [..., ceil(H/2), ceil(W/2), 2] -> int64 [..., H, W, 3] of depth-bit integers,
    channel 0 = B ("bgr") or R ("rgb")"""
    (cy, cvr, cug, cvg, cub), _ = coefficients(standard, full_range, depth)
    P, mid, yoff, _, _ = constants(depth, full_range)
    H, W = y.shape[-2:]
    up = np.repeat(np.repeat(samples(uv, depth), 2, axis=-3), 2, axis=-2)[..., :H, :W, :]   # nearest: pixel (y, x) <- pair (y >> 1, x >> 1)
    u, v = up[..., 0] - mid, up[..., 1] - mid
    l = np.maximum(samples(y, depth) - yoff, 0)
    r = np.clip((cy * l + cvr * v + 2 ** 19) >> 20, 0, P)
    g = np.clip((cy * l + cug * u + cvg * v + 2 ** 19) >> 20, 0, P)
    b = np.clip((cy * l + cub * u + 2 ** 19) >> 20, 0, P)
    return np.stack((b, g, r) if order == "bgr" else (r, g, b), axis=-1)


def encode(pix, depth=10, standard="bt601", full_range=False, order="bgr"):
    """integers [..., H, W, 3] in 0..P -> (y uint16 words [..., H, W], uv uint16 words [..., ceil(H/2), ceil(W/2), 2]), low bits zero"""
    _, (yr, yg, yb, ur, ug, ub, vr, vg, vb) = coefficients(standard, full_range, depth)
    P, mid, yoff, _, _ = constants(depth, full_range)
    p = np.asarray(pix).astype(np.int64)
    r, g, b = (p[..., 2], p[..., 1], p[..., 0]) if order == "bgr" else (p[..., 0], p[..., 1], p[..., 2])
    y = np.clip(((yr * r + yg * g + yb * b + 2 ** 19) >> 20) + yoff, 0, P)
    H, W = r.shape[-2:]
    ys = np.minimum(np.arange(0, H + (H & 1)), H - 1)      # past the last row / column: clamped
    xs = np.minimum(np.arange(0, W + (W & 1)), W - 1)

    def mean4(c):
        c = c[..., ys, :][..., :, xs]
        return (c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2] + 2) >> 2

    rm, gm, bm = mean4(r), mean4(g), mean4(b)
    u = np.clip(((ur * rm + ug * gm + ub * bm + 2 ** 19) >> 20) + mid, 0, P)
    v = np.clip(((vr * rm + vg * gm + vb * bm + 2 ** 19) >> 20) + mid, 0, P)
    return words(y, depth), words(np.stack((u, v), axis=-1), depth)


def normalise(pix, depth, mean=MEAN, std=STD):
    """depth-bit integers [..., H, W, 3] -> fp32 [..., 3, H, W]: ((float(v) / float(P)) - mean) / std, every step rounded to fp32"""
    P = np.float32(2 ** depth - 1)
    v = np.asarray(pix).astype(np.float32) / P
    v = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert v.dtype == np.float32
    return np.ascontiguousarray(np.moveaxis(v, -1, -3))


def quantise(x, depth, denormalize=True, mean=MEAN, std=STD):
    """fp32 [..., 3, H, W] -> int64 [..., H, W, 3]: trunc(clip(x std + mean, 0, 1) P) in float64, NaN -> 0"""
    v = np.moveaxis(np.asarray(x), -3, -1).astype(np.float64)
    if denormalize:
        v = v * np.asarray(std, np.float64) + np.asarray(mean, np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.clip(v, 0.0, 1.0) * float(2 ** depth - 1)).astype(np.int64)


def preprocess(y, uv, depth=10, standard="bt601", full_range=False, order="bgr", mean=MEAN, std=STD):
    return normalise(decode(y, uv, depth, standard, full_range, order), depth, mean, std)


def postprocess(x, depth=10, standard="bt601", full_range=False, order="bgr", denormalize=True, mean=MEAN, std=STD):
    return encode(quantise(x, depth, denormalize, mean, std), depth, standard, full_range, order)
