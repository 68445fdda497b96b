"""numpy restatement of the ACTIVE AREA DEFINITION (include/emavfi.h), written from its words: it looks at no kernel.

An image is [H, W, C] (C = 1: a Y plane; C = 3: bytes only) of bytes or of 16-bit words; a sample is the element itself, or
(word >> shift) & (2^depth - 1).  A frame, where the bars are put back, is a flat array of samples in one of the three dense layouts of
tests/static_oracle.py, whose `planes` this file uses.
"""
import numpy as np

from static_oracle import LAYOUTS, frame_samples, planes, sample  # noqa: F401  (re-exported)


def content(img, level, depth=8, shift=0):
    """bool [H, W]: any of the pixel's C samples is GREATER than level"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    return (sample(img, depth, shift) > int(level)).any(axis=2)


def bounds(img, level, depth=8, shift=0):
    """(top, bottom, left, right) of one image; no content: (H, 0, W, 0)"""
    c = content(img, level, depth, shift)
    H, W = c.shape
    ys, xs = np.nonzero(c.any(axis=1))[0], np.nonzero(c.any(axis=0))[0]
    if ys.size == 0:
        return H, 0, W, 0
    return int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1


def rect(all_bounds, H, W):
    """(top, left, height, width): the union of the bounds, grown outward to even rows and to columns that are multiples of 16, clipped to
    the frame; an empty union, or a rectangle that covers the frame, is the whole frame"""
    top, bottom, left, right = H, 0, W, 0
    for t, b, l, r in all_bounds:
        top, bottom, left, right = min(top, t), max(bottom, b), min(left, l), max(right, r)
    if bottom <= top or right <= left:
        return 0, 0, H, W
    top, left = top - top % 2, left - left % 16
    bottom, right = min(H, bottom + bottom % 2), min(W, right + (-right) % 16)
    return top, left, bottom - top, right - left


def level_units(tolerance, depth, yuv, full_range):
    """black plus floor(tolerance * (2^depth - 1)), at most 2^depth - 1; black is 16 << (depth - 8) for limited-range Y'CbCr and 0 otherwise"""
    full = (1 << depth) - 1
    return min(full, ((16 << (depth - 8)) if (yuv and not full_range) else 0) + int(np.floor(tolerance * full)))


def inside_masks(H, W, layout, C, r):
    """per plane of the layout a bool array of the plane's shape: the sample belongs to the rectangle r = (top, left, height, width) - a
    4:2:0 chroma sample (i, j) exactly when its 2 x 2 luma block does"""
    t, l, h, w = r
    luma = np.zeros((H, W), bool)
    luma[t:t + h, l:l + w] = True
    if layout == "interleaved":
        return (np.repeat(luma[:, :, None], C, axis=2),)
    chroma = luma[0::2, 0::2] & luma[0::2, 1::2] & luma[1::2, 0::2] & luma[1::2, 1::2]
    if layout == "nv12":
        return luma, np.repeat(chroma[:, :, None], 2, axis=2)
    return luma, chroma, chroma


def fill_outside(d, a, H, W, layout, C, r):
    """a copy of the flat frame `d` with a's elements (whole words) outside the rectangle; inside it d's"""
    out = np.array(d).reshape(-1).copy()
    for o, s, m in zip(planes(out, H, W, layout, C), planes(a, H, W, layout, C), inside_masks(H, W, layout, C, r)):
        o[~m] = s[~m]
    return out


def paste(pred, a, H, W, layout, C, r):
    """the whole frame of a prediction for the rectangle: a's elements outside it, inside it the elements of `pred`, a flat frame of the
    same layout at the rectangle's size"""
    t, l, h, w = r
    out = np.array(a).reshape(-1).copy()
    for o, p, m in zip(planes(out, H, W, layout, C), planes(pred, h, w, layout, C), inside_masks(H, W, layout, C, r)):
        o[m] = p.reshape(-1)
    return out


def crop(frame, H, W, layout, C, r):
    """the flat frame cut to the rectangle: a flat frame of the same layout at the rectangle's size"""
    return np.concatenate([p[m] for p, m in zip(planes(frame, H, W, layout, C), inside_masks(H, W, layout, C, r))])


def dense(pitched, H, rowbytes):
    """the dense copy of an image batch [n, rows >= H, pitch >= rowbytes] of bytes: what the pitched u8 entries are defined on"""
    return np.ascontiguousarray(np.asarray(pitched)[:, :H, :rowbytes])
