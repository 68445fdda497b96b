"""numpy restatement of the linear light definition (include/emavfi.h, "LINEAR LIGHT DEFINITION"): the tables of the three built-in transfer
functions from math.pow / math.exp, the encode as a search over the midpoints of neighbouring table values, the per-sample mean in light,
and the assembly of output frames from a table as emavfi_accumulate_frames_linear performs it - the coded rest of a frame by
tests/shutter_oracle.py.  Nothing here imports the package."""
import math

import numpy as np

import shutter_oracle

NODES = shutter_oracle.NODES
ONE, BIAS, LIMIT = 1 << 28, 1 << 26, 1 << 30
TRANSFERS = ("srgb", "bt709", "hlg")
DEPTHS = (8, 10, 12)


def inverse(name, x):
    """g(x) on x >= 0"""
    if name == "srgb":
        return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)
    if name == "bt709":
        alpha, beta = 1.09929682680944, 0.018053968510807
        return x / 4.5 if x < 4.5 * beta else math.pow((x + alpha - 1.0) / alpha, 1.0 / 0.45)
    if name == "hlg":
        a, b, c = 0.17883277, 0.28466892, 0.55991073
        return x * x / 3.0 if x <= 0.5 else (math.exp((x - c) / a) + b) / 12.0
    raise ValueError(name)


def code_range(depth, full_range):
    """(lo, hi): the codes of nominal black and white"""
    return (0, (1 << depth) - 1) if full_range else (16 << (depth - 8), 235 << (depth - 8))


def table(name, depth, full_range):
    """lin[v] = BIAS + round(ONE g(x)), g extended oddly below black; uint32 [2^depth]"""
    lo, hi = code_range(depth, full_range)
    out = np.empty(1 << depth, np.uint32)
    for v in range(1 << depth):
        x = (v - lo) / (hi - lo)
        g = -inverse(name, -x) if x < 0 else inverse(name, x)
        out[v] = BIAS + int(math.floor(ONE * g + 0.5)) if g >= 0 else BIAS - int(math.floor(ONE * -g + 0.5))
    return out


def affine(depth):
    """the table that reproduces the coded mean: BIAS + 65536 v"""
    return (BIAS + 65536 * np.arange(1 << depth, dtype=np.uint64)).astype(np.uint32)


def valid(lin):
    lin = np.asarray(lin, np.uint64)
    return bool((np.diff(lin.astype(np.int64)) > 0).all() and (lin < LIMIT).all())


def enc(L, lin):
    """the largest v with v == 0 or lin[v - 1] + lin[v] <= 2 L, per element of L: searchsorted on the midpoint sums of a valid table"""
    lin = np.asarray(lin, np.uint64)
    mids = lin[:-1] + lin[1:]                                          # mids[v - 1] belongs to code v
    return np.searchsorted(mids, 2 * np.asarray(L, np.uint64), side="right")


def mean(frames, weights, lin, sample_bytes=1, depth=8, shift=0):
    """per sample enc((sum w_j lin[s_j] + S / 2) / S) on uint8 frames, or on the depth-bit samples of the little-endian words they hold"""
    S = sum(weights)
    assert 0 < S <= 65535
    lin64 = np.asarray(lin, np.uint64)
    mask = (1 << depth) - 1
    if sample_bytes == 1:
        samples = [np.asarray(f, np.uint8).astype(np.int64) for f in frames]
    else:
        samples = [((np.ascontiguousarray(f).view("<u2").astype(np.int64) >> shift) & mask) for f in frames]
    acc = sum(np.uint64(w) * lin64[s] for s, w in zip(samples, weights))
    v = enc((acc + np.uint64(S // 2)) // np.uint64(S), lin)
    if sample_bytes == 1:
        return v.astype(np.uint8)
    return (v.astype(np.uint64) << np.uint64(shift)).astype("<u2").view(np.uint8).reshape(np.asarray(frames[0]).shape)


def accumulate(srcs, nodes, table, flags, lin, linear_bytes, sb=1, depth=8, shift=0):
    """the output frames of emavfi_accumulate_frames_linear: srcs / nodes uint8 [n, fb] (16-bit frames as their bytes), table of
    (taps, weights, f, h); the first linear_bytes bytes of a mixed frame in light, the rest shutter_oracle's coded mean"""
    out = shutter_oracle.accumulate(srcs, nodes, table, flags, sb, depth, shift)
    assert linear_bytes % sb == 0 and 0 <= linear_bytes <= out.shape[1]

    def frame(i):
        return nodes[i & ~NODES] if i & NODES else srcs[i]
    for k, (tp, ws, f, h) in enumerate(table):
        if (flags is not None and f and flags[f - 1]) or len(tp) == 1 or linear_bytes == 0:
            continue
        out[k, :linear_bytes] = mean([frame(t)[:linear_bytes] for t in tp], ws, lin, sb, depth, shift)
    return out
