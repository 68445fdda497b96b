"""numpy / Fraction restatement of the shutter definition (include/emavfi.h, "SHUTTER DEFINITION"): the exposure window and the cells of the
nodes as exact rationals in source intervals instead of the scaled integers the harness uses, the per-sample weighted mean, and the assembly
of output frames from a table as emavfi_accumulate_frames performs it.  Nothing here imports the package."""
from fractions import Fraction
from functools import reduce
from math import gcd

import numpy as np

NODES = 0x80000000      # the pool bit of a tap
LAUNCH_CAP = 8
MAX_TAPS = 33
MAX_SUM = 65535


def exposure(shutter):
    """e = shutter / 360; a float is taken at its shortest decimal form"""
    return Fraction(str(shutter) if isinstance(shutter, float) else shutter) / 360


def overlaps(Q, depth, shutter, r):
    """[(j, overlap)] of the window [r / Q, r / Q + e / Q] with the cell [(j - 1/2) / G, (j + 1/2) / G] of every node j = 0 .. G, as exact
    rationals in source intervals"""
    G, e = 1 << depth, exposure(shutter)
    lo = Fraction(r, Q)
    hi = lo + e / Q
    return [(j, max(Fraction(0), min(hi, Fraction(2 * j + 1, 2 * G)) - max(lo, Fraction(2 * j - 1, 2 * G)))) for j in range(G + 1)]


def refused(Q, depth, shutter):
    """what the rule refuses before any weight is looked at: an angle outside (0, 360], an exposure shorter than one node spacing"""
    e = exposure(shutter)
    return not 0 < e <= 1 or e / Q < Fraction(1, 1 << depth)


def taps(Q, depth, shutter, r):
    """[(j, w)]: the overlaps scaled to the smallest integers in their proportion; ValueError where the definition refuses"""
    if refused(Q, depth, shutter):
        raise ValueError("refused")
    nz = [(j, w) for j, w in overlaps(Q, depth, shutter, r) if w > 0]
    scale = reduce(lambda a, b: a * b // gcd(a, b), (w.denominator for _, w in nz))
    ints = [int(w * scale) for _, w in nz]
    g = reduce(gcd, ints)
    if sum(ints) // g > MAX_SUM:
        raise ValueError("refused")
    return [(j, w // g) for (j, _), w in zip(nz, ints)]


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


def mean(frames, weights, sample_bytes=1, depth=8, shift=0):
    """per sample (sum w_j s_j + S / 2) / S on uint8 frames, or on the depth-bit samples of the little-endian words they hold"""
    S = sum(weights)
    if sample_bytes == 1:
        acc = sum(w * f.astype(np.uint64) for f, w in zip(frames, weights))
        return ((acc + np.uint64(S // 2)) // np.uint64(S)).astype(np.uint8)
    mask = (1 << depth) - 1
    acc = sum(w * ((np.ascontiguousarray(f).view("<u2").astype(np.uint64) >> np.uint64(shift)) & np.uint64(mask)) for f, w in zip(frames, weights))
    v = (acc + np.uint64(S // 2)) // np.uint64(S)
    return (v << np.uint64(shift)).astype("<u2").view(np.uint8).reshape(frames[0].shape)


def accumulate(srcs, nodes, table, flags=None, sample_bytes=1, depth=8, shift=0):
    """the output frames of emavfi_accumulate_frames: srcs / nodes uint8 [n, ...] (16-bit frames as their bytes), table of
    (taps, weights, f, h)"""
    def frame(i):
        return nodes[i & ~NODES] if i & NODES else srcs[i]
    out = []
    for tp, ws, f, h in table:
        if flags is not None and f and flags[f - 1]:
            out.append(srcs[h].copy())
        elif len(tp) == 1:
            out.append(frame(tp[0]).copy())
        else:
            out.append(mean([frame(t) for t in tp], ws, sample_bytes, depth, shift))
    return np.stack(out)


# ---- the generated case of tests/host/host_check_shutter.cpp
HOST_SAMPLES = 4104
HOST_CASES = [(1, 1), (1, 2, 1), (5, 6, 1), (65534, 1), (1985,) * 32 + (2015,)]


def gen(n, full, t):
    """frame t of the host check: n samples, masked to `full`"""
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(t * 40503 + 12345)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & m
    return ((x >> np.uint64(9)) & np.uint64(full)).astype(np.int64)


def checksum(v):
    """sum over the samples of v[i] (i + 1), modulo 2^32"""
    return int((v.astype(np.uint64) * np.arange(1, v.size + 1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).sum() % (1 << 32))
