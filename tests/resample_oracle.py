"""numpy / Fraction restatement of the temporal resample definition (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION"): the time grid worked
out with exact rationals instead of the integer recurrences the harness uses, the per-sample blend, and the assembly of output frames from a
table as emavfi_resample_frames performs it.  Nothing here imports the package."""
from fractions import Fraction
from math import floor

import numpy as np

NODES = 0x80000000      # the pool bit of a table entry's a / b
LAUNCH_CAP = 64


def ratio(rate_in, rate_out):
    f = Fraction(rate_in) / Fraction(rate_out)
    return f.numerator, f.denominator


def count(n, rate_in, rate_out):
    """output frames of a clip of n frames: every k >= 0 whose time k Fi / Fo does not pass the last frame"""
    if n <= 0:
        return 0
    step, k = Fraction(rate_in) / Fraction(rate_out), 0
    while (k + 1) * step <= n - 1:
        k += 1
    return k + 1


def plan(n, rate_in, rate_out, depth, method):
    """[(k, s, j0, j1, w)] for the whole clip, from the rational time of every output; w = 256 normalised to node j0 + 1 alone"""
    step, G, out = Fraction(rate_in) / Fraction(rate_out), 1 << depth, []
    Q = step.denominator
    for k in range(count(n, rate_in, rate_out)):
        t = k * step
        s = floor(t)
        pos = (t - s) * G                       # the position in node units, 0 <= pos < G
        if method == "nearest":
            j = floor(pos + Fraction(1, 2))     # a tie goes to the later node
            out.append((k, s, j, j, 0))
        else:
            j0 = floor(pos)
            e = (pos - j0) * Q                  # an integer in 0..Q-1
            assert e.denominator == 1
            w = (256 * int(e) + Q // 2) // Q
            out.append((k, s, j0 + 1, j0 + 1, 0) if w == 256 else (k, s, j0, j0, 0) if w == 0 else (k, s, j0, j0 + 1, w))
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


def blend(a, b, w, sample_bytes=1, depth=8, shift=0):
    """per sample ((256 - w) A + w B + 128) >> 8 on uint8 frames, or on the depth-bit samples of the little-endian words they hold"""
    if sample_bytes == 1:
        return (((256 - w) * a.astype(np.int64) + w * b.astype(np.int64) + 128) >> 8).astype(np.uint8)
    wa, wb = (np.ascontiguousarray(v).view("<u2").astype(np.int64) for v in (a, b))
    mask = (1 << depth) - 1
    v = ((256 - w) * ((wa >> shift) & mask) + w * ((wb >> shift) & mask) + 128) >> 8
    return (v << shift).astype("<u2").view(np.uint8).reshape(a.shape)


def assemble(srcs, nodes, table, flags=None, sample_bytes=1, depth=8, shift=0):
    """the output frames of emavfi_resample_frames: srcs / nodes uint8 [n, ...] (16-bit frames as their bytes), table of (a, b, w, f, h)"""
    def frame(i):
        return nodes[i & ~NODES] if i & NODES else srcs[i]
    out = []
    for a, b, w, f, h in table:
        if flags is not None and f and flags[f - 1]:
            out.append(srcs[h].copy())
        elif w == 0:
            out.append(frame(a).copy())
        elif w == 256:
            out.append(frame(b).copy())
        else:
            out.append(blend(frame(a), frame(b), w, sample_bytes, depth, shift))
    return np.stack(out)


def gen(n, full):
    """the two generated frames of tests/host/host_check_resample.cpp: n samples each, masked to `full`"""
    i = np.arange(n, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    a = ((i * np.uint64(2654435761)) & m) >> np.uint64(7)
    b = (((((i * np.uint64(40503)) + np.uint64(12345)) & m) * np.uint64(2246822519)) & m) >> np.uint64(9)
    return (a & np.uint64(full)).astype(np.int64), (b & np.uint64(full)).astype(np.int64)


def checksum(v):
    """sum over the samples of v[i] (i + 1), modulo 2^32"""
    return int((v.astype(np.uint64) * np.arange(1, v.size + 1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).sum() % (1 << 32))
