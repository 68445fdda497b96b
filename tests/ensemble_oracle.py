"""numpy restatement of the ensemble definition of include/emavfi.h ("ENSEMBLE DEFINITION"): the flip codes, a member read through its flip,
the balanced fp32 summation tree, and the three ensembles as lists of (reversed?, flip) members.  Every addition is one numpy float32
addition of whole arrays - numpy never reassociates or contracts - and the scale is one float32 multiplication by the exact 1 / n."""
import numpy as np

FLIP_H, FLIP_V = 1, 2
FLIPS = (0, 3, 1, 2)          # the member order of "flip": the pairs {identity, HV}, {H, V}


def flip(t, f):
    """phi_f t over the last two axes of a float32 array"""
    t = np.asarray(t)
    assert t.dtype == np.float32 and t.ndim >= 2 and 0 <= f <= 3
    if f & FLIP_V:
        t = t[..., ::-1, :]
    if f & FLIP_H:
        t = t[..., :, ::-1]
    return t.copy(order="C")     # (ascontiguousarray would keep the negative stride of an axis of one element)


def tree(values):
    """the balanced pairwise tree of n in {1, 2, 4, 8} float32 arrays, in the order given, times 1 / n"""
    n = len(values)
    assert n in (1, 2, 4, 8) and all(v.dtype == np.float32 for v in values)
    level = list(values)
    while len(level) > 1:
        level = [level[i] + level[i + 1] for i in range(0, len(level), 2)]
        assert all(v.dtype == np.float32 for v in level)
    return level[0].copy() if n == 1 else level[0] * np.float32(1.0 / n)


def mean(members, flips):
    """emavfi_ensemble_mean_f32: member k's value at output position p is members[k][phi_{flips[k]} p]"""
    assert len(members) == len(flips)
    return tree([flip(m, f) for m, f in zip(members, flips)])


def running_mean(members, flips):
    """what the definition is NOT: the left-to-right sum ((m0 + m1) + m2) + ..., times 1 / n"""
    acc = flip(members[0], flips[0])
    for m, f in zip(members[1:], flips[1:]):
        acc = acc + flip(m, f)
    return acc * np.float32(1.0 / len(members))


def members_of(ensemble):
    """the members of an ensemble in tree order, as (reverse, flip): the member is F(phi_flip x, phi_flip y) read through `flip`, with
    (x, y) = (b, a) where `reverse` else (a, b)"""
    return {"reverse": [(False, 0), (True, 0)],
            "flip": [(False, f) for f in FLIPS],
            "full": [(False, f) for f in FLIPS] + [(True, f) for f in FLIPS]}[ensemble]


def generated(k, count):
    """`count` elements of generated member k (tests/host/host_check_ensemble.cpp, gen()): a signed 24-bit mantissa times 2^(e - 20), e in
    0..7 - exact in fp32 and of mixed magnitude, so that the additions round"""
    i = np.arange(count, dtype=np.uint64)
    h = ((i * 2654435761 + k * 40503 + 12345) & 0xFFFFFFFF) * 2246822519 & 0xFFFFFFFF
    mant = (h >> 8).astype(np.int64) - (1 << 23)
    return np.ldexp(mant.astype(np.float32), (h & 7).astype(np.int32) - 20).astype(np.float32)


def checksum(t):
    """sum of bits(t[i]) * (i + 1) modulo 2^32 over the flattened array"""
    b = np.ascontiguousarray(t, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64) & 0xFFFFFFFF).sum() & 0xFFFFFFFF)
