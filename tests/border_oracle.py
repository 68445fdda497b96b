"""numpy restatement of the border definition of include/emavfi.h ("BORDER DEFINITION"): the two index maps written out from their formulas
(not numpy.pad, which tests/test_border_cpu.py uses to check THIS file), pad and crop as pure gathers of 32-bit words - the arrays are
indexed through their uint32 view, so no bit pattern is touched - and the generated case of tests/host/host_check_border.cpp."""
import numpy as np

from ensemble_oracle import checksum, generated   # noqa: F401  (the generator and the checksum the host checks share)

REPLICATE, REFLECT = 0, 1
MODES = ("replicate", "reflect")
MAX = 64


def index(i, n, mode):
    """which sample of an axis of n samples position i of the extended axis reads"""
    assert n >= 1 and mode in (REPLICATE, REFLECT)
    if mode == REPLICATE:
        return min(max(i, 0), n - 1)
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = ((i % p) + p) % p          # (Python's % is already non-negative: the second step is the definition's, and changes nothing)
    return m if m <= n - 1 else p - m


def indices(n, N, mode):
    """the index vector of an axis: entry j of the n + 2 N is index(j - N, n, mode)"""
    mode = MODES.index(mode) if isinstance(mode, str) else mode
    return np.array([index(j - N, n, mode) for j in range(n + 2 * N)], dtype=np.int64)


def pad(t, N, mode):
    """pad_{N,mode} over the last two axes of a float32 array"""
    t = np.ascontiguousarray(t)
    assert t.dtype == np.float32 and t.ndim >= 2 and 0 <= N <= MAX
    H, W = t.shape[-2:]
    words = t.view(np.uint32)
    out = words[..., indices(H, N, mode), :][..., :, indices(W, N, mode)]
    return np.ascontiguousarray(out).view(np.float32)


def crop(t, N):
    """crop_N over the last two axes of a float32 array"""
    t = np.ascontiguousarray(t)
    assert t.dtype == np.float32 and t.ndim >= 2 and 0 <= N <= MAX and t.shape[-2] > 2 * N and t.shape[-1] > 2 * N
    H, W = t.shape[-2] - 2 * N, t.shape[-1] - 2 * N
    return np.ascontiguousarray(t.view(np.uint32)[..., N:N + H, N:N + W]).view(np.float32)


def host_case():
    """the 2-plane 5 x 7 picture of tests/host/host_check_border.cpp: generated(0, 70) with -0.0, inf and a NaN with a payload planted"""
    t = generated(0, 70).copy()
    w = t.view(np.uint32)
    w[0], w[3], w[69] = 0x80000000, 0x7F800000, 0x7FC12345
    return t.reshape(2, 5, 7)
