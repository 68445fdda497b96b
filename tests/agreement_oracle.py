"""numpy restatement of the agreement guard definition of include/emavfi.h ("AGREEMENT GUARD DEFINITION"), op for op: the disagreement is
one float32 subtraction and an absolute value, `flagged` is NOT (d <= tol) reduced over the channels, `held` is the maximum of `flagged`
over the window clipped to the frame, a kept pixel is one float32 addition and one multiplication by 0.5, a held pixel three roundings and
a clamp through which a NaN passes.  numpy never reassociates or contracts, and every array here is float32.

Also the input cases the CPU and the GPU tests share (`RANDOM_CASES`, `random_case`, `single_case`): the CPU tests check on the oracle that
every random case holds between a tenth and nine tenths of its pixels, the GPU tests run the same cases through the entry."""
import numpy as np

MAX_RADIUS = 16
MEAN = np.array((0.485, 0.456, 0.406), np.float32)     # lib.IMAGENET_MEAN / lib.IMAGENET_STD as the entry receives them: fp32
STD = np.array((0.229, 0.224, 0.225), np.float32)
F32 = np.float32


def stats(C, mean=None, std=None):
    """mean[C], std[C] as float32: the ImageNet triple for C = 3, else a fixed made-up set (C = 1, 2, 4 have no convention)"""
    if mean is None:
        mean = MEAN if C == 3 else np.array((0.5, 0.25, 0.375, 0.625), np.float32)[:C]
    if std is None:
        std = STD if C == 3 else np.array((0.25, 0.5, 0.125, 0.375), np.float32)[:C]
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    assert mean.shape == std.shape == (C,)
    return mean, std


def _check(*ts):
    for t in ts:
        assert t.dtype == np.float32 and t.ndim == 4 and t.shape == ts[0].shape, (t.dtype, t.shape)


def disagreement(u, v):
    """d = |u - v|: one float32 subtraction, then the sign cleared"""
    _check(u, v)
    with np.errstate(invalid="ignore"):
        d = np.abs(u - v)
    assert d.dtype == np.float32
    return d


def flagged(u, v, tol):
    """bool [B, H, W]: for some channel NOT (d <= tol) - a NaN in u or v flags"""
    tol = F32(tol)
    assert 0 <= tol <= 1
    with np.errstate(invalid="ignore"):
        return (~(disagreement(u, v) <= tol)).any(axis=1)


def dilate(flag, r):
    """bool [B, H, W]: the maximum of `flag` over the window [y - r, y + r] x [x - r, x + r] clipped to the frame"""
    assert flag.dtype == np.bool_ and flag.ndim == 3 and 0 <= r <= MAX_RADIUS
    B, H, W = flag.shape
    out = np.zeros_like(flag)
    for y in range(H):
        y0, y1 = max(0, y - r), min(H - 1, y + r)
        for x in range(W):
            x0, x1 = max(0, x - r), min(W - 1, x + r)
            out[:, y, x] = flag[:, y0:y1 + 1, x0:x1 + 1].max(axis=(1, 2))
    return out


def held(u, v, tol, r):
    return dilate(flagged(u, v, tol), r)


def kept(u, v):
    """(u + v) * 0.5f"""
    _check(u, v)
    with np.errstate(invalid="ignore"):
        out = (u + v) * F32(0.5)
    assert out.dtype == np.float32
    return out


def fallback(a, b, mean, std):
    """h = (a + b) * 0.5f; t = h * std[c]; t = t + mean[c]; t < 0 ? 0 : (t > 1 ? 1 : t) - both comparisons fail for a NaN"""
    _check(a, b)
    mean, std = stats(a.shape[1], mean, std)
    with np.errstate(invalid="ignore", over="ignore"):
        h = (a + b) * F32(0.5)
        t = h * std.reshape(1, -1, 1, 1)
        t = t + mean.reshape(1, -1, 1, 1)
        out = np.where(t < 0, F32(0), np.where(t > 1, F32(1), t))
    assert h.dtype == t.dtype == out.dtype == np.float32
    return out


def guard(u, v, a, b, tol, r=0, mean=None, std=None):
    """(out float32 [B, C, H, W], held bool [B, H, W], counts uint32 [B]) of emavfi_agreement_guard_f32"""
    _check(u, v, a, b)
    hold = held(u, v, tol, r)
    out = np.where(hold[:, None], fallback(a, b, mean, std), kept(u, v))
    return np.ascontiguousarray(out, dtype=np.float32), hold, hold.sum(axis=(1, 2)).astype(np.uint32)


def flip(t, f):
    """phi_f over the last two axes (the ensemble definition): f & 1 mirrors the columns, f & 2 the rows"""
    if f & 2:
        t = t[..., ::-1, :]
    if f & 1:
        t = t[..., :, ::-1]
    return t.copy(order="C")


def density(r):
    """the flag density at which about half the pixels of a large frame are held: p = 1 - 0.5^(1 / (2 r + 1)^2)"""
    return 1.0 - 0.5 ** (1.0 / (2 * r + 1) ** 2)


TOL_STEPS = 8              # the shared cases' tolerance: 8 steps of the 2^-10 grid
TOL = F32(TOL_STEPS / 1024.0)

# (shape, radius, seed) of the cases with random flags.  r = 16 runs only at 70 x 140; 1 x 1 has no random case (its share is 0 or 1).
# The seeds of the two one-line shapes (18 pixels, a one-dimensional window) were picked so that the ORACLE's held share lies in [0.1, 0.9]
# with something held and something kept in each sample (tests/test_agreement_cpu.py checks every case here); nothing was picked by
# looking at the device.
RANDOM_CASES = ([((2, 3, 23, 37), r, 1) for r in (0, 1, 3)]
                + [((1, 3, 70, 140), r, 2) for r in (0, 1, 3, 16)]
                + [((2, 3, 1, 9), r, seed) for r, seed in ((0, 3), (1, 15), (3, 53))]
                + [((2, 3, 9, 1), r, seed) for r, seed in ((0, 4), (1, 20), (3, 53))]
                + [((1, 4, 33, 64), r, 5) for r in (0, 1, 3)])


def sources(shape, seed):
    """a, b: normalised sources whose blend de-normalises to about [-0.15, 1.15], so that both clamps and the middle occur"""
    rng = np.random.default_rng(1000 + seed)
    return tuple(rng.uniform(-2.8, 3.0, shape).astype(np.float32) for _ in range(2))


def agreeing(shape, seed):
    """u, v on the 2^-10 grid in [0, 1] with every d in {0, 1, ..., TOL_STEPS} / 1024, either sign - all exact in float32, so d == TOL
    EXACTLY at about one sample in nine, and no sample is flagged at TOL"""
    rng = np.random.default_rng(seed)
    vk = rng.integers(TOL_STEPS + 1, 1024 - TOL_STEPS, shape)
    uk = vk + rng.integers(0, TOL_STEPS + 1, shape) * rng.choice((-1, 1), shape)
    return (uk / 1024.0).astype(np.float32), (vk / 1024.0).astype(np.float32)


def flag_pixel(u, v, b, y, x, c, kind):
    """makes pixel (b, y, x) flagged at TOL through channel c.  kind 0: v = 0 and u = the float32 next above TOL, so d is ONE ULP above
    the tolerance; kind 1: one grid step above, |u - v| = (TOL_STEPS + 1) / 1024, u below v; kind 2: the same with u above v"""
    if kind == 0:
        v[b, c, y, x] = 0
        u[b, c, y, x] = np.nextafter(TOL, F32(1))
    else:
        u[b, c, y, x] = v[b, c, y, x] + F32((TOL_STEPS + 1) / 1024.0) * (1 if kind == 2 else -1)


def random_case(shape, r, seed):
    """(u, v, a, b) with pixels flagged at density(r), each through one random channel and one random `kind`; tol is TOL"""
    B, C, H, W = shape
    u, v = agreeing(shape, seed)
    rng = np.random.default_rng(77 + seed)
    for b, y, x in np.argwhere(rng.random((B, H, W)) < density(r)):
        flag_pixel(u, v, b, y, x, rng.integers(C), rng.integers(3))
    return (u, v) + sources(shape, seed)


def single_case(shape, where, seed=9):
    """(u, v, a, b) with ONE flagged pixel per sample (one ulp above TOL, last channel) in otherwise agreeing inputs; `where`: "centre" or
    one of the corners "tl", "tr", "bl", "br"; None: nothing flagged"""
    B, C, H, W = shape
    u, v = agreeing(shape, seed)
    if where is not None:
        y, x = {"centre": (H // 2, W // 2), "tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}[where]
        for b in range(B):
            flag_pixel(u, v, b, y, x, C - 1, 0)
    return (u, v) + sources(shape, seed)


def checksum(t):
    """sum of bits(t[i]) * (i + 1) modulo 2^32 over the flattened float32 array (tests/host/host_check_agreement.cpp prints the same)"""
    b = np.ascontiguousarray(t, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64) & 0xFFFFFFFF).sum() & 0xFFFFFFFF)


def generated(k, shape, scale):
    """tensor k of the host check's generated case (host_check_agreement.cpp, gen()): a 16-bit hash times 2^-16, times `scale` - exact in
    float32 for a power-of-two scale"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    M = 0xFFFFFFFF
    h = (i * 2654435761 + k * 40503 + 12345) & M                 # a xor-shift mix: tensors and neighbours are uncorrelated
    h ^= h >> 16
    h = h * 2246822519 & M
    h ^= h >> 13
    h = h * 3266489917 & M
    h ^= h >> 16
    return ((h >> 16).astype(np.float32) * F32(scale / 65536.0)).reshape(shape)
