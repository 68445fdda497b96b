"""Static regions on the GPU: emavfi_static_guard_frames byte for byte against the numpy restatement of the static region definition
(tests/static_oracle.py), and the harness's static_guard in every mode against `where(core, source a, unguarded stream)` built from the
oracle and an unguarded run of the same interpolator.  Every comparison is bit-exact.

The kernel's tile is 64 rows x 128 columns of luma pixels (csrc/misc_kernels.hip, ST_TH x ST_TW): the frame sizes straddle it."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import static_oracle as oracle
import resample_oracle
import scene_oracle

pytestmark = pytest.mark.gpu

TH, TW = 64, 128
# one tile exactly, one tile + 2 in each axis (four tiles), and a size whose rows are multiples of 16 bytes in every layout and format
SIZES = [(2, 2), (2, 66), (66, 2), (40, 56), (TH, TW), (TH + 2, TW + 2), (TH + 2, TW + 32)]
RADII = (0, 1, 3, 16)
TOLS = (0, 2)
LAYOUTS = [("interleaved", 3), ("nv12", 1), ("i420", 1)]
KINDS = [("u8", 1, 8, 0), ("w10", 2, 10, 0), ("w10s6", 2, 10, 6), ("w16", 2, 16, 0)]     # (name, sample_bytes, depth, shift)
PAD_FILL = 0x5A


def at(H, W, layout, C, y, x, c=0):
    """the flat sample index of pixel (y, x): channel c when interleaved; at 4:2:0 c = 0: Y, 1: U, 2: V of the chroma sample that covers it"""
    if layout == "interleaved":
        return (y * W + x) * C + c
    if c == 0:
        return y * W + x
    if layout == "nv12":
        return H * W + (y // 2) * W + (x // 2) * 2 + (c - 1)
    return H * W + (c - 1) * (H * W // 4) + (y // 2) * (W // 2) + x // 2


def move(frame, i, k, depth, shift):
    """sample i of `frame` moves by k counts (down where up would overflow); the bits outside the sample stay"""
    mask = (1 << depth) - 1
    w = int(frame[i])
    s = (w >> shift) & mask
    s = s + k if s + k <= mask else s - k
    frame[i] = (w & ~(mask << shift)) | (s << shift)


def rand_frame(rng, n, sb):
    return rng.integers(0, 256, n).astype(np.uint8) if sb == 1 else rng.integers(0, 65536, n).astype(np.uint16)


def rejunk(rng, frame, sb, depth, shift):
    """the same samples, other bits around them"""
    if sb == 1 or depth == 16:
        return frame.copy()
    keep = ((1 << depth) - 1) << shift
    return ((frame & keep) | (rng.integers(0, 65536, frame.size).astype(np.uint16) & ~np.uint16(keep))).astype(np.uint16)


def variants(rng, a, H, W, layout, C, sb, depth, shift, r):
    """frames that differ from `a` in a few samples, by 1, 2 or 3 counts: b1 on tile corners and on the last row and column; b2 r and r + 1 away from
    the tile edges; b3 in chroma (interleaved: the last channel) only; b4 in luma (the first channel) only"""
    nc = C if layout == "interleaved" else 3

    def make(points):
        b = rejunk(rng, a, sb, depth, shift)
        for n, (y, x, c) in enumerate(sorted({(min(max(y, 0), H - 1), min(max(x, 0), W - 1), c) for y, x, c in points})):
            move(b, at(H, W, layout, C, y, x, c), 1 + n % 3, depth, shift)
        return b
    ch = nc - 1
    if H * W <= 4:
        b1 = make([(H - 1, W - 1, 0)])
    else:
        b1 = make([(TH - 1, TW - 1, 0), (TH, TW, ch), (TH - 1, TW, 0), (TH, TW - 1, ch), (H - 1, W - 1, 0), (H - 1, 3, ch), (5 % H, W - 1, 0)])
    b2 = make([(TH - r, 10, 0), (TH - r - 1, W - 20, ch), (TH - 1 + r, W // 2, 0), (5, TW - r, ch), (H - 7, TW - r - 1, 0), (H // 2, TW - 1 + r, 0)])
    b3 = make([(H // 2, W // 2, ch), (H - 1, 0, max(ch - 1, 0) if layout != "interleaved" else ch)])
    b4 = make([(H // 3, W // 3, 0), (0, W - 1, 0)])
    return [b1, b2, b3, b4]


def strided(frames, sb, pad, off=0):
    """`frames` (numpy [n, samples]) on the device as the bytes [n, frame_bytes] of a buffer whose frames lie frame_bytes + pad apart, `off` bytes
    into the allocation; the gaps hold PAD_FILL.  Returns (flat, view)"""
    data = torch.from_numpy(np.ascontiguousarray(frames).view(np.uint8).reshape(frames.shape[0], -1))
    n, fb = data.shape
    flat = torch.full((off + n * (fb + pad) + 64,), PAD_FILL, dtype=torch.uint8, device="cuda")
    view = flat[off:off + n * (fb + pad)].view(n, fb + pad)[:, :fb]
    view.copy_(data)
    return flat, view


def gaps_intact(flat, view, what):
    probe = flat.clone()
    probe[view.storage_offset():view.storage_offset() + view.shape[0] * view.stride(0)].view(view.shape[0], view.stride(0))[:, :view.shape[1]] = PAD_FILL
    assert bool((probe == PAD_FILL).all()), (what, "a byte outside the frames changed")


def call(dst, srcs, table, H, W, layout, C, sb, depth, shift, r, tol, with_counts=True):
    counts = torch.full((len(table),), -1, dtype=torch.int32, device="cuda") if with_counts else None      # every byte 0xFF before the call
    assert lib.static_guard_frames(dst, srcs, table, (H, W), layout=layout, C=C, sample_bytes=sb, depth=depth, shift=shift, radius=r, tol=tol,
                                   counts=counts).data_ptr() == dst.data_ptr()
    return counts.cpu().numpy() if with_counts else None


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("layout,C", LAYOUTS, ids=[l for l, _ in LAYOUTS])
def test_entry_is_the_oracle_byte_for_byte(layout, C, kind):
    name, sb, depth, shift = kind
    dt = np.uint8 if sb == 1 else np.uint16
    for H, W in SIZES:
        rng = np.random.default_rng(H * 131 + W + depth + shift)
        n = oracle.frame_samples(H, W, layout, C)
        a, third = rand_frame(rng, n, sb), rand_frame(rng, n, sb)
        for r in RADII:
            bs = variants(rng, a, H, W, layout, C, sb, depth, shift, r)
            src = np.stack([a] + bs + [rejunk(rng, a, sb, depth, shift)])
            table = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 0), (3, 3)]                       # (0, 5): the same samples; (3, 3): a == b
            sflat, srcs = strided(src, sb, 32)
            for tol in TOLS:
                what = (layout, name, (H, W), r, tol)
                dflat, dst = strided(np.stack([third] * len(table)), sb, 48)
                counts = call(dst, srcs, table, H, W, layout, C, sb, depth, shift, r, tol)
                got = dst.cpu().numpy().copy().view(dt)
                some = 0
                for k, (ia, ib) in enumerate(table):
                    want, count, core = oracle.guard(third, src[ia], src[ib], H, W, layout, C, depth, shift, r, tol)
                    assert counts[k] == count, (what, k, counts[k], count)
                    assert np.array_equal(got[k], want), (what, k, np.flatnonzero(got[k] != want)[:8])
                    some += 0 < count < H * W
                assert counts[4] == counts[6] == H * W and np.array_equal(got[4], src[0]) and np.array_equal(got[6], src[3]), what
                assert some or H * W <= 4 or r == 16, what                                         # the cases are not all trivial
                gaps_intact(dflat, dst, what)
                assert np.array_equal(srcs.cpu().numpy().copy().view(dt), src), (what, "the sources are only read")


@pytest.mark.parametrize("layout,C", LAYOUTS + [("interleaved", 1), ("interleaved", 2), ("interleaved", 4)], ids=lambda v: str(v))
def test_both_access_widths_agree_with_the_oracle(layout, C):
    """a tile-straddling frame whose rows allow 16-byte units, with all frames aligned (the wide form) and with sources and destination one
    sample off (bytes / words throughout)"""
    H, W, r = TH + 2, TW + 32, 3
    for name, sb, depth, shift in KINDS[:1] + KINDS[2:3]:
        rng = np.random.default_rng(C * 7 + sb)
        n = oracle.frame_samples(H, W, layout, C)
        a, third = rand_frame(rng, n, sb), rand_frame(rng, n, sb)
        src = np.stack([a] + variants(rng, a, H, W, layout, C, sb, depth, shift, r))
        table = [(0, 1), (0, 2), (3, 0), (4, 0)]
        want = [oracle.guard(third, src[ia], src[ib], H, W, layout, C, depth, shift, r, 1) for ia, ib in table]
        assert (n * sb) % 16 == 0
        for off_s, off_d in ((0, 0), (sb, sb), (0, sb), (sb, 0)):
            sflat, srcs = strided(src, sb, 32, off_s)
            dflat, dst = strided(np.stack([third] * len(table)), sb, 16, off_d)
            assert srcs.data_ptr() % 16 == off_s and dst.data_ptr() % 16 == off_d
            counts = call(dst, srcs, table, H, W, layout, C, sb, depth, shift, r, 1)
            got = dst.cpu().numpy().copy().view(third.dtype)
            for k, (w, count, _) in enumerate(want):
                assert counts[k] == count and np.array_equal(got[k], w), (layout, C, name, off_s, off_d, k)
            gaps_intact(dflat, dst, (layout, C, name, off_s, off_d))


@pytest.mark.parametrize("n_dst", [1, 65, 130])
def test_table_and_counts(n_dst):
    """more entries than one launch carries, a == b entries, counts NULL and counts that held 0xFF"""
    H, W, layout, C, sb, depth, shift, r = 40, 56, "nv12", 1, 1, 8, 0, 1
    rng = np.random.default_rng(n_dst)
    n = oracle.frame_samples(H, W, layout, C)
    a = rand_frame(rng, n, sb)
    src = np.stack([a] + variants(rng, a, H, W, layout, C, sb, depth, shift, r))
    table = [(int(i), int(j)) for i, j in rng.integers(0, 5, (n_dst, 2))]
    table[0] = (2, 2)
    d0 = np.stack([rand_frame(rng, n, sb) for _ in range(n_dst)])
    _, srcs = strided(src, sb, 0)
    pairs = {p: oracle.guard(np.zeros(n, np.uint8), src[p[0]], src[p[1]], H, W, layout, C, depth, shift, r, 0) for p in set(table)}
    want = np.stack([oracle.apply(d0[k], src[p[0]], pairs[p][2], H, W, layout, C) for k, p in enumerate(table)])
    dflat, dst = strided(d0, sb, 16)
    counts = call(dst, srcs, table, H, W, layout, C, sb, depth, shift, r, 0)
    assert np.array_equal(dst.cpu().numpy(), want) and list(counts) == [pairs[p][1] for p in table] and counts[0] == H * W
    gaps_intact(dflat, dst, n_dst)
    dflat, dst = strided(d0, sb, 16)
    assert call(dst, srcs, table, H, W, layout, C, sb, depth, shift, r, 0, with_counts=False) is None
    assert np.array_equal(dst.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="dst overlaps srcs"):
        lib.static_guard_frames(srcs[1:2], srcs, [(0, 1)], (H, W), layout=layout)
    with pytest.raises(RuntimeError, match=r"table\[0\].b"):
        lib.static_guard_frames(dst[:1], srcs, [(0, 5)], (H, W), layout=layout)


# ---------------------------------------------------------------- the harness
H, W, D, BAND = 40, 56, 3, 8
FORMATS = ["bgr24", "nv12", "yuv420p8", "yuv420p10", "p010"]
BYTE_FORMATS = FORMATS[:3]
NAMES = {lib.LAYOUT_INTERLEAVED: "interleaved", lib.LAYOUT_NV12: "nv12", lib.LAYOUT_I420: "i420"}


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
    return m


def clip(fmt, n, seed=1, Hs=H, Ws=W, band=BAND, levels=None):
    """n frames with a static top band and a static right column strip (luma and chroma) around a moving interior; `levels`: a brightness
    per frame for the interior (a cut), else noise"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        lo, hi = (0.0, 1.0) if levels is None else (levels[t], levels[t] + 0.2)
        if fmt == "bgr24":
            f = (rng.uniform(lo, hi, (Hs, Ws, 3)) * 255).astype(np.uint8)
        elif fmt in ("nv12", "yuv420p8"):
            f = (rng.uniform(lo, hi, (Hs * 3 // 2, Ws)) * 219 + 16).astype(np.uint8)
        else:
            depth = lib.DEPTHS.get(fmt) or lib.PLANAR_DEPTHS[fmt]
            f = ((rng.uniform(lo, hi, (Hs * 3 // 2, Ws)) * 876 + 64).astype(np.uint16) << (depth - 10 + (16 - depth if fmt in lib.DEPTHS else 0))).astype(np.uint16)
        if out:
            f0 = out[0]
            f[:band] = f0[:band]
            f[:Hs, Ws - band:] = f0[:Hs, Ws - band:]
            if fmt in lib.PLANAR_DEPTHS:
                c, c0 = f[Hs:].reshape(2, Hs // 2, Ws // 2), f0[Hs:].reshape(2, Hs // 2, Ws // 2)
                c[:, :band // 2] = c0[:, :band // 2]
                c[:, :, (Ws - band) // 2:] = c0[:, :, (Ws - band) // 2:]
            elif fmt != "bgr24":
                f[Hs:Hs + band // 2] = f0[Hs:Hs + band // 2]
                f[Hs:, Ws - band:] = f0[Hs:, Ws - band:]
        out.append(f)
    return out


def guard_np(fmt, d, a, b, r, tol=0, size=(H, W)):
    """(the frame d guarded against the pair (a, b) by the oracle, the core pixel count)"""
    layout, C, sb, depth, shift = lib.static_frame_format(fmt)
    out, count, _ = oracle.guard(d.reshape(-1), a.reshape(-1), b.reshape(-1), size[0], size[1], NAMES[layout], C, depth, shift, r, tol)
    return out.reshape(d.shape), count


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


def interpolator(model, fmt, **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, pixel_format=fmt, **kw)


def expected_pairs(fmt, plain, n_frames, factor, sources, r, tol=0, held=(), size=(H, W)):
    """the guarded stream of modes "reference" / "recursive" from the unguarded one: (frames, shares)"""
    plan = FrameInterpolator.emission_plan(n_frames, factor, 1, reference_quirks=False)
    assert len(plan) == len(plain)
    out, shares = [], []
    for item, f in zip(plan, plain):
        if item[0] == "pred":
            g, count = guard_np(fmt, f, sources[item[1]], sources[item[2]], r, tol, size)
            out.append(sources[item[1]] if item[1] in held else g)
            shares.append(count / (size[0] * size[1]))
        else:
            out.append(f)
    return out, shares


@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_and_recursive_modes_hold_the_static_regions(model, fmt):
    frames = clip(fmt, 5)
    for mode, factor, r in (("reference", 1, 2), ("recursive", 3, 2), ("reference", 2, 0), ("recursive", 1, 16)):
        plain = list(interpolator(model, fmt, mode=mode, interpolation_factor=factor).run(frames))
        fi = interpolator(model, fmt, mode=mode, interpolation_factor=factor, static_guard=r)
        got = list(fi.run(frames))
        want, shares = expected_pairs(fmt, plain, 5, factor, frames, r)
        same(got, want, (fmt, mode, factor, r))
        assert fi.static_share == shares and len(shares) == 4 * factor, (fmt, mode, factor, r)
        if r <= 2:
            assert all(0.05 < s < 0.5 for s in shares) and any(not np.array_equal(g, p) for g, p in zip(got, plain)), (fmt, mode, shares)
        # run_chunked inherits it
        fc = interpolator(model, fmt, mode=mode, interpolation_factor=factor, static_guard=r)
        same(list(fc.run_chunked(iter(frames), chunk_pairs=3)), want, (fmt, mode, factor, r, "run_chunked"))
        assert fc.static_share == shares
    # off: byte-identical to an interpolator built without the arguments
    same(list(interpolator(model, fmt, static_guard=None, static_tolerance=0.0).run(frames)), list(interpolator(model, fmt).run(frames)), (fmt, "off"))
    assert interpolator(model, fmt).static_share == []


@pytest.mark.parametrize("fmt", ["bgr24", "p010"])
def test_a_tolerance_widens_the_static_regions(model, fmt):
    frames = clip(fmt, 3, seed=4)
    layout, C, sb, depth, shift = lib.static_frame_format(fmt)
    rng = np.random.default_rng(9)
    for f in frames[1:]:                                     # the bands flicker by one count
        band = f[:BAND]
        band += (rng.integers(0, 2, band.shape) << shift).astype(f.dtype) * np.where(band >> shift < (1 << depth) - 1, 1, 0).astype(f.dtype)
    plain = list(interpolator(model, fmt).run(frames))
    full = (1 << depth) - 1
    for fraction, tol in ((0.0, 0), (1.5 / full, 1), (0.01, full // 100)):
        assert lib.static_tolerance_units(fraction, depth) == tol
        fi = interpolator(model, fmt, static_guard=1, static_tolerance=fraction)
        want, shares = expected_pairs(fmt, plain, 3, 1, frames, 1, tol)
        same(list(fi.run(frames)), want, (fmt, fraction))
        assert fi.static_share == shares
    assert shares[0] > expected_pairs(fmt, plain, 3, 1, frames, 1, 0)[1][0]


_trees = {}


def tree(model, fmt, key, f0, f1, depth):
    """nodes 0 .. 2^depth of the pair (f0, f1), unguarded, obtained independently: node j is the j-th prediction of mode "recursive" with
    factor 2^depth - 1"""
    if (fmt, key, depth) not in _trees:
        factor = (1 << depth) - 1
        out = list(interpolator(model, fmt, mode="recursive", interpolation_factor=factor).run([f0, f1]))
        assert len(out) == factor + 2
        _trees[fmt, key, depth] = [out[factor]] + out[:factor] + [out[-1]]
    return _trees[fmt, key, depth]


def expected_resample(model, fmt, outputs, frames, key, r, held=()):
    """outputs: (k, t0, m, j0, j1, w) per output -> (frames, shares): the guarded nodes selected or blended by the resample oracle"""
    sb, depth, shift = lib.resample_sample_format(fmt)
    out, shares = [], []
    for k, t0, m, j0, j1, w in outputs:
        f0, f1 = frames[t0], frames[t0 + m] if t0 + m < len(frames) else None
        dm = D + (m - 1).bit_length()
        inner = lambda j: 0 < j < 1 << dm
        if not (inner(j0) or inner(j1)):
            out.append(frames[t0] if (j0 == 0 or t0 in held) else f1)
            continue
        nodes = tree(model, fmt, (key, t0, t0 + m), f0, f1, dm)
        guarded = [f0] + [guard_np(fmt, nd, f0, f1, r)[0] for nd in nodes[1:-1]] + [f1]
        shares.append(guard_np(fmt, nodes[1], f0, f1, r)[1] / (H * W))
        if t0 in held:
            out.append(f0)
        elif w == 0:
            out.append(guarded[j0])
        else:
            a, b = guarded[j0], guarded[j1]
            out.append(resample_oracle.blend(a.view(np.uint8), b.view(np.uint8), w, sb, depth, shift).view(a.dtype))
    return out, shares


@pytest.mark.parametrize("fmt", FORMATS)
def test_resample_guards_the_nodes_before_it_selects_or_blends(model, fmt):
    frames = clip(fmt, 4, seed=2)
    for method in ("nearest", "blend"):
        plan = FrameInterpolator.resample_plan(4, 24, 60, D, method)
        fi = interpolator(model, fmt, mode="resample", rate_in=24, rate_out=60, resample_depth=D, resample_method=method, static_guard=2)
        got = list(fi.run(frames))
        want, shares = expected_resample(model, fmt, [(k, s, 1, j0, j1, w) for k, s, j0, j1, w in plan.outputs], frames, "clip2", 2)
        same(got, want, (fmt, method))
        assert fi.static_share == shares and len(shares) > 0 and all(0.05 < s < 0.5 for s in shares), (fmt, method, shares)
        plain = list(interpolator(model, fmt, mode="resample", rate_in=24, rate_out=60, resample_depth=D, resample_method=method).run(frames))
        assert any(not np.array_equal(g, p) for g, p in zip(got, plain))
        fc = interpolator(model, fmt, mode="resample", rate_in=24, rate_out=60, resample_depth=D, resample_method=method, static_guard=2)
        same(list(fc.run_chunked(iter(frames), chunk_pairs=2)), want, (fmt, method, "run_chunked"))
        assert fc.static_share == shares


@pytest.mark.parametrize("fmt", FORMATS)
def test_resample_with_dedup_guards_against_the_kept_frames(model, fmt):
    a, b, c, d = clip(fmt, 4, seed=3)
    frames = [a, b, b.copy(), c, d]                        # frame 2 repeats frame 1: kept 0, 1, 3, 4; the gap (1, 3) spans two intervals
    kept = [0, 1, 3, 4]
    for method in ("nearest", "blend"):
        plan = FrameInterpolator.resample_plan_dedup(kept, 24, 60, D, method)
        fi = interpolator(model, fmt, mode="resample", rate_in=24, rate_out=60, resample_depth=D, resample_method=method, dedup_threshold=0.0,
                          static_guard=2)
        got = list(fi.run(frames))
        assert [t for t, _ in fi.duplicates] == [2]
        want, shares = expected_resample(model, fmt, plan.outputs, frames, "clip3", 2)
        same(got, want, (fmt, method))
        assert fi.static_share == shares and len(shares) > 0


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
def test_with_a_resize_the_sources_are_the_device_resized_bytes(model, fmt):
    frames = clip(fmt, 4, seed=5, Hs=2 * H, Ws=2 * W, band=2 * BAND)
    for mode, factor in (("reference", 1), ("recursive", 3)):
        plain = list(interpolator(model, fmt, mode=mode, interpolation_factor=factor, scale=0.5).run(frames))
        # the unguarded stream carries the resized sources: each pair's earlier frame behind its predictions, the last frame at the end
        plan = FrameInterpolator.emission_plan(4, factor, 1, reference_quirks=False)
        small = {item[1]: f for item, f in zip(plan, plain) if item[0] != "pred"}
        assert sorted(small) == [0, 1, 2, 3] and small[0].shape == ((H, W, 3) if fmt == "bgr24" else (H * 3 // 2, W))
        fi = interpolator(model, fmt, mode=mode, interpolation_factor=factor, scale=0.5, static_guard=1)
        want, shares = expected_pairs(fmt, plain, 4, factor, small, 1)
        same(list(fi.run(frames)), want, (fmt, mode, "scale 0.5"))
        assert fi.static_share == shares and all(0.02 < s < 0.5 for s in shares), shares
    plain = list(interpolator(model, fmt, mode="resample", rate_in=30, rate_out=60, resample_depth=1, scale=0.5).run(frames))
    small = plain[0::2]
    fi = interpolator(model, fmt, mode="resample", rate_in=30, rate_out=60, resample_depth=1, scale=0.5, static_guard=1)
    got = list(fi.run(frames))
    want = [f if k % 2 == 0 else guard_np(fmt, f, small[k // 2], small[k // 2 + 1], 1)[0] for k, f in enumerate(plain)]
    same(got, want, (fmt, "resample", "scale 0.5"))
    assert fi.static_share == [guard_np(fmt, plain[k], small[k // 2], small[k // 2 + 1], 1)[1] / (H * W) for k in (1, 3, 5)]


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
def test_together_with_a_scene_cut_the_held_frame_wins_everywhere(model, fmt):
    frames = clip(fmt, 5, seed=6, levels=[0.1, 0.1, 0.7, 0.7, 0.7])      # the cut lies between frames 1 and 2; the bands stay
    img = (lambda f: f) if fmt == "bgr24" else (lambda f: f[:H, :, None])
    sig = scene_oracle.signature(np.stack([img(f) for f in frames]), "bgr")
    sc = [int(scene_oracle.score(sig[t], sig[t + 1], H, W)) for t in range(4)]
    rest = max(s for t, s in enumerate(sc) if t != 1)
    fraction = (sc[1] + rest) / 2 / (4080 * scene_oracle.cells(H, W))
    assert sc[1] > 4 * rest and rest < lib.scene_threshold_units(fraction, H, W) <= sc[1]
    for mode, factor in (("reference", 1), ("recursive", 3)):
        plain = list(interpolator(model, fmt, mode=mode, interpolation_factor=factor).run(frames))
        fi = interpolator(model, fmt, mode=mode, interpolation_factor=factor, scene_threshold=fraction, static_guard=2)
        want, shares = expected_pairs(fmt, plain, 5, factor, frames, 2, held={1})
        same(list(fi.run(frames)), want, (fmt, mode, "cut"))
        assert fi.scene_cuts == [(1, 2, sc[1])] and fi.static_share == shares
    plan = FrameInterpolator.resample_plan(5, 24, 60, D, "blend")
    fi = interpolator(model, fmt, mode="resample", rate_in=24, rate_out=60, resample_depth=D, resample_method="blend", scene_threshold=fraction,
                      static_guard=2)
    want, shares = expected_resample(model, fmt, [(k, s, 1, j0, j1, w) for k, s, j0, j1, w in plan.outputs], frames, "clip6", 2, held={1})
    same(list(fi.run(frames)), want, (fmt, "resample", "cut"))
    assert fi.scene_cuts == [(1, 2, sc[1])] and fi.static_share == shares


@pytest.mark.parametrize("fmt", ["yuv420p8", "yuv420p10"])
def test_command_line_static_guard(model, tmp_path, capsys, fmt):
    frames = clip(fmt, 4, seed=7)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 24, 1, colorspace="420jpeg" if fmt == "yuv420p8" else "420p10")) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1",
                   "--static-guard", "2", "--static-tolerance", "0"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "static guard held" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    fi = interpolator(model, fmt, static_guard=2)                       # seed 0, 8 channels, fp32: the fixture's model
    same(got, list(fi.run(frames)), ("cli", fmt))
    assert f"{100.0 * sum(fi.static_share) / len(fi.static_share):.2f} %" in err
    assert not np.array_equal(got[0], list(interpolator(model, fmt).run(frames))[0])
