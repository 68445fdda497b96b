"""The active area on the GPU: emavfi_active_bounds and emavfi_fill_outside_frames word for word / byte for byte against the numpy
restatement of the active area definition (tests/active_oracle.py), the pitched u8 entries against the dense ones on contiguous copies, and
the harness's active_area in every mode against the PASTE IDENTITY: what the plain harness yields for the host-cropped clip, pasted into
frames whose outside is the pair's earlier source frame.  Every comparison is bit-exact.

The kernels walk 16-byte units of a row, one 16-byte access where pointer, pitch and stride are multiples of 16 and bytes elsewhere: the
sizes have rows below, at and above a unit, with and without a remainder, and the layouts break each alignment condition in turn."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import active_oracle as oracle

pytestmark = pytest.mark.gpu

FILL = 0xFF                        # what lies between rows and frames: content at every level, should a kernel read it
SIZES = [(1, 1), (2, 2), (5, 7), (16, 16), (18, 40), (33, 48)]
KINDS = [("u8c1", 1, 1, 8, 0, 16), ("u8c3", 3, 1, 8, 0, 16), ("w10", 1, 2, 10, 0, 64), ("w10s6", 1, 2, 10, 6, 64)]   # (name, C, sample_bytes, depth, shift, level)
IMAGE_LAYOUTS = ("dense", "pitch16", "oddpitch", "slack")


def pitched(rows, layout, sb=1):
    """`rows` (numpy uint8 [n, H, rowbytes]) on the device in a buffer of FILL bytes, laid out as `layout` says; returns (flat, view):
    dense; rows padded to a longer multiple of 16; an odd pitch (odd in samples) from a base off the 16-byte lattice; dense frames with slack between them"""
    n, H, rb = rows.shape
    pitch = {"dense": rb, "pitch16": (rb + 16) // 16 * 16, "oddpitch": rb + sb, "slack": rb}[layout]
    bstride = H * pitch + (40 if layout == "slack" else 0)
    off = 2 if layout == "oddpitch" else 0
    flat = torch.full((off + n * bstride + 64,), FILL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (n, H, rb), (bstride, pitch, 1), off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    return flat, view


def gaps_intact(flat, view, what):
    probe = flat.clone()
    torch.as_strided(probe, view.shape, view.stride(), view.storage_offset()).fill_(FILL)
    assert bool((probe == FILL).all()), (what, "a byte outside the images changed")


def as_image(view, H, W, C, sb):
    """the byte rows [n, H, rowbytes] as the tensor the wrappers take: uint8 [n,H,W,C], or 16-bit words [n,H,W]"""
    if sb == 1:
        return view.unflatten(2, (W, C))
    n, (bs, pitch, _) = view.shape[0], view.stride()
    words = view._base.view(torch.int16) if view._base is not None else view.view(torch.int16)
    return torch.as_strided(words, (n, H, W), (bs // 2, pitch // 2, 1), view.storage_offset() // 2)


def images(rng, H, W, C, sb, depth, shift, level):
    """the contents of the issue as one batch [n, H, W, C] of elements: no content (samples at and below the level), full content, one pixel at
    each corner and in the middle, the level edge (everything AT the level, one sample one count above), and three frames with different bounds;
    words carry junk in the bits outside the sample"""
    full = (1 << depth) - 1
    dt = np.uint8 if sb == 1 else np.uint16
    none = rng.integers(0, level + 1, (H, W, C))
    out = [none.copy(), rng.integers(level + 1, full + 1, (H, W, C))]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        f = none.copy()
        f[y, x, C - 1] = level + 1 + int(rng.integers(0, full - level))
        out.append(f)
    edge = np.full((H, W, C), level)
    edge[H // 3, W // 2, 0] = level + 1
    out.append(edge)
    for k in range(3):
        f = none.copy()
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y1, x1 = int(rng.integers(y0, H)), int(rng.integers(x0, W))
        f[y0, x0, 0], f[y1, x1, C - 1], f[y0, x1, k % C] = full, level + 1, level + 2
        out.append(f)
    batch = (np.stack(out).astype(np.int64) << shift)
    if sb == 2:
        keep = full << shift
        batch = (batch & keep) | (rng.integers(0, 65536, batch.shape) & ~keep & 0xFFFF)
    return batch.astype(dt)


# ---------------------------------------------------------------- emavfi_active_bounds
@pytest.mark.parametrize("layout", IMAGE_LAYOUTS)
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_bounds_are_the_oracle_word_for_word(kind, layout):
    name, C, sb, depth, shift, level = kind
    for H, W in SIZES:
        rng = np.random.default_rng(H * 131 + W + depth + shift + C)
        batch = images(rng, H, W, C, sb, depth, shift, level)
        n = batch.shape[0]
        want = np.array([oracle.bounds(batch[k], level, depth, shift) for k in range(n)])
        assert (want[0] == (H, 0, W, 0)).all() and (want[1] == (0, H, 0, W)).all() and (want[2] == (0, 1, 0, 1)).all()
        assert (want[5] == (H - 1, H, W - 1, W)).all() and (want[7] == (H // 3, H // 3 + 1, W // 2, W // 2 + 1)).all()
        flat, view = pitched(batch.view(np.uint8).reshape(n, H, W * C * sb), layout, sb)
        img = as_image(view, H, W, C, sb)
        got = []
        for before in (0, -1):                                       # every byte 0x00 / 0xFF before the call
            out = torch.full((n, 4), before, dtype=torch.int32, device="cuda")
            assert lib.active_bounds(img, level, depth=depth, shift=shift, out=out).data_ptr() == out.data_ptr()
            got.append(out.cpu().numpy())
        assert np.array_equal(got[0], want), (name, layout, (H, W), got[0].tolist(), want.tolist())
        assert np.array_equal(got[1], want), (name, layout, (H, W), "a pre-filled buffer changes the words")
        # one image alone (n = 1: the batch stride is not looked at), and a level that leaves nothing
        one = lib.active_bounds(img[n - 1:], level, depth=depth, shift=shift).cpu().numpy()
        assert np.array_equal(one[0], want[n - 1])
        assert np.array_equal(lib.active_bounds(img, (1 << depth) - 1, depth=depth, shift=shift).cpu().numpy(), np.array([(H, 0, W, 0)] * n))
        gaps_intact(flat, view, (name, layout, (H, W)))


def test_bounds_of_pinned_host_images_and_of_many_rows():
    """the image may be pinned host memory; a 720p plane: a 2.39:1 picture in a 16:9 frame, and a single pixel"""
    rng = np.random.default_rng(5)
    img = np.full((2, 720, 1280, 1), 16, np.uint8)
    img[0, 88:632] = rng.integers(17, 236, (544, 1280, 1))
    img[1, 700, 3] = 17
    pinned = torch.from_numpy(img).pin_memory()
    want = np.array([oracle.bounds(f, 16) for f in img])
    assert want.tolist() == [[88, 632, 0, 1280], [700, 701, 3, 4]]
    assert np.array_equal(lib.active_bounds(pinned, 16, device="cuda").cpu().numpy(), want)
    assert np.array_equal(lib.active_bounds(pinned.cuda(), 16).cpu().numpy(), want)


# ---------------------------------------------------------------- emavfi_fill_outside_frames
LAYOUTS = [("interleaved", 3), ("nv12", 1), ("i420", 1)]


def rects(H, W):
    """rectangles that touch each edge, two strictly inside (one off the 16-byte lattice) and the frame itself"""
    return [(0, 0, 16, 32), (H - 16, W - 32, 16, 32), (0, 16, H, 16), (8, 0, 8, W), (8, 16, 16, 16), (2, 6, 10, 20), (0, 0, H, W)]


def pool(frames, pad, off=0):
    """`frames` (numpy [n, samples]) on the device as bytes [n, frame_bytes], frame_bytes + pad apart, `off` bytes into the allocation"""
    data = np.ascontiguousarray(frames).view(np.uint8).reshape(frames.shape[0], 1, -1)
    n, _, fb = data.shape
    flat = torch.full((off + n * (fb + pad) + 64,), FILL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (n, 1, fb), (fb + pad, fb, 1), off)
    view.copy_(torch.from_numpy(data))
    return flat, view, view[:, 0]


@pytest.mark.parametrize("sb", (1, 2))
@pytest.mark.parametrize("layout,C", LAYOUTS, ids=[l for l, _ in LAYOUTS])
def test_fill_outside_is_the_oracle_byte_for_byte(layout, C, sb):
    dt = np.uint8 if sb == 1 else np.uint16
    table = [0, 1, 2, 1, 1]                                        # a source that appears in several entries
    for H, W in ((32, 48), (34, 80)):
        rng = np.random.default_rng(H + W + sb)
        n = oracle.frame_samples(H, W, layout, C)
        srcs = rng.integers(0, 256 ** sb, (3, n)).astype(dt)
        d = rng.integers(0, 256 ** sb, (len(table), n)).astype(dt)  # the sentinels inside the rectangle
        for pad, off in ((0, 0), (32, 0), (6, 2)):                 # dense and aligned; strided and aligned; off the 16-byte lattice
            sflat, sview, s = pool(srcs, pad, off)
            for r in rects(H, W):
                what = (layout, sb, (H, W), (pad, off), r)
                dflat, dview, dst = pool(d, pad + 16, off)
                assert lib.fill_outside_frames(dst, s, table, (H, W), r, layout=layout, C=C, sample_bytes=sb).data_ptr() == dst.data_ptr()
                got = dst.cpu().numpy().view(dt)
                for k, a in enumerate(table):
                    want = oracle.fill_outside(d[k], srcs[a], H, W, layout, C, r)
                    assert np.array_equal(got[k], want), (what, k, int((got[k] != want).sum()))
                if r == (0, 0, H, W):
                    assert np.array_equal(got, d), (what, "the whole frame: dst stays untouched")
                gaps_intact(dflat, dview, what)
            assert np.array_equal(s.cpu().numpy().view(dt), srcs)
            gaps_intact(sflat, sview, (layout, sb, "srcs"))


def test_fill_outside_past_the_launch_cap():
    rng = np.random.default_rng(9)
    H, W, n_dst = 4, 16, 70
    assert n_dst > lib.RESAMPLE_LAUNCH_CAP
    srcs = rng.integers(0, 256, (5, H * W * 3)).astype(np.uint8)
    d = rng.integers(0, 256, (n_dst, H * W * 3)).astype(np.uint8)
    table = [int(v) for v in rng.integers(0, 5, n_dst)]
    table[64], table[69] = 4, 0                                    # the first entry of the second launch and the last one
    dst = torch.from_numpy(d).cuda()
    lib.fill_outside_frames(dst, torch.from_numpy(srcs).cuda(), table, (H, W), (2, 4, 2, 8), layout="interleaved", C=3)
    got = dst.cpu().numpy()
    for k in range(n_dst):
        assert np.array_equal(got[k], oracle.fill_outside(d[k], srcs[table[k]], H, W, "interleaved", 3, (2, 4, 2, 8))), k


# ---------------------------------------------------------------- the pitched u8 entries
@pytest.mark.parametrize("C", (3, 1))
@pytest.mark.parametrize("layout", IMAGE_LAYOUTS)
def test_pitched_u8_entries_are_the_dense_entries_bit_for_bit(layout, C):
    mean, std = lib.IMAGENET_MEAN[:C], lib.IMAGENET_STD[:C]
    for H, W in ((5, 7), (16, 16), (18, 40)):
        rng = np.random.default_rng(H + W + C)
        rows = rng.integers(0, 256, (3, H, W * C)).astype(np.uint8)
        rows[0, 0, :3] = (0, 255, 128)
        flat, view = pitched(rows, layout)
        img = view.unflatten(2, (W, C))
        dense = torch.from_numpy(rows.reshape(3, H, W, C)).cuda()
        want = lib.preprocess_u8(dense, mean=mean, std=std)
        got = lib.preprocess_u8_pitched(img, mean=mean, std=std)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), (layout, C, (H, W), "preprocess")
        gaps_intact(flat, view, (layout, C, (H, W), "preprocess"))
        # the way back: in and out of range, the exact ends, a NaN
        x = torch.from_numpy(rng.uniform(-0.3, 1.3, (3, C, H, W)).astype(np.float32)).cuda()
        x[0, 0, 0, 0], x[1, 0, 0, 0], x[2, 0, 0, 0], x[2, C - 1, H - 1, W - 1] = 0.0, 1.0, float("nan"), 254.5 / 255
        for denorm, src in ((False, x), (True, want)):
            ref = lib.postprocess_u8(src, denormalize=denorm, mean=mean, std=std)
            flat.fill_(FILL)
            assert lib.postprocess_u8_pitched(src, img, denormalize=denorm, mean=mean, std=std).data_ptr() == img.data_ptr()
            assert torch.equal(img, ref), (layout, C, (H, W), "postprocess", denorm)
            gaps_intact(flat, view, (layout, C, (H, W), "postprocess", denorm))


# ---------------------------------------------------------------- the harness
FH, FW, RECT = 48, 96, (8, 16, 32, 64)
FORMATS = ["bgr24", "nv12", "p010", "yuv420p8", "yuv420p10"]
NAMES = {lib.LAYOUT_INTERLEAVED: "interleaved", lib.LAYOUT_NV12: "nv12", lib.LAYOUT_I420: "i420"}
MODES = {"reference": dict(interpolation_factor=2), "recursive": dict(mode="recursive", interpolation_factor=3),
         "nearest": dict(mode="resample", rate_in=24, rate_out=60), "blend": dict(mode="resample", rate_in=24, rate_out=60, resample_method="blend"),
         "shutter": dict(mode="resample", rate_in=24, rate_out=48, shutter=180)}


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
    return m


def fmt_of(fmt):
    """(layout name, C, numpy dtype, frame shape at H x W, depth, shift, Y'CbCr)"""
    layout, C, sb, depth, shift = lib.static_frame_format(fmt)
    shape = (lambda H, W: (H, W, 3)) if fmt == "bgr24" else (lambda H, W: (H * 3 // 2, W))
    return NAMES[layout], C, (np.uint8 if sb == 1 else np.uint16), shape, depth, shift, fmt != "bgr24"


def frame(fmt, t, rect=RECT, bars=None, flip=False, H=FH, W=FW):
    """frame t of a smooth moving picture inside `rect` of an H x W frame whose outside is black (limited range: Y = 16 << (depth - 8)), or
    under `bars` = (rng, hi) noise of 0..hi counts above black in every sample; `flip`: the picture's negative (a hard cut).  Every sample of
    the picture lies well above black, so its bounds are the rectangle's."""
    layout, C, dt, shape, depth, shift, yuv = fmt_of(fmt)
    full = (1 << depth) - 1
    top, left, h, w = rect
    yy, xx = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.35 * np.sin(2 * np.pi * (xx + t) / 32.0) * np.cos(2 * np.pi * yy / 16.0)       # one pixel to the left per frame
    v = 1.0 - v if flip else v
    flat = np.zeros(oracle.frame_samples(H, W, layout, C), np.int64)
    pl = oracle.planes(flat, H, W, layout, C)
    if not yuv:
        pl[0][:] = 0 if bars is None else bars[0].integers(0, bars[1] + 1, pl[0].shape)
        pl[0][top:top + h, left:left + w] = np.stack([v, 0.8 * v + 0.1, 1.0 - v], axis=2) * 255
    else:
        black, grey = 16 << (depth - 8), 128 << (depth - 8)
        pl[0][:] = black + (0 if bars is None else bars[0].integers(0, bars[1] + 1, pl[0].shape))
        pl[0][top:top + h, left:left + w] = black + v * (219 << (depth - 8))
        c = v[0::2, 0::2]
        u, vv = grey + (c - 0.5) * (200 << (depth - 8)), grey - (c - 0.5) * (120 << (depth - 8))
        for p in pl[1:]:
            p[:] = grey if bars is None else bars[0].integers(0, full + 1, p.shape)          # chroma is not looked at
        box = (slice(top // 2, (top + h) // 2), slice(left // 2, (left + w) // 2))
        if layout == "nv12":
            pl[1][box + (0,)], pl[1][box + (1,)] = u, vv
        else:
            pl[1][box], pl[2][box] = u, vv
    return (flat << shift).astype(dt).reshape(shape(H, W))


def cropped(fmt, f, rect, H=FH, W=FW):
    layout, C, dt, shape, *_ = fmt_of(fmt)
    return oracle.crop(f.reshape(-1), H, W, layout, C, rect).reshape(shape(rect[2], rect[3]))


def pasted(fmt, pred, a, rect, H=FH, W=FW):
    layout, C, dt, shape, *_ = fmt_of(fmt)
    return oracle.paste(pred.reshape(-1), a.reshape(-1), H, W, layout, C, rect).reshape(shape(H, W))


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


def interpolator(model, fmt, **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, pixel_format=fmt, **kw)


def earlier_frames(n, kw):
    """per output of run() on n frames, in order: the index of the frame whose bars it carries - the pair's earlier frame, a source itself"""
    if kw.get("mode") != "resample":
        plan = FrameInterpolator.emission_plan(n, kw.get("interpolation_factor", 1), 1, reference_quirks=False)
        return [item[1] for item in plan]
    P, Q = FrameInterpolator.resample_ratio(kw["rate_in"], kw["rate_out"])
    return [min((k * P) // Q, n - 1) for k in range(((n - 1) * Q) // P + 1)]


def paste_identity(model, fmt, frames, rect, kw):
    """what the plain harness yields for the host-cropped clip, pasted into frames whose outside is the pair's earlier source frame"""
    plain = list(interpolator(model, fmt, **kw).run([cropped(fmt, f, rect) for f in frames]))
    idx = earlier_frames(len(frames), kw)
    assert len(idx) == len(plain)
    return [pasted(fmt, p, frames[i], rect) for p, i in zip(plain, idx)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_harness_yields_the_paste_identity(model, fmt, mode):
    kw = MODES[mode]
    frames = [frame(fmt, t) for t in range(4)]
    want = paste_identity(model, fmt, frames, RECT, kw)
    for area in ("auto", RECT):
        fi = interpolator(model, fmt, active_area=area, **kw)
        same(list(fi.run(frames)), want, (fmt, mode, area))
        assert fi.active_rect == RECT and fi.active_share == (32 * 64) / (48 * 96)
        assert fi.prepass_waits == (1 if area == "auto" else 0)                       # an explicit rectangle: no scan, no host wait
    # the rectangle was really cut: the whole-frame forward gives other bytes (zero padding at the picture's edge, not the bar)
    whole = list(interpolator(model, fmt, **kw).run(frames))
    assert any(not np.array_equal(a, b) for a, b in zip(whole, want))
    if kw.get("mode") != "resample":
        # bars that differ from frame to frame (content outside an explicit rectangle): every prediction carries its pair's EARLIER frame's
        noisy = [frame(fmt, t, bars=(np.random.default_rng(t), 200)) for t in range(4)]
        assert not np.array_equal(noisy[0][:8], noisy[1][:8])
        same(list(interpolator(model, fmt, active_area=RECT, **kw).run(noisy)), paste_identity(model, fmt, noisy, RECT, kw), (fmt, mode, "noisy bars"))


@pytest.mark.parametrize("fmt", ["bgr24", "nv12", "p010"])
def test_noise_up_to_the_tolerance_is_bar_one_count_above_it_is_picture(model, fmt):
    depth, yuv = fmt_of(fmt)[4], fmt != "bgr24"
    tol = 0.02
    level = lib.active_level_units(tol, depth, yuv, False)
    black = (16 << (depth - 8)) if yuv else 0
    hi = level - black
    assert hi == int(np.floor(tol * ((1 << depth) - 1))) and hi >= 5
    rng = np.random.default_rng(3)
    frames = [frame(fmt, t, bars=(rng, hi)) for t in range(3)]
    frames[0].reshape(-1)[0] = frames[2][FH - 1].reshape(-1)[-1] = (black + hi) << fmt_of(fmt)[5]      # the corners of the luma / first plane AT the level
    fi = interpolator(model, fmt, active_area="auto", active_tolerance=tol)
    out = list(fi.run(frames))
    assert fi.active_rect == RECT
    same(out, paste_identity(model, fmt, frames, RECT, {}), (fmt, "noise at the tolerance"))
    # one count above the tolerance in two opposite corners: the union covers the frame, the plain path runs
    frames[0].reshape(-1)[0] = frames[2][FH - 1].reshape(-1)[-1] = (black + hi + 1) << fmt_of(fmt)[5]
    out = list(fi.run(frames))
    assert fi.active_rect == (0, 0, FH, FW) and fi.active_share == 1.0
    same(out, list(interpolator(model, fmt).run(frames)), (fmt, "noise above the tolerance"))
    # without a tolerance the noise is picture too
    fi0 = interpolator(model, fmt, active_area="auto")
    list(fi0.run(frames))
    assert fi0.active_rect == (0, 0, FH, FW)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_clip_without_bars_is_the_plain_path(model, fmt):
    frames = [frame(fmt, t, rect=(0, 0, FH, FW)) for t in range(3)]
    for kw in (MODES["recursive"], MODES["blend"]):
        want = list(interpolator(model, fmt, **kw).run(frames))
        for area in ("auto", (0, 0, FH, FW)):
            fi = interpolator(model, fmt, active_area=area, **kw)
            same(list(fi.run(frames)), want, (fmt, area))
            assert fi.active_share == 1.0 and fi.active_rect == (0, 0, FH, FW)
    # a black clip: an empty union is the whole frame too
    dark = [frame(fmt, 0, rect=(0, 0, 2, 16)) for _ in range(3)]
    for f in dark:
        f[:2, :16] = f[4:6, :16]
    fi = interpolator(model, fmt, active_area="auto")
    same(list(fi.run(dark)), list(interpolator(model, fmt).run(dark)), (fmt, "dark"))
    assert fi.active_share == 1.0


def test_an_explicit_rectangle_is_checked_against_the_frame(model):
    frames = [frame("nv12", t) for t in range(2)]
    for rect, word in (((8, 16, 48, 64), "leaves"), ((8, 16, 32, 96), "leaves"), ((8, 16, 31, 64), "multiples of 2"), ((8, 16, 32, 60), "multiples of 16")):
        with pytest.raises(ValueError, match=word):
            list(interpolator(model, "nv12", active_area=rect).run(frames))
    fi = interpolator(model, "bgr24", active_area="auto")
    with pytest.raises(ValueError, match="world > 1 with active_area='auto'"):
        list(fi.run([frame("bgr24", t) for t in range(4)], rank=0, world=2))
    with pytest.raises(ValueError, match=r"evaluate\(\) with active_area"):
        fi.evaluate([frame("bgr24", t) for t in range(3)])


def test_composed_with_border_ensemble_static_guard_scene_and_dedup(model):
    """everything at once, held against the same paste identity; the cut and the duplicate are clear on the whole frame and on the picture alike"""
    fmt = "nv12"
    kw = dict(mode="resample", rate_in=24, rate_out=60, border=4, ensemble="reverse", static_guard=1, scene_threshold=0.06, dedup_threshold=0.0)
    frames = [frame(fmt, t) for t in (0, 1, 1, 2, 3)] + [frame(fmt, t, flip=True) for t in (4, 5)]     # frame 2 copies frame 1; a cut between frames 4 and 5
    plain = interpolator(model, fmt, **kw)
    want = [pasted(fmt, p, frames[0], RECT) for p in plain.run([cropped(fmt, f, RECT) for f in frames])]  # black bars: every frame's are frame 0's
    assert [t for t, _ in plain.duplicates] == [2] and [(a, b) for a, b, _ in plain.scene_cuts] == [(4, 5)] and plain.prepass_waits == 1
    for area in ("auto", RECT):
        fi = interpolator(model, fmt, active_area=area, **kw)
        same(list(fi.run(frames)), want, ("composed", area))
        assert fi.active_rect == RECT
        assert [t for t, _ in fi.duplicates] == [2] and [(a, b) for a, b, _ in fi.scene_cuts] == [(4, 5)]
        assert fi.prepass_waits == 1                                                   # "auto" and dedup share the upload and the one wait
        assert len(fi.static_share) == len(plain.static_share) and all(s > 0 for s in fi.static_share)


@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p10"])
def test_run_chunked(model, fmt):
    kw = MODES["reference"]
    frames = [frame(fmt, t) for t in range(7)]
    fi = interpolator(model, fmt, active_area=RECT, **kw)
    want = list(fi.run(frames))
    same(list(fi.run_chunked(iter(frames), chunk_pairs=2)), want, (fmt, "explicit"))
    fa = interpolator(model, fmt, active_area="auto", **kw)
    same(list(fa.run_chunked(iter(frames), chunk_pairs=2)), want, (fmt, "auto, the first chunk shows the final rectangle"))
    assert fa.prepass_waits == 3 and fa.active_rect == RECT
    # the third chunk (frames 4..6) has content outside the first chunks' rectangle: the rectangle grows there and never shrinks
    GROWN = (8, 16, 36, 80)
    frames = [frame(fmt, t) for t in range(5)] + [frame(fmt, t, rect=GROWN) for t in (5, 6)]
    seen, got = [], []
    for f in fa.run_chunked(iter(frames), chunk_pairs=2):
        got.append(f)
        seen.append(fa.active_rect)
    per = kw["interpolation_factor"] + 1
    assert seen[:4 * per] == [RECT] * (4 * per) and seen[4 * per:] == [GROWN] * (2 * per + 1) and len(got) == 6 * per + 1
    plan = FrameInterpolator.emission_plan(7, kw["interpolation_factor"], 1, reference_quirks=False)
    for item, g in zip(plan, got):
        if item[0] != "pred":
            assert np.array_equal(g, frames[item[1]]), ("a source frame comes out untouched", item)
    same(got[:4 * per], paste_identity(model, fmt, frames[:5], RECT, kw)[:4 * per], (fmt, "the first two chunks"))
    same(got[4 * per:], paste_identity(model, fmt, frames[4:], GROWN, kw), (fmt, "the grown chunk"))
    # a later chunk with a smaller picture keeps the rectangle
    frames = [frame(fmt, t, rect=GROWN) for t in range(3)] + [frame(fmt, t) for t in (3, 4, 5, 6)]   # the third chunk shows the small picture only
    out = list(fa.run_chunked(iter(frames), chunk_pairs=2))
    assert fa.active_rect == GROWN
    same(out, paste_identity(model, fmt, frames, GROWN, kw), (fmt, "never shrinks"))


@pytest.mark.parametrize("area", ["auto", "8,16,32,64"])
def test_command_line_active_area(model, tmp_path, capsys, area):
    fmt = "yuv420p8"
    frames = [frame(fmt, t) for t in range(4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(FW, FH, 24, 1, colorspace="420jpeg")) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1",
                   "--active-area", area])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "active area (8, 16, 32, 64) = 44.4 % of the frame" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    fi = interpolator(model, fmt, active_area="auto" if area == "auto" else RECT)      # seed 0, 8 channels, fp32: the fixture's model
    same(got, list(fi.run(frames)), ("cli", area))
    same(got, paste_identity(model, fmt, frames, RECT, dict(interpolation_factor=1)), ("cli", area, "paste"))
