"""Planar 4:2:0 frames on the GPU: emavfi_preprocess_yuv420p / emavfi_postprocess_yuv420p, the harness's pixel_format="yuv420p8" / "yuv420p10" /
"yuv420p12" / "yuv420p16", FrameInterpolator.run_chunked and the Y4M command line.  The planar entries are DEFINED by composition on the NV12 /
P010 entries (include/emavfi.h, "PLANAR 4:2:0"), so every check runs those on the interleaved (and shifted) planes on the same device and
compares - and compares with the numpy restatements (tests/nv12_oracle.py, tests/p010_oracle.py) as well.  Every comparison is equality."""
import io
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, lib, synth, y4m, cli
import nv12_oracle
import p010_oracle

pytestmark = pytest.mark.gpu

DEPTHS = (8, 10, 12, 16)
# odd sizes, one and several blocks, and widths on both sides of the widths the wide path starts at (16 columns at depth 8, 8 above)
SHAPES = [(1, 1), (2, 2), (3, 5), (6, 10), (23, 37), (24, 40), (32, 30), (32, 32), (32, 34), (32, 62), (32, 64), (32, 66), (45, 67), (46, 66)]
LAYOUTS = ["dense", "pad16", "odd", "bstride", "offset2"]
FILL = 0xA5
GUARD = 64          # floats in front of and behind an fp32 result
SENTINEL = -12345.0


def up(v, m):
    return (v + m - 1) // m * m


def colour_of(depth, n):
    standards = nv12_oracle.STANDARDS if depth == 8 else p010_oracle.STANDARDS
    return (*standards[n % len(standards)], "rgb" if (n // len(standards)) & 1 else "bgr")


def geometry(layout, rows, rowbytes, es):
    """(pointer offset, pitch, batch stride) in BYTES of one plane of `rows` rows of `rowbytes` bytes, samples of `es` bytes"""
    if layout == "dense":
        off, pitch = 0, rowbytes
    elif layout == "pad16":
        off, pitch = 0, up(rowbytes, 16) + 16
    elif layout == "odd":            # larger than the row, no multiple of 16; an odd number of bytes where the sample is a byte
        off, pitch = 0, (rowbytes + 3) | 1 if es == 1 else rowbytes + 6
    elif layout == "bstride":
        off, pitch = 0, up(rowbytes, 16)
    else:                            # "offset2": 2 bytes past a 16-byte boundary, aligned pitch
        off, pitch = 2, up(rowbytes, 16)
    return off, pitch, pitch * rows + (pitch * 3 + 32 if layout == "bstride" else 0)


def strided(layout, B, rows, cols, es):
    """a raw byte buffer full of FILL and a [B, rows, cols] view (uint8 or 16-bit words) into it"""
    off, pitch, bstride = geometry(layout, rows, cols * es, es)
    raw = torch.full((up(off + B * bstride + pitch + 64, 16),), FILL, dtype=torch.uint8, device="cuda")
    base = raw if es == 1 else raw[off % 2:].view(torch.int16)
    assert es == 1 or off % 2 == 0
    return raw, base.as_strided((B, rows, cols), (bstride // es, pitch // es, 1), storage_offset=off // es)


def planes(layout, B, H, W, depth):
    es, H2, W2 = (1 if depth == 8 else 2), (H + 1) // 2, (W + 1) // 2
    return [strided(layout, B, r, c, es) for r, c in ((H, W), (H2, W2), (H2, W2))]


def to_t(a):
    """numpy uint8 / uint16 -> torch uint8 / int16 with the same bits"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16))


def to_np(t):
    t = t.contiguous().cpu()
    return t.numpy() if t.dtype == torch.uint8 else t.view(torch.int16).numpy().view(np.uint16)


def interleave(u, v, depth):
    """planar chroma -> the interleaved plane of the NV12 / P010 entries, samples shifted to the top of the word (high garbage masked)"""
    uv = np.stack([u, v], axis=-1)
    return uv if depth == 8 else ((uv & np.uint16(2 ** depth - 1)) << (16 - depth)).astype(np.uint16)


def top(y, depth):
    return y if depth == 8 else ((y & np.uint16(2 ** depth - 1)) << (16 - depth)).astype(np.uint16)


def reference_pre(y, u, v, depth, colour, on_device=True):
    """what the definition says: the NV12 / P010 entry (or its numpy restatement) on the interleaved, shifted planes"""
    ys, uvs = top(y, depth), interleave(u, v, depth)
    if on_device:
        if depth == 8:
            return lib.preprocess_nv12(to_t(ys).cuda(), to_t(uvs).cuda(), *colour).cpu().numpy()
        return lib.preprocess_p010(to_t(ys).cuda(), to_t(uvs).cuda(), depth, *colour).cpu().numpy()
    if depth == 8:
        return p010_oracle.normalise(nv12_oracle.decode(ys, uvs, *colour), 8)
    return p010_oracle.preprocess(ys, uvs, depth, *colour)


def reference_post(x, depth, colour, denorm, on_device=True):
    """(y, u, v) planar: the NV12 / P010 entry's planes de-interleaved, words >> (16 - depth)"""
    if on_device:
        xt = torch.from_numpy(x).cuda()
        y, uv = (lib.postprocess_nv12(xt, *colour, denormalize=bool(denorm)) if depth == 8 else
                 lib.postprocess_p010(xt, depth, *colour, denormalize=bool(denorm)))
        y, uv = to_np(y), to_np(uv)
    elif depth == 8:
        y, uv = nv12_oracle.encode(p010_oracle.quantise(x, 8, bool(denorm)).astype(np.uint8), *colour)
    else:
        y, uv = p010_oracle.postprocess(x, depth, *colour, denormalize=bool(denorm))
    if depth > 8:
        y, uv = y >> (16 - depth), uv >> (16 - depth)
    return y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1])


def rand_planes(rng, B, H, W, depth):
    """random samples; at depth 10 / 12 with garbage in the high bits of every word"""
    dt, top_ = (np.uint8, 256) if depth == 8 else (np.uint16, 65536)
    return [rng.integers(0, top_, (B, r, c)).astype(dt) for r, c in ((H, W), ((H + 1) // 2, (W + 1) // 2), ((H + 1) // 2, (W + 1) // 2))]


def check_decode(ynp, unp, vnp, layout, depth, colour):
    B, H, W = ynp.shape
    bufs = planes(layout, B, H, W, depth)
    for (_, view), a in zip(bufs, (ynp, unp, vnp)):
        view.copy_(to_t(a))
    flat = torch.full((B * 3 * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = flat[GUARD:GUARD + B * 3 * H * W].view(B, 3, H, W)
    got = lib.preprocess_yuv420p(*(v for _, v in bufs), depth, *colour, out=out)
    assert got.data_ptr() == out.data_ptr()
    bits = got.cpu().numpy().view(np.int32)
    assert np.array_equal(bits, reference_pre(ynp, unp, vnp, depth, colour).view(np.int32)), ("entry", layout, depth, colour, (B, H, W))
    assert np.array_equal(bits, reference_pre(ynp, unp, vnp, depth, colour, on_device=False).view(np.int32)), ("oracle", layout, depth, colour, (B, H, W))
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "floats beyond [B,3,H,W] were written"
    return got


def encode_input(B, H, W, depth, denorm, seed):
    """fp32 [B,3,H,W] whose quantised integers are random and sit mid-interval, with NaN / Inf / out-of-range values sprinkled in"""
    rng = np.random.default_rng(seed)
    P = 2 ** depth - 1
    x = (rng.integers(0, P + 1, (B, H, W, 3)).astype(np.float64) + 0.5) / P
    if denorm:
        x = (x - np.array(p010_oracle.MEAN)) / np.array(p010_oracle.STD)
    x = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)
    flat = x.reshape(-1)
    for j, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 2.0, 1.0, 0.0, -0.0)):
        if flat.size > j:
            flat[(flat.size // 8 * j + 3 * j) % flat.size] = v
    return x


def check_encode(xnp, layout, depth, colour, denorm):
    B, _, H, W = xnp.shape
    bufs = planes(layout, B, H, W, depth)
    lib.postprocess_yuv420p(torch.from_numpy(xnp).cuda(), depth, *colour, denormalize=bool(denorm), out=tuple(v for _, v in bufs))
    want = reference_post(xnp, depth, colour, denorm)
    oracle = reference_post(xnp, depth, colour, denorm, on_device=False)
    expect = planes(layout, B, H, W, depth)        # images of the raw buffers: the planes where they belong, FILL everywhere else
    for name, (raw, view), (eraw, eview), w, o in zip("YUV", bufs, expect, want, oracle):
        assert np.array_equal(to_np(view), w), (name, "entry", layout, depth, colour, denorm, (B, H, W))
        assert np.array_equal(w, o), (name, "oracle", layout, depth, colour, denorm, (B, H, W))
        if depth > 8:
            assert not (to_np(view) >> depth).any() if depth < 16 else True, "the high bits of every word must be zero"
        eview.copy_(to_t(w))
        assert torch.equal(raw, eraw), ("bytes outside the plane were written", name, layout, depth, (B, H, W))
    return [v for _, v in bufs]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_equals_the_interleaved_entries(layout, depth):
    rng = np.random.default_rng(11 + depth)
    for n, ((H, W), B) in enumerate(itertools.product(SHAPES, (1, 3))):
        check_decode(*rand_planes(rng, B, H, W, depth), layout, depth, colour_of(depth, n + LAYOUTS.index(layout)))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_equals_the_interleaved_entries(layout, depth):
    for n, ((H, W), B) in enumerate(itertools.product(SHAPES, (1, 3))):
        check_encode(encode_input(B, H, W, depth, n & 1, seed=100 + n), layout, depth, colour_of(depth, n + LAYOUTS.index(layout)), n & 1)


@pytest.mark.parametrize("depth", (10, 12))
def test_high_bits_are_ignored_on_read(depth):
    rng = np.random.default_rng(77)
    dirty = rand_planes(rng, 2, 32, 64, depth)
    clean = [a & np.uint16(2 ** depth - 1) for a in dirty]
    assert all((d != c).any() for d, c in zip(dirty, clean))
    colour = ("bt709", False, "bgr")
    for layout in ("dense", "offset2"):                                   # the wide and the scalar form
        a, b = check_decode(*dirty, layout, depth, colour), check_decode(*clean, layout, depth, colour)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("depth", DEPTHS)
def test_wide_path_equals_scalar_path(depth):
    """the same frames once 16-byte aligned (16-byte accesses) and once through views 2 bytes off (scalar accesses)"""
    rng = np.random.default_rng(17)
    B, H, W = 3, 34, 96
    colour = colour_of(depth, depth)
    src = rand_planes(rng, B, H, W, depth)
    fast, slow = check_decode(*src, "pad16", depth, colour), check_decode(*src, "offset2", depth, colour)
    assert torch.equal(fast.view(torch.int32), slow.view(torch.int32))
    for denorm in (0, 1):
        x = encode_input(B, H, W, depth, denorm, seed=23)
        for f, s in zip(check_encode(x, "pad16", depth, colour, denorm), check_encode(x, "offset2", depth, colour, denorm)):
            assert torch.equal(f, s)


def test_default_outputs_numpy_pinned_planes_and_yv12():
    rng = np.random.default_rng(3)
    B, H, W = 2, 32, 48
    for depth in (8, 10):
        colour = colour_of(depth, 2)
        y, u, v = (a & (2 ** depth - 1) if depth > 8 else a for a in rand_planes(rng, B, H, W, depth))
        want = reference_pre(y, u, v, depth, colour)
        dev = [to_t(a).cuda() for a in (y, u, v)]
        got = lib.preprocess_yuv420p(*dev, depth, *colour)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
        pinned = lib.preprocess_yuv420p(*(to_t(a).pin_memory() for a in (y, u, v)), depth, *colour, device="cuda")
        assert torch.equal(pinned.view(torch.int32), got.view(torch.int32))
        if depth > 8:                                                     # numpy uint16 planes are uploaded
            assert torch.equal(lib.preprocess_yuv420p(y, u, v, depth, *colour, device="cuda").view(torch.int32), got.view(torch.int32))
        # YV12: the caller swaps two arguments
        swapped = lib.preprocess_yuv420p(dev[0], dev[2], dev[1], depth, *colour)
        assert np.array_equal(swapped.cpu().numpy().view(np.int32), reference_pre(y, v, u, depth, colour).view(np.int32))
        outs = lib.postprocess_yuv420p(got, depth, *colour)
        assert all(p.is_contiguous() and p.dtype == (torch.uint8 if depth == 8 else lib.word_dtype()) for p in outs)
        for p, w in zip(outs, reference_post(want, depth, colour, True)):
            assert np.array_equal(to_np(p), w)
        host = [torch.zeros(p.shape, dtype=torch.uint8 if depth == 8 else torch.int16).pin_memory() for p in outs]
        lib.postprocess_yuv420p(got, depth, *colour, out=tuple(host))
        torch.cuda.synchronize()
        assert all(np.array_equal(to_np(h), to_np(p)) for h, p in zip(host, outs))
    with pytest.raises(ValueError, match="rows of u"):
        lib.preprocess_yuv420p(torch.zeros(1, 4, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, 2, 8, dtype=torch.uint8, device="cuda")[:, :, ::2],
                               torch.zeros(1, 2, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="v must be"):
        lib.preprocess_yuv420p(torch.zeros(1, 4, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, 2, 4, dtype=torch.uint8, device="cuda"),
                               torch.zeros(1, 2, 5, dtype=torch.uint8, device="cuda"))


# ---------------------------------------------------------------- the harness
H, W, NFRAMES = 48, 64, 11
SEMI = {"yuv420p8": "nv12", "yuv420p10": "p010", "yuv420p12": "p012", "yuv420p16": "p016"}


def to_planar(frame, depth):
    """a contiguous NV12 / P010 frame [H*3/2, W] -> the planar frame of the same samples (words: the sample in the low bits)"""
    h = frame.shape[0] * 2 // 3
    uv = frame[h:].reshape(h // 2, frame.shape[1] // 2, 2)
    out = np.concatenate([frame[:h].reshape(-1), uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)]).reshape(frame.shape)
    return out if depth == 8 else out >> (16 - depth)


def clip_rgb(n=NFRAMES, cut=None):
    """a synthetic clip as [0,1] floats [n, H, W, 3]: smooth moving content; from frame `cut` on, another scene"""
    rng = np.random.default_rng(41)
    base = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy()
    clip = np.stack([np.clip(np.roll(base, 2 * i, axis=2).transpose(1, 2, 0) * 0.2 + 0.45 + rng.normal(0, 0.02, (H, W, 3)), 0, 1) for i in range(n)])
    if cut is not None:
        clip[cut:] = clip[cut:][:, ::-1] * 0.3       # upside down and dark: a hard cut by any measure
    return clip


def clips(fmt, cut=None):
    """(semi-planar frames, planar frames) of the same clip"""
    depth = lib.PLANAR_DEPTHS[fmt]
    rgb = clip_rgb(cut=cut)
    if depth == 8:
        semi = [np.concatenate([y, uv.reshape(uv.shape[0], -1)]) for y, uv in (nv12_oracle.encode((img * 255).astype(np.uint8)) for img in rgb)]
    else:
        semi = [np.concatenate([y, uv.reshape(uv.shape[0], -1)]) for y, uv in
                (p010_oracle.encode((img * (2 ** depth - 1)).astype(np.int64), depth) for img in rgb)]
    return semi, [to_planar(f, depth) for f in semi]


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    return m


def same(got, want, depth, shape=(H * 3 // 2, W)):
    dt = np.uint8 if depth == 8 else np.uint16
    return len(got) == len(want) and all(g.dtype == dt and g.shape == shape and np.array_equal(g, to_planar(w, depth)) for g, w in zip(got, want))


@pytest.mark.parametrize("factor,batch", [(1, 2), (1, 8), (3, 2), (3, 8)])
@pytest.mark.parametrize("fmt", list(SEMI))
def test_harness_stream_is_the_interleaved_stream_deinterleaved(model, fmt, factor, batch):
    depth = lib.PLANAR_DEPTHS[fmt]
    semi, planar = clips(fmt)
    yuv = dict(yuv_standard="bt2020" if depth == 16 else "bt709", yuv_full_range=depth == 12)
    for kw in (dict(reference_quirks=False), dict(reference_quirks=True), dict(zero_copy=True), dict(reference_quirks=False, copy_out=False)):
        want = [f.copy() for f in FrameInterpolator(model, factor, 1, batch_pairs=batch, pixel_format=SEMI[fmt], **yuv, **kw).run(semi)]
        fi = FrameInterpolator(model, factor, 1, batch_pairs=batch, pixel_format=fmt, **yuv, **kw)
        got = [f.copy() for f in fi.run(planar)]
        assert len(got) == fi.count_outputs(NFRAMES) and same(got, want, depth), (fmt, factor, batch, kw)


def test_harness_yuv420p8_resize_scene_cuts_and_evaluate_equal_nv12(model):
    semi, planar = clips("yuv420p8", cut=6)
    for quirks in (False, True):
        for kw in (dict(size=(24, 32)), dict(scene_threshold=0.1), dict(size=(24, 32), scene_threshold=0.1, zero_copy=quirks)):
            ref = FrameInterpolator(model, 1, 1, batch_pairs=2, reference_quirks=quirks, pixel_format="nv12", **kw)
            fi = FrameInterpolator(model, 1, 1, batch_pairs=2, reference_quirks=quirks, pixel_format="yuv420p8", **kw)
            want, got = list(ref.run(semi)), list(fi.run(planar))
            shape = (36, 32) if "size" in kw else (H * 3 // 2, W)
            assert same(got, want, 8, shape), (quirks, kw)
            if "scene_threshold" in kw:
                assert fi.scene_cuts == ref.scene_cuts and [c[:2] for c in fi.scene_cuts] == [(5, 6)] and fi.scene_scores == ref.scene_scores
    # the skip-branch ending with a resize: the tail frame is a device round trip of a resized planar frame
    kw = dict(size=(24, 32), batch_pairs=2)
    assert same(list(FrameInterpolator(model, 1, 2, pixel_format="yuv420p8", **kw).run(planar)),
                list(FrameInterpolator(model, 1, 2, pixel_format="nv12", **kw).run(semi)), 8, (36, 32))
    for kw in (dict(), dict(size=(24, 32))):
        a = FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="nv12", **kw).evaluate(semi, every=2)
        b = FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="yuv420p8", **kw).evaluate(planar, every=2)
        assert len(b) == 5 and b.channels == 1 and b.size == a.size and b.targets == a.targets


def test_harness_refuses_bad_frames_and_the_out_of_scope_combinations(model):
    fi = FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="yuv420p10")
    with pytest.raises(ValueError, match="uint16"):
        list(fi.run([np.zeros((72, 64), np.uint8)] * 2))
    with pytest.raises(ValueError, match="even H and W"):
        list(fi.run([np.zeros((35, 40), np.uint16)] * 2))
    with pytest.raises(ValueError, match="evaluate"):
        fi.evaluate([np.zeros((72, 64), np.uint16)] * 3)
    with pytest.raises(ValueError, match="uint8"):
        list(FrameInterpolator(model, 1, 1, pixel_format="yuv420p8").run([np.zeros((72, 64), np.uint16)] * 2))


# ---------------------------------------------------------------- run_chunked
@pytest.mark.parametrize("mode,factor", [("reference", 1), ("recursive", 3)])
@pytest.mark.parametrize("interval", [1, 2, 3])
def test_run_chunked_equals_run(model, interval, mode, factor):
    _, planar = clips("yuv420p8", cut=6)
    for n, k in enumerate((1, 4, 10, 64)):
        kw = dict(batch_pairs=2, mode=mode, pixel_format="yuv420p8", reference_quirks=bool(n & 1), scene_threshold=0.1 if n != 2 else None)
        ref = FrameInterpolator(model, factor, interval, **kw)
        want = list(ref.run(planar))
        fi = FrameInterpolator(model, factor, interval, **kw)
        got = list(fi.run_chunked(iter(planar), chunk_pairs=k))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (interval, mode, k)
        assert fi.scene_cuts == ref.scene_cuts and fi.scene_scores == ref.scene_scores, (interval, mode, k)    # global frame indices
        if kw["scene_threshold"] and interval == 1:
            assert [c[:2] for c in fi.scene_cuts] == [(5, 6)]
    assert list(FrameInterpolator(model, 1, interval, pixel_format="yuv420p8").run_chunked(iter([]))) == []
    one = list(FrameInterpolator(model, 1, interval, pixel_format="yuv420p8").run_chunked(iter(planar[:1]), chunk_pairs=1))
    assert len(one) == 1 and np.array_equal(one[0], list(FrameInterpolator(model, 1, interval, pixel_format="yuv420p8").run(planar[:1]))[0])


def test_run_chunked_deep_format(model):
    _, planar = clips("yuv420p10")
    want = list(FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="yuv420p10").run(planar))
    got = list(FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="yuv420p10").run_chunked((f for f in planar), chunk_pairs=5))
    assert len(got) == len(want) and all(g.dtype == np.uint16 and np.array_equal(g, w) for g, w in zip(got, want))


# ---------------------------------------------------------------- the command line
def write_y4m(path, frames, tag, extra=("XYSCSS=TEST",)):
    head = y4m.Y4MHeader(W, H, 30000, 1001, "p", "1:1", tag, tuple(x[1:] for x in extra))
    with y4m.Y4MWriter(str(path), head) as w:
        for f in frames:
            w.write(f)
    return head


@pytest.mark.parametrize("fmt,tag", [("yuv420p8", "420mpeg2"), ("yuv420p10", "420p10")])
def test_cli_writes_what_the_harness_yields(model, tmp_path, capsys, fmt, tag):
    _, planar = clips(fmt)
    head = write_y4m(tmp_path / "in.y4m", planar, tag)
    common = ["--synthetic-weights", "21", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2"]
    assert cli.main([str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), "--factor", "3", "--chunk-pairs", "4", *common]) == 0
    with y4m.Y4MReader(str(tmp_path / "out.y4m")) as r:
        assert r.header == head.for_output(3) and (r.header.fps_num, r.header.fps_den) == (120000, 1001) and r.header.extensions == ("YSCSS=TEST",)
        got = list(r)
    want = list(FrameInterpolator(model, 3, 1, batch_pairs=2, reference_quirks=False, pixel_format=fmt).run(planar))
    assert len(got) == len(want) == 41 and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    # the automatic factor: 29.97 fps -> factor 1
    assert cli.main([str(tmp_path / "in.y4m"), str(tmp_path / "auto.y4m"), "--reference-quirks", *common]) == 0
    with y4m.Y4MReader(str(tmp_path / "auto.y4m")) as r:
        assert (r.header.fps_num, r.header.fps_den) == (60000, 1001)
        got = list(r)
    want = list(FrameInterpolator(model, 1, 1, batch_pairs=2, reference_quirks=True, pixel_format=fmt).run(planar))
    assert len(got) == len(want) == 21 and all(np.array_equal(g, w) for g, w in zip(got, want))
    capsys.readouterr()
    if fmt == "yuv420p8":
        assert cli.main([str(tmp_path / "in.y4m"), "--evaluate", "--every", "2", *common]) == 0
        printed = capsys.readouterr().out.strip()
        assert printed == repr(FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format=fmt).evaluate(planar, every=2))
        assert cli.main([str(tmp_path / "in.y4m"), str(tmp_path / "half.y4m"), "--scale", "0.5", "--factor", "1", *common]) == 0
        with y4m.Y4MReader(str(tmp_path / "half.y4m")) as r:
            assert (r.header.width, r.header.height) == (W // 2, H // 2)
            got = list(r)
        want = list(FrameInterpolator(model, 1, 1, batch_pairs=2, reference_quirks=False, pixel_format=fmt, scale=0.5).run(planar))
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    else:
        assert cli.main([str(tmp_path / "in.y4m"), "--evaluate", *common]) != 0          # 16-bit frames are not scored
        assert "evaluate" in capsys.readouterr().err


def test_cli_refuses_422(tmp_path, capsys):
    (tmp_path / "bad.y4m").write_bytes(b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C422\nFRAME\n" + bytes(16))
    assert cli.main([str(tmp_path / "bad.y4m"), str(tmp_path / "out.y4m"), "--synthetic-weights", "0"]) != 0
    assert "C422" in capsys.readouterr().err
