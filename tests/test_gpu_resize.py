"""Frames resized on the GPU: emavfi_resize_u8, emavfi_preprocess_u8_resized, emavfi_preprocess_nv12_resized and the harness's scale / size
against the numpy restatement of the resize definition (tests/resize_oracle.py) composed with the kernels they are defined by.  Every
comparison is bit-exact."""
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, lib, synth
import nv12_oracle
import resize_oracle as oracle

pytestmark = pytest.mark.gpu

# (Hs, Ws) -> (Hd, Wd): odd source / non-integer ratio / remainders on both axes; up-scale; exact 2:1 on the wide path; identity; one-row and
# one-column sources (the i1 clamp); a one-pixel destination; tile edges crossed on both axes at any tile of 128 or less; weights near 0 and 2048
SHAPES = [((23, 37), (11, 18)), ((8, 8), (11, 13)), ((32, 48), (16, 24)), ((16, 16), (16, 16)), ((1, 9), (3, 4)), ((9, 1), (4, 3)),
          ((5, 7), (1, 1)), ((150, 200), (77, 133)), ((37, 53), (36, 52))]
IDS = ["%dx%d-%dx%d" % (*s, *d) for s, d in SHAPES]
LAYOUTS = ["dense", "pad16", "odd"]
SRC_FILL, DST_FILL = 0xA5, 0x5A
GUARD, SENTINEL = 64, -12345.0


def up(v, m):
    return (v + m - 1) // m * m


def strided(B, rows, rowbytes, layout, fill, inner):
    """a raw byte buffer full of `fill` and a [B, rows, *inner] view into it: `dense` rows, rows padded to a multiple of 16 plus 16, or an odd
    pitch; for B > 1 the batch stride is larger than the plane in every layout"""
    pitch = {"dense": rowbytes, "pad16": up(rowbytes, 16) + 16, "odd": rowbytes + 5}[layout]
    bstride = pitch * rows + ({"dense": 32, "pad16": 48, "odd": 7}[layout] if B > 1 else 0)
    raw = torch.full((B * bstride + pitch + 64,), fill, dtype=torch.uint8, device="cuda")
    st = [bstride, pitch] + [int(np.prod(inner[k + 1:])) for k in range(len(inner))]
    return raw, raw.as_strided((B, rows, *inner), st)


def image(B, H, W, C, layout, fill, data=None):
    raw, view = strided(B, H, W * C, layout, fill, (W, C))
    if data is not None:
        view.copy_(torch.from_numpy(data))
    return raw, view


def guarded_out(B, C, H, W):
    flat = torch.full((B * C * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return flat, flat[GUARD:GUARD + B * C * H * W].view(B, C, H, W)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_resize_u8_is_the_oracle_byte_for_byte(shape):
    (Hs, Ws), (Hd, Wd) = shape
    rng = np.random.default_rng(Hs * 131 + Ws)
    for C, B, layout in itertools.product((1, 2, 3, 4), (1, 2), LAYOUTS):
        src = rng.integers(0, 256, (B, Hs, Ws, C), dtype=np.uint8)
        want = oracle.resize(src, (Hd, Wd))
        _, s = image(B, Hs, Ws, C, layout, SRC_FILL, src)
        draw, d = image(B, Hd, Wd, C, layout, DST_FILL)
        got = lib.resize_u8(s, (Hd, Wd), out=d)
        assert got.data_ptr() == d.data_ptr()
        eraw, e = image(B, Hd, Wd, C, layout, DST_FILL, want)
        assert torch.equal(d, e), (shape, C, B, layout)                           # source padding did not leak in
        assert torch.equal(draw, eraw), ("destination padding was written", shape, C, B, layout)
    dense = lib.resize_u8(torch.from_numpy(src).cuda(), (Hd, Wd))                 # out=None: a dense result
    assert dense.is_contiguous() and np.array_equal(dense.cpu().numpy(), want)


def test_resize_u8_properties_on_the_device():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 46, 74, 3), dtype=np.uint8)
    x = torch.from_numpy(img).cuda()
    assert torch.equal(lib.resize_u8(x, (46, 74)), x)
    p = img.astype(np.int64)
    half = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(lib.resize_u8(x, (23, 37)).cpu().numpy(), half)
    assert (lib.resize_u8(torch.full((1, 37, 53, 2), 201, dtype=torch.uint8, device="cuda"), (50, 11)) == 201).all()
    got = lib.resize_u8(x, (31, 100)).cpu().numpy().astype(np.float64)
    assert np.abs(got - oracle.real_bilinear(img, (31, 100))).max() <= 0.6245 + 1e-6


def test_resize_u8_beyond_the_staged_span_and_from_pinned_memory():
    """a 12:1 reduction (the tile's source span does not fit LDS: the taps come from global memory) and a pinned host source"""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (1, 400, 1000, 3), dtype=np.uint8)
    assert np.array_equal(lib.resize_u8(torch.from_numpy(src).cuda(), (33, 83)).cpu().numpy(), oracle.resize(src, (33, 83)))
    small = rng.integers(0, 256, (2, 23, 37, 3), dtype=np.uint8)
    got = lib.resize_u8(torch.from_numpy(small).pin_memory(), (11, 18), device="cuda")
    assert np.array_equal(got.cpu().numpy(), oracle.resize(small, (11, 18)))
    x = lib.preprocess_u8(torch.from_numpy(src).cuda(), size=(33, 83))
    assert torch.equal(bits(x), bits(lib.preprocess_u8(torch.from_numpy(oracle.resize(src, (33, 83))).cuda())))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_preprocess_u8_resized_is_preprocess_of_the_resized_bytes(shape):
    (Hs, Ws), (Hd, Wd) = shape
    rng = np.random.default_rng(Hs * 17 + Wd)
    stats = {1: ((0.4,), (0.3,)), 2: ((0.4, 0.5), (0.3, 0.2)), 3: (lib.IMAGENET_MEAN, lib.IMAGENET_STD), 4: ((0.4, 0.5, 0.6, 0.1), (0.3, 0.2, 0.25, 0.9))}
    for C, B in itertools.product((1, 2, 3, 4), (1, 2)):
        mean, std = stats[C]
        src = torch.from_numpy(rng.integers(0, 256, (B, Hs, Ws, C), dtype=np.uint8)).cuda()
        rs = lib.resize_u8(src, (Hd, Wd))
        assert np.array_equal(rs.cpu().numpy(), oracle.resize(src.cpu().numpy(), (Hd, Wd)))
        want = lib.preprocess_u8(rs, mean, std)
        flat, out = guarded_out(B, C, Hd, Wd)
        got = lib.preprocess_u8(src, mean, std, out=out, size=(Hd, Wd))
        assert got.data_ptr() == out.data_ptr() and torch.equal(bits(got), bits(want)), (shape, C, B)
        assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "bytes beyond [B,C,Hd,Wd] were written"
        both = torch.full((B, Hd, Wd, C), DST_FILL, dtype=torch.uint8, device="cuda")
        got2 = lib.preprocess_u8(src, mean, std, size=(Hd, Wd), resized_out=both)
        assert torch.equal(both, rs) and torch.equal(bits(got2), bits(want)), (shape, C, B, "resized_out")


NV12_SHAPES = [((23, 37), (11, 18)), ((8, 8), (11, 13)), ((32, 48), (16, 24)), ((16, 16), (16, 16)), ((1, 9), (3, 4)), ((9, 1), (4, 3)),
               ((5, 7), (1, 1)), ((150, 200), (77, 133)), ((37, 53), (36, 52)), ((150, 200), (76, 132)), ((45, 67), (90, 131))]
COLOURS = [(s, f, o) for (s, f) in nv12_oracle.STANDARDS for o in ("bgr", "rgb")]


def nv12_planes(B, H, W, layout, fill, y=None, uv=None):
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    yraw, yv = strided(B, H, W, layout, fill, (W,))
    uvraw, uvv = strided(B, H2, 2 * W2, layout if layout != "odd" else "pad16", fill, (W2, 2))
    if layout == "odd":   # an odd pitch would break the 2-byte alignment of the UV rows: two bytes past a 16-byte boundary instead
        uvraw = torch.full((uvraw.numel() + 2,), fill, dtype=torch.uint8, device="cuda")
        uvv = uvraw.as_strided(uvv.shape, uvv.stride(), storage_offset=2)
    if y is not None:
        yv.copy_(torch.from_numpy(y))
        uvv.copy_(torch.from_numpy(uv))
    return yraw, yv, uvraw, uvv


def check_nv12(ynp, uvnp, size, layout, colour, with_out):
    standard, full, order = colour
    B, Hs, Ws = ynp.shape
    Hd, Wd = size
    _, y, _, uv = nv12_planes(B, Hs, Ws, layout, SRC_FILL, ynp, uvnp)
    # the definition: preprocess_nv12 of the planes resize_u8 produces (Y as 1 channel, UV as 2 channels)
    ry = lib.resize_u8(y.unsqueeze(-1), (Hd, Wd)).squeeze(-1)
    ruv = lib.resize_u8(uv, ((Hd + 1) // 2, (Wd + 1) // 2))
    wy, wuv = oracle.resize_nv12(ynp, uvnp, (Hd, Wd))
    assert np.array_equal(ry.cpu().numpy(), wy) and np.array_equal(ruv.cpu().numpy(), wuv)
    want = lib.preprocess_nv12(ry, ruv, standard, full, order)
    flat, out = guarded_out(B, 3, Hd, Wd)
    if with_out:
        yraw, yo, uvraw, uvo = nv12_planes(B, Hd, Wd, layout, DST_FILL)
        got = lib.preprocess_nv12(y, uv, standard, full, order, out=out, size=(Hd, Wd), resized_out=(yo, uvo))
        eyraw, _, euvraw, _ = nv12_planes(B, Hd, Wd, layout, DST_FILL, wy, wuv)
        assert torch.equal(yraw, eyraw) and torch.equal(uvraw, euvraw), ("resized planes / their padding", ynp.shape, size, layout)
    else:
        got = lib.preprocess_nv12(y, uv, standard, full, order, out=out, size=(Hd, Wd))
    assert torch.equal(bits(got), bits(want)), (ynp.shape, size, layout, colour, with_out)
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "bytes beyond [B,3,Hd,Wd] were written"
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
def test_preprocess_nv12_resized_is_preprocess_of_the_resized_planes(layout):
    rng = np.random.default_rng(29)
    for n, (((Hs, Ws), size), B) in enumerate(itertools.product(NV12_SHAPES, (1, 2))):
        y = rng.integers(0, 256, (B, Hs, Ws), dtype=np.uint8)
        uv = rng.integers(0, 256, (B, (Hs + 1) // 2, (Ws + 1) // 2, 2), dtype=np.uint8)
        a = check_nv12(y, uv, size, layout, COLOURS[n % len(COLOURS)], with_out=True)
        b = check_nv12(y, uv, size, layout, COLOURS[n % len(COLOURS)], with_out=False)
        assert torch.equal(bits(a), bits(b))          # NULL for the optional planes does not change the fp32


@pytest.mark.parametrize("standard,full,order", COLOURS)
def test_preprocess_nv12_resized_every_colour_definition(standard, full, order):
    rng = np.random.default_rng(31)
    y = rng.integers(0, 256, (2, 45, 67), dtype=np.uint8)
    uv = rng.integers(0, 256, (2, 23, 34, 2), dtype=np.uint8)
    check_nv12(y, uv, (21, 35), "dense", (standard, full, order), with_out=True)
    # only one optional plane
    yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    yo = torch.zeros(2, 21, 35, dtype=torch.uint8, device="cuda")
    uvo = torch.zeros(2, 11, 18, 2, dtype=torch.uint8, device="cuda")
    a = lib.preprocess_nv12(yd, uvd, standard, full, order, size=(21, 35), resized_out=(yo, None))
    b = lib.preprocess_nv12(yd, uvd, standard, full, order, size=(21, 35), resized_out=(None, uvo))
    wy, wuv = oracle.resize_nv12(y, uv, (21, 35))
    assert torch.equal(bits(a), bits(b)) and np.array_equal(yo.cpu().numpy(), wy) and np.array_equal(uvo.cpu().numpy(), wuv)


def test_wide_path_equals_scalar_path():
    """the same image once through 16-byte aligned buffers (16-byte loads and stores, dword byte stores) and once through views that start
    one byte (u8) / two bytes (NV12) later (byte loads, scalar stores)"""
    rng = np.random.default_rng(37)
    B, Hs, Ws, Hd, Wd = 2, 96, 160, 48, 80
    for C in (1, 2, 3, 4):
        src = rng.integers(0, 256, (B, Hs, Ws, C), dtype=np.uint8)
        want = torch.from_numpy(oracle.resize(src, (Hd, Wd))).cuda()
        res = []
        for off in (0, 1):
            sraw = torch.full((B * Hs * Ws * C + 16,), SRC_FILL, dtype=torch.uint8, device="cuda")
            s = sraw[off:off + B * Hs * Ws * C].view(B, Hs, Ws, C)
            s.copy_(torch.from_numpy(src))
            draw = torch.full((B * Hd * Wd * C + 16,), DST_FILL, dtype=torch.uint8, device="cuda")
            d = draw[off:off + B * Hd * Wd * C].view(B, Hd, Wd, C)
            assert s.data_ptr() % 16 == off and d.data_ptr() % 16 == off
            lib.resize_u8(s, (Hd, Wd), out=d)
            assert torch.equal(d, want), (C, off)
            assert (draw[:off] == DST_FILL).all() and (draw[off + d.numel():] == DST_FILL).all()
            mean, std = (0.4, 0.5, 0.6, 0.1)[:C], (0.3, 0.2, 0.25, 0.9)[:C]
            rs = torch.empty(B * Hd * Wd * C + 16, dtype=torch.uint8, device="cuda")[off:off + B * Hd * Wd * C].view(B, Hd, Wd, C)
            f = lib.preprocess_u8(s, mean, std, size=(Hd, Wd), resized_out=rs)
            assert torch.equal(rs, want)
            res.append(f)
        assert torch.equal(bits(res[0]), bits(res[1])), C
    y = rng.integers(0, 256, (B, Hs, Ws), dtype=np.uint8)
    uv = rng.integers(0, 256, (B, Hs // 2, Ws // 2, 2), dtype=np.uint8)
    fast = check_nv12(y, uv, (Hd, Wd), "pad16", COLOURS[0], with_out=True)
    slow = check_nv12(y, uv, (Hd, Wd), "odd", COLOURS[0], with_out=True)
    assert torch.equal(bits(fast), bits(slow))


# ---------------------------------------------------------------- the harness
NFRAMES = 5


def pack(y, uv):
    return np.concatenate([y, uv.reshape(uv.shape[0], -1)], axis=0)


def unpack(frame):
    h = frame.shape[0] * 2 // 3
    return frame[:h], frame[h:].reshape(h // 2, frame.shape[1] // 2, 2)


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    return m


def source_frames(H, W, fmt):
    rng = np.random.default_rng(H * 7 + W)
    base = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy()
    frames = []
    for i in range(NFRAMES):
        img = np.clip(np.roll(base, 2 * i, axis=2).transpose(1, 2, 0) * 0.2 + 0.45 + rng.normal(0, 0.02, (H, W, 3)), 0, 1)
        u8 = (img * 255).astype(np.uint8)
        frames.append(pack(*nv12_oracle.encode(u8)) if fmt == "nv12" else u8)
    return frames


def oracle_resized(frame, size, fmt):
    if fmt == "nv12":
        return pack(*oracle.resize_nv12(*unpack(frame), size))
    return oracle.resize(frame, size)


@pytest.mark.parametrize("src,kw,size,fmt", [((48, 80), dict(scale=0.5), (24, 40), "bgr24"), ((46, 74), dict(size=(23, 37)), (23, 37), "bgr24"),
                                             ((48, 80), dict(scale=0.5), (24, 40), "nv12")], ids=["bgr24-scale", "bgr24-size-odd", "nv12-scale"])
def test_harness_resizes_like_the_oracle(model, src, kw, size, fmt):
    frames = source_frames(*src, fmt)
    small = [oracle_resized(f, size, fmt) for f in frames]
    for factor, interval, quirks in itertools.product((1, 3), (1, 2), (True, False)):
        want = list(FrameInterpolator(model, factor, interval, batch_pairs=2, reference_quirks=quirks, pixel_format=fmt).run(small))
        fi = FrameInterpolator(model, factor, interval, batch_pairs=2, reference_quirks=quirks, pixel_format=fmt, **kw)
        got = list(fi.run(frames))
        assert len(got) == len(want) == fi.count_outputs(NFRAMES) > 0
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.shape == w.shape == small[0].shape
            assert np.array_equal(g, w), (fmt, kw, factor, interval, quirks, k)
    zc = list(FrameInterpolator(model, 1, 1, batch_pairs=4, pixel_format=fmt, zero_copy=True, reference_quirks=False, **kw).run(frames))
    want = list(FrameInterpolator(model, 1, 1, batch_pairs=4, pixel_format=fmt, reference_quirks=False).run(small))
    assert len(zc) == len(want) and all(np.array_equal(g, w) for g, w in zip(zc, want)), "zero_copy"


def test_harness_without_scale_or_size_is_unchanged(model):
    """the default path: exactly postprocess_u8(model(preprocess_u8(...))) on the frames as they are, as before the resize existed"""
    frames = source_frames(48, 80, "bgr24")
    x = lib.preprocess_u8(torch.from_numpy(np.stack(frames)).cuda())
    with torch.no_grad():
        out = torch.cat([model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)])
    pred, src = lib.postprocess_u8(out).cpu().numpy(), lib.postprocess_u8(x).cpu().numpy()
    got = list(FrameInterpolator(model, 1, 1, batch_pairs=2).run(frames))
    same = list(FrameInterpolator(model, 1, 1, batch_pairs=2, scale=None, size=None).run(frames))
    assert len(got) == len(same) == 2 * (NFRAMES - 1) + 1 and all(np.array_equal(a, b) for a, b in zip(got, same))
    for i in range(NFRAMES - 1):
        assert np.array_equal(got[2 * i], pred[i]) and np.array_equal(got[2 * i + 1], src[i]), i
    assert np.array_equal(got[-1], frames[-1])
    raw = list(FrameInterpolator(model, 1, 1, batch_pairs=2, reference_quirks=False).run(frames))
    assert all(raw[2 * i + 1] is frames[i] or np.array_equal(raw[2 * i + 1], frames[i]) for i in range(NFRAMES - 1))
    with pytest.raises(ValueError, match="even destination"):
        list(FrameInterpolator(model, pixel_format="nv12", scale=0.5).run(source_frames(46, 80, "nv12")))    # 23 x 40
