"""High-bit-depth frames on the GPU: emavfi_preprocess_p010 / emavfi_postprocess_p010 and the harness's pixel_format="p010" / "p012" / "p016"
against the numpy restatement of the definition (tests/p010_oracle.py).  Every comparison is equality: fp32 results bit for bit, planes
word for word, padding byte for byte."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, lib, synth
import nv12_oracle
import p010_oracle as oracle

pytestmark = pytest.mark.gpu

# tests/test_gpu_nv12.py's LAYOUTS with the block width halved: 1x1, odd, one fast block, fast blocks, fast blocks + remainder, odd + remainder
SHAPES = [(1, 1), (3, 5), (2, 8), (4, 24), (6, 26), (7, 9)]
LAYOUTS = ["dense", "pad16", "odd", "bstride", "offset2", "b1stride"]
B1STRIDE = ((5, 36), 1)   # "b1stride" is this one case: four 8-column blocks, a 4-column remainder and an odd bottom row of one frame
COLOURS = [(d, s, f, o) for d in oracle.DEPTHS for (s, f) in oracle.STANDARDS for o in ("bgr", "rgb")]
FILL = 0xA5
GUARD = 64          # floats in front of and behind an fp32 result
SENTINEL = -12345.0


def up(v, m):
    return (v + m - 1) // m * m


def geometry(layout, H, W):
    """(pointer offset, pitch, batch stride) in BYTES for the Y plane [H, W] and for the UV plane [ceil(H/2), 2 ceil(W/2)] of 16-bit words"""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    out = []
    for rows, rowbytes, align in ((H, 2 * W, 2), (H2, 4 * W2, 4)):
        if layout == "dense":
            off, pitch = 0, rowbytes
        elif layout == "pad16":
            off, pitch = 0, up(rowbytes, 16) + 16
        elif layout == "odd":                    # larger than the row and no multiple of 16: scalar path, rows at every legal misalignment
            off, pitch = 0, rowbytes + 3 * align
        elif layout in ("bstride", "b1stride"):
            off, pitch = 0, up(rowbytes, 16)
        else:                                    # "offset2": the Y plane 2 bytes, the UV plane 4 bytes past a 16-byte boundary, aligned pitch
            off, pitch = align, up(rowbytes, 16)
        # "b1stride": everything 16-byte aligned but the batch stride, legal and never used at B == 1 - the 16-byte accesses must be taken
        bstride = pitch * rows + (pitch * 3 + 32 if layout == "bstride" else 4 if layout == "b1stride" else 0)
        out.append((off, pitch, bstride))
    return out


def strided(shape, off, pitch, bstride):
    """a raw byte buffer full of FILL and a [B, rows, ...] view of 16-bit words into it"""
    B = shape[0]
    raw = torch.full((up(off + B * bstride + pitch + 64, 16),), FILL, dtype=torch.uint8, device="cuda")
    strides = (bstride // 2, pitch // 2, 1) if len(shape) == 3 else (bstride // 2, pitch // 2, 2, 1)
    return raw, raw.view(torch.int16).as_strided(shape, strides, storage_offset=off // 2)


def planes(layout, B, H, W):
    (yo, yp, yb), (uo, upitch, ub) = geometry(layout, H, W)
    yraw, y = strided((B, H, W), yo, yp, yb)
    uvraw, uv = strided((B, (H + 1) // 2, (W + 1) // 2, 2), uo, upitch, ub)
    return yraw, y, uvraw, uv


def cases(layout, batches):
    return [B1STRIDE] if layout == "b1stride" else itertools.product(SHAPES, batches)


def entry_args(y, uv, colour):
    """the C entries' plane and colour arguments with the views' own batch strides: lib's wrappers pass the dense value at B == 1"""
    depth, standard, full, order = colour
    return ((y.data_ptr(), 2 * y.stride(1), 2 * y.stride(0), uv.data_ptr(), 2 * uv.stride(1), 2 * uv.stride(0)),
            (depth, lib.yuv_standard_code_deep(standard, full), lib._order_code(order)))


def to_t(a):
    """numpy uint16 -> torch int16 with the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16))


def to_np(t):
    """a tensor of 16-bit words -> numpy uint16"""
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def guarded_out(B, H, W):
    flat = torch.full((B * 3 * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return flat, flat[GUARD:GUARD + B * 3 * H * W].view(B, 3, H, W)


def check_decode(ynp, uvnp, layout, colour, want=None):
    depth, standard, full, order = colour
    B, H, W = ynp.shape
    _, y, _, uv = planes(layout, B, H, W)
    y.copy_(to_t(ynp))
    uv.copy_(to_t(uvnp))
    flat, out = guarded_out(B, H, W)
    if layout == "b1stride":
        pl, codes = entry_args(y, uv, colour)
        assert 2 * y.stride(0) % 16 == 4 and lib.load().emavfi_preprocess_p010(*pl, out.data_ptr(), B, H, W, *codes, *lib._stats(oracle.MEAN, oracle.STD, 3),
                                                                               lib._stream()) == 0, lib.last_error()
        got = out
    else:
        got = lib.preprocess_p010(y, uv, depth, standard, full, order, out=out)
    if want is None:
        want = oracle.preprocess(ynp, uvnp, depth, standard, full, order)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (layout, colour, (B, H, W))
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "floats beyond [B,3,H,W] were written"
    return got


def rand_words(rng, shape, depth, junk=False):
    w = rng.integers(0, 2 ** depth, shape, dtype=np.int64) << (16 - depth)
    if junk and depth < 16:
        w |= rng.integers(0, 2 ** (16 - depth), shape, dtype=np.int64)
    return w.astype(np.uint16)


@pytest.mark.parametrize("code", range(6))
def test_decode_depth10_every_chroma_pair_at_the_luma_edges(code):
    """2048 x 2048: all 1024 x 1024 (U, V) pairs, one per 2x2 block; luma cycles through 0, yoff - 1, yoff, yoff + Yr, P so that a pair's four
    pixels in the two frames of the batch see all five"""
    standard, full = oracle.STANDARDS[code]
    order = "rgb" if code & 1 else "bgr"
    P, _, yoff, Yr, _ = oracle.constants(10, full)
    edges = np.array([0, max(yoff - 1, 0), yoff, yoff + Yr, P], np.int64)
    uv = oracle.words(np.stack(np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij"), axis=-1), 10)
    idx = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)     # a block's pixels: base + {0, 1, 3, 4} mod 5, the second frame adds + 2
    y = oracle.words(np.stack([edges[idx % 5], edges[(idx + 2) % 5]]), 10)
    check_decode(y, np.stack([uv, uv]), "dense", (10, standard, full, order))


@pytest.mark.parametrize("depth", [12, 16])
def test_decode_deeper_samples_and_extremes(depth):
    rng = np.random.default_rng(depth)
    P = 2 ** depth - 1
    for n, (standard, full) in enumerate(oracle.STANDARDS):
        y, uv = rand_words(rng, (1, 128, 192), depth), rand_words(rng, (1, 64, 96, 2), depth)
        ext = oracle.words(np.array([0, 1, P // 2, P // 2 + 1, P - 1, P]), depth)
        y[0, :6, :6] = ext[:, None]                                       # every luma extreme ...
        uv[0, :3, :3] = ext[rng.integers(0, 6, (3, 3, 2))]
        uv[0, 0, 0], uv[0, 0, 1], uv[0, 0, 2], uv[0, 1, 0] = (ext[0], ext[0]), (ext[5], ext[5]), (ext[0], ext[5]), (ext[5], ext[0])   # ... under the chroma corners
        check_decode(y, uv, "dense", (depth, standard, full, "rgb" if n & 1 else "bgr"))


def test_low_bits_are_ignored_on_read():
    rng = np.random.default_rng(77)
    for depth in (10, 12):
        clean_y, clean_uv = rand_words(rng, (2, 16, 24), depth), rand_words(rng, (2, 8, 12, 2), depth)
        low = (1 << (16 - depth)) - 1
        dirty_y = clean_y | rng.integers(0, low + 1, clean_y.shape).astype(np.uint16)
        dirty_uv = clean_uv | rng.integers(0, low + 1, clean_uv.shape).astype(np.uint16)
        assert (dirty_y != clean_y).any() and (dirty_uv != clean_uv).any()
        want = oracle.preprocess(clean_y, clean_uv, depth, "bt709", False, "bgr")
        for layout in ("dense", "offset2"):                               # the fast and the scalar form
            check_decode(dirty_y, dirty_uv, layout, (depth, "bt709", False, "bgr"), want=want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_shapes_pitches_and_paths(layout):
    rng = np.random.default_rng(11)
    for n, ((H, W), B) in enumerate(cases(layout, (1, 2))):
        colour = COLOURS[(7 * n + LAYOUTS.index(layout)) % len(COLOURS)]
        y = rand_words(rng, (B, H, W), colour[0], junk=True)
        uv = rand_words(rng, (B, (H + 1) // 2, (W + 1) // 2, 2), colour[0], junk=True)
        check_decode(y, uv, layout, colour)


def encode_input(B, H, W, depth, denorm, seed):
    """fp32 [B,3,H,W] whose quantised integers are random, with constructed 2x2 blocks in front, the exact k / P boundaries of the first row
    with their fp32 neighbours, and NaN / Inf / out-of-range values sprinkled in"""
    rng = np.random.default_rng(seed)
    P = 2 ** depth - 1
    q = rng.integers(0, P + 1, (B, H, W, 3), dtype=np.int64)
    blocks = [np.array(b, np.int64) for b in (
        [[[1] * 3, [1] * 3], [[0] * 3, [0] * 3]],                              # sum 2 = 4 * 0 + 2: the .5 tie of the mean
        [[[P] * 3, [P] * 3], [[P] * 3, [P - 2] * 3]],                          # sum 4 P - 2
        [[[0] * 3] * 2] * 2, [[[P] * 3] * 2] * 2,                              # all-0, all-P
        [[[P, 0, 0]] * 2] * 2, [[[0, P, 0]] * 2] * 2, [[[0, 0, P]] * 2] * 2,   # primaries: U / V extremes, the clip at P
        [[[P, P, 0]] * 2] * 2, [[[0, P, P]] * 2] * 2, [[[P, 0, P]] * 2] * 2)]
    k = 0
    for b in range(B):
        for y0 in range(0, H - 1, 2):
            for x0 in range(0, W - 1, 2):
                if k < len(blocks):
                    q[b, y0:y0 + 2, x0:x0 + 2] = blocks[k]
                    k += 1
    x = (q.astype(np.float64) + 0.5) / P                                       # mid-interval: the fp32 rounding cannot cross an integer
    if denorm:
        x = (x - np.array(oracle.MEAN)) / np.array(oracle.STD)
    x = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)
    if H * W >= 9 and not denorm:                                              # exact boundaries k / P and their neighbours, last row
        kk = rng.integers(0, P + 1, W)
        edge = (kk.astype(np.float64) / P).astype(np.float32)
        x[0, 0, -1], x[0, 1, -1], x[0, 2, -1] = edge, np.nextafter(edge, np.float32(-1)), np.nextafter(edge, np.float32(2))
    flat = x.reshape(-1)
    if flat.size >= 64:
        for j, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 2.0, 1.0, 0.0, -0.0)):
            flat[(flat.size // 8 * j + 3 * j) % flat.size] = v
    return x


def check_encode(xnp, layout, colour, denorm):
    depth, standard, full, order = colour
    B, _, H, W = xnp.shape
    yraw, y, uvraw, uv = planes(layout, B, H, W)
    if layout == "b1stride":
        pl, codes = entry_args(y, uv, colour)
        x = torch.from_numpy(xnp).cuda()
        assert 2 * uv.stride(0) % 16 == 4 and lib.load().emavfi_postprocess_p010(x.data_ptr(), *pl, B, H, W, *codes,
                                                                                 *lib._stats(oracle.MEAN, oracle.STD, 3, ctypes.c_double), denorm,
                                                                                 lib._stream()) == 0, lib.last_error()
    else:
        lib.postprocess_p010(torch.from_numpy(xnp).cuda(), depth, standard, full, order, denormalize=bool(denorm), out=(y, uv))
    ywant, uvwant = oracle.postprocess(xnp, depth, standard, full, order, denormalize=bool(denorm))
    low = np.uint16((1 << (16 - depth)) - 1)
    assert not (to_np(y) & low).any() and not (to_np(uv) & low).any(), "low bits must be written as zero"
    # expected images of the two raw buffers: the planes where they belong, FILL everywhere else (pitch padding, slack, the front offset)
    eyraw, ey, euvraw, euv = planes(layout, B, H, W)
    ey.copy_(to_t(ywant))
    euv.copy_(to_t(uvwant))
    assert torch.equal(y, ey), ("Y", layout, colour, denorm, (B, H, W))
    assert torch.equal(uv, euv), ("UV", layout, colour, denorm, (B, H, W))
    assert torch.equal(yraw, eyraw) and torch.equal(uvraw, euvraw), ("bytes outside the planes were written", layout, (B, H, W))
    return y, uv


@pytest.mark.parametrize("denorm", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_shapes_pitches_and_paths(layout, denorm):
    for n, ((H, W), B) in enumerate(cases(layout, (1, 2))):
        colour = COLOURS[(5 * n + 3 * denorm + LAYOUTS.index(layout)) % len(COLOURS)]
        check_encode(encode_input(B, H, W, colour[0], denorm, seed=100 + n), layout, colour, denorm)


@pytest.mark.parametrize("depth", oracle.DEPTHS)
def test_encode_every_colour_definition(depth):
    for n, (standard, full) in enumerate(oracle.STANDARDS):
        for denorm in (0, 1):
            check_encode(encode_input(2, 32, 48, depth, denorm, seed=7 + n), "dense", (depth, standard, full, "rgb" if (n + denorm) & 1 else "bgr"), denorm)


def test_default_outputs_numpy_and_pinned_planes():
    """out=None allocates dense planes of lib.word_dtype(); numpy uint16 planes are uploaded; the word side may be pinned host memory"""
    rng = np.random.default_rng(3)
    B, H, W = 2, 32, 48
    ynp, uvnp = rand_words(rng, (B, H, W), 10), rand_words(rng, (B, H // 2, W // 2, 2), 10)
    want = oracle.preprocess(ynp, uvnp, 10, "bt2020", False)
    got = lib.preprocess_p010(ynp, uvnp, 10, "bt2020", device="cuda")
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    yh, uvh = to_t(ynp).view(lib.word_dtype()).pin_memory(), to_t(uvnp).pin_memory()        # either 16-bit dtype is taken
    pinned = lib.preprocess_p010(yh, uvh, 10, "bt2020", device="cuda")
    assert torch.equal(pinned.view(torch.int32), got.view(torch.int32))
    ywant, uvwant = oracle.postprocess(want, 10, "bt2020", False)
    y, uv = lib.postprocess_p010(got, 10, "bt2020")
    assert y.dtype == uv.dtype == lib.word_dtype() and y.is_contiguous() and uv.is_contiguous()
    assert np.array_equal(to_np(y), ywant) and np.array_equal(to_np(uv), uvwant)
    yo, uvo = torch.zeros(B, H, W, dtype=torch.int16).pin_memory(), torch.zeros(B, H // 2, W // 2, 2, dtype=torch.int16).pin_memory()
    lib.postprocess_p010(got, 10, "bt2020", out=(yo, uvo))
    torch.cuda.synchronize()
    assert np.array_equal(yo.numpy().view(np.uint16), ywant) and np.array_equal(uvo.numpy().view(np.uint16), uvwant)
    with pytest.raises(ValueError, match="dense"):
        lib.preprocess_p010(torch.zeros(1, 4, 8, dtype=torch.int16, device="cuda")[:, :, ::2], torch.zeros(1, 2, 2, 2, dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError, match="16-bit"):
        lib.preprocess_p010(torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda"), torch.zeros(1, 2, 2, 2, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="depth"):
        lib.preprocess_p010(ynp, uvnp, 8, device="cuda")


def test_fast_path_equals_scalar_path():
    """the same frames once 16-byte aligned (16-byte accesses) and once through a view 2 / 4 bytes off (scalar accesses)"""
    rng = np.random.default_rng(17)
    B, H, W = 2, 32, 64
    for colour in (COLOURS[0], COLOURS[21], COLOURS[35]):
        depth = colour[0]
        ynp, uvnp = rand_words(rng, (B, H, W), depth, junk=True), rand_words(rng, (B, H // 2, W // 2, 2), depth, junk=True)
        want = oracle.preprocess(ynp, uvnp, *colour)
        fast = check_decode(ynp, uvnp, "pad16", colour, want=want)
        slow = check_decode(ynp, uvnp, "offset2", colour, want=want)
        assert torch.equal(fast.view(torch.int32), slow.view(torch.int32))
        for denorm in (0, 1):
            x = encode_input(B, H, W, depth, denorm, seed=23)
            yf, uvf = check_encode(x, "pad16", colour, denorm)
            ys, uvs = check_encode(x, "offset2", colour, denorm)
            assert torch.equal(yf, ys) and torch.equal(uvf, uvs)


# ---------------------------------------------------------------- the harness
H, W, NFRAMES = 24, 40, 11


def pack(y, uv):
    return np.concatenate([y, uv.reshape(uv.shape[0], -1)], axis=0)


def unpack(frame):
    h = frame.shape[0] * 2 // 3
    return frame[:h], frame[h:].reshape(h // 2, frame.shape[1] // 2, 2)


def clip_rgb():
    """the synthetic clip as [0,1] floats [NFRAMES, H, W, 3]: smooth content, so that predictions are not noise"""
    rng = np.random.default_rng(41)
    base = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy()
    return np.stack([np.clip(np.roll(base, 2 * i, axis=2).transpose(1, 2, 0) * 0.2 + 0.45 + rng.normal(0, 0.02, (H, W, 3)), 0, 1)
                     for i in range(NFRAMES)])


def build_case(fmt, standard, full, recursive_factor=None):
    """frames, the model, and per frame / per pair everything the harness's output is made of, computed outside the harness with the
    stand-alone entries and the model's forward"""
    depth = lib.DEPTHS[fmt]
    P = 2 ** depth - 1
    frames = [pack(*oracle.encode((img * P).astype(np.int64), depth, standard, full)) for img in clip_rgb()]
    model = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    ys, uvs = np.stack([unpack(f)[0] for f in frames]), np.stack([unpack(f)[1] for f in frames])
    x = lib.preprocess_p010(ys, uvs, depth, standard, full, device="cuda")

    def enc(t, denorm):
        y, uv = lib.postprocess_p010(t, depth, standard, full, denormalize=denorm)
        return [pack(a, b) for a, b in zip(to_np(y), to_np(uv))]

    mean, std = (torch.tensor(v, device="cuda").view(1, 3, 1, 1) for v in (lib.IMAGENET_MEAN, lib.IMAGENET_STD))

    def mids(a, b, levels):
        m = model(a, b)
        if levels == 1:
            return [m]
        mn = (m - mean) / std
        return mids(a, mn, levels - 1) + [m] + mids(mn, b, levels - 1)

    with torch.no_grad():
        if recursive_factor:
            levels = (recursive_factor + 1).bit_length() - 1
            out = [torch.cat(mids(x[i:i + 1], x[i + 1:i + 2], levels)) for i in range(NFRAMES - 1)]     # [pair][j]
        else:
            out = [model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)]
    pred = {q: [enc(o, q) for o in out] for q in (False, True)}
    return {"fmt": fmt, "yuv": dict(yuv_standard=standard, yuv_full_range=full), "frames": frames, "model": model, "pred": pred,
            "roundtrip": enc(x, True), "recursive": bool(recursive_factor)}


@pytest.fixture(scope="module")
def p010_case():
    return build_case("p010", "bt709", False)


def expected_stream(case, factor, quirks):
    want = []
    for item in FrameInterpolator.emission_plan(NFRAMES, factor, 1, reference_quirks=quirks):
        if item[0] == "pred":
            assert item[2] == item[1] + 1
            want.append(case["pred"][quirks][item[1]][item[3] if case["recursive"] else 0])
        elif item[0] == "src":
            want.append(case["roundtrip"][item[1]] if quirks else case["frames"][item[1]])
        else:
            assert item[2] is False
            want.append(case["frames"][item[1]])
    return want


def same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint16 and g.shape == (H * 3 // 2, W) and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("factor,batch", [(1, 2), (1, 8), (3, 2), (3, 8)])
def test_harness_p010(p010_case, factor, batch):
    case = p010_case
    frames, model, kw = case["frames"], case["model"], dict(pixel_format="p010", **case["yuv"])
    for quirks in (False, True):
        want = expected_stream(case, factor, quirks)
        fi = FrameInterpolator(model, factor, 1, batch_pairs=batch, reference_quirks=quirks, **kw)
        got = list(fi.run(frames))
        assert len(got) == fi.count_outputs(NFRAMES) and same(got, want), (factor, batch, quirks)
        views = [f.copy() for f in FrameInterpolator(model, factor, 1, batch_pairs=batch, reference_quirks=quirks, copy_out=False, **kw).run(frames)]
        assert same(views, want), (factor, batch, quirks, "copy_out=False")
    zc = list(FrameInterpolator(model, factor, 1, batch_pairs=batch, zero_copy=True, **kw).run(frames))
    assert same(zc, expected_stream(case, factor, True)), (factor, batch, "zero_copy")


def test_harness_p016_bt2020_full_range_recursive():
    case = build_case("p016", "bt2020", True, recursive_factor=3)
    for quirks in (False, True):
        fi = FrameInterpolator(case["model"], 3, 1, batch_pairs=2, reference_quirks=quirks, mode="recursive", pixel_format="p016", **case["yuv"])
        assert same(list(fi.run(case["frames"])), expected_stream(case, 3, quirks)), quirks


def test_harness_refuses_bad_frames_and_the_out_of_scope_combinations(p010_case):
    model, frames = p010_case["model"], p010_case["frames"]
    fi = FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="p010")
    with pytest.raises(ValueError, match="uint16"):
        list(fi.run([f.astype(np.uint8) for f in frames[:2]]))
    with pytest.raises(ValueError, match="uint16"):
        list(fi.run([np.zeros((H, W, 3), np.uint16)] * 2))
    with pytest.raises(ValueError, match="even H and W"):
        list(fi.run([np.zeros((35, 40), np.uint16)] * 2))
    with pytest.raises(ValueError, match="even H and W"):
        list(fi.run([np.zeros((36, 39), np.uint16)] * 2))
    with pytest.raises(ValueError, match="evaluate"):
        fi.evaluate(frames)
    with pytest.raises(ValueError, match="scale / size"):
        FrameInterpolator(model, pixel_format="p012", scale=0.5)
    with pytest.raises(ValueError, match="scene_threshold"):
        FrameInterpolator(model, pixel_format="p016", scene_threshold=0.1)
    with pytest.raises(ValueError, match="bt601"):
        FrameInterpolator(model, pixel_format="nv12", yuv_standard="bt2020")


def test_harness_bgr24_and_nv12_are_unchanged(p010_case):
    """the 8-bit streams of the same clip: exactly what the stand-alone 8-bit entries and the forward give, as before the 16-bit formats existed"""
    model = p010_case["model"]
    bgr = [(img * 255).astype(np.uint8) for img in clip_rgb()]
    nv12 = [pack(*nv12_oracle.encode(f)) for f in bgr]
    x = lib.preprocess_u8(torch.from_numpy(np.stack(bgr)).cuda())
    with torch.no_grad():
        out = torch.cat([model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)])
    pred, src = lib.postprocess_u8(out).cpu().numpy(), lib.postprocess_u8(x).cpu().numpy()
    got = list(FrameInterpolator(model, 1, 1, batch_pairs=2).run(bgr))
    assert len(got) == 2 * (NFRAMES - 1) + 1 and np.array_equal(got[-1], bgr[-1])
    for i in range(NFRAMES - 1):
        assert got[2 * i].dtype == np.uint8 and np.array_equal(got[2 * i], pred[i]) and np.array_equal(got[2 * i + 1], src[i]), i
    ys = torch.from_numpy(np.stack([unpack(f)[0] for f in nv12])).cuda()
    uvs = torch.from_numpy(np.stack([unpack(f)[1] for f in nv12])).cuda()
    x = lib.preprocess_nv12(ys, uvs)
    with torch.no_grad():
        out = torch.cat([model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)])
    enc = lambda t: [pack(a, b) for a, b in zip(*(p.cpu().numpy() for p in lib.postprocess_nv12(t)))]
    pred, src = enc(out), enc(x)
    got = list(FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="nv12").run(nv12))
    assert len(got) == 2 * (NFRAMES - 1) + 1 and np.array_equal(got[-1], nv12[-1])
    for i in range(NFRAMES - 1):
        assert got[2 * i].dtype == np.uint8 and np.array_equal(got[2 * i], pred[i]) and np.array_equal(got[2 * i + 1], src[i]), i
