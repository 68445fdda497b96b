"""NV12 frames on the GPU: emavfi_preprocess_nv12 / emavfi_postprocess_nv12 and the harness's pixel_format="nv12" against the numpy
restatement of the colour definition (tests/nv12_oracle.py) composed with the u8 kernels they are defined by.  Every comparison is
bit-exact."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, lib, synth
import nv12_oracle as oracle

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (1, 1), (3, 5), (6, 10), (23, 37), (24, 40), (32, 30), (32, 32), (32, 34), (46, 66), (45, 67)]
LAYOUTS = ["dense", "pad16", "odd", "bstride", "offset2", "b1stride"]
B1STRIDE = ((5, 36), 1)   # "b1stride" is this one case: two 16-column blocks, a 4-column remainder and an odd bottom row of one frame
COLOURS = [(s, f, o) for (s, f) in oracle.STANDARDS for o in ("bgr", "rgb")]
FILL = 0xFF
GUARD = 64          # floats in front of and behind an fp32 result
SENTINEL = -12345.0


def up(v, m):
    return (v + m - 1) // m * m


def geometry(layout, H, W):
    """(pointer offset, pitch, batch stride) in bytes for the Y plane [H, W] and for the UV plane [ceil(H/2), 2 ceil(W/2)]"""
    H2, W2b = (H + 1) // 2, 2 * ((W + 1) // 2)
    out = []
    for rows, rowbytes in ((H, W), (H2, W2b)):
        if layout == "dense":
            off, pitch = 0, rowbytes
        elif layout == "pad16":
            off, pitch = 0, up(rowbytes, 16) + 16
        elif layout == "odd":                    # W + 3 rounded up to even: scalar path, a misaligned second row
            off, pitch = 0, up(W + 3, 2)
        elif layout in ("bstride", "b1stride"):
            off, pitch = 0, up(rowbytes, 16)
        else:                                    # "offset2": 2 bytes past a 16-byte boundary, aligned pitch
            off, pitch = 2, up(rowbytes, 16)
        # "b1stride": everything 16-byte aligned but the batch stride, legal and never used at B == 1 - the 16-byte accesses must be taken
        bstride = pitch * rows + (pitch * 3 + 32 if layout == "bstride" else 2 if layout == "b1stride" else 0)
        out.append((off, pitch, bstride))
    return out


def strided(shape, off, pitch, bstride, dev="cuda"):
    """a raw byte buffer full of FILL and a [B, rows, ...] view into it"""
    B, rows = shape[0], shape[1]
    raw = torch.full((off + B * bstride + pitch + 64,), FILL, dtype=torch.uint8, device=dev)
    strides = (bstride, pitch, 1) if len(shape) == 3 else (bstride, pitch, 2, 1)
    return raw, raw.as_strided(shape, strides, storage_offset=off)


def planes(layout, B, H, W):
    (yo, yp, yb), (uo, upitch, ub) = geometry(layout, H, W)
    yraw, y = strided((B, H, W), yo, yp, yb)
    uvraw, uv = strided((B, (H + 1) // 2, (W + 1) // 2, 2), uo, upitch, ub)
    return yraw, y, uvraw, uv


def cases(layout, batches):
    return [B1STRIDE] if layout == "b1stride" else itertools.product(SHAPES, batches)


def entry_args(y, uv, colour):
    """the C entries' plane and colour arguments with the views' own batch strides: lib's wrappers pass the dense value at B == 1"""
    standard, full, order = colour
    return (y.data_ptr(), y.stride(1), y.stride(0), uv.data_ptr(), uv.stride(1), uv.stride(0)), (lib.yuv_standard_code(standard, full), lib._order_code(order))


def guarded_out(B, H, W):
    flat = torch.full((B * 3 * H * W + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return flat, flat[GUARD:GUARD + B * 3 * H * W].view(B, 3, H, W)


def check_decode(ynp, uvnp, layout, colour):
    standard, full, order = colour
    B, H, W = ynp.shape
    _, y, _, uv = planes(layout, B, H, W)
    y.copy_(torch.from_numpy(ynp))
    uv.copy_(torch.from_numpy(uvnp))
    flat, out = guarded_out(B, H, W)
    if layout == "b1stride":
        pl, codes = entry_args(y, uv, colour)
        assert y.stride(0) % 16 == 2 and lib.load().emavfi_preprocess_nv12(*pl, out.data_ptr(), B, H, W, *codes, *lib._stats(lib.IMAGENET_MEAN, lib.IMAGENET_STD, 3),
                                                                           lib._stream()) == 0, lib.last_error()
        got = out
    else:
        got = lib.preprocess_nv12(y, uv, standard, full, order, out=out)
    want = lib.preprocess_u8(torch.from_numpy(oracle.decode(ynp, uvnp, standard, full, order)).cuda())
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (layout, colour, (B, H, W))
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "bytes beyond [B,3,H,W] were written"
    return got


@pytest.mark.parametrize("standard,full,order", COLOURS)
def test_decode_every_chroma_pair_and_the_luma_edges(standard, full, order):
    """512 x 512: all 65 536 (U, V) pairs, one per 2x2 block, under random Y and under Y cycling through the range edges - saturation on
    both sides of every channel"""
    rng = np.random.default_rng(5)
    uv = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).astype(np.uint8)
    edges = np.array([0, 1, 15, 16, 17, 128, 234, 235, 236, 254, 255], np.uint8)
    y = np.stack([rng.integers(0, 256, (512, 512), dtype=np.uint8), edges[np.arange(512 * 512) % 11].reshape(512, 512)])
    check_decode(y, np.stack([uv, uv]), "dense", (standard, full, order))
    pix = oracle.decode(y, np.stack([uv, uv]), standard, full, order)
    assert pix.min() == 0 and pix.max() == 255


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_shapes_pitches_and_paths(layout):
    rng = np.random.default_rng(11)
    for n, ((H, W), B) in enumerate(cases(layout, (1, 3))):
        y = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
        uv = rng.integers(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), dtype=np.uint8)
        check_decode(y, uv, layout, COLOURS[n % len(COLOURS)])


def encode_input(B, H, W, denorm, seed):
    """fp32 [B,3,H,W] whose u8 bytes are random, with constructed 2x2 blocks in front and NaN / Inf sprinkled in"""
    rng = np.random.default_rng(seed)
    by = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    blocks = [np.array(b, np.uint8) for b in (
        [[[1] * 3, [1] * 3], [[0] * 3, [0] * 3]],                              # sum 2 = 4 * 0 + 2: the .5 tie of the mean
        [[[255] * 3, [255] * 3], [[255] * 3, [253] * 3]],                      # sum 1018 = 4 * 254 + 2
        [[[7, 100, 200], [8, 101, 201]], [[8, 102, 201], [7, 103, 200]]],      # sums 30, 406, 802: ties in all three channels
        [[[0] * 3] * 2] * 2, [[[255] * 3] * 2] * 2,                            # all-0, all-255
        [[[255, 0, 0]] * 2] * 2, [[[0, 255, 0]] * 2] * 2, [[[0, 0, 255]] * 2] * 2,   # primaries: U / V extremes, the full-range 255 clip
        [[[255, 255, 0]] * 2] * 2, [[[0, 255, 255]] * 2] * 2, [[[255, 0, 255]] * 2] * 2)]
    k = 0
    for b in range(B):
        for y0 in range(0, H - 1, 2):
            for x0 in range(0, W - 1, 2):
                if k < 2 * len(blocks):
                    by[b, y0:y0 + 2, x0:x0 + 2] = blocks[k % len(blocks)]
                    k += 1
    x = (by.astype(np.float64) + 0.5) / 255.0
    if denorm:
        x = (x - np.array(lib.IMAGENET_MEAN)) / np.array(lib.IMAGENET_STD)
    x = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)
    flat = x.reshape(-1)
    for j, v in enumerate((np.nan, np.inf, -np.inf, -1.0, 2.0, 1.0, 0.0)):
        flat[(flat.size // 7 * j + 3 * j) % flat.size] = v
    return torch.from_numpy(x).cuda()


def check_encode(x, layout, colour, denorm):
    standard, full, order = colour
    B, _, H, W = x.shape
    yraw, y, uvraw, uv = planes(layout, B, H, W)
    if layout == "b1stride":
        pl, codes = entry_args(y, uv, colour)
        assert uv.stride(0) % 16 == 2 and lib.load().emavfi_postprocess_nv12(x.data_ptr(), *pl, B, H, W, *codes,
                                                                             *lib._stats(lib.IMAGENET_MEAN, lib.IMAGENET_STD, 3, ctypes.c_double), denorm,
                                                                             lib._stream()) == 0, lib.last_error()
    else:
        lib.postprocess_nv12(x, standard, full, order, denormalize=bool(denorm), out=(y, uv))
    u8 = lib.postprocess_u8(x, denormalize=bool(denorm)).cpu().numpy()
    ywant, uvwant = oracle.encode(u8, standard, full, order)
    # expected images of the two raw buffers: the planes where they belong, FILL everywhere else (pitch padding, slack, the front offset)
    eyraw, ey, euvraw, euv = planes(layout, B, H, W)
    ey.copy_(torch.from_numpy(ywant))
    euv.copy_(torch.from_numpy(uvwant))
    assert torch.equal(y, ey), ("Y", layout, colour, denorm, (B, H, W))
    assert torch.equal(uv, euv), ("UV", layout, colour, denorm, (B, H, W))
    assert torch.equal(yraw, eyraw) and torch.equal(uvraw, euvraw), ("padding bytes were written", layout, (B, H, W))
    return y, uv


@pytest.mark.parametrize("denorm", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_shapes_pitches_and_paths(layout, denorm):
    for n, ((H, W), B) in enumerate(cases(layout, (1, 3))):
        check_encode(encode_input(B, H, W, denorm, seed=100 + n), layout, COLOURS[(n + 3 * denorm) % len(COLOURS)], denorm)


@pytest.mark.parametrize("standard,full,order", COLOURS)
def test_encode_every_colour_definition(standard, full, order):
    for denorm in (0, 1):
        check_encode(encode_input(2, 64, 96, denorm, seed=7), "dense", (standard, full, order), denorm)


def test_default_outputs_and_pinned_planes():
    """out=None allocates dense planes; the byte side may be pinned host memory (read / written in place)"""
    rng = np.random.default_rng(3)
    B, H, W = 2, 32, 48
    ynp = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    uvnp = rng.integers(0, 256, (B, H // 2, W // 2, 2), dtype=np.uint8)
    want = lib.preprocess_u8(torch.from_numpy(oracle.decode(ynp, uvnp)).cuda())
    yh, uvh = torch.from_numpy(ynp).pin_memory(), torch.from_numpy(uvnp).pin_memory()
    got = lib.preprocess_nv12(yh, uvh, device="cuda")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    y, uv = lib.postprocess_nv12(got)
    ywant, uvwant = oracle.encode(lib.postprocess_u8(got).cpu().numpy())
    assert y.is_contiguous() and uv.is_contiguous()
    assert (y.cpu().numpy() == ywant).all() and (uv.cpu().numpy() == uvwant).all()
    yo, uvo = torch.zeros(B, H, W, dtype=torch.uint8).pin_memory(), torch.zeros(B, H // 2, W // 2, 2, dtype=torch.uint8).pin_memory()
    lib.postprocess_nv12(got, out=(yo, uvo))
    torch.cuda.synchronize()
    assert (yo.numpy() == ywant).all() and (uvo.numpy() == uvwant).all()
    with pytest.raises(ValueError, match="dense"):
        lib.preprocess_nv12(torch.zeros(1, 4, 8, dtype=torch.uint8, device="cuda")[:, :, ::2], torch.zeros(1, 2, 2, 2, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="uv must be"):
        lib.preprocess_nv12(torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda"), torch.zeros(1, 2, 3, 2, dtype=torch.uint8, device="cuda"))


def test_fast_path_equals_scalar_path():
    """the same frames once 16-byte aligned (16-byte accesses) and once through a view 2 bytes off (scalar accesses)"""
    rng = np.random.default_rng(17)
    B, H, W = 2, 64, 128
    ynp = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    uvnp = rng.integers(0, 256, (B, H // 2, W // 2, 2), dtype=np.uint8)
    for colour in (COLOURS[0], COLOURS[7]):
        fast = check_decode(ynp, uvnp, "pad16", colour)
        slow = check_decode(ynp, uvnp, "offset2", colour)
        assert torch.equal(fast.view(torch.int32), slow.view(torch.int32))
        for denorm in (0, 1):
            x = encode_input(B, H, W, denorm, seed=23)
            yf, uvf = check_encode(x, "pad16", colour, denorm)
            ys, uvs = check_encode(x, "offset2", colour, denorm)
            assert torch.equal(yf, ys) and torch.equal(uvf, uvs)


# ---------------------------------------------------------------- the harness
H, W, NFRAMES = 48, 64, 11


def pack(y, uv):
    return np.concatenate([y, uv.reshape(uv.shape[0], -1)], axis=0)


def unpack(frame):
    h = frame.shape[0] * 2 // 3
    return frame[:h], frame[h:].reshape(h // 2, frame.shape[1] // 2, 2)


@pytest.fixture(scope="module")
def stream_case():
    """frames, the model, and per frame / per pair everything the harness's output is made of, computed once outside the harness"""
    rng = np.random.default_rng(41)
    base = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy()              # smooth content, so that predictions are not noise
    frames = []
    for i in range(NFRAMES):
        img = np.clip(np.roll(base, 2 * i, axis=2).transpose(1, 2, 0) * 0.2 + 0.45 + rng.normal(0, 0.02, (H, W, 3)), 0, 1)
        frames.append(pack(*oracle.encode((img * 255).astype(np.uint8))))
    model = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    ys = torch.from_numpy(np.stack([unpack(f)[0] for f in frames])).cuda()
    uvs = torch.from_numpy(np.stack([unpack(f)[1] for f in frames])).cuda()
    x = lib.preprocess_nv12(ys, uvs)
    enc = lambda t, denorm: [pack(y, uv) for y, uv in zip(*oracle.encode(lib.postprocess_u8(t, denormalize=denorm).cpu().numpy()))]
    with torch.no_grad():
        out = torch.cat([model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)])
    return {"frames": frames, "model": model, "pred": {q: enc(out, q) for q in (False, True)}, "roundtrip": enc(x, True)}


def expected_stream(case, factor, quirks):
    want = []
    for item in FrameInterpolator.emission_plan(NFRAMES, factor, 1, reference_quirks=quirks):
        if item[0] == "pred":
            assert item[2] == item[1] + 1
            want.append(case["pred"][quirks][item[1]])
        elif item[0] == "src":
            want.append(case["roundtrip"][item[1]] if quirks else case["frames"][item[1]])
        else:
            assert item[2] is False
            want.append(case["frames"][item[1]])
    return want


@pytest.mark.parametrize("factor,batch", [(1, 2), (1, 8), (3, 2), (3, 8)])
def test_harness_nv12(stream_case, factor, batch):
    frames, model = stream_case["frames"], stream_case["model"]
    for quirks in (False, True):
        want = expected_stream(stream_case, factor, quirks)
        fi = FrameInterpolator(model, factor, 1, batch_pairs=batch, reference_quirks=quirks, pixel_format="nv12")
        got = list(fi.run(frames))
        assert len(got) == len(want) == fi.count_outputs(NFRAMES)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.shape == (H * 3 // 2, W)
            assert np.array_equal(g, w), (factor, batch, quirks, k)
        views = [f.copy() for f in FrameInterpolator(model, factor, 1, batch_pairs=batch, reference_quirks=quirks, pixel_format="nv12",
                                                     copy_out=False).run(frames)]
        assert len(views) == len(want) and all(np.array_equal(g, w) for g, w in zip(views, want)), (factor, batch, quirks, "copy_out=False")
    zc = list(FrameInterpolator(model, factor, 1, batch_pairs=batch, pixel_format="nv12", zero_copy=True).run(frames))
    want = expected_stream(stream_case, factor, True)
    assert len(zc) == len(want) and all(np.array_equal(g, w) for g, w in zip(zc, want)), (factor, batch, "zero_copy")


def test_harness_nv12_other_standard_and_bad_frames(stream_case):
    frames, model = stream_case["frames"], stream_case["model"]
    fi = FrameInterpolator(model, 1, 1, batch_pairs=2, pixel_format="nv12", yuv_standard="bt709", yuv_full_range=True)
    got = list(fi.run(frames[:3]))
    ys = torch.from_numpy(np.stack([unpack(f)[0] for f in frames[:3]])).cuda()
    uvs = torch.from_numpy(np.stack([unpack(f)[1] for f in frames[:3]])).cuda()
    x = lib.preprocess_nv12(ys, uvs, "bt709", True)
    with torch.no_grad():
        p = model(x[0:1], x[1:2])
    y, uv = oracle.encode(lib.postprocess_u8(p).cpu().numpy(), "bt709", True)
    assert np.array_equal(got[0], pack(y[0], uv[0]))
    y, uv = oracle.encode(lib.postprocess_u8(x[0:1]).cpu().numpy(), "bt709", True)
    assert np.array_equal(got[1], pack(y[0], uv[0]))
    with pytest.raises(ValueError, match="NV12"):
        list(fi.run([np.zeros((H, W, 3), np.uint8)] * 2))
    with pytest.raises(ValueError, match="even H and W"):
        list(fi.run([np.zeros((70, 64), np.uint8)] * 2))
    with pytest.raises(ValueError, match="pixel_format"):
        FrameInterpolator(model, pixel_format="i420")


def test_harness_bgr24_is_unchanged(stream_case):
    """the default path on the decoded frames: exactly postprocess_u8(model(preprocess_u8(...))), as before NV12 existed"""
    model = stream_case["model"]
    frames = [oracle.decode(*unpack(f)) for f in stream_case["frames"]]
    x = lib.preprocess_u8(torch.from_numpy(np.stack(frames)).cuda())
    with torch.no_grad():
        out = torch.cat([model(x[i:i + 1], x[i + 1:i + 2]) for i in range(NFRAMES - 1)])
    pred, src = lib.postprocess_u8(out).cpu().numpy(), lib.postprocess_u8(x).cpu().numpy()
    got = list(FrameInterpolator(model, 1, 1, batch_pairs=2).run(frames))
    assert FrameInterpolator(model).pixel_format == "bgr24"
    assert len(got) == 2 * (NFRAMES - 1) + 1
    for i in range(NFRAMES - 1):
        assert np.array_equal(got[2 * i], pred[i]) and np.array_equal(got[2 * i + 1], src[i]), i
    assert np.array_equal(got[-1], frames[-1])
