"""Scene cuts on the GPU: emavfi_luma_signature_u8, emavfi_scene_flags, emavfi_hold_frames_u8 and the harness's scene_threshold against the
numpy restatement of the scene-cut definition (tests/scene_oracle.py).  Every comparison is bit-exact."""
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, lib, synth
import nv12_oracle
import scene_oracle as oracle

pytestmark = pytest.mark.gpu

# empty cells on both axes; one pixel per cell; uneven cells; 16-byte units straddling cell edges and the edges of a workgroup's 8 cells, a
# scalar remainder; more rows per cell than one; cells wider than 64 pixels (several units per cell per row, at C = 1)
SHAPES = [(1, 1), (5, 7), (32, 32), (33, 47), (45, 100), (70, 130), (64, 2100)]
LAYOUTS = ["dense", "pad16", "odd"]
SRC_FILL = 0xA5          # would change a sum if padding were read
GUARD, SENTINEL = 64, -7


def up(v, m):
    return (v + m - 1) // m * m


def image(B, H, W, C, layout, data, pinned=False):
    """a raw byte buffer full of SRC_FILL and a [B,H,W,C] view into it holding `data`: dense rows, rows padded to a multiple of 16 plus 16, or
    an odd pitch; for B > 1 the batch stride is larger than the plane in every layout"""
    row = W * C
    pitch = {"dense": row, "pad16": up(row, 16) + 16, "odd": row + 5}[layout]
    bstride = pitch * H + ({"dense": 32, "pad16": 48, "odd": 7}[layout] if B > 1 else 0)
    raw = torch.full((B * bstride + pitch + 64,), SRC_FILL, dtype=torch.uint8)
    raw = raw.pin_memory() if pinned else raw.cuda()
    view = raw.as_strided((B, H, W, C), (bstride, pitch, C, 1))
    view.copy_(torch.from_numpy(data))
    return view


def guarded_sig(B):
    flat = torch.full((B * 1024 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return flat, flat[GUARD:GUARD + B * 1024].view(B, 1024)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_signature_is_the_oracle_word_for_word(shape):
    H, W = shape
    rng = np.random.default_rng(H * 131 + W)
    for C, B, order, layout in itertools.product((1,) if W > 2000 else (1, 3), (1, 3), ("bgr", "rgb"), LAYOUTS):
        src = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
        want = oracle.signature(src, order)
        flat, out = guarded_sig(B)
        got = lib.luma_signature_u8(image(B, H, W, C, layout, src), order=order, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(out.cpu().numpy(), want), (shape, C, B, order, layout)       # all B * 1024 words written, padding not read
        assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "words beyond [B,1024] were written"
    fresh = lib.luma_signature_u8(torch.from_numpy(src).cuda(), order=order)               # out=None
    assert fresh.dtype == torch.int32 and np.array_equal(fresh.cpu().numpy(), want)


def test_signature_known_answers_pinned_source_and_both_access_paths():
    n = oracle.cell_pixels(70, 130).reshape(-1)
    const = lib.luma_signature_u8(torch.full((2, 70, 130, 3), 201, dtype=torch.uint8, device="cuda"))
    assert np.array_equal(const.cpu().numpy(), np.broadcast_to(n * 201, (2, 1024)))
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, (2, 45, 100, 3), dtype=np.uint8)
    want = oracle.signature(src)
    for layout in LAYOUTS:
        got = lib.luma_signature_u8(image(2, 45, 100, 3, layout, src, pinned=True), device="cuda")
        assert np.array_equal(got.cpu().numpy(), want), ("pinned", layout)
    # the same image through a 16-byte aligned buffer (16-byte loads) and through a view that starts one byte later (byte loads)
    for C in (1, 3):
        img = rng.integers(0, 256, (3, 96, 160, C), dtype=np.uint8)
        res = []
        for off in (0, 1):
            raw = torch.full((img.size + 16,), SRC_FILL, dtype=torch.uint8, device="cuda")
            v = raw[off:off + img.size].view(img.shape)
            v.copy_(torch.from_numpy(img))
            assert v.data_ptr() % 16 == off
            res.append(lib.luma_signature_u8(v))
        assert torch.equal(res[0], res[1]) and np.array_equal(res[0].cpu().numpy(), oracle.signature(img)), C
    # a Y plane inside packed NV12 frames: pitch W, batch stride H * 3 / 2 * W
    nv = torch.from_numpy(rng.integers(0, 256, (3, 72, 64), dtype=np.uint8)).cuda()
    got = lib.luma_signature_u8(nv[:, :48].unsqueeze(-1))
    assert np.array_equal(got.cpu().numpy(), oracle.signature(nv[:, :48].cpu().numpy()[..., None]))


@pytest.mark.parametrize("shape", [(45, 100), (5, 7), (720, 1280)], ids=["45x100", "5x7", "720x1280"])
def test_scene_flags_scores_and_thresholds(shape):
    H, W = shape
    rng = np.random.default_rng(H + W)
    frames = np.stack([np.clip(rng.integers(0, 256, (H, W, 3)) * (0.3 + 0.15 * i), 0, 255).astype(np.uint8) for i in range(5)])
    want_sig = oracle.signature(frames)
    sig = lib.luma_signature_u8(torch.from_numpy(frames).cuda())
    assert np.array_equal(sig.cpu().numpy(), want_sig)
    s = oracle.score(want_sig[:4], want_sig[1:], H, W)
    assert s.min() > 0 and len(set(s.tolist())) == 4
    guard = torch.full((2, 4 + 2 * GUARD), SENTINEL, dtype=torch.int32, device="cuda")
    fl, sc = guard[0, GUARD:GUARD + 4], guard[1, GUARD:GUARD + 4]
    for k in range(4):
        f, c = lib.scene_flags(sig[:4], sig[1:], (H, W), int(s[k]), flags=fl, scores=sc)
        assert np.array_equal(c.cpu().numpy(), s) and np.array_equal(f.cpu().numpy(), (s >= s[k]).astype(np.int32)) and f[k] == 1
        f, c = lib.scene_flags(sig[:4], sig[1:], (H, W), int(s[k]) + 1)
        assert np.array_equal(c.cpu().numpy(), s) and np.array_equal(f.cpu().numpy(), (s >= s[k] + 1).astype(np.int32)) and f[k] == 0
    assert (guard[:, :GUARD] == SENTINEL).all() and (guard[:, -GUARD:] == SENTINEL).all()
    # stride 0: every frame against frame 0 (as [1024] and as [1,1024]); strided rows; scores = NULL
    s0 = oracle.score(want_sig[:1], want_sig, H, W)
    for one in (sig[0], sig[:1]):
        f, c = lib.scene_flags(one, sig, (H, W), int(np.sort(s0)[2]))
        assert np.array_equal(c.cpu().numpy(), s0) and np.array_equal(f.cpu().numpy(), (s0 >= np.sort(s0)[2]).astype(np.int32)) and c[0] == 0
    f, c = lib.scene_flags(sig[0:4:2], sig[1:5:2], (H, W), 0)
    assert np.array_equal(c.cpu().numpy(), s[::2]) and (f == 1).all()
    f, c = lib.scene_flags(sig[:4], sig[1:], (H, W), int(s[2]), with_scores=False)
    assert c is None and np.array_equal(f.cpu().numpy(), (s >= s[2]).astype(np.int32))
    black, white = torch.zeros(1, H, W, 3, dtype=torch.uint8, device="cuda"), torch.full((1, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    f, c = lib.scene_flags(lib.luma_signature_u8(black), lib.luma_signature_u8(white), (H, W), lib.scene_threshold_units(1.0, H, W))
    assert int(c[0]) == 4080 * oracle.cells(H, W) and int(f[0]) == 1


@pytest.mark.parametrize("fb", [2553, 4608])
def test_hold_frames_copies_flagged_frames_and_nothing_else(fb):
    rng = np.random.default_rng(fb)
    n = 3
    for (doff, aoff), pad, rep, pattern in itertools.product(itertools.product((0, 1, 16), repeat=2), (48, 7), (1, 3),
                                                              ((0, 0, 0), (1, 1, 1), (0, 1, 0), (5, 0, -1))):
        ds, as_ = fb + pad, fb + pad + 16
        draw = torch.from_numpy(rng.integers(0, 256, (GUARD + doff + n * rep * ds + GUARD,), dtype=np.uint8)).cuda()
        araw = torch.from_numpy(rng.integers(0, 256, (GUARD + aoff + n * as_ + GUARD,), dtype=np.uint8)).cuda()
        draw = draw[(-draw.data_ptr()) % 16:]                       # a 16-byte aligned base, then the offset under test
        araw = araw[(-araw.data_ptr()) % 16:]
        dst = draw.as_strided((n * rep, fb), (ds, 1), storage_offset=draw.storage_offset() + GUARD + doff)
        alt = araw.as_strided((n, fb), (as_, 1), storage_offset=araw.storage_offset() + GUARD + aoff)
        assert dst.data_ptr() % 16 == doff % 16 and alt.data_ptr() % 16 == aoff % 16
        want, akeep = draw.clone(), araw.clone()
        wv = want.as_strided(dst.shape, dst.stride(), storage_offset=want.storage_offset() + GUARD + doff)
        for k in range(n):
            if pattern[k]:
                wv[k * rep:(k + 1) * rep] = alt[k]
        flags = torch.tensor(pattern, dtype=torch.int32, device="cuda")
        assert lib.hold_frames_u8(dst, alt, flags, rep).data_ptr() == dst.data_ptr()
        assert torch.equal(draw, want), ("frames / gaps / guard bands", fb, doff, aoff, pad, rep, pattern)
        assert torch.equal(araw, akeep)
    # a 3-D frame shape, one pair (the strides then mean nothing), pinned destination and source
    d = torch.zeros(3, 23, 37, 3, dtype=torch.uint8).pin_memory()
    a = torch.from_numpy(rng.integers(1, 256, (1, 23, 37, 3), dtype=np.uint8)).pin_memory()
    lib.hold_frames_u8(d, a, torch.ones(1, dtype=torch.int32, device="cuda"), 3)
    torch.cuda.synchronize()
    assert all(torch.equal(d[r], a[0]) for r in range(3))


# ---------------------------------------------------------------- the harness
H0, W0, NFRAMES, CUT = 48, 64, 7, (3, 4)


def pack(y, uv):
    return np.concatenate([y, uv.reshape(uv.shape[0], -1)], axis=0)


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    return m


def two_shots(H, W, fmt):
    """frames 0..3: one translating pattern; frames 4..6: an unrelated, much brighter one"""
    rng = np.random.default_rng(H * 7 + W)
    a = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy().transpose(1, 2, 0)
    b = synth.synthetic_frames(4, 1, H, W, "natural")[0][0].numpy().transpose(1, 2, 0)[::-1, ::-1]
    frames = []
    for i in range(NFRAMES):
        base, gain, lift = (a, 0.2, 0.15) if i <= CUT[0] else (b, 0.2, 0.70)
        img = np.clip(np.roll(base, 2 * i, axis=1) * gain + lift + rng.normal(0, 0.01, (H, W, 3)), 0, 1)
        u8 = (img * 255).astype(np.uint8)
        frames.append(pack(*nv12_oracle.encode(u8)) if fmt == "nv12" else u8)
    return frames


def oracle_scores(frames, fmt):
    """{(i, j): score} of every pair of frames the tests below form, at the size the frames arrive at"""
    if fmt == "nv12":
        H = frames[0].shape[0] * 2 // 3
        sig = oracle.signature(np.stack([f[:H] for f in frames])[..., None])
    else:
        H = frames[0].shape[0]
        sig = oracle.signature(np.stack(frames), "bgr")
    W = frames[0].shape[1]
    return {(i, i + 1): int(oracle.score(sig[i], sig[i + 1], H, W)) for i in range(len(frames) - 1)}, (H, W)


def separating_fraction(frames, fmt):
    """a scene_threshold only the cut pair reaches - by the oracle alone, which must separate the two groups by a wide margin"""
    scores, (H, W) = oracle_scores(frames, fmt)
    cut, rest = scores[CUT], max(v for k, v in scores.items() if k != CUT)
    assert cut > 4 * rest > 0, (cut, rest)                         # the oracle tells the cut from motion: neither "none" nor "all" passes
    fraction = (cut + rest) / 2 / (4080 * oracle.cells(H, W))
    assert rest < lib.scene_threshold_units(fraction, H, W) <= cut and 0 < fraction <= 1
    return fraction, scores


def check_run(model, frames, fmt, factor, mode, interval=1, batch_pairs=2, **kw):
    fraction, scores = separating_fraction(frames, fmt)
    args = dict(interpolation_factor=factor, frame_interval=interval, batch_pairs=batch_pairs, mode=mode, pixel_format=fmt, **kw)
    plain = list(FrameInterpolator(model, **args).run(frames))
    fi = FrameInterpolator(model, scene_threshold=fraction, **args)
    got = list(fi.run(frames))
    pairs, _, _ = FrameInterpolator.schedule(len(frames), interval)
    assert len(got) == len(plain) == fi.count_outputs(len(frames)) and CUT in pairs
    p = pairs.index(CUT)
    held = range(p * (factor + 1), p * (factor + 1) + factor)
    for k, (g, w) in enumerate(zip(got, plain)):
        assert g.dtype == np.uint8 and g.shape == w.shape
        if k in held:
            assert np.array_equal(g, got[p * (factor + 1) + factor]), ("held frame", k, args)     # the source frame yielded right after them
            assert not np.array_equal(g, w), ("the plain prediction differs from the held frame", k)
        else:
            assert np.array_equal(g, w), ("untouched frame", k, args)
    assert fi.scene_cuts == [(*CUT, scores[CUT])], (fi.scene_cuts, args)
    assert fi.scene_scores == [(a, b, scores[(a, b)]) for a, b in pairs if (a, b) in scores] and len(fi.scene_scores) == len(pairs)
    return fi, got, plain


@pytest.mark.parametrize("quirks", [True, False], ids=["quirks", "plain"])
@pytest.mark.parametrize("fmt", ["bgr24", "nv12"])
def test_harness_holds_the_earlier_frame_across_the_cut(model, fmt, quirks):
    frames = two_shots(H0, W0, fmt)
    for (factor, mode), zc in itertools.product(((2, "reference"), (3, "recursive")), (False, True)):
        check_run(model, frames, fmt, factor, mode, reference_quirks=quirks, zero_copy=zc)


@pytest.mark.parametrize("quirks", [True, False], ids=["quirks", "plain"])
def test_harness_with_a_resize_decides_at_the_source_size(model, quirks):
    frames = two_shots(2 * H0, 2 * W0, "bgr24")
    _, got, _ = check_run(model, frames, "bgr24", 2, "reference", reference_quirks=quirks, scale=0.5)
    assert got[0].shape == (H0, W0, 3)


def test_harness_threshold_nobody_reaches_interval_two_and_ranks(model):
    frames = two_shots(H0, W0, "bgr24")
    fraction, scores = separating_fraction(frames, "bgr24")
    plain = list(FrameInterpolator(model, 2, 1, batch_pairs=2).run(frames))
    off = FrameInterpolator(model, 2, 1, batch_pairs=2, scene_threshold=1.0)
    got = list(off.run(frames))
    assert len(got) == len(plain) and all(np.array_equal(g, w) for g, w in zip(got, plain))
    assert off.scene_cuts == [] and [s[2] for s in off.scene_scores] == [scores[(i, i + 1)] for i in range(NFRAMES - 1)]
    # frame_interval 2: pairs (1,2), (3,4), (5,6) in one batch - their frames sit at rows 0, 2, 4 and 1, 3, 5 of the slot
    for quirks in (True, False):
        check_run(model, frames, "bgr24", 2, "reference", interval=2, batch_pairs=4, reference_quirks=quirks)
    # two ranks: a pair's decision needs only its two frames
    whole = FrameInterpolator(model, 2, 1, batch_pairs=2, scene_threshold=fraction)
    want = list(whole.run(frames))
    parts, cuts = [], []
    for rank in range(2):
        fi = FrameInterpolator(model, 2, 1, batch_pairs=2, scene_threshold=fraction)
        parts += list(fi.run(frames, rank=rank, world=2))
        cuts += fi.scene_cuts
    assert len(parts) == len(want) and all(np.array_equal(g, w) for g, w in zip(parts, want))
    assert cuts == whole.scene_cuts == [(*CUT, scores[CUT])]


def test_harness_rows_that_form_no_run_take_one_launch_per_pair(model):
    """run() always stages arithmetic runs; the per-pair fall-back of the two scene legs is driven directly"""
    frames = two_shots(H0, W0, "bgr24")
    fi = FrameInterpolator(model, 1, 1, batch_pairs=4, scene_threshold=0.5)
    fi._alloc(frames[0].shape)
    slot = fi._slots[0]
    slot["d_in"][:5].copy_(torch.from_numpy(np.stack(frames[1:6])))
    ia, ib = [0, 2, 3], [3, 4, 4]                                 # frames (1,4), (3,5), (4,5): only the first two straddle the cut
    assert fi._run(slot["sig"], ia) is None and fi._run(slot["sig"], [4, 2, 0]) is None and fi._run(slot["sig"], [0, 2, 4]) is not None
    sig = oracle.signature(np.stack(frames[1:6]))
    s = [int(oracle.score(sig[a], sig[b], H0, W0)) for a, b in zip(ia, ib)]
    fi._scene_units = min(s[0], s[1])
    assert s[2] < fi._scene_units
    fi._scene_decide(slot, slot["d_in"][:5], ia, ib)
    assert slot["fs"][:, :3].cpu().tolist() == [[1, 1, 0], s]
    before = torch.from_numpy(np.random.default_rng(0).integers(0, 256, tuple(slot["d_pred"].shape), dtype=np.uint8)).cuda()
    slot["d_pred"].copy_(before)
    fi._scene_hold(slot, slot["d_pred"], slot["d_in"], ia, 1)
    want = before.clone()
    want[0], want[1] = slot["d_in"][0], slot["d_in"][2]
    assert torch.equal(slot["d_pred"], want)
