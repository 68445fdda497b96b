"""Duplicate frames on the GPU: emavfi_frame_diff_cells / emavfi_duplicate_flags word for word against the numpy restatement of the
duplicate-frame definition (tests/dedup_oracle.py), and the harness's mode "resample" with dedup_threshold against the symbolic plan, its
nodes obtained independently from mode "recursive" on each gap's two frames.  Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import dedup_oracle as oracle
import resample_oracle
import scene_oracle
from workspace_harness import assert_guards, guarded

pytestmark = pytest.mark.gpu

POISON, GUARD_FILL = 0xCB, 0x5A
SHAPES = [(5, 7), (31, 33), (33, 47), (40, 56), (64, 80), (37, 16384)]
# (name, channels, order, depth, shift): bytes as a Y plane and as interleaved colour in both orders, words as the planar and P010 formats hold them
KINDS = [("y8", 1, "bgr", 8, 0), ("bgr", 3, "bgr", 8, 0), ("rgb", 3, "rgb", 8, 0), ("w10", 1, "bgr", 10, 0), ("w10s6", 1, "bgr", 10, 6), ("w16", 1, "bgr", 16, 0)]
NF = 4


def up(v, m):
    return (v + m - 1) // m * m


def images(H, W, C, depth, shift, seed):
    """NF images, words with the bits outside the sample set at random too; image 2 is image 1 with the luma of a few pixels moved by exactly one
    count (every channel of a colour pixel goes up by one), image 3 is image 2"""
    rng = np.random.default_rng(seed)
    idx = np.arange(0, H * W, max(1, H * W // 5))
    if depth == 8:
        f = rng.integers(0, 256, (NF, H, W, C), dtype=np.uint8)
        px = f[1].reshape(H * W, C)
        px[idx] = np.clip(px[idx], 1, 254)
        f[2] = f[1]
        f[2].reshape(H * W, C)[idx] += 1
    else:
        f = rng.integers(0, 65536, (NF, H, W), dtype=np.uint16)
        f[2] = f[1]
        f[2].reshape(-1)[idx] ^= 1 << shift
    f[3] = f[2]
    return f


def surface(data, layout):
    """`data` on the device as a strided tensor in an allocation that ends with its last sample.  "dense": rows and images packed; "aligned":
    the pitch rounded up to 16 bytes from a 256-byte aligned base (16-byte loads, and a scalar remainder where W is no multiple of 16); "odd":
    rows and images an odd number of samples further apart than they need be, the pitch no multiple of 16 bytes, the base one sample off
    (scalar code throughout)"""
    es, n, H = data.dtype.itemsize, data.shape[0], data.shape[1]
    row = int(np.prod(data.shape[2:]))                    # samples
    if layout == "dense":
        pitch, extra, off = row, 0, 0
    elif layout == "aligned":
        pitch, extra, off = up(row * es, 16) // es, 0, 0
    else:
        pad = next(p for p in (3, 5, 7, 9) if ((row + p) * es) % 16)
        pitch, extra, off = row + pad, 5, 1
    bstride = pitch * H + extra
    total = off + (n - 1) * bstride + (H - 1) * pitch + row
    dt = torch.uint8 if es == 1 else torch.int16
    raw = torch.full((total,), 0x3C, dtype=dt, device="cuda")
    strides = (bstride, pitch, data.shape[3], 1) if data.ndim == 4 else (bstride, pitch, 1)
    view = raw.as_strided(tuple(data.shape), strides, off)
    view.copy_(torch.from_numpy(data.view(np.uint8 if es == 1 else np.int16)))
    return view


def poisoned(shape):
    """(flat, view): an int32 tensor of `shape`, every byte POISON, between guard bands"""
    nbytes = 4 * int(np.prod(shape))
    flat, body = guarded(nbytes, POISON, GUARD_FILL, device="cuda")
    return flat, body.view(torch.int32).view(shape), nbytes


def run_entry(a, b, order, depth, shift, threshold, device=None):
    n = a.shape[0]
    cf, cells, cb = poisoned((n, 1024))
    ff, flags, fb = poisoned((n,))
    sf, scores, sb = poisoned((n,))
    assert lib.frame_diff_cells(a, b, order=order, depth=depth, shift=shift, out=cells, device=device).data_ptr() == cells.data_ptr()
    lib.duplicate_flags(cells, threshold, flags=flags, scores=scores)
    for flat, nbytes, what in ((cf, cb, "cells"), (ff, fb, "flags"), (sf, sb, "scores")):
        assert_guards(flat, nbytes, GUARD_FILL, what=what)
    return cells.cpu().numpy().view(np.uint32).astype(np.int64), flags.cpu().numpy(), scores.cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_entries_are_the_oracle_word_for_word(shape):
    H, W = shape
    for ki, (name, C, order, depth, shift) in enumerate(KINDS):
        data = images(H, W, C, depth, shift, seed=H * 7 + ki)
        want = oracle.cells(data[:-1], data[1:], order, depth, shift)                  # the consecutive pairs, computed once per kind
        assert want[0].max() > 16 and 0 < want[1].max() <= 16 and not want[2].any()
        thr = int(want[1].max())
        for layout in ("dense", "aligned", "odd"):
            what = (shape, name, layout)
            s = surface(data, layout)
            # overlapping a / b from one buffer: image k against image k + 1
            cells, flags, scores = run_entry(s[:-1], s[1:], order, depth, shift, thr)
            assert np.array_equal(cells, want), what
            assert np.array_equal(scores, oracle.score(want)) and np.array_equal(flags, oracle.flags(want, thr)) and list(flags) == [0, 1, 1], what
            assert np.array_equal(s.cpu().numpy().view(data.dtype), data), what        # both images are only read
            # separate buffers on different layouts, and item 1 of the batch alone
            t = surface(data[1:], "aligned" if layout == "odd" else "odd")
            cells2, flags2, _ = run_entry(s[:-1], t, order, depth, shift, 0)
            assert np.array_equal(cells2, want) and list(flags2) == [0, 0, 1], what
            one, _, sc1 = run_entry(s[1:2], s[2:3], order, depth, shift, 0)
            assert np.array_equal(one[0], want[1]) and sc1[0] == want[1].max(), what
        # pinned sources: the kernel reads host memory in place
        host = torch.from_numpy(data.view(np.uint8 if depth == 8 else np.int16)).pin_memory()
        cells, flags, _ = run_entry(host[:-1], host[1:], order, depth, shift, 0, device="cuda")
        torch.cuda.synchronize()
        assert np.array_equal(cells, want) and list(flags) == [0, 0, 1], (shape, name, "pinned")


def test_known_answers():
    rng = np.random.default_rng(41)
    H, W = 128, 160                                            # every cell holds 4 x 5 = 20 pixels
    for name, C, order, depth, shift in KINDS:
        a = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8) if depth == 8 else rng.integers(0, 65536, (1, H, W), dtype=np.uint16)
        if depth == 8:
            a[0, 50, 77] = np.clip(a[0, 50, 77], 1, 254)
        b = a.copy()
        if depth == 8:
            b[0, 50, 77] += 1                                      # every channel by one count: the luma moves by exactly one
        else:
            b[0, 50, 77] ^= np.array(1 << shift, dtype=b.dtype)
        d = [surface(v, "aligned") for v in (a, b)]
        cells, flags, scores = run_entry(d[0], d[0], order, depth, shift, 0)
        assert not cells.any() and scores[0] == 0 and flags[0] == 1, (name, "identical images")
        cells, flags, scores = run_entry(d[0], d[1], order, depth, shift, 0)
        cell = (50 * 32 // H) * 32 + 77 * 32 // W
        assert np.count_nonzero(cells) == 1 and cells[0, cell] == 1 == scores[0] and flags[0] == 0, (name, "one sample by one count")
        assert lib.duplicate_flags(torch.from_numpy(cells.astype(np.int32)).cuda(), 1)[0].item() == 1
        # a change confined to one cell scores the same whatever the other 1023 cells hold
        a2 = rng.integers(0, 256, a.shape, dtype=np.uint8) if depth == 8 else rng.integers(0, 65536, a.shape, dtype=np.uint16)
        b2 = a2.copy()
        for src, dst in ((a, a2), (b, b2)):
            dst[0, 48:52, 75:80] = src[0, 48:52, 75:80]
        b[0, 48:52, 75:80] = b2[0, 48:52, 75:80] = rng.integers(0, 256, b[0, 48:52, 75:80].shape).astype(b.dtype) << (shift if depth != 8 else 0)
        s1 = run_entry(surface(a, "dense"), surface(b, "odd"), order, depth, shift, 0)[2][0]
        s2 = run_entry(surface(a2, "odd"), surface(b2, "dense"), order, depth, shift, 0)[2][0]
        assert s1 == s2 == oracle.score(oracle.cells(a, b, order, depth, shift))[0] > 16, name


def test_a_cell_sum_above_2_to_32():
    """8192 x 8224 at depth 16, 0 against 65535: a cell holds 256 x 257 = 65 792 pixels, the smallest shape at which a cell's sum of absolute
    differences (65 792 x 65 535) passes 2^32; every cell's measure is 16 x 65 535"""
    H, W = 8192, 8224
    assert (H // 32) * (W // 32) * 65535 > 2 ** 32 > 256 * 256 * 65535            # a 256 x 256 cell still fits 32 bits
    a = torch.zeros(1, H, W, dtype=torch.int16, device="cuda")
    b = torch.full((1, H, W), -1, dtype=torch.int16, device="cuda")
    cells, flags, scores = run_entry(a, b, "bgr", 16, 0, 1048559)
    assert (cells == 1048560).all() and scores[0] == 1048560 and flags[0] == 0
    assert lib.duplicate_flags(torch.from_numpy(cells.astype(np.int32)).cuda(), 1048560)[0].item() == 1


# ---------------------------------------------------------------- the harness
H, W, D = 40, 56, 3
FORMATS = ["bgr24", "yuv420p8", "nv12", "yuv420p10", "p010"]
BYTE_FORMATS = FORMATS[:3]       # scene_threshold reads bytes: the 16-bit formats refuse it


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
    return m


def distinct(fmt, n, seed=1):
    """n frames of which no two have the same luma"""
    rng = np.random.default_rng(seed)
    if fmt == "bgr24":
        return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    if fmt in ("nv12", "yuv420p8"):
        return [rng.integers(16, 236, (H * 3 // 2, W), dtype=np.uint8) for _ in range(n)]
    depth = lib.DEPTHS.get(fmt) or lib.PLANAR_DEPTHS[fmt]
    shift = 16 - depth if fmt in lib.DEPTHS else 0
    return [(rng.integers(64, 940, (H * 3 // 2, W)) << (depth - 10 + shift)).astype(np.uint16) for _ in range(n)]


def letters(fmt, word, seed=1):
    """a clip spelt as letters: equal letters are copies of one frame"""
    pool = dict(zip(sorted(set(word)), distinct(fmt, len(set(word)), seed)))
    return [pool[c].copy() for c in word]


def luma_pair_cells(fmt, f0, f1):
    """the oracle's cells of two frames as the harness scores them: interleaved colour, or the Y plane"""
    _, depth, shift = lib.resample_sample_format(fmt)
    if fmt == "bgr24":
        return oracle.cells(f0, f1, "bgr")
    y0, y1 = f0[:H], f1[:H]
    return oracle.cells(y0[..., None], y1[..., None]) if depth == 8 else oracle.cells(y0, y1, depth=depth, shift=shift)


def resampler(model, fmt, rate_in, rate_out, method="nearest", **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, mode="resample", pixel_format=fmt, rate_in=rate_in, rate_out=rate_out,
                             resample_depth=D, resample_method=method, **kw)


_trees = {}


def tree(model, fmt, key, f0, f1, depth):
    """nodes 0 .. 2^depth of the pair (f0, f1), obtained independently: node j is the j-th prediction of mode "recursive" with factor 2^depth - 1"""
    if (fmt, key, depth) not in _trees:
        factor = (1 << depth) - 1
        out = list(FrameInterpolator(model, factor, 1, batch_pairs=2, reference_quirks=False, mode="recursive", pixel_format=fmt).run([f0, f1]))
        assert len(out) == factor + 2
        _trees[fmt, key, depth] = [out[factor]] + out[:factor] + [out[-1]]
    return _trees[fmt, key, depth]


def expected(model, fmt, plan, frames, clip_key, held=()):
    sb, depth, shift = lib.resample_sample_format(fmt)
    out = []
    for k, t0, m, j0, j1, w in plan.outputs:
        if (j0 == 0 and w == 0) or (t0 in held and k * plan.P - t0 * plan.Q > 0):
            out.append(frames[t0])
            continue
        nodes = tree(model, fmt, (clip_key, t0, t0 + m), frames[t0], frames[t0 + m], plan.D + oracle.log2_ceil(m))
        if w == 0:
            out.append(nodes[j0])
        else:
            a, b = nodes[j0], nodes[j1]
            out.append(resample_oracle.blend(a.view(np.uint8), b.view(np.uint8), w, sb, depth, shift).view(a.dtype))
    return out


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_clip_without_copies_is_untouched(model, fmt):
    frames = distinct(fmt, 6)
    for rates, method in (((24, 60), "nearest"), ((24, 60), "blend"), ((24, 24), "nearest")):
        fi = resampler(model, fmt, *rates, method, dedup_threshold=0)
        same(list(fi.run(frames)), list(resampler(model, fmt, *rates, method).run(frames)), (fmt, rates, method))
        assert fi.duplicates == [] and [t for t, _ in fi.dedup_scores] == [1, 2, 3, 4, 5] and all(sc > 0 for _, sc in fi.dedup_scores)


@pytest.mark.parametrize("fmt", FORMATS)
def test_copies_are_dropped_and_the_gap_is_interpolated(model, fmt):
    word = "AABCCCDD"
    frames = letters(fmt, word)
    kept = [0, 2, 3, 6, 7]                                  # t = 1, 4, 5 are dropped; t = 7 copies t = 6 but is the last frame
    scores = [int(oracle.score(luma_pair_cells(fmt, frames[t - 1], frames[t]))) for t in range(1, 8)]
    assert [s == 0 for s in scores] == [True, False, False, True, True, False, True]
    assert FrameInterpolator.dedup_kept([s == 0 for s in scores], 8) == kept
    for rates, method, count in (((24, 24), "nearest", 8), ((24, 24), "blend", 8), ((24, 60), "blend", 18)):
        plan = FrameInterpolator.resample_plan_dedup(kept, *rates, D, method)
        assert len(plan.outputs) == count == len(FrameInterpolator.resample_plan(8, *rates, D, method).outputs)
        fi = resampler(model, fmt, *rates, method, dedup_threshold=0)
        got = list(fi.run(frames))
        same(got, expected(model, fmt, plan, frames, word), (fmt, rates, method))
        assert fi.duplicates == [(1, 0), (4, 0), (5, 0)] and fi.dedup_scores == [(t, scores[t - 1]) for t in range(1, 8)]
        if rates == (24, 24):
            # de-judder: the copies are gone - an interpolated frame stands where frame 1 repeated frame 0
            assert np.array_equal(got[0], frames[0]) and not np.array_equal(got[1], frames[0]) and np.array_equal(got[2], frames[2])
            assert not np.array_equal(got[4], frames[3]) and not np.array_equal(got[5], frames[3]) and np.array_equal(got[7], frames[7])


@pytest.mark.parametrize("fmt", FORMATS)
def test_max_run_1_keeps_every_second_copy(model, fmt):
    word = "AAAAB"
    frames = letters(fmt, word, seed=2)
    fi = resampler(model, fmt, 24, 24, dedup_threshold=0, dedup_max_run=1)
    got = list(fi.run(frames))
    assert [t for t, _ in fi.duplicates] == [1, 3] and len(fi.dedup_scores) == 4
    plan = FrameInterpolator.resample_plan_dedup([0, 2, 4], 24, 24, D, "nearest")
    assert [o[1:5] for o in plan.outputs] == [(0, 2, 0, 0), (0, 2, 8, 8), (2, 2, 0, 0), (2, 2, 8, 8), (4, 1, 0, 0)]
    same(got, expected(model, fmt, plan, frames, word), fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunks_concatenate_to_the_whole(model, fmt):
    frames = letters(fmt, "ABCDDDEFFG", seed=3)             # the copies 3, 4, 5 straddle the chunk boundary at frame 4; frame 8 copies frame 7
    kw = dict(dedup_threshold=0, dedup_span=4)
    fi = resampler(model, fmt, 24, 60, "blend", **kw)
    whole = list(fi.run(frames))
    dups, scores = fi.duplicates, fi.dedup_scores
    assert [t for t, _ in dups] == [5] and [t for t, _ in scores] == list(range(1, 10))       # 4 and 8 are kept: the span rule
    assert len(whole) == fi.count_outputs(10) == 23
    fc = resampler(model, fmt, 24, 60, "blend", **kw)
    same(list(fc.run_chunked(iter(frames), chunk_pairs=4)), whole, (fmt, "run_chunked(chunk_pairs=4)"))
    assert fc.duplicates == dups and fc.dedup_scores == scores
    with pytest.raises(ValueError, match="dedup_span"):
        next(fc.run_chunked(iter(frames), chunk_pairs=6))
    with pytest.raises(ValueError, match="world"):
        next(fc.run(frames, 0, 2))


@pytest.mark.parametrize("fmt", BYTE_FORMATS)
def test_a_cut_across_a_gap_holds_the_kept_frame(model, fmt):
    rng = np.random.default_rng(8)

    def frame(level):
        y = np.clip(rng.random((H, W)) * 0.2 + level, 0, 1)
        if fmt == "bgr24":
            return (np.repeat(y[..., None], 3, axis=2) * 255).astype(np.uint8)
        return np.concatenate([(y * 219 + 16).astype(np.uint8), np.full((H // 2, W), 128, np.uint8)])
    d0, d1, b0, b1 = frame(0.15), frame(0.15), frame(0.70), frame(0.70)
    frames = [d0, d1, d1.copy(), b0, b1]                     # kept: 0, 1, 3, 4 - the gap (1, 3) goes from dark to bright
    kept = [0, 1, 3, 4]
    img = (lambda f: f) if fmt == "bgr24" else (lambda f: f[:H, :, None])
    sig = scene_oracle.signature(np.stack([img(f) for f in frames]), "bgr")
    sc = {(a, b): int(scene_oracle.score(sig[a], sig[b], H, W)) for a, b in zip(kept, kept[1:])}
    rest = max(v for k, v in sc.items() if k != (1, 3))
    fraction = (sc[1, 3] + rest) / 2 / (4080 * scene_oracle.cells(H, W))
    assert sc[1, 3] > 4 * rest > 0 and rest < lib.scene_threshold_units(fraction, H, W) <= sc[1, 3]
    for rates, method in (((24, 60), "blend"), ((24, 24), "nearest")):
        plain = list(resampler(model, fmt, *rates, method, dedup_threshold=0).run(frames))
        fi = resampler(model, fmt, *rates, method, dedup_threshold=0, scene_threshold=fraction)
        got = list(fi.run(frames))
        plan = FrameInterpolator.resample_plan_dedup(kept, *rates, D, method)
        assert len(got) == len(plain) == len(plan.outputs)
        held = 0
        for (k, t0, m, *_), g, p in zip(plan.outputs, got, plain):
            if t0 == 1 and k * plan.P - t0 * plan.Q > 0:
                assert m == 2 and np.array_equal(g, frames[1]) and not np.array_equal(g, p), ("held output", k)
                held += 1
            else:
                assert np.array_equal(g, p), ("untouched output", k)
        assert held == (5 if rates == (24, 60) else 1)       # k = 3 .. 7 (the time of the dropped frame included) / k = 2
        assert fi.duplicates == [(2, 0)] and fi.scene_cuts == [(1, 3, sc[1, 3])] and fi.scene_scores == [(a, b, sc[a, b]) for a, b in zip(kept, kept[1:])]


def test_command_line_dedup(model, tmp_path, capsys):
    frames = letters("yuv420p8", "AABCCCDD")
    src, dst = tmp_path / "in24.y4m", tmp_path / "out60.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 24, 1)) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2",
                   "--output-fps", "60", "--dedup", "0"])
    err = capsys.readouterr().err
    assert rc == 0 and "18 frames out" in err and "3 duplicate frames dropped" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
        assert (r.header.fps_num, r.header.fps_den, r.header.width, r.header.height) == (60, 1, W, H)
    same(got, list(resampler(model, "yuv420p8", 24, 60, dedup_threshold=0).run(frames)), "cli")      # seed 0, 8 channels, fp32: the fixture's model
    assert not np.array_equal(got[1], list(resampler(model, "yuv420p8", 24, 60).run(frames))[1])
