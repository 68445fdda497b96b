"""Frame metrics on the GPU: emavfi_frame_metrics_u8 against the numpy restatement of the frame-metric definition (tests/metrics_oracle.py).
Every comparison is bit-exact: both words {sse, ssimq} of every image pair and channel."""
import functools
import itertools

import numpy as np
import pytest
import torch

from emavfi import lib
import metrics_oracle as oracle

pytestmark = pytest.mark.gpu

# one window; no window (SSE only) on either axis; smaller than any tile of 32 x 32 windows; windows straddling tile edges on both axes and
# 16-byte units straddling the halo (45 x 100 and 70 x 130: 2 x 3 and 2 x 4 tiles with ragged last tiles)
SHAPES = [(11, 11), (10, 40), (40, 10), (12, 27), (45, 100), (70, 130)]
LAYOUTS = ["dense", "pad16", "odd"]
FILL_A, FILL_B = 0xA5, 0x3C          # padding bytes: would change a sum if padding were read
GUARD, SENTINEL = 16, -7


def up(v, m):
    return (v + m - 1) // m * m


def image(layout, data, fill, pinned=False):
    """a raw byte buffer full of `fill` and a [B,H,W,C] view into it holding `data`: dense rows, rows padded to a multiple of 16 plus 16, or
    an odd pitch; for B > 1 the batch stride is larger than the plane in every layout"""
    B, H, W, C = data.shape
    row = W * C
    pitch = {"dense": row, "pad16": up(row, 16) + 16, "odd": row + 5}[layout]
    bstride = pitch * H + ({"dense": 32, "pad16": 48, "odd": 7}[layout] if B > 1 else 0)
    raw = torch.full((B * bstride + pitch + 64,), fill, dtype=torch.uint8)
    raw = raw.pin_memory() if pinned else raw.cuda()
    view = raw.as_strided((B, H, W, C), (bstride, pitch, C, 1))
    view.copy_(torch.tensor(data))
    return view


@functools.lru_cache(maxsize=None)
def pair(B, H, W, C, kind):
    """(a, b, the oracle's [B, C, 2]) - computed once per case and shared, never modified"""
    rng = np.random.default_rng(B * 1000003 + H * 131 + W * 7 + C + len(kind))
    a = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    if kind == "random":
        b = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    elif kind == "noisy":                 # a copy with a few counts of noise: SSIM near 1, every channel different
        b = np.clip(a.astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    else:                                 # "shift": the same image one pixel to the right
        a = (np.add.outer(np.arange(H) * 3, np.arange(W) * 5)[None, :, :, None] + rng.integers(0, 9, (B, H, W, C))).astype(np.uint8)
        b = np.roll(a, 1, axis=2)
    for v in (a, b):
        v.setflags(write=False)
    want = oracle.metrics(a, b)
    want.setflags(write=False)
    return a, b, want


def guarded_out(B, C, pinned=False):
    flat = torch.full((B * C * 2 + 2 * GUARD,), SENTINEL, dtype=torch.int64)
    flat = flat.pin_memory() if pinned else flat.cuda()
    return flat, flat[GUARD:GUARD + B * C * 2].view(B, C, 2)


def run(a, b, B, C, **kw):
    """the library's result with sentinel words around `out`, which starts out holding garbage"""
    flat, out = guarded_out(B, C)
    got = lib.frame_metrics_u8(a, b, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "words beyond [B,C,2] were written"
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_metrics_are_the_oracle_word_for_word(shape):
    H, W = shape
    for C, B, kind in itertools.product((1, 3), (1, 3), ("random", "noisy", "shift")):
        a, b, want = pair(B, H, W, C, kind)
        for la, lb in (("dense", "dense"), ("pad16", "odd"), ("odd", "pad16"), ("pad16", "pad16")):
            got = run(image(la, a, FILL_A), image(lb, b, FILL_B), B, C)
            assert np.array_equal(got, want), (shape, C, B, kind, la, lb)     # every word written, padding not read
    if H < oracle.WIN or W < oracle.WIN:
        assert (want[..., 1] == 0).all() and (want[..., 0] > 0).all()        # no window, and still the squared differences
    fresh = lib.frame_metrics_u8(torch.tensor(a).cuda(), torch.tensor(b).cuda())     # out=None
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (B, C, 2) and np.array_equal(fresh.cpu().numpy(), want)


def test_many_tiles_in_a_row():
    a, b, want = pair(1, 24, 2100, 1, "noisy")
    for layout in LAYOUTS:
        assert np.array_equal(run(image(layout, a, FILL_A), image(layout, b, FILL_B), 1, 1), want), layout


def test_one_720p_colour_pair_and_two_runs_agree():
    a, b, want = pair(1, 720, 1280, 3, "noisy")
    da, db = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    first, second = run(da, db, 1, 3), run(da, db, 1, 3)
    assert np.array_equal(first, want) and np.array_equal(second, first)
    p = [lib.psnr(int(want[0, c, 0]), 720 * 1280) for c in range(3)]
    s = [lib.ssim(int(want[0, c, 1]), 720, 1280) for c in range(3)]
    assert all(40.0 < v < 60.0 for v in p) and all(0.9 < v < 1.0 for v in s), (p, s)          # +-3 counts of noise


def test_known_answers_on_the_device():
    H, W = 45, 100
    n, wins = H * W, oracle.windows(H, W)
    img = torch.tensor(pair(1, H, W, 3, "random")[0]).cuda()
    same = lib.frame_metrics_u8(img, img.clone()).cpu().numpy()
    assert (same[..., 0] == 0).all() and (same[..., 1] == wins * 2 ** 32).all()
    for u, v in ((0, 255), (255, 0), (17, 200), (128, 128)):
        got = lib.frame_metrics_u8(torch.full((1, H, W, 2), u, dtype=torch.uint8, device="cuda"),
                                   torch.full((1, H, W, 2), v, dtype=torch.uint8, device="cuda")).cpu().numpy()
        q = int(np.floor((2.0 * u * v + oracle.C1) / ((float(u * u) + float(v * v)) + oracle.C1) * 4294967296.0))
        assert (got[..., 0] == n * (u - v) ** 2).all() and (got[..., 1] == wins * q).all(), (u, v)


def test_item_k_of_a_batch_equals_the_pair_alone_and_c_up_to_4():
    for C in (2, 4):
        a, b, want = pair(3, 45, 100, C, "noisy")
        da, db = image("pad16", a, FILL_A), image("odd", b, FILL_B)
        assert np.array_equal(run(da, db, 3, C), want)
        for k in range(3):
            assert np.array_equal(run(da[k:k + 1], db[k:k + 1], 1, C), want[k:k + 1]), (C, k)
    # strided batches: every second frame of one side against consecutive frames of the other
    a, b, _ = pair(3, 45, 100, 3, "random")
    da, db = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    assert np.array_equal(run(da[0:3:2], db[1:3], 2, 3), oracle.metrics(a[0:3:2], b[1:3]))


def test_pinned_sources_pinned_out_and_both_access_paths():
    a, b, want = pair(3, 45, 100, 3, "noisy")
    for layout in LAYOUTS:
        got = run(image(layout, a, FILL_A, pinned=True), image(layout, b, FILL_B), 3, 3, device="cuda")
        assert np.array_equal(got, want), ("pinned a", layout)
    flat, out = guarded_out(3, 3, pinned=True)
    lib.frame_metrics_u8(torch.tensor(a).cuda(), torch.tensor(b).cuda(), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.numpy(), want) and (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all()
    # the same image through a 16-byte aligned view (16-byte loads) and through a view that starts one byte later (byte loads)
    for C in (1, 3):
        a, b, want = pair(3, 48, 80, C, "random")          # rows of 80 / 240 bytes: a dense aligned view takes the wide path
        res = []
        for off in (0, 1):
            views = []
            for data, fill in ((a, FILL_A), (b, FILL_B)):
                raw = torch.full((data.size + 16,), fill, dtype=torch.uint8, device="cuda")
                v = raw[off:off + data.size].view(data.shape)
                v.copy_(torch.tensor(data))
                assert v.data_ptr() % 16 == off
                views.append(v)
            res.append(run(views[0], views[1], 3, C))
        assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], want), C
    # Y planes inside packed NV12 frames: pitch W, batch stride H * 3 / 2 * W
    rng = np.random.default_rng(5)
    nv_a, nv_b = (torch.tensor(rng.integers(0, 256, (3, 72, 64), dtype=np.uint8)).cuda() for _ in range(2))
    got = lib.frame_metrics_u8(nv_a[:, :48].unsqueeze(-1), nv_b[:, :48].unsqueeze(-1)).cpu().numpy()
    assert np.array_equal(got, oracle.metrics(nv_a[:, :48].cpu().numpy()[..., None], nv_b[:, :48].cpu().numpy()[..., None]))


def test_python_wrapper_refuses_mismatched_images():
    a = torch.zeros(1, 12, 12, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        lib.frame_metrics_u8(a, torch.zeros(1, 12, 13, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        lib.frame_metrics_u8(a, a, out=torch.zeros(1, 3, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="1..4"):
        lib.frame_metrics_u8(torch.zeros(1, 12, 12, 5, dtype=torch.uint8, device="cuda"), torch.zeros(1, 12, 12, 5, dtype=torch.uint8, device="cuda"))
