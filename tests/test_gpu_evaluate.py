"""FrameInterpolator.evaluate on the GPU: the held-out protocol through the harness's slots and lanes must equal, word for word, what the same
steps give by hand for each target - the model's forward on frames t - 1 and t + 1, postprocess_u8(denormalize=False), and the numpy oracle of
the frame-metric definition (tests/metrics_oracle.py) on the bytes against frame t."""
import math

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, Evaluation, FrameInterpolator, lib, synth
import metrics_oracle as oracle

pytestmark = pytest.mark.gpu

NFRAMES = 7
SIZES = [(40, 56), (23, 37)]


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    return m


def clip(H, W, fmt="bgr24", n=NFRAMES):
    """one translating synthetic pattern with a little noise per frame; NV12: the blue channel as Y over a random UV plane"""
    rng = np.random.default_rng(H * 7 + W)
    base = synth.synthetic_frames_u8(9, 1, H, W + 4 * n, "natural")[0][0]
    frames = [np.clip(base[:, 3 * i:3 * i + W].astype(np.int64) + rng.integers(-2, 3, (H, W, 3)), 0, 255).astype(np.uint8) for i in range(n)]
    if fmt == "nv12":
        frames = [np.concatenate([f[..., 0], rng.integers(96, 160, (H // 2, W), dtype=np.uint8)], axis=0) for f in frames]
    return frames


def by_hand(model, frames, t, fmt="bgr24", size=None):
    """(predicted bytes, true bytes) of target t as [1, H, W, C] arrays, one step at a time"""
    dev = lambda f: torch.from_numpy(np.ascontiguousarray(f)).unsqueeze(0).cuda()
    if fmt == "nv12":
        H = frames[0].shape[0] * 2 // 3
        planes = lambda f: (dev(f[:H]), dev(f[H:].reshape(H // 2, -1, 2)))
        x1, x2 = (lib.preprocess_nv12(*planes(frames[k])) for k in (t - 1, t + 1))
        with torch.no_grad():
            y, _ = lib.postprocess_nv12(model(x1, x2), denormalize=False)
        return y.cpu().numpy()[..., None], frames[t][None, :H, :, None]
    x1, x2 = (lib.preprocess_u8(dev(frames[k]), size=size) for k in (t - 1, t + 1))
    with torch.no_grad():
        pred = lib.postprocess_u8(model(x1, x2), denormalize=False)
    truth = lib.resize_u8(dev(frames[t]), size) if size is not None else dev(frames[t])
    return pred.cpu().numpy(), truth.cpu().numpy()


@pytest.fixture(scope="module")
def expected(model):
    """(H, W, fmt, size) -> {t: the oracle's [C, 2] words}, computed once per configuration for every target 1..5"""
    cache = {}

    def get(H, W, fmt="bgr24", size=None):
        key = (H, W, fmt, size)
        if key not in cache:
            frames = clip(H, W, fmt)
            cache[key] = {t: oracle.metrics(*by_hand(model, frames, t, fmt, size))[0] for t in range(1, NFRAMES - 1)}
        return cache[key]
    return get


def check(ev, want, targets, size, C):
    assert isinstance(ev, Evaluation) and ev.size == size and ev.channels == C and [r.t for r in ev] == targets
    H, W = size
    for r in ev:
        w = want[r.t]
        assert r.sse == tuple(int(v) for v in w[:, 0]) and r.ssimq == tuple(int(v) for v in w[:, 1]), r.t
        assert r.sse_all == int(w[:, 0].sum()) and r.psnr_all == oracle.psnr(int(w[:, 0].sum()), H * W * C)
        assert r.psnr == tuple(oracle.psnr(int(v), H * W) for v in w[:, 0])
        assert r.ssim == tuple(oracle.ssim(int(v), H, W) for v in w[:, 1]) and r.ssim_all == sum(r.ssim) / C
        assert all(v > 0 for v in r.sse) and all(math.isfinite(v) for v in r.psnr + r.ssim)  # noisy ground truth: no prediction is exact
    assert ev.psnr == sum(r.psnr_all for r in ev) / len(ev) and ev.ssim == sum(r.ssim_all for r in ev) / len(ev)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_evaluate_equals_the_steps_done_by_hand(model, expected, size):
    H, W = size
    frames, want = clip(H, W), expected(H, W)
    # 7 frames, 5 targets, 2 per batch: targets cross batch and slot boundaries (three batches over two slots, the last one short)
    fi = FrameInterpolator(model, batch_pairs=2)
    check(fi.evaluate(frames), want, [1, 2, 3, 4, 5], size, 3)
    check(fi.evaluate(frames, every=2), want, [1, 3, 5], size, 3)          # the targets' staged rows are two apart
    check(fi.evaluate(iter(frames), every=3), want, [1, 4], size, 3)       # three apart; any iterable
    # options that shape run()'s output do not reach evaluate()
    other = FrameInterpolator(model, interpolation_factor=3, frame_interval=2, batch_pairs=3, reference_quirks=False, mode="recursive",
                              scene_threshold=0.01, zero_copy=True)
    check(other.evaluate(frames), want, [1, 2, 3, 4, 5], size, 3)
    # two ranks: contiguous shares, concatenated in rank order
    parts = [FrameInterpolator(model, batch_pairs=2).evaluate(frames, rank=r, world=2) for r in range(2)]
    assert [r.t for r in parts[0]] == [1, 2, 3] and [r.t for r in parts[1]] == [4, 5]
    assert parts[0].targets + parts[1].targets == fi.evaluate(frames).targets


def test_evaluate_nv12_scores_the_y_planes(model, expected):
    H, W = 40, 56
    fi = FrameInterpolator(model, batch_pairs=2, pixel_format="nv12")
    check(fi.evaluate(clip(H, W, "nv12")), expected(H, W, "nv12"), [1, 2, 3, 4, 5], (H, W), 1)


def test_evaluate_with_size_scores_against_the_resized_ground_truth(model, expected):
    H, W, size = 40, 56, (23, 37)
    for quirks in (True, False):
        fi = FrameInterpolator(model, batch_pairs=2, size=size, reference_quirks=quirks)
        check(fi.evaluate(clip(H, W)), expected(H, W, "bgr24", size), [1, 2, 3, 4, 5], size, 3)


def test_run_is_untouched_by_evaluate_and_short_clips_are_empty(model):
    H, W = 40, 56
    frames = clip(H, W)
    want = list(FrameInterpolator(model, 2, 1, batch_pairs=2).run(frames))
    fi = FrameInterpolator(model, 2, 1, batch_pairs=2)
    before = list(fi.run(frames))
    ev = fi.evaluate(frames)
    after = list(fi.run(frames))            # now on the buffers evaluate() allocated
    assert len(ev) == 5 and len(before) == len(after) == len(want)
    assert all(np.array_equal(g, w) for g, w in zip(before, want)) and all(np.array_equal(g, w) for g, w in zip(after, want))
    assert fi.evaluate(frames).targets == ev.targets
    for n in (0, 1, 2):
        empty = fi.evaluate(frames[:n])
        assert len(empty) == 0 and empty.targets == [] and math.isnan(empty.psnr) and math.isnan(empty.ssim)
    assert len(fi.evaluate(frames[:3])) == 1
    with pytest.raises(ValueError, match="every"):
        fi.evaluate(frames, every=0)
    with pytest.raises(ValueError, match="same-shape"):
        fi.evaluate(frames[:3] + [frames[3][:-1]])
