"""The harness's three lanes under stretch: a slot of the batch pipeline (emavfi/stream.py) may be reused only after its last reader, also
when the lanes do not finish in their usual order.  One lane at a time - the pre lane, the caller's stream, the post lane, the draining host
- is made about 20 ms slower per call, many times a 24 x 40 batch, and the multi-batch run must still give, byte for byte, what a single-batch
run of the same clip gives: a single batch reuses no slot.  Every other property of the harness has its byte comparison elsewhere
(tests/test_stream.py, tests/test_gpu_*.py); this file only moves the lanes against each other."""
import time

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, synth

pytestmark = pytest.mark.gpu

H, W = 24, 40
DELAY_MS = 20.0          # what a stretched call lasts, about
LANES = ["pre", "main", "post", "host"]
# kind -> (frames, constructor arguments, batch_pairs of the stretched run, its batches, batch_pairs of the single-batch expectation)
KINDS = {
    "run": (9, dict(interpolation_factor=1), 2, 5, 8),          # 8 pairs, a half-size head batch: 1, 2, 2, 2, 1 - each slot reused at least twice
    "resample": (7, dict(mode="resample", rate_in=24, rate_out=60, resample_depth=3, reference_quirks=False), 2, 3, 6),
    "evaluate": (9, dict(), 2, 4, 7),                           # 7 targets: 2, 2, 2, 1
}


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=21, mid_channels=8), strict=True)
    return m


@pytest.fixture(scope="module")
def cycles():
    """the spin count that makes one torch.cuda._sleep last about DELAY_MS, from one event-timed call (after one that loads the kernel)"""
    probe = 2_000_000
    torch.cuda._sleep(1000)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(probe)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    assert ms > 0.05, f"the probe of {probe} cycles took {ms} ms: too short to calibrate from"
    return int(probe * DELAY_MS / ms)


def clip(n):
    return list(np.random.default_rng(1000 + n).integers(0, 256, (n, H, W, 3), dtype=np.uint8))


def go(fi, kind, frames, pause=0.0):
    """what the harness gives for the clip: the yielded frames, copied, or evaluate()'s targets; `pause`: the consumer's sleep per frame"""
    if kind == "evaluate":
        return fi.evaluate(frames, every=1).targets
    out = []
    for v in fi.run(frames):
        if pause:
            time.sleep(pause)
        out.append(v.copy())
    return out


def same(got, want, kind):
    if kind == "evaluate":
        assert [r.t for r in got] == [r.t for r in want]
        for g, w in zip(got, want):
            assert g == w, g.t
    else:
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), k


@pytest.fixture(scope="module")
def unstretched(model):
    """(kind, extra constructor arguments) -> (the single-batch run's result, ms per batch of the unstretched multi-batch run, event-timed
    on its second pass), computed once; the unstretched multi-batch run must already equal the single-batch one"""
    cache = {}

    def get(kind, **extra):
        key = (kind, tuple(sorted(extra.items())))
        if key not in cache:
            n, kw, bp, batches, bp_one = KINDS[kind]
            frames = clip(n)
            want = go(FrameInterpolator(model, batch_pairs=bp_one, **kw, **extra), kind, frames)
            fi = FrameInterpolator(model, batch_pairs=bp, **kw, **extra)
            same(go(fi, kind, frames), want, kind)             # also the warm-up: buffers, streams, packed weights
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            got = go(fi, kind, frames)
            t1.record()
            t1.synchronize()
            same(got, want, kind)
            cache[key] = (want, t0.elapsed_time(t1) / batches)
        return cache[key]
    return get


def stretch(fi, lane, cycles):
    """makes every call on `lane` about DELAY_MS longer; returns the list the stretched calls are counted in"""
    calls = []

    def slow(inner):
        def call(*args, **kwargs):
            calls.append(1)
            torch.cuda._sleep(cycles)          # ordinary work on the current stream: the lane the harness made current
            return inner(*args, **kwargs)
        return call
    if lane == "pre":
        fi._pre_kernel = slow(fi._pre_kernel)
    elif lane == "post":
        fi._post_kernel = slow(fi._post_kernel)
    elif lane == "main":
        fi.model = slow(fi.model)
    return calls


def check(model, unstretched, cycles, kind, lane, **extra):
    n, kw, bp, batches, _ = KINDS[kind]
    want, per_batch_ms = unstretched(kind, **extra)
    print(f"{kind} {extra} {lane}: delay {DELAY_MS} ms ({cycles} cycles), unstretched {per_batch_ms:.3f} ms per batch")
    assert DELAY_MS >= 5 * per_batch_ms, (f"miscalibrated: a delay of {DELAY_MS} ms is not five times the unstretched run's "
                                          f"{per_batch_ms:.3f} ms per batch")
    frames = clip(n)
    if lane == "host":
        fi = FrameInterpolator(model, batch_pairs=bp, copy_out=False, **kw, **extra)
        got = go(fi, kind, frames, pause=DELAY_MS / 1000)
    else:
        fi = FrameInterpolator(model, batch_pairs=bp, **kw, **extra)
        calls = stretch(fi, lane, cycles)
        got = go(fi, kind, frames)
        assert len(calls) >= batches, f"the {lane} lane was stretched {len(calls)} times over {batches} batches"
    same(got, want, kind)


@pytest.mark.parametrize("lane", LANES)
@pytest.mark.parametrize("quirks", [True, False], ids=["quirks", "plain"])
@pytest.mark.parametrize("zero_copy", [False, True], ids=["copy", "zero_copy"])
def test_run_reuses_a_slot_only_after_its_last_reader(model, unstretched, cycles, zero_copy, quirks, lane):
    check(model, unstretched, cycles, "run", lane, zero_copy=zero_copy, reference_quirks=quirks)


@pytest.mark.parametrize("lane", LANES)
def test_resample_reuses_a_slot_only_after_its_last_reader(model, unstretched, cycles, lane):
    check(model, unstretched, cycles, "resample", lane)


@pytest.mark.parametrize("lane", LANES[:3])
def test_evaluate_reuses_a_slot_only_after_its_last_reader(model, unstretched, cycles, lane):
    check(model, unstretched, cycles, "evaluate", lane)
