"""FrameInterpolator(numa="auto"): the host side of the streaming harness placed on the device's NUMA node.  Frames are bit-identical
to numa="off", and the plan is the one emavfi.dist.numa_plan computes from the host's sysfs."""
import os

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, synth, dist as vdist

pytestmark = pytest.mark.gpu


def test_stream_numa_auto_is_bit_identical_to_off():
    model = EMA_VFI(compute_dtype="bf16").to("cuda:0").eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    u8, _ = synth.synthetic_frames_u8(31, 1, 96, 160, "natural")
    frames = [np.roll(u8[0], 4 * i, axis=1) for i in range(9)]
    mask = sorted(os.sched_getaffinity(0))
    for factor in (1, 3):
        off = list(FrameInterpolator(model, interpolation_factor=factor, batch_pairs=4).run(frames))
        fi = FrameInterpolator(model, interpolation_factor=factor, batch_pairs=4, numa="auto")
        auto = list(fi.run(frames))
        assert len(auto) == len(off) == 8 * (factor + 1) + 1
        assert all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(auto, off)), factor
        assert fi.numa == vdist.numa_plan(0)
        assert FrameInterpolator(model, interpolation_factor=factor).numa is None
    plan = fi.numa
    print(plan)
    if plan["bind"]:
        # the staging pool is the plan's own, its workers run on the plan's CPUs, the unbound pool is another one
        pool = fi._copy_pool()
        assert pool is not FrameInterpolator._pool
        masks = {tuple(m) for m in pool.map(lambda _: sorted(os.sched_getaffinity(0)), range(32))}
        assert masks == {tuple(plan["cpus"])}
        assert all(fi._slots[k][b].is_pinned() for k in range(2) for b in ("h_in", "h_pred", "h_src"))
    assert sorted(os.sched_getaffinity(0)) == mask          # the harness never rebinds the calling thread


def test_numa_option_is_checked():
    model = EMA_VFI(mid_channels=8, compute_dtype="bf16").to("cuda:0").eval()
    with pytest.raises(ValueError):
        FrameInterpolator(model, numa="on")
