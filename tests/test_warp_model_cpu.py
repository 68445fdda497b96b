"""tests/warp_model.py held to ATen on the CPU: the per-element model the GPU gate uses (tests/test_gpu_warp_lattice.py) must itself
stay inside its bound against oracle.warp (F.grid_sample, the reference's own operator) on EVERY case builder, non-finite flows and
non-finite frames included - the latter is what pins "an out-of-range corner is skipped, whatever the frame holds there" to ATen.
And the carrier weights: under the fp32 oracle and under the autocast restatement a forward's `flow` tap IS the prescribed field."""
import numpy as np
import pytest
import torch

import warp_model as wm
from oracle import emavfi_oracle as oracle
from rounding_model import storage_round


def aten(f2, flow):
    return oracle.warp(torch.from_numpy(f2), torch.from_numpy(flow)).numpy()


@pytest.mark.parametrize("shape", wm.SHAPES)
def test_model_against_aten_on_every_case(shape):
    B, H, W = shape
    f2 = wm.frame(B, 3, H, W)
    cases = dict(wm.flow_cases(B, H, W))
    cases.update(wm.nonfinite_flow_cases(B, H, W))
    fails, worst, n, copies = [], 0.0, 0, 0
    for name, flow in cases.items():
        ref, bound, copy = wm.warp_model(f2, flow)
        f, ratio, size = wm.gate(aten(f2, flow), ref, bound, copy, label=f"{shape} {name}")
        fails += f
        worst, n, copies = max(worst, ratio), n + size, copies + int(copy.sum())
    print(f"SUMMARY {shape}: {len(cases)} cases, ATen err / bound max {worst:.3f}, {copies} copied pixels exact, excluded 0 of {n}")
    assert not fails, "\n".join(fails)
    assert copies > 0


@pytest.mark.parametrize("shape", wm.SHAPES)
def test_out_of_range_corners_are_skipped_whatever_the_frame_holds(shape):
    """NaN at (0, 0), +-Inf in two more corners, NaN inside: with every corner dead ATen returns exactly 0 - it never reads the frame."""
    B, H, W = shape
    f2 = wm.nonfinite_frame(wm.frame(B, 3, H, W))
    fails = []
    for name, flow in wm.nonfinite_frame_flows(B, H, W).items():
        ref, bound, copy = wm.warp_model(f2, flow)
        got = aten(f2, flow)
        fails += wm.gate(got, ref, bound, copy, label=f"{shape} {name}")[0]
        if name == "far outside" and max(H, W) > 1:      # (a one-pixel axis has i = 0 whatever the flow)
            assert not np.isnan(ref).any() and (ref == 0).all() and (got == 0).all(), name
    assert not fails, "\n".join(fails)


def test_integer_targets_copy_the_source_where_the_round_trip_is_exact():
    """size - 1 a power of two (H = 33, 65): iy is the integer itself, and so is ix in the first and the last column at least."""
    for B, H, W in ((1, 33, 64), (1, 65, 68)):
        f2 = wm.frame(B, 3, H, W)
        for d in (0.0, 1.0, -8.0, 9.0):
            flow = np.zeros((B, 2, H, W), dtype=np.float32)
            flow[:, 1] = d
            ref, _, copy = wm.warp_model(f2, flow)
            rows = np.arange(H)[(np.arange(H) + d >= 0) & (np.arange(H) + d <= H - 1)]
            assert copy[:, :, rows][..., [0, W - 1]].all()
            assert np.array_equal(ref[:, :, rows, 0], f2[:, :, rows + int(d), 0])


def test_stored_bound_restates_the_rounding_model():
    from rounding_model import _stored
    ref = torch.randn(64, dtype=torch.float64) * 3
    d = torch.rand(64, dtype=torch.float64) * 1e-6
    for store in ("bf16", "fp16", "fp32"):
        assert np.array_equal(wm.stored(ref.numpy(), d.numpy(), store), _stored(ref, d, store).numpy())


@pytest.mark.parametrize("mid", [8, 64])
def test_carrier_weights_make_the_forward_compute_the_prescribed_flow(mid):
    """fp32 oracle and the autocast (fp16) restatement: the `flow` tap equals the field bit for bit, `warped` is the warp by it."""
    B, H, W = 2, 17, 23
    sd = wm.carrier_state_dict(mid)
    cases = wm.carrier_flow_cases(B, H, W)
    for name in ("random quarters 15.75", "edges -1 | size+0", "const xy -15.75"):
        want = torch.from_numpy(cases[name])
        f1, f2 = wm.carrier_frames(cases[name])
        for forward in (oracle.forward, oracle.forward_autocast16):
            taps = {}
            forward(sd, f1, f2, taps=taps)
            assert torch.equal(taps["flow"], want), (mid, name, forward.__name__)
            assert torch.equal(taps["warped"], oracle.warp(f2, want)), (mid, name, forward.__name__)


def test_carrier_planes_survive_both_storage_types():
    for name, flow in wm.carrier_flow_cases(2, 33, 68).items():
        f1, _ = wm.carrier_frames(flow)
        for dtype in ("bf16", "fp16"):
            assert torch.equal(storage_round(f1, dtype), f1), (name, dtype)
            assert torch.equal(storage_round(torch.from_numpy(flow), dtype), torch.from_numpy(flow)), (name, dtype)
