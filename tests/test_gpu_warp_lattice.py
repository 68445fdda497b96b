"""The flow warp pinned where bilinear sampling bends - lattice, border and window edges - per element (tests/warp_model.py).

A random flow almost never puts a sample on an integer position, on -1, size - 1 or size, or on the hand-over between the tiled
kernel's LDS window (reach 8 px around a 32 x 64 tile) and its global gather.  Here every case is a WHOLE flow field built for one of
those places (warp_model.flow_cases), every element is held to a bound derived from the kernel's arithmetic - four fp32 products, three
additions, coordinates bit-identical to the fp32 model - and NONE is excluded.

  lib.warp          warp_nchw_kernel<false> (W % 4 != 0), warp_nchw_kernel<true> (W % 4 == 0, C != 3), warp_tiled_kernel<3, void>
                    (W % 4 == 0, C == 3; the shapes give grids with nwg % 8 == 0, != 0 and nwg < 8: the XCD tile permutation).  Every
                    finite case, the far / overflowing / infinite / NaN flows, and a frame2 that holds NaN and +-Inf at the CLAMPED
                    addresses of dead corners (pixel (0, 0), row 0, column 0): ATen skips an out-of-range corner, so must the kernel.
  forwards          carrier weights (warp_model.carrier_state_dict) make the forward compute a prescribed field of quarters exactly, so
                    the warp INSIDE it runs at the edges too: warp_tiled_kernel<3, float> (fp32, fp32x3, amp16; aligned 16-channel
                    store at mid 64, generic store at mid 8), warp_tiled_kernel<3, half_t | bf16_t> (row-mapped body of the compact
                    4-channel tail at mid 64; item-mapped body at mid 8 and, with EMAVFI_NO_FUSED_OFFSET=1, at mid 64 with its
                    ps - coff == 16 store) and warp_fused_kernel<T> (W % 4 != 0).  `flow` must equal the field bit for bit (a check of
                    the fused flow head at exact values, reported separately), `warped` is held to the model plus the store's half
                    unit and must EQUAL the storage rounding of lib.warp(frame2, flow).  amp16's second (fp16) destination feeds the
                    first attention block only and is visible through no tap: it is not probed here.

Assertions (warp_model.gate): the NaN pattern equals the model's; finite wherever the model is; every element within its bound, exact
where the bound is 0 (every dead sample); where the model's weights are exactly (1, 0, 0, 0) on in-range corners - integer targets on
an axis whose size - 1 is a power of two (H = 33, 65) and x = 0 / W - 1 at least - the result is frame2's pixel bit for bit.

Why every case stays inside every buffer (read from csrc/misc_kernels.hip before the first run; nothing here provokes a fault):
  * warp_tap tests the corner coordinates as FLOATS against [0, size - 1]; the integer xi / yi is (int) of a float that passed such a
    test (so it lies in [-1, size - 1] and converts exactly) or the literal 0: a far, infinite or NaN coordinate never reaches an
    int conversion.  The four addresses are max(., 0) / min(. + 1, size - 1): always pixels of the plane, whatever the flow;
  * the tiled kernel reads its LDS window only when all four clamped corners lie in rows [wy0, wy0 + 48] and columns [wx0, wx0 + 83]
    of it (`inside`); otherwise it gathers at the clamped global addresses above.  Window pieces outside the image are DMA'd from a
    64-float zero page, 16 bytes each; a piece inside starts at a multiple of 4 columns and W % 4 == 0, so it ends inside its row;
  * threads of a tile past H or W load flow from pixel 0 and store nothing (`live`, `y >= H || x >= W`);
  * a non-finite frame2 value is data: it changes no address.  The carrier forwards keep |flow| < 16 and all values finite."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import warp_model as wm
from emavfi import EMA_VFI, lib
from rounding_model import storage_round

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NCHW_SHAPES = {"scalar": [(2, 3, 17, 23), (1, 3, 1, 9), (1, 3, 9, 1), (1, 3, 1, 1)],
               "vec4": [(1, 1, 8, 12), (2, 4, 33, 68)],
               "tiled": [(1, 3, 1, 4), (1, 3, 64, 64), (3, 3, 40, 68), (1, 3, 33, 132), (1, 3, 65, 128), (5, 3, 8, 8)]}
ALL_NCHW = [(path, s) for path, shapes in NCHW_SHAPES.items() for s in shapes]
FORWARD_MODES = [("fp32", 64), ("fp32x3", 64), ("amp16", 64), ("bf16", 64), ("fp16", 64), ("fp32", 8), ("bf16", 8)]
FORWARD_SHAPES = [(1, 40, 68), (2, 33, 128), (1, 65, 132), (1, 17, 23), (1, 1, 9)]       # the last two: warp_fused_kernel
WARP_LABEL = {"fp32": "warp_fused<f32>", "fp32x3": "warp_fused<f32>", "amp16": "warp_fused<f32>", "bf16": "warp_fused<bf16>", "fp16": "warp_fused<f16>"}


def path_of(C, W):
    return "scalar" if W % 4 else ("tiled" if C == 3 else "vec4")


def run_warp(f2, flow):
    return lib.warp(torch.from_numpy(f2).to(DEV), torch.from_numpy(flow).to(DEV)).cpu().numpy()


@pytest.mark.parametrize("path,shape", ALL_NCHW)
def test_warp_entry_on_every_case(path, shape):
    B, C, H, W = shape
    assert path_of(C, W) == path
    f2 = wm.frame(B, C, H, W)
    cases = dict(wm.flow_cases(B, H, W))
    cases.update(wm.nonfinite_flow_cases(B, H, W))
    fails, worst, n, copies = [], 0.0, 0, 0
    for name, flow in cases.items():
        ref, bound, copy = wm.warp_model(f2, flow)
        f, ratio, size = wm.gate(run_warp(f2, flow), ref, bound, copy, label=f"{path} {shape} {name}")
        print(f"lib.warp {path} {shape} {name}: err / bound max {ratio:.3f}, excluded 0 of {size}")
        fails += f
        worst, n, copies = max(worst, ratio), n + size, copies + int(copy.sum())
    print(f"SUMMARY lib.warp {path} {shape}: {len(cases)} cases, err / bound max {worst:.3f}, {copies} copied pixels bit-exact, excluded 0 of {n}")
    assert not fails, "\n".join(fails)
    assert copies > 0


@pytest.mark.parametrize("path,shape", ALL_NCHW)
def test_warp_entry_skips_out_of_range_corners_of_a_nonfinite_frame(path, shape):
    """frame2 with NaN at (0, 0), +Inf at (0, W - 1), -Inf at (H - 1, 0), NaN inside: a dead corner's clamped address holds them, and
    the result there is still exactly what ATen returns - 0 for a sample with every corner dead."""
    B, C, H, W = shape
    f2 = wm.nonfinite_frame(wm.frame(B, C, H, W))
    fails, worst, n = [], 0.0, 0
    for name, flow in wm.nonfinite_frame_flows(B, H, W).items():
        ref, bound, copy = wm.warp_model(f2, flow)
        got = run_warp(f2, flow)
        f, ratio, size = wm.gate(got, ref, bound, copy, label=f"{path} {shape} {name}")
        print(f"lib.warp non-finite frame {path} {shape} {name}: err / bound max {ratio:.3f}, excluded 0 of {size}")
        fails += f
        worst, n = max(worst, ratio), n + size
        if name == "far outside" and max(H, W) > 1 and not (got == 0).all():
            fails.append(f"{path} {shape} {name}: {int((got != 0).sum())} elements are not 0")
    print(f"SUMMARY lib.warp non-finite frame {path} {shape}: err / bound max {worst:.3f}, excluded 0 of {n}")
    assert not fails, "\n".join(fails)


def stores_f16(launches, dtype):
    """Plan::feat16: a bf16 model whose first pack is the one-launch kernel keeps `feat` and the warped tail as IEEE f16, and then its
    readers are listed as f16 kernels (conv_name: "conv3x3<f16,...>")."""
    return dtype == "fp16" or (dtype == "bf16" and any(name.startswith("conv3x3<f16") for name, _, _ in launches))


def forward_gate(mode, mid, shape):
    """Every carrier case of `shape` through one model -> (flow failures, warped failures, summary line)."""
    B, H, W = shape
    launches = lib.forward_launches(3, mid, 3, B, H, W, mode)
    assert sum(name == WARP_LABEL[mode] for name, _, _ in launches) == 1, [name for name, _, _ in launches]
    store = "fp32" if mode in ("fp32", "fp32x3", "amp16") else ("fp16" if stores_f16(launches, mode) else "bf16")
    model = EMA_VFI(mid_channels=mid, compute_dtype=mode).to(DEV).eval()
    model.load_state_dict(wm.carrier_state_dict(mid), strict=True)
    cases = wm.carrier_flow_cases(B, H, W)
    flow_fails, fails, worst, n = [], [], 0.0, 0
    for name, flow in cases.items():
        f1, f2 = wm.carrier_frames(flow)
        with torch.no_grad():
            _, taps = model(f1.to(DEV), f2.to(DEV), return_taps=True)
        label = f"{mode} mid={mid} {shape} {name}"
        got_flow = taps["flow"].float().cpu()
        if not torch.equal(got_flow, torch.from_numpy(flow)):
            flow_fails.append(f"{label}: the flow head is off the prescribed field in {int((got_flow != torch.from_numpy(flow)).sum())} elements, "
                              f"max {(got_flow - torch.from_numpy(flow)).abs().max().item():.3e}")
            continue
        ref, bound, copy = wm.warp_model(f2.numpy(), flow)
        got = taps["warped"].float().cpu()
        f, ratio, size = wm.gate(got.numpy(), ref, wm.stored(ref, bound, store), copy, storage_round(torch.from_numpy(ref), store).numpy(), label)
        print(f"forward {label}: err / bound max {ratio:.3f}, excluded 0 of {size}")
        fails += f
        worst, n = max(worst, ratio), n + size
        dead =(ref == 0) & (bound == 0)                 # (the f16 store's subnormal term leaves no zero bound: a dead sample stores 0)
        if bool((got.numpy()[dead] != 0).any()):
            fails.append(f"{label}: {int((got.numpy()[dead] != 0).sum())} dead samples are not 0")
        alone =storage_round(lib.warp(f2.to(DEV), taps["flow"].float().contiguous()).cpu(), store)
        if not torch.equal(got, alone):
            fails.append(f"{label}: {int((got != alone).sum())} of {got.numel()} elements differ from the stored stand-alone warp")
    kernel = "warp_tiled_kernel" if W % 4 == 0 else "warp_fused_kernel"
    line = f"SUMMARY forward {mode} mid={mid} {shape} {kernel}, stored as {store}: {len(cases)} cases, err / bound max {worst:.3f}, excluded 0 of {n}"
    return flow_fails, fails, line


@pytest.mark.parametrize("shape", FORWARD_SHAPES)
@pytest.mark.parametrize("mode,mid", FORWARD_MODES)
def test_warp_inside_the_forward_on_a_prescribed_flow(mode, mid, shape):
    flow_fails, fails, line = forward_gate(mode, mid, shape)
    print(line)
    assert not flow_fails, "FLOW HEAD (not the warp):\n" + "\n".join(flow_fails)
    assert not fails, "\n".join(fails)


_CHILD = r"""
import sys
sys.path[:0] = %(paths)r
import test_gpu_warp_lattice as t
from emavfi import lib
B, H, W = %(shape)r
for mode in ("bf16", "fp16"):
    fused = lib.forward_launches(3, 64, 3, B, H, W, mode)
    assert not any(name.startswith("conv3x3<f16") for name, _, _ in fused) or mode == "fp16", "the bf16 model still stores f16: the compact tail is on"
    flow_fails, fails, line = t.forward_gate(mode, 64, (B, H, W))
    print(line)
    assert not flow_fails, "FLOW HEAD (not the warp):\n" + "\n".join(flow_fails)
    assert not fails, "\n".join(fails)
"""


def test_item_mapped_16_bit_body_with_the_compact_tail_off():
    """EMAVFI_NO_FUSED_OFFSET=1 (latched once per process: a child) runs the packs as two launches, so the warp writes channels 64..79 of
    the 80-channel fusion pixels - warp_tiled_kernel<3, half_t | bf16_t>'s item-mapped body and its ps - coff == 16 store - and the bf16
    model stores bf16.  One shape of several tiles, every carrier case."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = _CHILD % {"paths": [here, root, os.path.join(root, "video-frame-interpolation_amd")], "shape": (2, 33, 128)}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, EMAVFI_NO_FUSED_OFFSET="1"))
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("stored as bf16") == 1 and r.stdout.count("stored as fp16") == 1


# MEASURED (MI355X; this file's own SUMMARY lines; 60 passed; excluded elements: 0 in every case; the file takes 7 s, the child 3 s of it).
# err / bound max, smallest ... largest over the shapes of a path (ATen's CPU kernel against the same model: <= 0.79):
#   lib.warp           warp_nchw_kernel<false>            0.000 (1 x 1) ... 0.745     non-finite frame 0.000 ... 0.388
#                      warp_nchw_kernel<true>             0.352 ... 0.697             non-finite frame 0.227 ... 0.465
#                      warp_tiled_kernel<3, void>         0.214 (1 x 4) ... 0.776     non-finite frame 0.000 ... 0.615
#   forwards           fp32, fp32x3, amp16 (mid 64), fp32 (mid 8): the same figures in all four - the same flow, frame and arithmetic
#                      warp_tiled_kernel<3, float>        0.661 ... 0.807
#                      warp_fused_kernel<float>           0.335 ... 0.526
#                      bf16 and fp16 at mid 64 (stored as f16), bound = model + half a unit of the store
#                      warp_tiled_kernel<3, T> row-mapped 0.998 ... 0.999             warp_fused_kernel<T> 0.863 ... 0.990
#                      bf16 at mid 8 (stored as bf16)
#                      warp_tiled_kernel<3, bf16_t> items 0.994 ... 0.996             warp_fused_kernel<bf16_t> 0.841 ... 0.994
#                      compact tail off (child), mid 64   bf16 0.996, fp16 0.998
#   (a 16-bit figure near 1 is the store's own half unit: the bound of a value just above a power of two is the rounding error itself)
#   `flow` equalled the prescribed field bit for bit in every mode, shape and case; `warped` equalled the stored stand-alone warp in all.
#   Before the out-of-range corners were selected on their validity, 11 of the 12 non-finite-frame cases failed (NaN where ATen has 0:
#   2 346 of 2 346 elements of 2 x 3 x 17 x 23 under "far outside"); the 1 x 1 image has no out-of-range corner.
