"""motion_estimation gated LAYER BY LAYER, per element, through exact pass-through weights (tests/motion_probe.py): the outputs of .0
(a0: the feat half on the matrix cores, the broadcast-context half folded into the fp32 per-border-class bias table of ctx_finish_kernel)
and of .1 (a1: in the 16-bit modes at the reference width computed by conv_ring.inl's HEAD variant, whose rows never leave the LDS) are
brought out through the `flow` tap, mid / 2 forwards each, and every gated quantity is compared with a float64 reference built from the
GPU's OWN previous tensor - so every gate bites to half a unit of the store and no bound has to absorb a flipped intermediate rounding
(what the three-layer chain bounds of tests/test_gpu_conv_rounding_model.py and tests/test_gpu_fp32x3_rounding_model.py must).
tests/test_motion_probe_cpu.py shows on the CPU that a correct fold is inside the a0 gates at these shapes and that a wrong class index
on one edge, a table of the wrong sample or a miscounted tap is outside them at most of the elements it touches.

Weights synthetic_state_dict(seed=5), natural frames of seed 43.  Per (mode, shape):
  * probe A, a0: identity .1, moving selector .2.  The flow planes must be non-negative and unchanged by the storage rounding (an
    EQUALITY: the pass-through held).  Reference: motion_probe.a0_model on the GPU's own `feat` and `ctx` taps - bound, and in the
    16-bit modes the nearest-rounding gates (mismatch share <= MISMATCH_CAP, one unit).  The worst ratio and the element count are
    printed per border class.  Where a fused head exists, position k = 0 is repeated with the head as its own launch (SW_NO_HEAD) and
    must return the same bits: with the mid / 2 selector positions this pins the fused head's weight packing for every input channel;
  * probe B, a1: the real .1, moving selector.  Reference: conv_model on the GPU's own a0, the same three gates.  With the fused head
    the launch list must name `conv3x3+head` - the gate is on the HEAD variant's main contraction -, and four positions are repeated
    under SW_NO_HEAD (the unfused ring kernel has its own single-layer gates elsewhere);
  * probe C, the real head: gate_last_layer on the GPU's own a1, fused and under SW_NO_HEAD.
Modes: mid 64 in bf16 and fp16 (the ring kernel; bf16 keeps `feat` as f16 and hands bf16 on, Plan::feat16), again for probe A alone with
EMAVFI_CONV_RING=0 in a child process (the layout switches are latched once per process), which runs conv3x3_persist16_kernel's
bias_mode 1; mid 64 in fp32 (bound only) and fp32x3 (the split model with the context half as `pre` term, bound and z gates: the
helpers of the fp32x3 flow test); mid 8 in bf16 and fp32, mid 16 in fp16 (the tile kernel's conv_init_acc, separate head launches).
amp16 is not run: its table is rounded by policy; its statement is the autocast restatement of tests/test_gpu_parity.py.
measured: see MEASURED at the end of this file."""
import os
import subprocess
import sys
import time

import pytest
import torch

from conv_cases import set_env
from emavfi import EMA_VFI, lib, synth
from motion_probe import OTHER_SHAPES, RING_SHAPES, a0_model, assemble, border_class, gate_figures, model_w0
from rounding_model import MISMATCH_CAP, U32, Z_MAX, Z_RMS, accumulation_variance, carried, chain_stats_x3, conv64, conv_model, conv_model_x3, storage_round, z_gates
from test_gpu_conv_rounding_model import family_of, gate_last_layer, model_layer, switch   # noqa: F401  (switch: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (mid_channels, dtype, shapes, fused head)
MODES = [(64, "bf16", RING_SHAPES, True), (64, "fp16", RING_SHAPES, True), (64, "fp32", OTHER_SHAPES, False), (64, "fp32x3", OTHER_SHAPES, False),
         (8, "bf16", OTHER_SHAPES, False), (8, "fp32", OTHER_SHAPES, False), (16, "fp16", OTHER_SHAPES, False)]
CASES = [(m, d, sh, h) for m, d, shapes, h in MODES for sh in shapes]
case_id = lambda c: f"mid{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}x{c[2][2]}"


def three_gates(got, ref, bound, d, store, label, fails):
    """gate_layer's assertions (tests/test_gpu_conv_rounding_model.py) on a tensor that came out of the forward; returns err / bound."""
    assert got.shape == ref.shape and torch.isfinite(got).all(), label
    ratio, share, units = gate_figures(got, ref, bound, d, store)
    print(f"{label}: err / bound max {ratio.max().item():.3f}; mismatches {100 * share:.4f} % (<= {units:.0f} units)")
    if ratio.max().item() > 1.0:
        fails.append(f"{label}: an element exceeds the rounding model's worst case ({ratio.max().item():.3f}x)")
    if share > MISMATCH_CAP or units > 1.0:
        fails.append(f"{label}: not a round-to-nearest store of the float64 value ({100 * share:.3f} % differ, up to {units:.0f} units)")
    return ratio


def split_gates(got, ref, bound, sigma, label, fails):
    """the fp32x3 file's gates: err / bound <= 1 for every element, rms z <= 1, max |z| <= 6; returns err / bound."""
    assert got.shape == ref.shape and torch.isfinite(got).all(), label
    ratio, rms, zmax = z_gates(got, ref, bound, sigma)
    print(f"{label}: err / bound max {ratio:.3f}; rms z {rms:.3f}; max |z| {zmax:.2f}")
    if ratio > 1.0:
        fails.append(f"{label}: an element exceeds the split model's worst case ({ratio:.3f}x)")
    if rms > Z_RMS or zmax > Z_MAX:
        fails.append(f"{label}: outside the statistical gate (rms z {rms:.3f}, max |z| {zmax:.2f})")
    return (got.double() - ref).abs() / bound


def per_class(ratio, H, W, label):
    """worst err / bound and element count of every border class present; every class of the shape must have elements"""
    cls = border_class(H, W)
    rows = []
    for c in cls.unique().tolist():
        sel = ratio[:, :, cls == c]
        assert sel.numel() > 0, (label, c)
        rows.append(f"{c}: {sel.max().item():.3f} ({sel.numel()})")
    print(f"{label}: worst ratio (elements) per border class - " + ", ".join(rows))


def x3_layer0(sd, mid, feat, ctx):
    """motion_estimation.0 for chain_stats_x3: the split convolution on feat, the context half as float64 `pre` term (value, bound,
    variance) - as tests/test_gpu_fp32x3_rounding_model.py::test_flow_of_the_forward_from_its_feat_and_ctx_taps builds it."""
    B, _, H, W = feat.shape
    w0, b0 = sd["motion_estimation.0.0.weight"].float(), sd["motion_estimation.0.0.bias"].float()
    ctx_b = ctx.view(B, mid, 1, 1).expand(B, mid, H, W)
    wc = model_w0(w0, mid, "fp32")[:, mid:].double()
    half = conv64(ctx_b, wc)
    half_mag = conv64(ctx_b.abs(), wc.abs()) + b0.double().abs().view(1, -1, 1, 1)
    nt = 9 * mid + 1
    half_var = accumulation_variance(nt, b0.double().view(1, -1, 1, 1), half, conv64(ctx_b.double() ** 2, wc ** 2)) + (U32 * half_mag) ** 2 / 3
    return {"w": w0[:, :mid].contiguous(), "b": b0, "act": "relu", "pre": (half, 2 * nt * U32 * half_mag, half_var)}


def probe(mid, dtype, shape, fused_head, set_switch, probes="ABC"):
    """One (mode, shape): the probes named in `probes`; returns the list of failures.  set_switch(bit, on) or None (no fused head to
    switch off)."""
    B, H, W = shape
    x3 = dtype == "fp32x3"
    store = "fp32" if x3 else dtype
    label = f"mid {mid} {dtype} {shape}"
    sd = synth.synthetic_state_dict(seed=5, mid_channels=mid)
    if os.environ.get("EMAVFI_CACHE") != "0":
        raise RuntimeError("the probe repacks the weights for every selector position: run it with EMAVFI_CACHE=0 (no blob files)")
    f1, f2 = (f.to(DEV) for f in synth.synthetic_frames(43, B, H, W, "natural"))
    model = EMA_VFI(mid_channels=mid, compute_dtype=dtype).to(DEV).eval()
    nfw = [0]

    def run(sd_k):
        model.load_state_dict(sd_k, strict=True)
        nfw[0] += 1
        return lib.forward_flow(model.packed_weights(lib.dtype_code(dtype), torch.device(DEV)), f1, f2, mid, 3, dtype).cpu()

    def head_fused():
        return any("conv3x3+head" in n for n, _, _ in lib.forward_launches(3, mid, 3, B, H, W, dtype))

    def no_head(on):
        if set_switch is not None:
            set_switch(lib.SW_NO_HEAD, on)
            assert head_fused() == (not on)

    no_head(False)
    assert head_fused() == fused_head
    model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        _, taps = model(f1, f2, return_taps=True)
    feat, ctx, flow = (taps[k].float().cpu() for k in ("feat", "ctx", "flow"))
    assert all(torch.isfinite(t).all() for t in (feat, ctx, flow))
    if B == 2:
        assert (ctx[0] != ctx[1]).any()
    fails = []
    held = (lambda t: carried(t).float()) if x3 else (lambda t: storage_round(t, store))

    # ---- probe A
    a0 = assemble(run, sd, mid, keep_m1=False)
    assert a0.shape == (B, mid, H, W) and (a0 >= 0).all() and torch.equal(held(a0), a0), f"{label}: the pass-through did not return stored non-negative values"
    if x3:
        ref, bound, sigma = chain_stats_x3(feat, [x3_layer0(sd, mid, feat, ctx)])
        ratio = split_gates(a0, ref, bound, sigma, f"{label} a0", fails)
    else:
        w0m, b0 = model_w0(sd["motion_estimation.0.0.weight"], mid, dtype), sd["motion_estimation.0.0.bias"].float()
        ratio = three_gates(a0, *a0_model(feat, ctx, w0m, b0, store), store, f"{label} a0", fails)
    per_class(ratio, H, W, f"{label} a0")
    if fused_head:
        no_head(True)
        part = assemble(run, sd, mid, keep_m1=False, ks=(0,))
        no_head(False)
        assert torch.equal(part[:, :2], a0[:, :2]), f"{label}: the head as its own launch returns other bits of a0 than the fused head"
    if "B" not in probes:
        return fails

    # ---- probe B
    L1 = model_layer(sd, "motion_estimation.1.0", "fp32" if x3 else dtype)
    a1 = assemble(run, sd, mid, keep_m1=True)
    assert (a1 >= 0).all() and torch.equal(held(a1), a1)
    if x3:
        ref1, bound1, sigma1, _ = conv_model_x3(a0, L1["w"], L1["b"], 1, "relu", with_truth=False)
        split_gates(a1, ref1, bound1, sigma1, f"{label} a1", fails)
    else:
        ref1, bound1, d1 = conv_model(a0, L1["w"], L1["b"], 1, "relu", store, fp32_products=dtype == "fp32")
        three_gates(a1, ref1, bound1, d1, store, f"{label} a1", fails)
    if fused_head:
        ks = (0, 7, 16, mid // 2 - 1)
        ch = [c for k in ks for c in (2 * k, 2 * k + 1)]
        no_head(True)
        part = assemble(run, sd, mid, keep_m1=True, ks=ks)[:, ch]
        no_head(False)
        three_gates(part, ref1[:, ch], bound1[:, ch], d1[:, ch], store, f"{label} a1, head as its own launch, positions {ks}", fails)
        print(f"{label}: those channels of a1 from the two launch sequences are {'the same bits' if torch.equal(part, a1[:, ch]) else 'NOT the same bits'}")

    # ---- probe C
    head = model_layer(sd, "motion_estimation.2", "fp32" if x3 else dtype, act="none", store="fp32")
    for own_launch in ((False, True) if fused_head else (False,)):
        no_head(own_launch)
        got = run(sd) if own_launch else flow
        name = f"{label} flow, head {'as its own launch' if own_launch else ('fused' if fused_head else 'launch')}"
        if x3:
            refc, boundc, sigmac = chain_stats_x3(a1, [dict(w=head["w"], b=head["b"], act="none", planar=True)])
            split_gates(got, refc, boundc, sigmac, name, fails)
        elif dtype == "fp32":
            refc, boundc, dc = conv_model(a1, head["w"], head["b"], 1, "none", "fp32", fp32_products=True)
            three_gates(got, refc, boundc, dc, "fp32", name, fails)
        else:
            gate_last_layer(got, a1, head, "fp32", name, fails)
    no_head(False)
    assert torch.equal(run(sd), flow), f"{label}: forward_flow and the flow tap differ"
    print(f"{label}: {nfw[0]} forwards")
    return fails


def test_shape_lists_reach_all_sixteen_border_classes_in_every_mode():
    for mid, dtype, shapes, _ in MODES:
        seen = set()
        for _, H, W in shapes:
            seen |= set(border_class(H, W).unique().tolist())
        assert seen == set(range(16)), (mid, dtype)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_motion_estimation_layer_by_layer(case, switch, monkeypatch):
    mid, dtype, shape, fused_head = case
    set_env(monkeypatch, {})
    monkeypatch.setenv("EMAVFI_CACHE", "0")     # mid / 2 repacked blobs per probe: nothing to keep
    B, H, W = shape
    names = [n for n, _, _ in lib.forward_launches(3, mid, 3, B, H, W, dtype)]
    m0 = [n for n in names if "motion_estimation.0" in n]
    assert len(m0) == 1
    if mid == 64 and dtype in ("bf16", "fp16"):
        assert family_of(64, 64, 1, dtype, {}) == "ring2" and m0[0].startswith("conv3x3<f16,ck=64,nf=2,s=1>") and sum(n.startswith("conv3x3+conv3x3") for n in names) == 1
    t0 = time.perf_counter()
    fails = probe(mid, dtype, shape, fused_head, switch if fused_head else None)
    print(f"{case_id(case)}: {time.perf_counter() - t0:.2f} s")
    assert not fails, "\n".join(fails)


_CHILD = r"""
import sys
sys.path[:0] = %(paths)r
import test_gpu_motion_layers as t
from emavfi import lib
assert lib.load().emavfi_layout_tag() & 2, "EMAVFI_CONV_RING=0 was not latched"
fails = []
for dtype in ("bf16", "fp16"):
    assert t.family_of(64, 64, 1, dtype, {"EMAVFI_CONV_RING": "0"}) == "persist16"
    for B, H, W in t.RING_SHAPES:
        names = [n for n, _, _ in lib.forward_launches(3, 64, 3, B, H, W, dtype)]
        m0 = [n for n in names if "motion_estimation.0" in n]
        ring_only = [n for n in names if "+head" in n or n.startswith(("conv3x3+conv3x3", "conv_first+conv3x3")) or (dtype == "bf16" and n.startswith("conv3x3<f16"))]
        assert len(m0) == 1 and m0[0].startswith("conv3x3<" + ("bf16" if dtype == "bf16" else "f16") + ",ck=64,nf=2,s=1>") and not ring_only, names
        fails += t.probe(64, dtype, (B, H, W), False, None, probes="A")
assert not fails, "\n".join(fails)
print("persist16 probes done")
"""


def test_a0_on_the_persistent_kernel_with_the_ring_kernels_off():
    """EMAVFI_CONV_RING=0 (a layout switch, latched once per process: a child): motion_estimation.0 at the reference width runs
    conv3x3_persist16_kernel with bias_mode 1 - the third place the class index is computed.  Probe A alone, bf16 and fp16, the ring
    list's shapes.  The family: the library's own layout tag says the ring kernels are off, the launch list names no launch only they
    have (fused head, fused pairs, f16 kernels in the bf16 model) and motion_estimation.0 as one 64-channel chunk of two fragments,
    which family_of() maps to persist16."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = _CHILD % {"paths": [here, root, os.path.join(root, "video-frame-interpolation_amd")]}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, EMAVFI_CONV_RING="0", EMAVFI_CACHE="0"))
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("persist16 probes done") == 1 and r.stdout.count(" a0: err / bound max") == 2 * len(RING_SHAPES)


# MEASURED (MI355X, this file's own output; 41 passed, the file takes 8 s, the child 3.5 s of it).  Per mode, over its shapes: the range of
# max(err / bound), the largest mismatch share (every mismatch one unit), forwards and wall time per case.
#   mode                 a0                           a1                           flow (real head)                per case
#   mid 64 bf16 (ring)   0.617 ... 0.840, 0.0066 %    0.765 ... 0.946, 0.0083 %    fused <= 0.001, own <= 0.004    71 forwards, 0.12 ... 0.19 s
#   mid 64 fp16 (ring)   0.319 ... 0.449, 0.0496 %    0.705 ... 0.807, 0.0496 %    fused <= 0.002, own <= 0.006    71 forwards, 0.12 ... 0.17 s
#   mid 64 fp32          <= 0.001                     0.002 ... 0.004              0.001 ... 0.008                 65 forwards, 0.15 ... 0.16 s
#   mid 64 fp32x3        <= 0.002; z 0.142, 1.28      <= 0.007; z 0.177, 1.10      <= 0.006; z 0.183, 0.63         65 forwards, 0.14 s        (z: largest rms, largest max |z|)
#   mid 8 bf16 (tile)    0.603 ... 0.909, none        0.589 ... 0.960, none        <= 0.018                        9 forwards, 0.02 s
#   mid 8 fp32           0.001 ... 0.004              0.007 ... 0.014              0.002 ... 0.032                 9 forwards, 0.02 s
#   mid 16 fp16 (tile)   0.715 ... 0.794, none        0.711 ... 0.887, none        0.004 ... 0.012                 17 forwards, 0.03 s
#   child, ring off      bf16 0.606 ... 0.776, 0.0126 %;  fp16 0.314 ... 0.452, 0.0456 %   (conv3x3_persist16_kernel, probe A alone)
# (the first case of a process adds the library's load: 0.45 s.)  a1 of the four positions repeated with the head as its own launch:
# 0.596 ... 0.927 (bf16), 0.477 ... 0.728 (fp16), mismatches <= 0.0661 %, and in every case THE SAME BITS as the fused launch's rows: the
# HEAD variant's main contraction repeats the plain ring kernel's arithmetic.  Position 0 of a0 with the head as its own launch: the
# same bits in all 14 cases.  All 16 border classes have elements in every mode (the per-class lines; the corner classes' 64
# elements per sample reach 0.4 ... 0.75 in bf16, the interior's thousands 0.72 ... 0.78).  The a0 ratios of fp16 sit lower than a single layer's 0.7 ... 0.85
# because the model counts the whole 128-channel layer with rounded products (2 n roundings) where the kernel rounds some 650 times.
# One pixel, one column and one row run in every mode, the 16-bit forward at the reference width included (1 x 1 x 1 had not been run).
