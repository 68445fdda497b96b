"""tests/motion_probe.py tested on its own, with the CPU as the "kernel" (as tests/test_rounding_model_cpu.py does for the convolution
gates): the pass-through weights return motion_estimation.0's output exactly, the shape lists reach all 16 border classes, a correct
restatement of the context fold (motion_probe.cpu_kernel) is inside the a0 gates of tests/test_gpu_motion_layers.py at every shape that
file runs, and every planted border-class error (motion_probe.MUTATIONS) is outside them - at shares of the elements it touches that
are CONDITIONS here, not measurements.  feat and ctx come from the CPU oracle on the GPU file's weights and frames
(synthetic_state_dict(seed=5), natural frames of seed 43), rounded as the forward stores them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from emavfi import synth
from motion_probe import MUTATIONS, OTHER_SHAPES, RING_SHAPES, a0_model, assemble, border_class, cpu_kernel, gate_figures, model_w0
from oracle import emavfi_oracle as oracle
from rounding_model import MISMATCH_CAP, storage_round

# (mid_channels, dtype, shapes): what the GPU file runs (its fp32x3 mode shares the fp32 cases' class arithmetic: the tile kernel)
CONFIGS = [(64, "bf16", RING_SHAPES), (64, "fp16", RING_SHAPES), (64, "fp32", OTHER_SHAPES), (8, "bf16", OTHER_SHAPES), (8, "fp32", OTHER_SHAPES),
           (16, "fp16", OTHER_SHAPES)]
CASES = [(m, d, sh) for m, d, shapes in CONFIGS for sh in shapes]
case_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def oracle_taps(mid, shape):
    B, H, W = shape
    sd = synth.synthetic_state_dict(seed=5, mid_channels=mid)
    f1, f2 = synth.synthetic_frames(43, B, H, W, "natural")
    with torch.no_grad():
        feat = oracle.feature_extraction(sd, f1, f2)
        ctx = oracle.context_encoding(sd, feat)
    return sd, feat, ctx


def case(mid, dtype, shape):
    """(feat as stored - f16 in the bf16 model at the reference width, Plan::feat16 -, ctx, model weight, bias)"""
    sd, feat, ctx = oracle_taps(mid, shape)
    feat = storage_round(feat, dtype, as_f16=dtype == "bf16" and mid == 64)
    return feat, ctx, model_w0(sd["motion_estimation.0.0.weight"], mid, dtype), sd["motion_estimation.0.0.bias"]


def test_shape_lists_reach_all_sixteen_border_classes():
    for shapes in (RING_SHAPES, OTHER_SHAPES):
        seen = set()
        for _, H, W in shapes:
            seen |= set(border_class(H, W).unique().tolist())
        assert seen == set(range(16)), sorted(set(range(16)) - seen)
    c = border_class(3, 4)
    assert c.tolist() == [[10, 11, 11, 9], [14, 15, 15, 13], [6, 7, 7, 5]] and border_class(1, 1).item() == 0 and border_class(2, 1).tolist() == [[8], [4]]


@pytest.mark.parametrize("mid", [64, 8])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_pass_through_weights_return_a0_exactly(mid, dtype):
    """cpu_kernel's a0 through motion_estimation.1 / .2 as the oracle computes them (fp32 convolution, ReLU behind .1) with the
    selector weights: torch.equal with a0, every channel - and with the real .1 weights the same head returns the oracle's a1."""
    shape = (2, 5, 7)
    feat, ctx, w0m, b0 = case(mid, dtype, shape)
    sd = oracle_taps(mid, shape)[0]
    a0, _ = cpu_kernel(feat, ctx, w0m, b0, dtype)
    assert (a0 > 0).any() and (a0 >= 0).all()

    def run(sd_k):
        a1 = F.relu(oracle.conv3x3(a0, sd_k["motion_estimation.1.0.weight"], sd_k["motion_estimation.1.0.bias"]))
        return oracle.conv3x3(a1, sd_k["motion_estimation.2.weight"], sd_k["motion_estimation.2.bias"])
    assert torch.equal(assemble(run, sd, mid, keep_m1=False), a0)
    a1 = F.relu(oracle.conv3x3(a0, sd["motion_estimation.1.0.weight"], sd["motion_estimation.1.0.bias"]))
    assert torch.equal(assemble(run, sd, mid, keep_m1=True), a1)
    part = assemble(run, sd, mid, keep_m1=False, ks=(1, 3))
    assert torch.equal(part[:, [2, 3, 6, 7]], a0[:, [2, 3, 6, 7]]) and torch.isnan(part[:, [0, 1, 4, 5]]).all()


@pytest.mark.parametrize("mid,dtype,shape", CASES, ids=case_id)
def test_clean_cpu_kernel_is_inside_the_a0_gates(mid, dtype, shape):
    """measured: err / bound max up to 0.92 in the 16-bit types (the store's half unit; 0.41 in fp16 at mid 64, where the 2 n rounded
    products of the 128-channel model weigh more), <= 0.005 in fp32; mismatches <= 0.19 %, one unit."""
    feat, ctx, w0m, b0 = case(mid, dtype, shape)
    if shape[0] == 2:
        assert (ctx[0] != ctx[1]).all()
    a0, touched = cpu_kernel(feat, ctx, w0m, b0, dtype)
    assert not touched.any()
    ratio, share, units = gate_figures(a0, *a0_model(feat, ctx, w0m, b0, dtype), dtype)
    print(f"mid {mid} {dtype} {shape}: err / bound max {ratio.max().item():.3f}; mismatches {100 * share:.3f} % (<= {units:.0f} units)")
    assert ratio.max().item() <= 1.0 and share <= MISMATCH_CAP and units <= 1.0


@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("mid,dtype,shapes", CONFIGS, ids=case_id)
def test_every_mutation_is_outside_the_a0_bound(mid, dtype, shapes, name):
    """Per shape of the list the mutation touches: the gate fails (err / bound > 1 somewhere), and of the LIVE elements of the touched
    pixels - reference or mutated value above zero; where both are clamped by the ReLU nothing can show - at least 90 % ("interior
    class everywhere": every border pixel is touched) or at least half (every other mutation) lie outside the bound.  Every mutation
    must touch at least one shape of every list."""
    need = 0.9 if name == "interior class everywhere" else 0.5
    seen = 0
    for shape in shapes:
        feat, ctx, w0m, b0 = case(mid, dtype, shape)
        bad, touched = cpu_kernel(feat, ctx, w0m, b0, dtype, hook=MUTATIONS[name])
        if not touched.any():      # (one sample, one pixel, one row or one column: some mutations change nothing there)
            continue
        ref, bound, d = a0_model(feat, ctx, w0m, b0, dtype)
        ratio = gate_figures(bad, ref, bound, d, dtype)[0]
        live = touched.unsqueeze(1) & ((ref > 0) | (bad > 0))
        if not live.any():
            continue
        seen += 1
        share = (ratio[live] > 1.0).double().mean().item()
        print(f"{name}, mid {mid} {dtype} {shape}: {int(live.sum())} live touched elements, {100 * share:.1f} % outside the bound, median {ratio[live].median().item():.0f}x")
        assert ratio.max().item() > 1.0 and share >= need, (name, shape, share)
    assert seen > 0
