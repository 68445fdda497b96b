"""Pins oracle/emavfi_oracle.py to vectors captured from the reference's own
EMA_VFI.forward (tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from emavfi import synth
from oracle import emavfi_oracle as oracle

STAGES = ("feat", "ctx", "flow", "warped", "fused_0", "fused_1", "fused_2", "out")


@pytest.mark.parametrize("name", ["tiny_mid8_24x40.npz", "tiny_mid8_23x37.npz"])
def test_tiny_every_stage(name):
    g = load_golden(name)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    # the committed weights are exactly what the hash generator produces
    regen = synth.synthetic_state_dict(seed=11 if "24x40" in name else 12, mid_channels=8)
    for k, v in regen.items():
        assert torch.equal(v, sd[k]), k
    taps = {}
    oracle.forward(sd, torch.from_numpy(g["frame1"]), torch.from_numpy(g["frame2"]), taps=taps)
    for k in STAGES:
        assert np.abs(taps[k].numpy() - g["tap." + k]).max() <= 1e-5, k
    # channel routing of the pack (ema_vfi.py:57-59) against the hooked raw offset_conv output
    for i in range(3):
        raw = torch.from_numpy(g[f"tap.raw_{i}"])
        assert torch.allclose(taps[f"offset_{i}"], torch.cat([raw[:, 0:9], raw[:, 18:27]], 1), atol=1e-5)
        assert torch.allclose(taps[f"mask_{i}"], torch.sigmoid(raw[:, 9:18]), atol=1e-6)


def test_config1_rubberwhale_crop():
    """BASELINE.json configs[0]: one 256x256 Middlebury triplet through the CPU forward."""
    g = load_golden("cfg1_rubberwhale_256.npz")
    u8 = g["triplet_u8"]
    f1, f2 = synth._to_model_range(u8[0:1]), synth._to_model_range(u8[2:3])
    assert f1.min() >= -2.12 and f1.max() <= 2.65
    taps = {}
    out = oracle.forward(synth.synthetic_state_dict(seed=0), f1, f2, taps=taps)
    assert np.abs(out.numpy() - g["out"]).max() <= 1e-5
    assert np.abs(taps["flow"].numpy() - g["flow"]).max() <= 1e-4
    for k in STAGES:
        t = taps[k].double()
        got = np.array([t.mean().item(), t.pow(2).sum().sqrt().item(), t.abs().max().item()])
        assert np.allclose(got, g["stats." + k], rtol=1e-5, atol=1e-6), k


def test_large_256_stress_samples():
    g = load_golden("large_checks.npz")
    B, H, W, seed, kind = (int(v) for v in g["256s.meta"])
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "stress" if kind else "natural")
    taps = {}
    oracle.forward(synth.synthetic_state_dict(seed=0), f1, f2, taps=taps)
    for k in STAGES:
        got = taps[k].contiguous().view(-1)[torch.from_numpy(g[f"256s.pos.{k}"])].numpy()
        assert np.abs(got - g[f"256s.val.{k}"]).max() <= 2e-5 * max(1.0, np.abs(got).max()), k


def test_large_odd_samples():
    """mid=64 at 203x331 (B = 2, stress input, flows up to 16 px): odd in both dimensions, so every pyramid level (102x166, 51x83) and
    every tile grid ends in a partial tile.  The oracle against the sampled pixels of the reference's own run
    (tests/golden/large_odd.npz, `make_golden.py odd`)."""
    g = load_golden("large_odd.npz")
    B, H, W, seed, kind = (int(v) for v in g["odd.meta"])
    assert (B, H, W, kind) == (2, 203, 331, 1)
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "stress")
    taps = {}
    oracle.forward(synth.synthetic_state_dict(seed=0), f1, f2, taps=taps)
    for k in STAGES:
        got = taps[k].contiguous().view(-1)[torch.from_numpy(g[f"odd.pos.{k}"])].numpy()
        assert np.abs(got - g[f"odd.val.{k}"]).max() <= 2e-5 * max(1.0, np.abs(got).max()), k


@pytest.mark.parametrize("fname,tag,p99", [("large_offsets.npz", "off", 4.0), ("large_offsets16.npz", "off16", 10.0)])
def test_large_offsets_samples(fname, tag, p99):
    """(round 6: also large_offsets16.npz, `make_golden.py offsets16` - offsets spanning about +-16 px, p99 11.3, max 23.8.)
    mid=64 at 120x200 with the offset convolutions scaled (synthetic_state_dict(offset_std = 3, offset_bias = 3)) so that the
    deformable offsets span about +-8 px: the oracle against the sampled pixels of the reference's own run
    (tests/golden/large_offsets.npz, `make_golden.py offsets`; replayed on the GPU, where these offsets drive the pack kernels through their
    fix-up loop, in tests/test_gpu_parity.py)."""
    g = load_golden(fname)
    B, H, W, seed, kind = (int(v) for v in g[f"{tag}.meta"])
    std, bias = (float(v) for v in g[f"{tag}.recipe"])
    assert (B, H, W, kind) == (1, 120, 200, 0) and g[f"{tag}.abs_offset_quantiles"][1] > p99   # p99 of |offset| beyond the R = 2 window
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "natural")
    taps = {}
    oracle.forward(synth.synthetic_state_dict(seed=0, offset_std=std, offset_bias=bias), f1, f2, taps=taps)
    for k in STAGES:
        got = taps[k].contiguous().view(-1)[torch.from_numpy(g[f"{tag}.pos.{k}"])].numpy()
        assert np.abs(got - g[f"{tag}.val.{k}"]).max() <= 2e-5 * max(1.0, np.abs(got).max()), k


@pytest.mark.parametrize("name,exact", [("amp_mid8_23x37.npz", True), ("amp_mid64_40x56.npz", False)])
def test_autocast_restatement_against_the_reference_forward_under_cpu_autocast(name, exact):
    """SURVEY 8f-2 / VERDICT r3 item 6b.  inference.py:159 runs the forward under torch.cuda.amp.autocast(); no GPU run of the reference
    exists here, but its forward DOES execute under torch.autocast("cpu", dtype=torch.float16) (tests/golden/make_golden.py amp: the
    reference's own forward / warp / pack, the DCN stand-in behind torchvision's cast-to-float autocast wrapper).  For every op on
    this path the CPU and CUDA autocast lists of torch 2.10 agree - conv2d / linear: lower precision (weight and bias cast);
    grid_sampler: fp32; cat: promote to the widest input; relu / sigmoid / tanh / adaptive_avg_pool2d / `+ 1` / `/ 2`: not listed, run
    in the dtype they receive - so the stage dtypes recorded in the fixture are the ones oracle.forward_autocast16 (the CUDA policy,
    restated) assumes, and its VALUES can be held to the executed run: bit for bit at mid_channels 8; at mid_channels 64 within a
    few fp16 steps - oneDNN's fp16 convolution sums its 576..1152 products in another order than F.conv2d on the fp16-rounded
    fp32 inputs does (5 % of `feat` differs by one step), which is the freedom any GPU convolution has as well."""
    g = load_golden(name)
    mid, B, H, W, seed, kind = (int(v) for v in g["meta"])
    sd = synth.synthetic_state_dict(seed=seed, mid_channels=mid)
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "stress" if kind else "natural")
    # the dtypes the reference's modules produced under autocast: what the restatement's comments claim
    dt = dict(s.split("=") for s in g["dtypes"].tolist())
    assert all(dt[k] == "float16" for k in dt if k.startswith(("feat_ext", "context_encoding", "motion_estimation", "reconstruction")))
    assert dt["warp"] == "float32" and dt["out"] == "float16"
    for i in range(3):
        assert dt[f"attention_blocks.{i}.offset_conv"] == "float16" and dt[f"attention_blocks.{i}.dcn_v2"] == "float32" and dt[f"attention_blocks.{i}"] == "float32"
    taps = {}
    out = oracle.forward_autocast16(sd, f1, f2, taps=taps)
    assert torch.equal(out, out.half().float())        # the frame is an fp16 tensor's worth of values
    for k in STAGES:
        want, got = torch.from_numpy(g["tap." + k]), taps[k]
        if str(g["dtype." + k]) == "float16":
            assert torch.equal(got, got.half().float()), k
        d = (got - want).abs()
        if exact:
            assert d.max().item() == 0.0, (k, d.max().item())
        else:
            # steps of the stage's own fp16 grid at its magnitude (fp32 stages: of an fp16 grid too - their inputs are fp16 values)
            step = 2.0 ** -10 * max(1.0, float(want.abs().max()))
            assert d.max().item() <= 6 * step and d.mean().item() <= 0.2 * step, (k, d.max().item() / step, d.mean().item() / step)


def test_large_1080_fixture_is_consistent_with_the_720_one():
    """large_1080.npz (reference forward at 1920x1080, BASELINE configs[4]'s frame size; replayed on the GPU in
    tests/test_gpu_parity.py): same generator, same weights - a cheap CPU-side sanity check of the file itself."""
    g = load_golden("large_1080.npz")
    B, H, W, seed, kind = (int(v) for v in g["1080.meta"])
    assert (B, H, W, kind) == (1, 1080, 1920, 0)
    assert g["1080.val.out"].min() >= 0.0 and g["1080.val.out"].max() <= 1.0 and g["1080.val.out"].shape == (4096,)
    assert g["1080.pos.feat"].max() < 64 * H * W and g["1080.stats.flow"][2] > 1.0
    # warped samples are bilinear blends of frame2 pixels: inside frame2's range
    _, f2 = synth.synthetic_frames(seed, B, 8, 8, "natural")
    assert np.abs(g["1080.val.warped"]).max() <= 2.7
