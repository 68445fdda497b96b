"""EMAVFI_F32X3 (round 6): fp32-ACCURATE contractions on the f16 matrix pipe - every nn.Conv2d / nn.Linear as the
three-term split x_hi w_hi + x_hi w_lo + x_lo w_hi (IEEE f16 halves, exact products, fp32 accumulation), activations stored as their
two f16 halves, the warp / pool and the sampling geometry of the three deform_conv2d the fp32 ones (their contraction: the same split at
the reference width, exact fp32 elsewhere; gated per element in tests/test_gpu_fp32x3_rounding_model.py) - held to THE SAME GATES as the exact
fp32 mode on every reference-run fixture: <= 1e-3 max-abs on the frame (BASELINE.json), <= 5e-4 relative on every stage.  It is a
separately named mode: `fp32` stays the parity mode everywhere else.  Reference: ema_vfi.py:7-14 (conv / conv_block), :110-147."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from emavfi import EMA_VFI, lib, synth
from oracle import emavfi_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STAGES = ("feat", "ctx", "flow", "warped", "fused_0", "fused_1", "fused_2", "out")


def make_model(sd, mid=64, dtype="fp32x3"):
    m = EMA_VFI(mid_channels=mid, compute_dtype=dtype).to(DEV).eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.mark.parametrize("Cin,Cout,stride,H,W", [(6, 64, 1, 33, 47), (64, 64, 1, 40, 70), (67, 27, 1, 21, 35), (67, 64, 1, 19, 66), (64, 128, 2, 37, 53),
                                                 (128, 256, 2, 18, 30), (256, 256, 1, 9, 14), (64, 32, 1, 16, 40), (32, 3, 1, 16, 40), (64, 2, 1, 8, 33),
                                                 (8, 8, 1, 12, 20), (11, 27, 1, 12, 20)])
def test_conv3x3_split_is_fp32_accurate(Cin, Cout, stride, H, W):
    """One layer through the stage entry (the generic tile kernel on 3 virtual chunks per real one) against the float64 convolution:
    the error class of an fp32 convolution - measured 3e-7 .. 1.4e-6 of the largest output (ATen's fp32 convolution, which sums in blocks:
    2.5e-7 .. 3.9e-7; the MFMA accumulates its up to 6 912 exact products in one fp32 chain per output), 250-1000 x below the f16 kernel."""
    g = torch.Generator().manual_seed(Cin * 1000 + Cout)
    x = torch.randn(2, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    truth = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
    scale = truth.abs().max().item()
    e32 = (F.conv2d(x, w, b, stride=stride, padding=1).double() - truth).abs().max().item() / scale
    got = lib.conv3x3(x.to(DEV), w.to(DEV), b.to(DEV), stride=stride, dtype="fp32x3").cpu()
    e3 = (got.double() - truth).abs().max().item() / scale
    try:
        e16 = (lib.conv3x3(x.to(DEV), w.to(DEV), b.to(DEV), stride=stride, dtype="fp16").cpu().double() - truth).abs().max().item() / scale
    except RuntimeError:      # (the f16 stage entry has no channels-last form of the <= 4-channel planar heads)
        e16 = float("inf")
    print(f"{Cin}->{Cout}/{stride}: fp32 (ATen) {e32:.2e}  f16x3 {e3:.2e}  f16 {e16:.2e}")
    assert e3 <= 3e-6 and e3 <= 8 * e32 and e3 * 100 <= e16
    relu = lib.conv3x3(x.to(DEV), w.to(DEV), b.to(DEV), stride=stride, act=lib.ACT_RELU, dtype="fp32x3").cpu()
    assert (relu.double() - truth.clamp(min=0)).abs().max().item() / scale <= 3e-6


@pytest.mark.parametrize("name", ["tiny_mid8_24x40.npz", "tiny_mid8_23x37.npz"])
def test_forward_tiny_all_stages(name):
    g = load_golden(name)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    m = make_model(sd, mid=8)
    with torch.no_grad():
        out, taps = m(torch.from_numpy(g["frame1"]).to(DEV), torch.from_numpy(g["frame2"]).to(DEV), return_taps=True)
    for k in STAGES:
        ref = torch.from_numpy(g["tap." + k])
        err = (taps[k].cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err <= 2e-4, (k, err)
    assert (out.cpu() - torch.from_numpy(g["tap.out"])).abs().max().item() <= 1e-3


def _large(fname, tag, kind=None, recipe=None):
    g = load_golden(fname)
    B, H, W, seed, k = (int(v) for v in g[f"{tag}.meta"])
    sd = synth.synthetic_state_dict(seed=0) if recipe is None else synth.synthetic_state_dict(seed=0, offset_std=recipe[0], offset_bias=recipe[1])
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "stress" if k else "natural")
    m = make_model(sd)
    with torch.no_grad():
        out, taps = m(f1.to(DEV), f2.to(DEV), return_taps=True)
    worst = {}
    for s in STAGES:
        got = taps[s].contiguous().view(-1).cpu()[torch.from_numpy(g[f"{tag}.pos.{s}"])]
        ref = torch.from_numpy(g[f"{tag}.val.{s}"])
        err = (got - ref).abs().max().item()
        lim = 1e-3 if s == "out" else 5e-4 * max(1.0, ref.abs().max().item())
        worst[s] = err / lim
        assert err <= lim, (tag, s, err, lim)
    print(f"fp32x3 {tag}: worst stage at {max(worst.values()):.3f} of its fp32 gate ({max(worst, key=worst.get)}); frame max-abs {worst['out'] * 1e-3:.2e}")
    return out


@pytest.mark.parametrize("tag", ["256", "256s", "720", "odd", "1080"])
def test_forward_reference_run_samples_under_the_fp32_gates(tag):
    """The reference's own forward at 256^2 (natural, stress), 1280x720, 203x331 (odd, stress, B = 2) and 1920x1080: sampled pixels of
    every stage, the exact-fp32 mode's gates."""
    _large({"1080": "large_1080.npz", "odd": "large_odd.npz"}.get(tag, "large_checks.npz"), tag)


@pytest.mark.parametrize("fixture", ["large_offsets.npz:off", "large_offsets16.npz:off16"])
def test_forward_large_offsets_under_the_fp32_gates(fixture):
    fname, tag = fixture.split(":")
    g = load_golden(fname)
    _large(fname, tag, recipe=tuple(float(v) for v in g[f"{tag}.recipe"]))


def test_forward_config1_rubberwhale_and_agreement_with_the_exact_mode():
    g = load_golden("cfg1_rubberwhale_256.npz")
    u8 = g["triplet_u8"]
    f1, f2 = synth._to_model_range(u8[0:1]), synth._to_model_range(u8[2:3])
    sd = synth.synthetic_state_dict(seed=0)
    with torch.no_grad():
        out3 = make_model(sd)(f1.to(DEV), f2.to(DEV)).cpu()
        out32 = make_model(sd, dtype="fp32")(f1.to(DEV), f2.to(DEV)).cpu()
    assert (out3 - torch.from_numpy(g["out"])).abs().max().item() <= 1e-3
    d = (out3 - out32).abs().max().item()
    print(f"fp32x3 vs exact fp32 on RubberWhale 256: max-abs {d:.2e}")
    assert d <= 2e-5 and out3.dtype == torch.float32 and 0.0 <= out3.min().item() and out3.max().item() <= 1.0


def test_properties_at_the_benchmarked_size():
    """B = 8 x 720p: run-to-run bit-exact, a sample of the batch equals the same sample alone bit for bit, and the frame agrees with the
    exact-fp32 mode's to 2e-5."""
    sd = synth.synthetic_state_dict(seed=0)
    f1, f2 = synth.fast_frames(55, 8, 720, 1280, device=DEV)
    m = make_model(sd)
    with torch.no_grad():
        a = m(f1, f2)
        b = m(f1, f2)
        assert torch.equal(a, b) and torch.isfinite(a).all()
        one = m(f1[5:6].contiguous(), f2[5:6].contiguous())
        assert torch.equal(a[5:6], one)
        ref = make_model(sd, dtype="fp32")(f1[5:6].contiguous(), f2[5:6].contiguous())
    d = (one - ref).abs().max().item()
    print(f"fp32x3 vs exact fp32, one 720p frame of the batch: max-abs {d:.2e}")
    assert d <= 2e-5


def test_stage_entries_refuse_the_mode_they_do_not_have():
    x = torch.randn(1, 67, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="F32X3"):
        lib.mdcn(x, torch.randn(27, 67, 3, 3, device=DEV), torch.zeros(27, device=DEV), torch.randn(67, 67, 3, 3, device=DEV), None, dtype="fp32x3")


@pytest.mark.parametrize("mid,B,H,W", [(64, 1, 1, 40), (64, 1, 33, 1), (64, 2, 5, 7), (64, 1, 75, 131), (16, 2, 23, 37), (32, 1, 24, 40), (8, 1, 9, 70)])
def test_forward_ragged_sizes_and_other_widths_against_the_oracle(mid, B, H, W):
    """Images smaller than a tile, one row, one column, ragged remainders, and the narrower models (generic fp32 deformable kernel instead
    of the LDS-window one): the frame against the CPU oracle under the fp32 gate, the flow and the fused tensors at 5e-4 relative."""
    sd = synth.synthetic_state_dict(seed=3, mid_channels=mid)
    f1, f2 = synth.synthetic_frames(40 + H, B, H, W, "natural")
    ref = {}
    oracle.forward(sd, f1, f2, taps=ref)
    m = make_model(sd, mid=mid)
    with torch.no_grad():
        out, taps = m(f1.to(DEV), f2.to(DEV), return_taps=True)
    assert (out.cpu() - ref["out"]).abs().max().item() <= 1e-3
    for k in ("feat", "flow", "fused_2"):
        err = (taps[k].cpu() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item())
        assert err <= 5e-4, (k, err)


def test_forward_is_graph_capturable_and_replays_bit_identically():
    """The split mode's launch sequence (21 launches and the census clear, a launch of its own) under torch.cuda.graph: the replay equals the eager result bit for bit,
    also with new frames written into the captured inputs."""
    sd = synth.synthetic_state_dict(seed=0)
    m = make_model(sd)
    f1, f2 = (t.to(DEV) for t in synth.synthetic_frames(61, 2, 72, 104, "natural"))
    g1, g2 = (t.to(DEV) for t in synth.synthetic_frames(62, 2, 72, 104, "stress"))
    side = torch.cuda.Stream()
    with torch.no_grad():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                eager = m(f1, f2).clone()
            eager2 = m(g1, g2).clone()
        torch.cuda.current_stream().wait_stream(side)
        a, b = f1.clone(), f2.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(a, b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        a.copy_(g1); b.copy_(g2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager2)
