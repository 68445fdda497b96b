"""The window-free route of the one-launch ModulatedDeformConvPack (deform_gather3.inl; include/emavfi.h, EMAVFI_ROUTE_GATHER) and the
per-block route selection of the forward (emavfi_forward_routed, EMA_VFI.pack_policy).

  * the gather route against the oracle block under test_gpu_mdcn's derived gates (hard bound, z rms <= 1, z max <= 6): both 16-bit
    dtypes, every input form the forward hands over, ragged shapes and borders, offsets from +-0.3 to +-30 px, saturated mask logits;
  * bit-identity with the window route wherever that one's census shows no fix-up group, and identical census rows at any offsets;
  * the full forward under pack_policy "gather" on the reference-run fixtures, under test_gpu_parity's gates for the window route;
  * "window" / mask 0 equal emavfi_forward; graph capture; the pipelined forward."""
import random

import pytest
import torch

from emavfi import lib, synth
from test_gpu_mdcn import DEV, error_model, make_case, storage_round, weight_round
from test_gpu_parity import load_golden, make_model, psnr

pytestmark = pytest.mark.gpu

FORMS = [(0, "plain"), (lib.MDCN_SPLIT_TAIL, "split tail"), (lib.MDCN_IN_F16, "in f16"), (lib.MDCN_IN_F16 | lib.MDCN_OUT_F16, "in+out f16"),
         (lib.MDCN_SPLIT_TAIL | lib.MDCN_IN_F16, "split tail + in f16")]


def forms_of(dtype):
    return FORMS if dtype == "bf16" else [f for f in FORMS if not f[0] & (lib.MDCN_IN_F16 | lib.MDCN_OUT_F16)]


def stored(case, dtype, flags):
    x, ow, ob, dw, db = case
    xs = storage_round(x, dtype, as_f16=bool(flags & lib.MDCN_IN_F16))
    return xs, weight_round(ow, dtype), ob, weight_round(dw, dtype), db


def run(dtype, case, flags, route):
    return lib.mdcn(*(t.to(DEV) for t in case), dtype=dtype, flags=flags, route=route).cpu()


def gate(dtype, case, flags=0, label=""):
    """test_gpu_mdcn.run_and_gate on the gather route"""
    xs, ows, ob, dws, db = s = stored(case, dtype, flags)
    out_f16 = bool(flags & lib.MDCN_OUT_F16)
    store_eps = 2.0 ** -11 if (dtype == "fp16" or out_f16) else 2.0 ** -8
    got = run(dtype, s, flags, "gather")
    ref, hard, sigma = error_model(xs, ows, ob, dws, db, store_eps)
    assert got.shape == ref.shape and torch.isfinite(got).all(), label
    err = (got - ref).abs().double()
    ratio = (err / hard.double()).max().item()
    z = err / sigma.double()
    zr, zm = z.pow(2).mean().sqrt().item(), z.max().item()
    print(f"gather {label}: max err {err.max().item():.3e}; err / hard bound max {ratio:.3f}; z rms {zr:.3f} max {zm:.2f}")
    assert ratio <= 1.0, f"{label}: an element exceeds the worst-case bound ({ratio:.3f}x)"
    assert zr <= 1.0 and zm <= 6.0, f"{label}: error distribution wider than the rounding model (z rms {zr:.3f}, max {zm:.2f})"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_route_matches_the_oracle_block(dtype):
    rng = random.Random(7 if dtype == "bf16" else 8)
    shapes = [(2, 75, 131), (1, 1, 40), (1, 33, 1), (1, 5, 7), (3, 16, 16)] + [(rng.randint(1, 3), rng.randint(1, 150), rng.randint(1, 200)) for _ in range(3)]
    for k, (B, H, W) in enumerate(shapes):
        flags, name = forms_of(dtype)[k % len(forms_of(dtype))]
        gate(dtype, make_case(300 + k, B, 67, H, W), flags, f"{dtype} {B}x{H}x{W} {name}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_route_far_offsets_and_saturated_masks(dtype):
    """Offsets from +-0.3 px to +-30 px (taps pushed far outside, out of the image near the border), mask logits at +-15."""
    for k, (ws, bs) in enumerate(((0.005, 0.3), (0.05, 1.5), (0.4, 8.0), (1.0, 30.0))):
        for flags, name in forms_of(dtype):
            gate(dtype, make_case(400 + k, 2, 67, 37, 53, off_w_scale=ws, off_b_scale=bs), flags, f"{dtype} offsets +-{bs} {name}")
    for far, taps in ((7.0, (2, 5, 8)), (30.0, (0, 4))):
        gate(dtype, make_case(int(far), 1, 67, 40, 64, far_taps=taps, far=far), 0, f"{dtype} far {far} px taps {taps}")
    gate(dtype, make_case(77, 1, 67, 9, 70, far_taps=(0, 8), far=40.0), 0, f"{dtype} far 40 px (9-row image)")
    gate(dtype, make_case(5, 1, 67, 24, 40, mask_logit=15.0), 0, f"{dtype} mask logits +-15")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_equals_window_where_nothing_leaves_the_window(dtype):
    for k, (B, H, W) in enumerate(((1, 16, 16), (2, 37, 53), (1, 5, 7), (3, 48, 80), (1, 1, 40))):
        for flags, name in forms_of(dtype):
            s = stored(make_case(500 + k, B, 67, H, W, off_w_scale=0.005, off_b_scale=0.3), dtype, flags)
            win = run(dtype, s, flags, "window")
            row = lib.mdcn_census(B, 67, H, W, dtype=dtype, flags=flags, device=DEV)[0]
            assert row["fixup_wave_taps"] == 0, (name, row)
            gat = run(dtype, s, flags, "gather")
            assert torch.equal(win.view(torch.int32), gat.view(torch.int32)), f"{dtype} {B}x{H}x{W} {name}: not bit-identical"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_both_routes_report_the_same_census(dtype):
    for k, (ws, bs) in enumerate(((0.005, 0.3), (0.15, 3.0), (0.4, 8.0))):
        s = stored(make_case(600 + k, 2, 67, 37, 53, off_w_scale=ws, off_b_scale=bs), dtype, 0)
        rows = {}
        for route in ("window", "gather"):
            run(dtype, s, 0, route)
            rows[route] = lib.mdcn_census(2, 67, 37, 53, dtype=dtype, device=DEV)[0]
        print(dtype, bs, rows)
        assert rows["window"] == rows["gather"]
        if bs >= 3.0:
            assert rows["gather"]["fixup_wave_taps"] > 0


@pytest.mark.parametrize("fixture", ["large_offsets.npz:off", "large_offsets16.npz:off16"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_forward_gather_policy_vs_reference_run(dtype, fixture):
    """test_gpu_parity.test_forward_large_offsets_vs_reference_run's gates, every block on the gather route."""
    fname, tag = fixture.split(":")
    g = load_golden(fname)
    B, H, W, seed, kind = (int(v) for v in g[f"{tag}.meta"])
    std, bias = (float(v) for v in g[f"{tag}.recipe"])
    sd = synth.synthetic_state_dict(seed=0, offset_std=std, offset_bias=bias)
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "natural")
    m = make_model(sd, dtype=dtype)
    m.pack_policy = "gather"
    with torch.no_grad():
        out = m(f1.to(DEV), f2.to(DEV))
    got = out.contiguous().view(-1).cpu()[torch.from_numpy(g[f"{tag}.pos.out"])]
    ref = torch.from_numpy(g[f"{tag}.val.out"])
    p, err = psnr(got, ref), (got - ref).abs().max().item()
    print(f"gather policy, large offsets ({tag}), {dtype}: PSNR {p:.1f} dB, max-abs {err:.3e}")
    min_psnr, max_abs = {"bf16": (52.0, 2.5e-2), "fp16": (68.0, 4e-3)}[dtype]
    assert p >= min_psnr and err <= max_abs
    rows = m.pack_census()
    assert all(r is not None and r["route"] == "gather" and r["fixup_share"] > 0.05 for r in rows)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_forward_gather_policy_config1_rubberwhale(dtype):
    """cfg1_rubberwhale_256 with every block gathered: equal to the window policy within the 16-bit rounding class of the window route
    itself (the headline offsets stay inside the window, so the frames are bit-identical)."""
    sd = synth.synthetic_state_dict(seed=0)
    f1, f2 = synth.synthetic_frames(3, 1, 256, 256, "natural")
    outs = {}
    for pol in ("window", "gather"):
        m = make_model(sd, dtype=dtype)
        m.pack_policy = pol
        with torch.no_grad():
            outs[pol] = m(f1.to(DEV), f2.to(DEV)).cpu()
        rows = m.pack_census()
    if all(r["fixup_wave_taps"] == 0 for r in rows):
        assert torch.equal(outs["window"], outs["gather"])
    else:
        assert (outs["window"] - outs["gather"]).abs().max().item() <= 4e-3


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_window_policy_and_mask_zero_equal_emavfi_forward(dtype):
    sd = synth.synthetic_state_dict(seed=0)
    f1, f2 = (t.to(DEV) for t in synth.synthetic_frames(4, 2, 64, 96, "natural"))
    m = make_model(sd, dtype=dtype)
    assert m.pack_policy == "window"
    with torch.no_grad():
        a = m(f1, f2)
        packed = m.packed_weights(lib.dtype_code(dtype), f1.device)
        L = lib.load()
        nws = L.emavfi_workspace_bytes(3, 64, 3, 2, 64, 96, lib.dtype_code(dtype))
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        b = torch.empty_like(f1)
        lib.check(L.emavfi_forward_routed(3, 64, 3, packed.data_ptr(), packed.numel(), f1.data_ptr(), f2.data_ptr(), b.data_ptr(), ws.data_ptr(),
                                          nws, 2, 64, 96, lib.dtype_code(dtype), None, None, None, 0, 0, lib._stream()), "emavfi_forward_routed")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert lib.forward_launches(3, 64, 3, 2, 64, 96, dtype, gather_blocks=0) == lib.forward_launches(3, 64, 3, 2, 64, 96, dtype)


def _scaled_sd(s_px):
    """the synthetic recipe with every block's offsets at about +-s_px"""
    return synth.synthetic_state_dict(seed=0, offset_std=0.5 * s_px, offset_bias=0.5 * s_px)


def test_gather_policy_raises_without_a_one_launch_pack():
    f1, f2 = (t.to(DEV) for t in synth.synthetic_frames(5, 1, 32, 48, "natural"))
    m = make_model(synth.synthetic_state_dict(seed=0), dtype="fp32")
    with torch.no_grad():
        m.pack_policy = "gather"
        with pytest.raises(RuntimeError, match="no gather route"):
            m(f1, f2)


def _capture(m, f1, f2):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            m(f1, f2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = m(f1, f2)
    return g, out


@pytest.mark.parametrize("policy", ["gather"])
def test_graph_capture_under_routed_policies(policy):
    f1, f2 = (t.to(DEV) for t in synth.synthetic_frames(6, 2, 64, 96, "natural"))
    m = make_model(_scaled_sd(8.0), dtype="bf16")
    m.pack_policy = policy
    g, out = _capture(m, f1, f2)
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = m(f1, f2)
    assert torch.equal(out, eager)
    n1, n2 = (t.to(DEV) for t in synth.synthetic_frames(7, 2, 64, 96, "natural"))
    f1.copy_(n1)
    f2.copy_(n2)
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager = m(f1, f2)
    assert torch.equal(out, eager)


def test_pipelined_forward_under_gather_policy():
    f1, f2 = (t.to(DEV) for t in synth.synthetic_frames(8, 4, 64, 96, "natural"))
    m = make_model(_scaled_sd(8.0), dtype="bf16")
    m.pack_policy = "gather"
    with torch.no_grad():
        one = m(f1, f2)
        m.pipeline = 2
        a = m(f1, f2)
        b = m(f1, f2)
    torch.cuda.synchronize()
    assert torch.equal(one, a) and torch.equal(a, b)
