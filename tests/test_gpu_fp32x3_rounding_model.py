"""The three-term f16 split mode (`fp32x3`, EMAVFI_F32X3) gated PER ELEMENT at the precision it claims, against the float64 model of
tests/rounding_model.py (conv_model_x3: derived there, nothing tuned; tests/test_rounding_model_cpu.py shows on the CPU that a correct
kernel is inside its gates and that a lost low half, a missing term, a low half from the neighbouring pixel, a dropped output lo and a
w_lo in the wrong tap are outside, at the cases run here).  tests/test_gpu_fp32x3.py holds the mode to the exact mode's parity gates
(5e-4 of a stage, 1e-3 on the frame): three to four orders of magnitude above one low half (2^-11), which those gates cannot see.

Everything runs through lib.conv3x3(..., dtype="fp32x3") and the forward: the mode has ONE convolution route (conv_geometry(x3 = true):
the tile kernel on virtual chunks 3 c + t), so the stage entry runs the kernel, the weight packing (pack_conv's x3 branch) and the layout
kernels (nchw_to_cl_x3 / cl_to_nchw_x3) the forward runs.
  * the split and the layouts by EQUALITY: a centre-tap identity returns carried(x) bit for bit over a sweep of every binade, ties,
    subnormal halves and the largest f16 number;
  * impulse known answers with ZERO tolerance: every (cout, cin, tap) of w_hi AND w_lo, x_hi and x_lo (rounding_model.impulse_case_x3).
    One pair cannot have it: the planar 32 -> 3 head exists with tanh01 only (the library builds no planar kernel without it), so its
    impulses are held to tanh01 of the exact value within TANH_TERM = 2^-21, what the kernel's tanh may be off by;
  * random layers under the two gates - err / bound <= 1 for EVERY element, rms(z) <= 1 and max |z| <= 6 - at every channel pair the
    forward runs, at tile remainders, at three magnitudes;
  * the range contract's finite side;
  * the forward layer by layer on its own taps: feat, ctx, flow, fused_i, out.
measured: see MEASURED at the end of this file."""
import functools

import pytest
import torch

from conv_cases import X3_PAIRS, X3_SCALES, set_env, split_sweep, x3_act, x3_layer, x3_pair_id, x3_shapes
from emavfi import EMA_VFI, lib, synth
from rounding_model import (F16_MAX, TANH_TERM, U22, U32, Z_MAX, Z_RMS, accumulation_variance, activation, carried, chain_stats_x3, conv64, conv_model_x3,
                            impulse_case_x3, pool_linear_model_x3, terms_x3, z_gates)
import deform_model as dm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT = {"none": lib.ACT_NONE, "relu": lib.ACT_RELU, "tanh01": lib.ACT_TANH01}


def run(x, w, b, stride=1, act="none"):
    return lib.conv3x3(x.to(DEV), w.to(DEV), b.to(DEV), stride=stride, act=ACT[act], dtype="fp32x3").cpu()


def gate(got, x, w, b, stride, act, label, fails):
    """One layer's result against conv_model_x3 on the operands it read; prints the figures, appends to `fails` what is outside a gate.
    No element is excluded."""
    ref3, bound, sigma, _ = conv_model_x3(x, w, b, stride, act, with_truth=False)
    assert got.shape == ref3.shape and torch.isfinite(got).all(), label
    ratio, rms, zmax = z_gates(got, ref3, bound, sigma)
    print(f"{label}: err / bound max {ratio:.3f}; rms z {rms:.3f}; max |z| {zmax:.2f}")
    if ratio > 1.0:
        fails.append(f"{label}: an element exceeds the split model's worst case ({ratio:.3f}x)")
    if rms > Z_RMS or zmax > Z_MAX:
        fails.append(f"{label}: outside the statistical gate (rms z {rms:.3f}, max |z| {zmax:.2f})")
    return ratio, rms, zmax


# ------------------------------------------------------------------------------------------------------------ split and layouts
@pytest.mark.parametrize("C", [3, 6, 8, 16, 17, 64, 67])
def test_identity_layer_returns_the_carried_input_bit_for_bit(C, monkeypatch):
    """Cin = Cout = C, weight = the centre-tap identity (w_lo = 0), zero bias, no activation: the accumulator of output (o, y, x) is
    x_hi + x_lo of input (o, y, x) and exact zeros, i.e. carried(x), which fp32 holds exactly, and the epilogue's split of it carries
    the same value (tests/test_rounding_model_cpu.py, test_split22_properties): the output EQUALS carried(x).  x walks the operand sweep
    (conv_cases.split_sweep) with a stride coprime to its length, so every channel, pixel parity and tile position sees every kind of
    value.  C = 3 .. 67 covers a padded pixel (3, 6, 8 -> 16; 17 -> 32; 67 -> 80) and the exact ones; the shapes one pixel, one row
    wider than two tiles, a ragged tile and several tiles, B = 2.  Pins nchw_to_cl_x3, cl_to_nchw_x3, the packing of a weight whose lo
    is zero, and an epilogue that must reproduce both halves."""
    set_env(monkeypatch, {})
    sweep = split_sweep()
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    for H, W in ((1, 1), (1, 70), (5, 7), (33, 47)):
        n = 2 * C * H * W
        x = sweep[(torch.arange(n) * 37 + C + H) % sweep.numel()].view(2, C, H, W)
        got = run(x, w, torch.zeros(C))
        want = carried(x).float()
        wrong = got != want
        assert got.shape == want.shape and not wrong.any(), \
            f"C={C} {H}x{W}: {int(wrong.sum())} of {n} elements, first at {wrong.nonzero()[0].tolist()}: x {x[wrong][0].item()!r} -> {got[wrong][0].item()!r}, want {want[wrong][0].item()!r}"


IMPULSE = X3_PAIRS + [(8, 16, 2, False)]     # (8 -> 16 at stride 2: context_encoding.0 of the narrowest model)


@pytest.mark.parametrize("pair", IMPULSE, ids=x3_pair_id)
def test_impulses_return_the_three_terms_of_single_weights_exactly(pair, monkeypatch):
    """rounding_model.impulse_case_x3: impulses 1 + 3 * 2^-13 (x_hi = 1, x_lo = 3 * 2^-13), weights k + w_lo with a w_lo that differs
    between neighbouring (o, c, tap), zero bias, no activation.  Every output element is 0 or x_hi w_hi + x_hi w_lo + x_lo w_hi of ONE
    weight - at most 22 bits, exact in fp32 in any order - so the output EQUALS carried() of it: every (cout, cin, tap) of the packed
    w_hi and w_lo in their virtual chunks, and the x_lo tile of term 2.  The second image moves the field onto the last row and column;
    the stride-2 pairs see impulses on both parities.  The planar head exists with tanh01 only: tanh01 of the same values (weights / 4,
    still exact), to TANH_TERM = 2^-21 - where the head's slope (0.057 .. 0.5) times a w_lo of up to 2^-11 |w| is 2^-14 .. 2^-11."""
    cin, cout, stride, head = pair
    set_env(monkeypatch, {})
    g = torch.Generator().manual_seed(cin * 7 + cout)
    for shift in (False, True):
        x, w, want = impulse_case_x3(cin, cout, stride, shift, g, scale=0.25 if head else 1.0)
        got = run(x, w, torch.zeros(cout), stride, "tanh01" if head else "none")
        assert got.shape == want.shape and int((want != 0).sum()) >= cin
        if head:
            err = (got.double() - activation(want, "tanh01")).abs().max().item()
            assert err <= TANH_TERM, (shift, err)
            continue
        wrong = got.double() != carried(want.float())
        assert not wrong.any(), f"{pair} shift={shift}: {int(wrong.sum())} of {got.numel()} elements, first at {wrong.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------------------ random layers
@pytest.mark.parametrize("k", X3_SCALES, ids=lambda k: f"scale2^{k}")
@pytest.mark.parametrize("pair", X3_PAIRS, ids=x3_pair_id)
def test_single_layers_stay_inside_the_split_model(pair, k, monkeypatch):
    """conv_cases.x3_layer: x ~ N(0, 1) scaled per input channel by 2^-3 .. 2^3 and as a whole by 2^k (k = 0, -10: every lo subnormal,
    10: up to 3e4), w ~ N(0, 1 / (9 Cin)) - Kaiming scale, w_lo subnormal -, B = 2, `none` and `relu` alternating over the shapes
    (tile remainders in both directions; odd and even sizes under stride 2), tanh01 on the planar head.  Both gates of conv_model_x3,
    every element.  measured: see MEASURED."""
    cin, cout, stride, head = pair
    set_env(monkeypatch, {})
    fails = []
    for i, (H, W) in enumerate(x3_shapes(stride)):
        act = x3_act(pair, i)
        x, w, b = x3_layer(pair, H, W, k)
        gate(run(x, w, b, stride, act), x, w, b, stride, act, f"{x3_pair_id(pair)} {act} 2x{H}x{W} 2^{k}", fails)
    assert not fails, "\n".join(fails)


def test_inputs_up_to_the_largest_f16_number_stay_finite_and_inside_the_model(monkeypatch):
    """The range contract's finite side (include/emavfi.h): |x| up to 65504 - the sweep's top values planted into a random field scaled
    so that its largest magnitude IS 65504 - with weights at half the Kaiming scale, so that every accumulator stays below 65504 (checked on the
    model: |ref| + bound < 65504): finite, inside both gates.  (An accumulator of 65520 or more stores hi = inf: not run.)"""
    set_env(monkeypatch, {})
    fails = []
    for pair, (H, W) in (((64, 64, 1, False), (33, 47)), ((6, 64, 1, False), (5, 7)), ((64, 128, 2, False), (37, 53))):
        x, w, b = x3_layer(pair, H, W, 0)
        x = (x / x.abs().max() * F16_MAX).clamp(-F16_MAX, F16_MAX)
        top = torch.tensor([F16_MAX, -F16_MAX, torch.nextafter(torch.tensor(F16_MAX), torch.tensor(0.0)).item(), F16_MAX / 2])
        x.view(-1)[torch.arange(0, x.numel(), 97)] = top[torch.arange(0, x.numel(), 97) % 4]
        w = w / 2
        ref3, bound, _, _ = conv_model_x3(x, w, b, pair[2], "none", with_truth=False)
        assert x.abs().max().item() == F16_MAX and (ref3.abs() + bound).max().item() < F16_MAX
        gate(run(x, w, b, pair[2], "none"), x, w, b, pair[2], "none", f"range {x3_pair_id(pair)} 2x{H}x{W} (|ref| <= {ref3.abs().max().item():.0f})", fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------ the forward, on its own taps
# (mid_channels, (B, H, W)): one pixel row, an odd pooled size on one pool partial (5 x 9 = 45), one that spans two (9 x 18 = 162 >= 128),
# and the narrowest model (generic fp32 deformable kernel, pack_input_x3's 16-channel path all the same: 2 x 3 channels pad to 16);
# 3 x 4 pools ONE pixel.  natural and stress frames.
FORWARD = [(64, (1, 1, 7)), (64, (1, 17, 33)), (64, (2, 33, 70)), (8, (2, 23, 37))]
FORWARD_CASES = [(m, sh, kind) for m, sh in FORWARD for kind in ("natural", "stress")] + [(64, (1, 3, 4), "natural")]
case_id = lambda c: f"mid{c[0]}-{c[1][0]}x{c[1][1]}x{c[1][2]}-{c[2]}" if isinstance(c, tuple) else str(c)


@functools.lru_cache(maxsize=None)
def forward_case(mid, shape, kind):
    """One fp32x3 forward with taps, computed once and shared by the tests below (nothing modifies it)."""
    B, H, W = shape
    sd = synth.synthetic_state_dict(seed=6, mid_channels=mid)
    f1, f2 = synth.synthetic_frames(41, B, H, W, kind)
    model = EMA_VFI(mid_channels=mid, compute_dtype="fp32x3").to(DEV).eval()
    model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        _, taps = model(f1.to(DEV), f2.to(DEV), return_taps=True)
    names = [n for n, _, _ in lib.forward_launches(3, mid, 3, B, H, W, "fp32x3")]
    return sd, f1, f2, {k: v.float().cpu() for k, v in taps.items()}, names


def layer(sd, name, act="relu", stride=1):
    return {"w": sd[name + ".weight"].float(), "b": sd[name + ".bias"].float(), "act": act, "stride": stride}


def chain(x, layers, label, fails):
    """The layers one at a time through lib.conv3x3, each gated against conv_model_x3 on the GPU's own previous output."""
    outs, a = [], x
    for k, L in enumerate(layers):
        got = run(a, L["w"], L["b"], L["stride"], L["act"])
        gate(got, a, L["w"], L["b"], L["stride"], L["act"], f"{label} layer {k}", fails)
        outs.append(got)
        a = got
    return outs


def tap_against_last_layer(tap, chain_out, a_in, L, label, fails):
    """The forward's tensor against the model of its LAST layer on the chain's intermediate, and how it differs from the chain's own
    result.  No bit equality is asked between the two: the chain splits hi + lo of an intermediate AGAIN, which moves hi to the neighbour
    where lo was exactly half a unit (some 2^-13 of the elements) and changes the dropped lo x lo term there."""
    ratio, rms, zmax = gate(tap, a_in, L["w"], L["b"], L["stride"], L["act"], label, fails)
    differ = tap != chain_out
    share = differ.double().mean().item()
    zd = 0.0
    if differ.any():
        ref3, _, sigma, _ = conv_model_x3(a_in, L["w"], L["b"], L["stride"], L["act"], with_truth=False)
        zd = ((tap.double() - ref3).abs() / sigma)[differ].max().item()
    print(f"{label}: chain and forward differ in {100 * share:.4f} % of the elements (largest |z| of those {zd:.2f})")
    return share


@pytest.mark.parametrize("case", FORWARD_CASES[:-1], ids=case_id)
def test_feat_of_the_forward_layer_by_layer(case):
    """pack_input_x3 (frames -> [hi | lo], its 16-channel path) + feat_ext_conv1 + the feature blocks: the four layers one at a time from
    the frames, each inside both gates on the GPU's own previous output; then the forward's `feat` tap - cl_to_nchw_x3 with a pixel
    stride wider than the channels, beside the out32 side store - against the last layer's model on the chain's intermediate."""
    mid, shape, kind = case
    sd, f1, f2, taps, names = forward_case(*case)
    assert sum(n == "pack_input" for n in names) == 1
    layers = [layer(sd, "feat_ext_conv1.0")] + [layer(sd, f"feat_ext_blocks.conv_block_{i}.0") for i in range(3)]
    fails = []
    label = f"feat {case_id(case)}"
    outs = chain(torch.cat([f1, f2], dim=1), layers, label, fails)
    tap_against_last_layer(taps["feat"], outs[3], outs[2], layers[3], label + " tap", fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", FORWARD_CASES, ids=case_id)
def test_ctx_of_the_forward_from_its_feat_tap(case):
    """context_encoding: the three convolutions as a chain from the `feat` tap, each inside both gates; then the pool over the doubled
    [hi | lo] channels, the fold that adds the two sums (launch_ctx_finish with a lo offset), and the fp32 Linear (ctx_finish_kernel:
    fp32 FMAs on the fp32 weights), in float64 on the chain's own last output against the `ctx` tap: rounding_model.pool_linear_model_x3,
    its bound AND its z gates.  The forward's c2 is not a tap and is not the chain's bit for bit (tap_against_last_layer): both are
    correct kernels about the chain's float64 reference, two standard deviations of chain_stats_x3 apart in squares.
    What the bound pins: a fold that reads the wrong offset (hi twice: 2^-11 of |ctx| and up), a pool that misses or repeats pixels or
    partials.  What only the z gates pin: a pool or a fold that DROPS the lo halves, or adds those of other channels - 1e-5 of |ctx|
    at 162 pooled pixels, inside the bound, and rms z 5 .. 19 against 0.1 for a correct pool (tests/test_rounding_model_cpu.py,
    test_split_pool_and_fold_statistics_pass_a_correct_kernel_and_fail_a_lost_lo, at these pooled sizes)."""
    mid, shape, kind = case
    sd, f1, f2, taps, names = forward_case(*case)
    assert sum(n == "avg_pool_partial" for n in names) == 1 and not any("tile sums" in n for n in names)
    layers = [layer(sd, "context_encoding.0.0", stride=2), layer(sd, "context_encoding.1.0", stride=2), layer(sd, "context_encoding.2.0")]
    fails = []
    label = f"ctx {case_id(case)}"
    outs = chain(taps["feat"], layers, label, fails)
    _, _, sd_c2 = chain_stats_x3(taps["feat"], layers)
    c2 = outs[2]
    npix = c2.shape[2] * c2.shape[3]
    ref, bound, sigma = pool_linear_model_x3(c2, sd_c2, sd["context_encoding.5.weight"], sd["context_encoding.5.bias"])
    got = taps["ctx"]
    assert got.shape == ref.shape and torch.isfinite(got).all()
    ratio, rms, zmax = z_gates(got, ref, bound, sigma)
    print(f"{label}: {npix} pooled pixels; max err {(got.double() - ref).abs().max().item():.3e} (|ctx| <= {ref.abs().max().item():.3g}; bound <= {bound.max().item():.2e}, "
          f"sigma <= {sigma.max().item():.2e}); err / bound max {ratio:.3f}; rms z {rms:.3f}; max |z| {zmax:.2f}")
    if ratio > 1.0:
        fails.append(f"{label}: ctx outside the fp32-sum bound on the chain's own c2 ({ratio:.3f}x)")
    if rms > Z_RMS or zmax > Z_MAX:
        fails.append(f"{label}: ctx outside the statistical gate (rms z {rms:.3f}, max |z| {zmax:.2f})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", FORWARD_CASES[:-1], ids=case_id)
def test_flow_of_the_forward_from_its_feat_and_ctx_taps(case):
    """motion_estimation.0 (the split convolution on `feat`; the context half folded into an fp32 per-border-class bias table:
    ctx_finish_kernel, fp32 FMAs on the fp32 weights) -> .1 -> .2 (planar fp32).  Neither intermediate is a tap and the bias table
    cannot be handed to the stage entry; the layer-by-layer gates of this stage are tests/test_gpu_motion_layers.py (exact pass-through
    weights bring both intermediates out).  Here the flow of the real weights is held to chain_stats_x3 over the three layers: its rigorous chain bound, as
    tests/test_gpu_conv_rounding_model.py does for the 16-bit modes (as coarse as there: worst cases multiplied through three layers),
    AND the z gates on the chain's standard deviation (some 1e-6 px), which is what a lost low half in .0 or .1 - 2^-12 of a layer's
    terms, 1e-4 px - cannot pass.  The context half: float64 convolution of ctx broadcast over the image (zero padded: the border
    classes) with the fp32 weights, counted with rounded products, 2 (9 mid + 1) 2^-24 sum|terms|."""
    mid, (B, H, W), kind = case
    sd, f1, f2, taps, names = forward_case(*case)
    assert not any("+head" in n for n in names)
    w0, b0 = sd["motion_estimation.0.0.weight"].float(), sd["motion_estimation.0.0.bias"].float()
    ctx_b = taps["ctx"].view(B, mid, 1, 1).expand(B, mid, H, W)
    wc = w0[:, mid:].double()
    half = conv64(ctx_b, wc)
    half_mag = conv64(ctx_b.abs(), wc.abs()) + b0.double().abs().view(1, -1, 1, 1)
    nt = 9 * mid + 1
    half_var = accumulation_variance(nt, b0.double().view(1, -1, 1, 1), half, conv64(ctx_b.double() ** 2, wc ** 2)) + (U32 * half_mag) ** 2 / 3   # (last: the products round too)
    layers = [{"w": w0[:, :mid].contiguous(), "b": b0, "act": "relu", "pre": (half, 2 * nt * U32 * half_mag, half_var)},
              layer(sd, "motion_estimation.1.0"), dict(layer(sd, "motion_estimation.2", act="none"), planar=True)]
    ref, bound, sd_ = chain_stats_x3(taps["feat"], layers)
    flow = taps["flow"]
    assert flow.shape == ref.shape and torch.isfinite(flow).all()
    ratio, rms, zmax = z_gates(flow, ref, bound, sd_)
    err = (flow.double() - ref).abs()
    print(f"flow {case_id(case)}: max err {err.max().item():.3e} px (|flow| <= {ref.abs().max().item():.3g}; sd <= {sd_.max().item():.2e}, chain bound <= {bound.max().item():.2e}); "
          f"err / chain bound max {ratio:.4f}; rms z {rms:.3f}; max |z| {zmax:.2f}")
    assert ratio <= 1.0 and rms <= Z_RMS and zmax <= Z_MAX


@pytest.mark.parametrize("case", FORWARD_CASES[:-1], ids=case_id)
def test_out_of_the_forward_from_its_last_fused_tap(case):
    """reconstruction.0 / .1 / .2 as a chain from the `fused_2` tap - the convolution reads its [hi | lo] halves (the DCN's own
    epilogue at mid_channels 64, convert_cl_kernel's split elsewhere), which are split22 of the fp32 tap, the halves the stage entry
    makes of it -, each layer inside both gates; then the frame against the head's model on the chain's own reconstruction.1."""
    mid, shape, kind = case
    sd, f1, f2, taps, names = forward_case(*case)
    layers = [layer(sd, "reconstruction.0.0"), layer(sd, "reconstruction.1.0"), layer(sd, "reconstruction.2", act="tanh01")]
    fails = []
    label = f"out {case_id(case)}"
    outs = chain(taps["fused_2"], layers, label, fails)
    tap_against_last_layer(taps["out"], outs[2], outs[1], layers[2], label + " tap", fails)
    assert not fails, "\n".join(fails)


def offsets_and_masks64(x, w, b):
    """(offset [B,18,H,W], mask [B,9,H,W], d_raw [B,1,H,W], var_off [B,18,H,W], var_logit [B,9,H,W]) of the split offset convolution in
    float64 on the fp32 tensor x whose halves it reads: 27 raw channels -> chunk(3) -> offset = cat(first, third), mask =
    sigmoid(second) (oracle.offset_and_mask).  d_raw = the pixel's worst raw channel of (3 n + 1) 2^-24 sum|terms|, 2^-21 sum|terms| for
    halves that are split differently where a lo is exactly half a unit (block 0 reads the halves the last feature layer wrote, not
    those of the tap), and the fp32 rounding of the value itself; the variances: the same terms as in chain_stats_x3."""
    N = 3 * 9 * x.shape[1] + 1
    raw, mag, sq = terms_x3(x, w, b, 1)
    d_raw = ((N + 8) * U32 * mag + U32 * raw.abs()).amax(dim=1, keepdim=True)
    start = b.double().view(1, -1, 1, 1)
    var = accumulation_variance(N, start, raw - start, sq) + 2.0 ** -54 * conv64(x.double() ** 2, w.double() ** 2) + (U32 * raw) ** 2 / 3
    o1, m, o2 = torch.chunk(raw, 3, dim=1)
    v1, vm, v2 = torch.chunk(var, 3, dim=1)
    return torch.cat((o1, o2), dim=1), torch.sigmoid(m), d_raw, torch.cat((v1, v2), dim=1), vm


@pytest.mark.parametrize("case", FORWARD_CASES[:-1], ids=case_id)
def test_fused_blocks_of_the_forward_from_their_input_taps(case):
    """fused_i from fused_(i-1) (block 0: from cat(feat, warped)), per element.  Which deformable kernel the mode runs is read off the
    launch list, and it must be what plan_forward (build_plan: dcn32[i].x3 = x3 || amp where deform_f32w_shape holds) says: at
    mid_channels 64 deform_f32w_kernel<true> - fp32 sampling, the three-term f16 split in the contraction: deform_model.bound_x3 -, at
    mid_channels 8 the generic fp32 kernel: bound_fp32.  The DCN reads the fp32 fusion tensor, the offset convolution its [hi | lo]
    split (fusion_split_warped / split16_cl_kernel, the DCN epilogue's halves): float64 three-term convolution of split22(tap).
    Added to the kernel's bound, as tests/test_gpu_mdcn.py::error_model does: the offsets' and the mask logits' own error d_raw (the
    split convolution's (3 n + 1) 2^-24 sum|terms|; positions are fp32 sums: two roundings of up to 2^-24 (size + |offset|) more)
    times the sampled field's slope (one-sided differences over 1e-3 px, x 1.5) resp. a quarter of it (the sigmoid's slope) plus 2^-21.
    Block 0 reads `feat` UNSPLIT (the out32 side store), which no tap shows: the tap's carried value is within split_error of it.
    That bound is rigorous and coarse (the offsets' worst case times the slope is most of it: a lost low half in the contraction,
    2^-12 of the terms, stays inside), so the same terms also enter as standard deviations - per tap the output's signed slope against
    dy, dx and the mask logit times their standard deviations, the contraction's accumulation as in conv_model_x3 - under the z gates."""
    mid, (B, H, W), kind = case
    sd, f1, f2, taps, names = forward_case(*case)
    split_dcn = sum("three-term f16 split contraction" in n for n in names)
    assert split_dcn == (3 if mid == 64 else 0) and sum("dcn_v2" in n for n in names) == 3
    bound_fn = dm.bound_x3 if split_dcn else dm.bound_fp32
    fails = []
    x = torch.cat([taps["feat"], taps["warped"]], dim=1)
    for i in range(3):
        ow, ob = sd[f"attention_blocks.{i}.offset_conv.weight"].float(), sd[f"attention_blocks.{i}.offset_conv.bias"].float()
        w, b = sd[f"attention_blocks.{i}.dcn_v2.weight"].float(), sd[f"attention_blocks.{i}.dcn_v2.bias"].float()
        off, msk, d_raw, var_off, var_logit = offsets_and_masks64(x, ow, ob)
        off32, msk32 = off.float(), msk.float()
        ref, bound, _ = bound_fn(x, off32, msk32, w, b)
        reach = max(H, W) + off.abs().amax(dim=1, keepdim=True)
        d_pos, var_pos = d_raw + 2 * U32 * reach, (2 * U32 * reach) ** 2 / 3
        pos = dm.tap_positions(off32, H, W)
        step, sens, plain, cols, var = 1e-3, [], [], [], 0.0
        for k in range(9):
            py, px = pos[k][0].double(), pos[k][1].double()
            mk, wk = msk[:, k].unsqueeze(1), w[:, :, k // 3, k % 3].double()
            con = lambda t: torch.einsum("oc,bchw->bohw", wk, t)
            base = dm.sample64(x, py, px)
            dy = [(dm.sample64(x, py + sg * step, px) - base) / step for sg in (1, -1)]
            dx = [(dm.sample64(x, py, px + sg * step) - base) / step for sg in (1, -1)]
            sens.append((torch.maximum(dy[0].abs(), dy[1].abs()) + torch.maximum(dx[0].abs(), dx[1].abs())) * mk)
            plain.append(dm.sample64(x.abs(), py, px))
            cols.append(base * mk)
            # the output's slope against this tap's dy, dx and mask logit: the contraction of the signed one-sided differences
            gy2 = torch.maximum(con(dy[0] * mk) ** 2, con(dy[1] * mk) ** 2)
            gx2 = torch.maximum(con(dx[0] * mk) ** 2, con(dx[1] * mk) ** 2)
            var = var + gy2 * (var_off[:, 2 * k:2 * k + 1] + var_pos) + gx2 * (var_off[:, 2 * k + 1:2 * k + 2] + var_pos) \
                + con(base) ** 2 * (var_logit[:, k:k + 1] / 16 + (2.0 ** -21) ** 2 / 3)
        b_offset = 1.5 * d_pos * dm.contract64(sens, w.abs())
        b_mask = (d_raw / 4 + 2.0 ** -21 + U32) * dm.contract64(plain, w.abs())
        total = bound + b_offset + b_mask
        # the kernel's own part in standard deviations: the accumulation as in conv_model_x3, seven fp32 roundings per blended value,
        # the split's 3 * 2^-22 per product and 2^-25 (|w| + |x|) (deform_model.bound_x3), or the fp32 kernel's rounded products
        T2 = dm.contract64([c ** 2 for c in cols], w.double() ** 2)
        n_acc = (3 if split_dcn else 1) * 9 * x.shape[1] + 1
        bb = b.double().view(1, -1, 1, 1)
        var = var + accumulation_variance(n_acc, bb, ref - bb, T2) + (7 * U32) ** 2 / 3 * T2
        if split_dcn:
            var = var + (3 * U22) ** 2 / 3 * T2 + (2.0 ** -25) ** 2 / 3 * (w.double().pow(2).sum(dim=(1, 2, 3)).view(1, -1, 1, 1) + sum((c ** 2).sum(dim=1, keepdim=True) for c in cols))
        else:
            var = var + U32 ** 2 / 3 * T2
        if i == 0:      # the fp32 `feat` the DCN read is within split_error of the tap
            dx0 = torch.cat([(U22 * taps["feat"].double().abs()).clamp_min(2.0 ** -25), torch.zeros_like(taps["warped"]).double()], dim=1)
            total = total + dm.contract64([dm.sample64(dx0, pos[k][0], pos[k][1]) * msk[:, k].unsqueeze(1) for k in range(9)], w.abs())
            var = var + dm.contract64([dm.sample64(dx0 ** 2, pos[k][0], pos[k][1]) * msk[:, k].unsqueeze(1) ** 2 for k in range(9)], w.double() ** 2) / 3
        got = taps[f"fused_{i}"]
        assert got.shape == ref.shape and torch.isfinite(got).all()
        err = (got.double() - ref).abs()
        ratio, rms, zmax = z_gates(got, ref, total, var.sqrt())
        print(f"fused_{i} {case_id(case)} ({'split' if split_dcn else 'fp32'} DCN): max err {err.max().item():.3e} (|fused| <= {ref.abs().max().item():.3g}); err / bound max {ratio:.3f} "
              f"(the kernel's own share of the bound there {100 * (bound / total).reshape(-1)[(err / total).argmax()].item():.0f} %); rms z {rms:.3f}; max |z| {zmax:.2f}")
        if ratio > 1.0:
            fails.append(f"fused_{i} {case_id(case)}: an element exceeds the deformable model's bound on the GPU's own input tap ({ratio:.3f}x)")
        if rms > Z_RMS or zmax > Z_MAX:
            fails.append(f"fused_{i} {case_id(case)}: outside the statistical gate (rms z {rms:.3f}, max |z| {zmax:.2f})")
        x = got
    assert not fails, "\n".join(fails)


# MEASURED (MI355X, this file's own output): err / bound max, rms(z), max |z| of every case.  Single layers (B = 2), at the three scales:
#   pair            act     H x W   2^0                  2^-10                2^10                
#   6to64s1         none    1x1     0.023, 0.160, 0.62   0.000, 0.000, 0.00   0.020, 0.146, 0.62  
#   6to64s1         relu    1x70    0.023, 0.138, 0.98   0.755, 0.021, 1.00   0.028, 0.132, 0.86  
#   6to64s1         none    70x1    0.025, 0.190, 1.20   0.844, 0.044, 1.00   0.028, 0.182, 0.92  
#   6to64s1         relu    5x7     0.029, 0.174, 1.26   0.371, 0.015, 1.00   0.026, 0.165, 1.12  
#   6to64s1         none    33x47   0.050, 0.257, 1.74   0.723, 0.051, 1.00   0.048, 0.257, 1.89  
#   64to64s1        none    1x1     0.001, 0.089, 0.27   0.000, 0.000, 0.00   0.003, 0.096, 0.43  
#   64to64s1        relu    1x70    0.002, 0.096, 0.65   0.054, 0.052, 1.00   0.002, 0.096, 0.72  
#   64to64s1        none    70x1    0.002, 0.137, 0.77   0.062, 0.068, 1.00   0.003, 0.135, 0.70  
#   64to64s1        relu    5x7     0.002, 0.145, 1.02   0.041, 0.075, 1.00   0.002, 0.142, 1.16  
#   64to64s1        none    33x47   0.004, 0.223, 1.45   0.038, 0.112, 1.00   0.004, 0.222, 1.69  
#   64to128s2       none    1x1     0.002, 0.081, 0.25   0.215, 0.062, 1.00   0.002, 0.093, 0.40  
#   64to128s2       relu    1x70    0.002, 0.090, 0.67   0.065, 0.041, 1.00   0.002, 0.094, 0.77  
#   64to128s2       none    70x1    0.002, 0.129, 0.65   0.079, 0.069, 1.00   0.002, 0.125, 0.62  
#   64to128s2       relu    5x7     0.002, 0.115, 0.67   0.042, 0.065, 1.00   0.002, 0.115, 0.66  
#   64to128s2       none    33x47   0.003, 0.202, 1.39   0.041, 0.105, 1.00   0.003, 0.202, 1.35  
#   64to128s2       relu    37x53   0.003, 0.143, 1.44   0.038, 0.074, 1.00   0.003, 0.144, 1.31  
#   64to128s2       none    36x52   0.003, 0.205, 1.32   0.047, 0.105, 1.00   0.004, 0.206, 1.34  
#   128to256s2      none    1x1     0.001, 0.077, 0.31   0.000, 0.000, 0.00   0.001, 0.074, 0.30  
#   128to256s2      relu    1x70    0.001, 0.084, 0.66   0.021, 0.049, 1.00   0.001, 0.083, 0.65  
#   128to256s2      none    70x1    0.001, 0.121, 0.77   0.029, 0.065, 1.00   0.001, 0.119, 0.65  
#   128to256s2      relu    5x7     0.001, 0.118, 1.01   0.015, 0.074, 1.00   0.001, 0.115, 0.96  
#   128to256s2      none    33x47   0.001, 0.193, 1.31   0.015, 0.120, 1.00   0.002, 0.193, 1.91  
#   128to256s2      relu    37x53   0.002, 0.136, 1.39   0.015, 0.086, 1.00   0.001, 0.138, 1.52  
#   128to256s2      none    36x52   0.001, 0.197, 1.43   0.013, 0.122, 1.00   0.002, 0.197, 1.52  
#   256to256s1      none    1x1     0.000, 0.073, 0.32   0.017, 0.076, 1.00   0.000, 0.071, 0.28  
#   256to256s1      relu    1x70    0.001, 0.082, 0.59   0.010, 0.061, 1.00   0.001, 0.084, 0.65  
#   256to256s1      none    70x1    0.001, 0.117, 0.71   0.010, 0.084, 1.00   0.001, 0.118, 0.81  
#   256to256s1      relu    5x7     0.000, 0.128, 1.07   0.005, 0.089, 1.00   0.001, 0.127, 1.11  
#   256to256s1      none    33x47   0.001, 0.198, 1.64   0.005, 0.146, 1.00   0.001, 0.199, 1.37  
#   64to2s1         none    1x1     0.000, 0.051, 0.09   0.000, 0.000, 0.00   0.000, 0.104, 0.14  
#   64to2s1         relu    1x70    0.001, 0.084, 0.50   0.000, 0.000, 0.00   0.002, 0.112, 0.77  
#   64to2s1         none    70x1    0.002, 0.141, 0.66   0.051, 0.084, 1.00   0.001, 0.127, 0.46  
#   64to2s1         relu    5x7     0.001, 0.160, 0.73   0.000, 0.000, 0.00   0.001, 0.133, 0.68  
#   64to2s1         none    33x47   0.004, 0.217, 1.43   0.027, 0.111, 1.00   0.003, 0.223, 1.28  
#   67to27s1        none    1x1     0.001, 0.080, 0.20   0.000, 0.000, 0.00   0.001, 0.092, 0.20  
#   67to27s1        relu    1x70    0.003, 0.099, 0.80   0.055, 0.036, 1.00   0.003, 0.098, 0.93  
#   67to27s1        none    70x1    0.003, 0.143, 0.83   0.062, 0.074, 1.00   0.003, 0.142, 0.82  
#   67to27s1        relu    5x7     0.002, 0.149, 0.80   0.019, 0.051, 1.00   0.003, 0.153, 1.48  
#   67to27s1        none    33x47   0.004, 0.230, 1.70   0.030, 0.114, 1.00   0.003, 0.229, 1.43  
#   67to64s1        none    1x1     0.002, 0.090, 0.34   0.000, 0.000, 0.00   0.001, 0.093, 0.22  
#   67to64s1        relu    1x70    0.003, 0.100, 0.78   0.068, 0.057, 1.00   0.003, 0.100, 0.64  
#   67to64s1        none    70x1    0.002, 0.142, 0.76   0.065, 0.073, 1.00   0.003, 0.141, 0.95  
#   67to64s1        relu    5x7     0.002, 0.147, 0.98   0.027, 0.056, 1.00   0.002, 0.143, 0.98  
#   67to64s1        none    33x47   0.004, 0.231, 1.72   0.031, 0.113, 1.00   0.004, 0.231, 1.70  
#   64to32s1        none    1x1     0.001, 0.102, 0.23   0.000, 0.000, 0.00   0.001, 0.081, 0.19  
#   64to32s1        relu    1x70    0.002, 0.090, 0.66   0.059, 0.042, 1.00   0.003, 0.100, 0.83  
#   64to32s1        none    70x1    0.002, 0.136, 0.69   0.061, 0.054, 1.00   0.003, 0.136, 0.72  
#   64to32s1        relu    5x7     0.002, 0.138, 1.05   0.037, 0.047, 1.00   0.002, 0.137, 0.90  
#   64to32s1        none    33x47   0.004, 0.223, 1.49   0.032, 0.111, 1.00   0.004, 0.222, 1.41  
#   32to3s1tanh01   tanh01  1x1     0.001, 0.048, 0.10   0.052, 0.058, 0.10   0.000, 0.000, 0.00  
#   32to3s1tanh01   tanh01  1x70    0.001, 0.044, 0.19   0.046, 0.047, 0.11   0.000, 0.000, 0.01  
#   32to3s1tanh01   tanh01  70x1    0.001, 0.054, 0.21   0.048, 0.051, 0.11   0.000, 0.000, 0.00  
#   32to3s1tanh01   tanh01  5x7     0.000, 0.039, 0.15   0.036, 0.051, 0.11   0.000, 0.005, 0.07  
#   32to3s1tanh01   tanh01  33x47   0.001, 0.043, 0.49   0.044, 0.050, 0.11   0.000, 0.000, 0.01  
#   8to8s1          none    1x1     0.013, 0.178, 0.56   0.000, 0.000, 0.00   0.005, 0.093, 0.18  
#   8to8s1          relu    1x70    0.012, 0.115, 0.61   0.533, 0.030, 1.00   0.015, 0.122, 0.71  
#   8to8s1          none    70x1    0.017, 0.175, 0.53   0.000, 0.000, 0.00   0.014, 0.163, 0.80  
#   8to8s1          relu    5x7     0.016, 0.152, 0.91   0.000, 0.000, 0.00   0.011, 0.140, 0.74  
#   8to8s1          none    33x47   0.026, 0.236, 1.45   0.447, 0.066, 1.00   0.023, 0.235, 1.24  
#   11to27s1        none    1x1     0.010, 0.170, 0.39   0.000, 0.000, 0.00   0.010, 0.121, 0.36  
#   11to27s1        relu    1x70    0.018, 0.136, 0.94   0.707, 0.033, 1.00   0.015, 0.128, 0.86  
#   11to27s1        none    70x1    0.020, 0.183, 0.89   0.612, 0.043, 1.00   0.018, 0.182, 0.94  
#   11to27s1        relu    5x7     0.016, 0.178, 1.33   0.285, 0.061, 1.00   0.020, 0.171, 1.10  
#   11to27s1        none    33x47   0.026, 0.272, 2.09   0.433, 0.074, 1.00   0.022, 0.270, 1.75  
#   16to16s1        none    1x1     0.007, 0.129, 0.35   0.000, 0.000, 0.00   0.005, 0.092, 0.31  
#   16to16s1        relu    1x70    0.008, 0.109, 0.64   0.305, 0.042, 1.00   0.009, 0.112, 0.74  
#   16to16s1        none    70x1    0.009, 0.154, 0.71   0.297, 0.060, 1.00   0.011, 0.152, 0.80  
#   16to16s1        relu    5x7     0.012, 0.149, 1.07   0.149, 0.067, 1.00   0.007, 0.152, 1.02  
#   16to16s1        none    33x47   0.014, 0.229, 1.37   0.230, 0.078, 1.00   0.017, 0.229, 1.65  
# Range contract (largest |x| = 65504): 64to64s1 33x47: 0.005, 0.223, 1.94;  6to64s1 5x7: 0.038, 0.240, 1.16;  64to128s2 37x53: 0.003, 0.205, 1.56
# The forward on its own taps, per case.  feat / out: the layers one at a time (largest figure over the layers); the tap against its last
# layer's model; the share of elements in which chain and forward differ (largest |z| of those).  ctx: pooled pixels, max err, the
# three figures.  flow: max err in px, the three figures (the first against the chain bound).  fused_i: max err, the three figures.
#   mid64-1x1x7-natural
#     feat    layers 0.015, 0.14, 0.72;  tap 0.002, 0.14, 0.60;  differ 0.0000 % (0.00)
#     ctx     layers 0.003, 0.13, 0.69;  2 px, 3.309e-08: 0.002, 0.037, 0.11
#     flow    5.179e-07 px: 0.0001, 0.157, 0.34
#     fused_0 (split DCN) 1.018e-07: 0.001, 0.262, 1.05
#     fused_1 (split DCN) 1.032e-07: 0.001, 0.323, 1.09
#     fused_2 (split DCN) 1.043e-07: 0.001, 0.360, 1.37
#     out     layers 0.005, 0.14, 0.77;  tap 0.005, 0.11, 0.21;  differ 0.0000 % (0.00)
#   mid64-1x1x7-stress
#     feat    layers 0.018, 0.13, 0.55;  tap 0.001, 0.12, 0.54;  differ 12.2768 % (0.54)
#     ctx     layers 0.001, 0.12, 0.55;  2 px, 1.753e-08: 0.001, 0.019, 0.05
#     flow    6.445e-07 px: 0.0000, 0.166, 0.41
#     fused_0 (split DCN) 1.285e-07: 0.000, 0.186, 0.56
#     fused_1 (split DCN) 9.776e-08: 0.001, 0.286, 1.11
#     fused_2 (split DCN) 1.213e-07: 0.001, 0.368, 1.44
#     out     layers 0.007, 0.17, 0.77;  tap 0.007, 0.08, 0.21;  differ 4.7619 % (0.12)
#   mid64-1x17x33-natural
#     feat    layers 0.027, 0.19, 1.79;  tap 0.002, 0.17, 1.42;  differ 25.3259 % (1.42)
#     ctx     layers 0.002, 0.15, 1.42;  45 px, 7.164e-08: 0.001, 0.016, 0.04
#     flow    4.916e-06 px: 0.0000, 0.193, 0.82
#     fused_0 (split DCN) 1.992e-06: 0.001, 0.264, 1.27
#     fused_1 (split DCN) 7.875e-07: 0.000, 0.254, 1.39
#     fused_2 (split DCN) 5.882e-07: 0.001, 0.281, 1.33
#     out     layers 0.003, 0.17, 1.49;  tap 0.003, 0.12, 0.44;  differ 12.7154 % (0.44)
#   mid64-1x17x33-stress
#     feat    layers 0.021, 0.18, 1.56;  tap 0.002, 0.15, 1.35;  differ 12.5279 % (1.35)
#     ctx     layers 0.003, 0.16, 1.48;  45 px, 2.271e-07: 0.001, 0.013, 0.04
#     flow    1.321e-05 px: 0.0000, 0.160, 0.64
#     fused_0 (split DCN) 6.523e-06: 0.000, 0.219, 1.21
#     fused_1 (split DCN) 3.978e-06: 0.000, 0.211, 1.26
#     fused_2 (split DCN) 1.614e-06: 0.000, 0.223, 1.07
#     out     layers 0.002, 0.16, 1.38;  tap 0.002, 0.10, 0.51;  differ 9.6257 % (0.31)
#   mid64-2x33x70-natural
#     feat    layers 0.023, 0.19, 1.58;  tap 0.002, 0.16, 1.60;  differ 22.6339 % (1.60)
#     ctx     layers 0.003, 0.15, 1.44;  162 px, 1.354e-07: 0.001, 0.030, 0.09
#     flow    1.120e-05 px: 0.0000, 0.194, 0.84
#     fused_0 (split DCN) 4.761e-06: 0.001, 0.235, 1.88
#     fused_1 (split DCN) 3.868e-06: 0.001, 0.233, 1.91
#     fused_2 (split DCN) 1.818e-06: 0.001, 0.252, 1.63
#     out     layers 0.005, 0.17, 2.17;  tap 0.005, 0.11, 0.63;  differ 14.5455 % (0.63)
#   mid64-2x33x70-stress
#     feat    layers 0.032, 0.18, 1.83;  tap 0.003, 0.16, 1.61;  differ 13.7666 % (1.51)
#     ctx     layers 0.003, 0.16, 1.57;  162 px, 3.480e-07: 0.001, 0.026, 0.09
#     flow    1.656e-05 px: 0.0000, 0.162, 0.79
#     fused_0 (split DCN) 1.440e-05: 0.000, 0.177, 1.71
#     fused_1 (split DCN) 7.605e-06: 0.000, 0.163, 1.28
#     fused_2 (split DCN) 4.215e-06: 0.000, 0.179, 1.74
#     out     layers 0.004, 0.17, 1.60;  tap 0.003, 0.10, 0.59;  differ 14.5743 % (0.48)
#   mid8-2x23x37-natural
#     feat    layers 0.047, 0.20, 1.57;  tap 0.047, 0.20, 1.09;  differ 0.2497 % (1.01)
#     ctx     layers 0.020, 0.19, 1.31;  60 px, 1.991e-08: 0.003, 0.043, 0.08
#     flow    8.996e-07 px: 0.0004, 0.219, 0.83
#     fused_0 (fp32 DCN) 1.730e-06: 0.015, 0.207, 1.61
#     fused_1 (fp32 DCN) 4.727e-07: 0.007, 0.239, 1.48
#     fused_2 (fp32 DCN) 2.976e-07: 0.008, 0.296, 2.57
#     out     layers 0.043, 0.20, 1.36;  tap 0.043, 0.06, 0.30;  differ 0.5875 % (0.16)
#   mid8-2x23x37-stress
#     feat    layers 0.025, 0.17, 1.40;  tap 0.019, 0.15, 1.09;  differ 1.9976 % (1.09)
#     ctx     layers 0.025, 0.16, 1.14;  60 px, 3.698e-08: 0.002, 0.023, 0.05
#     flow    1.885e-06 px: 0.0003, 0.137, 0.97
#     fused_0 (fp32 DCN) 2.494e-06: 0.008, 0.145, 1.10
#     fused_1 (fp32 DCN) 1.011e-06: 0.004, 0.127, 1.03
#     fused_2 (fp32 DCN) 5.719e-07: 0.005, 0.137, 1.24
#     out     layers 0.037, 0.22, 1.92;  tap 0.037, 0.06, 0.32;  differ 1.9193 % (0.20)
#   mid64-1x3x4-natural
#     ctx     layers 0.001, 0.14, 0.49;  1 px, 6.485e-08: 0.003, 0.041, 0.14
# The MFMA's accumulation stays at a few per cent of the worst case and a quarter of the sequential-sum standard deviation (the CPU
# kernel of tests/test_rounding_model_cpu.py, which adds sixteen products at a time as well: 0.06 .. 0.26).  At 2^-10 every output's lo
# is subnormal and the only error is a whole step of it, 2^-24, at a few elements: max |z| = 1.00 exactly, and up to 0.84 of a bound
# that is little more than that step (half a step, 2^-25, is what separates a value from its OWN split, not two splits from each other:
# rounding_model's section comment).  Every identity and impulse case is exact.
# The differing share is far above the 2^-13 of the elements whose hi moves when hi + lo is split again: each of those feeds 9 pixels x
# 64 channels of the next layer, whose fp32 sums then differ in their last places, through three layers - 576 x 2^-13 = 7 % per layer.
# Those elements sit inside the same gates as the rest.  ctx: a lost lo half would be 5 sigma and more (tests/test_rounding_model_cpu.py).
