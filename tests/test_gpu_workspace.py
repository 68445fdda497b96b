"""Every compute entry is independent of what its workspace held before the call.

The statement is the same for every case and has no tolerance (tests/workspace_harness.py, run_case): the entry runs with EXACTLY
the bytes its *_workspace_bytes function reported, the workspace pre-filled with 0x00, with 0xFF (NaN in f16, bf16 and fp32,
0xFFFFFFFF as a counter) and with 0x7B (finite and huge in all three), on guard-banded inputs and into guard-banded, sentinel-filled
outputs and taps.  The three results are bit-identical to each other and to the call through the ordinary cached workspace
(lib.workspace: grow-only, holding an earlier test's finite activations); every guard of the workspace, the inputs and the outputs is
unchanged; every output element is written and finite; the census words, where the entry has a census, are identical too; one byte
less workspace is refused with EMAVFI_E_WORKSPACE.  The 0x00 run is made twice first, so a case that is not deterministic fails as
that and not as a workspace dependence.

What this cannot see: an overrun from one carved sub-buffer of the workspace into the next one.  Only a dependence of the result on
the prior contents and a write beyond the outer guards are observable from outside the library.

Shapes are the smallest that reach the partial-tile, strip, window and row paths named at each case; all frames and weights are
synthetic (emavfi.synth, torch generators); nothing is read from the reference."""
import math

import pytest
import torch

from emavfi import EMA_VFI, lib, synth
from test_gpu_conv_rounding_model import ALL_SWITCHES, FAMILIES, NO_RING, OLD32, expect_family, set_env
from workspace_harness import DEV, debug_switch, run_case

pytestmark = pytest.mark.gpu

# (B, H, W) of the forward and the path each reaches
FORWARD_SHAPES = [
    (1, 1, 7),      # one row, less than a tile, a strip and a window in every kernel; a 1 x 1 image at both lower pyramid levels
    (2, 23, 37),    # odd at every pyramid level (12 x 19, 6 x 10), W % 4 != 0 (the scalar warp), 16 x 16 pack tiles with remainders
    (1, 17, 125),   # two strips of the 62-column pitch plus one column; one row beyond a pack tile
    (1, 33, 62),    # exactly one strip; two pack tiles and one row
    (1, 48, 64),    # whole 16 x 16 pack tiles, the tiled warp (W % 4 == 0)
]
MODES = ["fp32", "bf16", "fp16", "amp16", "fp32x3"]
SWITCHES = {"no_tailfuse": lib.SW_NO_TAILFUSE, "no_poolfuse": lib.SW_NO_POOLFUSE, "no_head": lib.SW_NO_HEAD, "no_conv_first": lib.SW_NO_CONV_FIRST}

# offset_std / offset_bias of synth.synthetic_state_dict per frame kind.  natural: the recipe's own, offsets within about +-2 px - what
# the pack's window holds.  stress: the recipe of tests/golden/large_offsets.npz, about +-8 px - most (wave, tap) groups leave the window
OFFSETS = {"natural": (1.0, 1.0), "stress": (3.0, 3.0)}
_models = {}


def can_leave_window(H, W):
    """The pack stages a window around each 16 x 16 tile, and a sample outside the IMAGE is a zero, not a fix-up.  So only an image of
    more than one tile has samples that are inside it and outside some tile's window: (1, 1, 7) and (2, 16, 16) cannot reach the fix-up
    loop whatever the offsets are, and are not asked to"""
    return H > 16 or W > 16


def model_of(mid, mode, kind="natural"):
    key = (mid, mode, kind)
    if key not in _models:
        m = EMA_VFI(mid_channels=mid, compute_dtype=mode).to(DEV).eval()
        std, bias = OFFSETS[kind]
        m.load_state_dict(synth.synthetic_state_dict(seed=3, mid_channels=mid, offset_std=std, offset_bias=bias), strict=True)
        m.pipeline = 1
        _models[key] = m
    m = _models[key]
    m.pack_policy, m.pack_adapt = "window", None
    return m


def leaves(kind, shape):
    return kind == "stress" and can_leave_window(*shape[1:])


def forward_enqueue(model):
    """the part of forward_call that only enqueues work (what tests/test_gpu_graph_replay.py captures): every tap of one forward"""
    def call(inp):
        with torch.no_grad():
            _, taps = model(inp[0], inp[1], return_taps=True)
        return dict(taps)
    return call


def forward_census(model, leaves_window=False):
    """the part of forward_call that reads back: the census of the forward that ran last on the current stream.
    leaves_window: the case is there for the fix-up arena and the census counters, so every block that has a census must have
    counted wave-taps in the fix-up loop and samples outside the window - in every run, or the case covers less than it says"""
    def read():
        census = model.pack_census()
        if leaves_window:
            assert all(r is None or (r["fixup_wave_taps"] > 0 and r["samples_outside_window"] > 0) for r in census), \
                f"no sample left the window in some block: {census}"
        return {"census": census}
    return read


def forward_call(model, adaptive=False, leaves_window=False):
    """forward_enqueue, then forward_census"""
    enqueue, read = forward_enqueue(model), forward_census(model, leaves_window)

    def call(inp):
        if adaptive:
            model._route_states.clear()   # a freshly initialised route state per run (allocated through torch.empty: guard-banded)
        res = enqueue(inp)
        res.update(read())
        if adaptive:
            res["route_state"] = next(iter(model._route_states.values()))
        return res
    return call


def frames(B, H, W, kind, seed=17):
    # stress: i.i.d. bytes, run with the large-offset weights (OFFSETS) - flows and offsets that leave the pack's window
    return list(synth.synthetic_frames(seed, B, H, W, kind))


@pytest.mark.parametrize("kind", ["natural", "stress"])
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_forward(mode, shape, kind, monkeypatch):
    """EMA_VFI(mid_channels = 64)(f1, f2, return_taps=True): out, feat, ctx, flow, warped, fused_0..2 and the census"""
    set_env(monkeypatch, {})
    call = forward_call(model_of(64, mode, kind), leaves_window=leaves(kind, shape))
    run_case(monkeypatch, f"forward {mode} {shape} {kind}", call, frames(*shape, kind))


@pytest.mark.parametrize("kind", ["natural", "stress"])
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("route", ["gather", "adapt"])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_forward_pack_routes(mode, route, shape, kind, monkeypatch):
    """the other two pack routes of the 16-bit modes (the window route is test_forward): pack_policy = "gather" - the window-free
    kernel, no window DMA, corner gathers from the fusion tensor and the compact tail; pack_adapt - the routed pack reading the route
    word of a fresh, guard-banded route state, plus route_select on the census"""
    set_env(monkeypatch, {})
    model = model_of(64, mode, kind)
    if route == "gather":
        model.pack_policy = "gather"
    else:
        model.pack_adapt = (0.75, 0.65)
    try:
        call = forward_call(model, adaptive=route == "adapt", leaves_window=leaves(kind, shape))
        run_case(monkeypatch, f"forward {mode} {route} {shape} {kind}", call, frames(*shape, kind))
    finally:
        model.pack_policy, model.pack_adapt = "window", None
        model._route_states.clear()


@pytest.mark.parametrize("kind", ["natural", "stress"])
@pytest.mark.parametrize("name", sorted(SWITCHES))
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_forward_unfused_launches(mode, name, kind, monkeypatch):
    """(2, 23, 37) with one debug switch set: reconstruction.1 + .2 as two launches (no_tailfuse), context_encoding.2 stored and pooled
    (no_poolfuse), the flow head as its own launch (no_head), pack_input + feat_ext_conv1 as the tile kernel (no_conv_first) - the
    paths the parity tests rest on"""
    set_env(monkeypatch, {})
    launches = lambda: [n for n, _, _ in lib.forward_launches(3, 64, 3, 2, 23, 37, mode)]
    default = launches()
    with debug_switch(SWITCHES[name]):
        assert launches() != default, f"{name} selects no other launch at (2, 23, 37) in {mode}: {default}"
        call = forward_call(model_of(64, mode, kind), leaves_window=leaves(kind, (2, 23, 37)))
        run_case(monkeypatch, f"forward {mode} {name} {kind}", call, frames(2, 23, 37, kind))


@pytest.mark.parametrize("kind", ["natural", "stress"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_forward_mid8(mode, kind, monkeypatch):
    """mid_channels = 8 at (2, 23, 37): the generic tile kernels, conv3x3 + the global-gather DCN per attention block"""
    set_env(monkeypatch, {})
    run_case(monkeypatch, f"forward mid 8 {mode} {kind}", forward_call(model_of(8, mode, kind)), frames(2, 23, 37, kind))


# ------------------------------------------------------------------------------------------------ stage entries
def conv_params(g, pairs):
    out = []
    for cout, cin in pairs:
        out += [torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5, torch.randn(cout, generator=g) * 0.1]
    return out


@pytest.mark.parametrize("pool", ["poolfuse", "no_poolfuse"])
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 1, 7)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "amp16"])
def test_context(mode, shape, pool, monkeypatch):
    """lib.context at mid_channels 64.  (2, 37, 53): 19 x 27 then 10 x 14 - odd rows and columns at both stride-2 layers, a partial
    32 x 4 tile of the fused pool; (1, 1, 7): one row, 1 x 4 then 1 x 2"""
    set_env(monkeypatch, {})
    B, H, W = shape
    g = torch.Generator().manual_seed(700 + H)
    feat = torch.randn(B, 64, H, W, generator=g).relu()
    params = conv_params(g, ((128, 64), (256, 128), (256, 256))) + [torch.randn(64, 256, generator=g) / 16, torch.randn(64, generator=g) * 0.1]
    with debug_switch(lib.SW_NO_POOLFUSE, pool == "no_poolfuse"):
        run_case(monkeypatch, f"context {mode} {shape} {pool}", lambda inp: lib.context(inp[0], inp[1:], dtype=mode), [feat] + params)


@pytest.mark.parametrize("tail", ["tailfuse", "no_tailfuse"])
@pytest.mark.parametrize("shape", [(1, 2, 62), (1, 17, 125)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "amp16"])
def test_reconstruct(mode, shape, tail, monkeypatch):
    """lib.reconstruct at mid_channels 64.  (1, 2, 62): exactly one strip, fewer rows than the row ring holds; (1, 17, 125): two strips
    and one column, the im2col tail of 67 -> 64 at both strip edges"""
    set_env(monkeypatch, {})
    B, H, W = shape
    g = torch.Generator().manual_seed(800 + W)
    fused = torch.randn(B, 67, H, W, generator=g)
    params = conv_params(g, ((64, 67), (32, 64), (3, 32)))
    with debug_switch(lib.SW_NO_TAILFUSE, tail == "no_tailfuse"):
        run_case(monkeypatch, f"reconstruct {mode} {shape} {tail}", lambda inp: lib.reconstruct(inp[0], inp[1:], dtype=mode), [fused] + params)


def mdcn_case(seed, B, H, W, far):
    """x, offset_conv weight / bias, dcn_v2 weight / bias at C = 67.  far = 0: offsets of about +-2 px, inside the staged window; else
    taps 2, 5 and 8 are pushed `far` px away (raw channels 0..8 | 18..26 are the offsets, ema_vfi.py:56-58): the fix-up loop"""
    g = torch.Generator().manual_seed(seed)
    C = 67
    x = torch.randn(B, C, H, W, generator=g)
    ow = (torch.rand(27, C, 3, 3, generator=g) * 2 - 1) * 0.05
    ob = (torch.rand(27, generator=g) * 2 - 1) * 1.5
    if far:
        for t in (2, 5, 8):
            for c in (2 * t, 2 * t + 1):
                ob[c if c < 9 else c + 9] = far if (c + t) % 2 == 0 else -far
    return [x, ow, ob, torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9), torch.randn(C, generator=g) * 0.1]


# the f16 links of a bf16 forward: IN_F16 alone and with SPLIT_TAIL are the forms its packs take on f16 producers, IN + OUT between packs
F16_LINK = lib.MDCN_IN_F16 | lib.MDCN_OUT_F16
MDCN_CASES = [(m, r, f) for m in ("bf16", "fp16") for r in ("window", "gather") for f in (0, lib.MDCN_SPLIT_TAIL)] + \
             [("bf16", r, f) for r in ("window", "gather")
              for f in (lib.MDCN_IN_F16, lib.MDCN_IN_F16 | lib.MDCN_SPLIT_TAIL, F16_LINK, F16_LINK | lib.MDCN_SPLIT_TAIL)] + \
             [("fp32", "window", 0), ("amp16", "window", 0)]


@pytest.mark.parametrize("far", [0.0, 7.0], ids=["inside", "beyond"])
@pytest.mark.parametrize("shape", [(1, 17, 33), (2, 16, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode,route,flags", MDCN_CASES)
def test_mdcn(mode, route, flags, shape, far, monkeypatch):
    """lib.mdcn at C = 67 and its census.  (1, 17, 33): 2 x 3 pack tiles, one row and one column beyond whole tiles - the window DMA's
    border classes, the zero page, the last pixel of the compact tail; (2, 16, 16): one whole tile per sample (beyond: samples leave the
    image, not the window).  fp32 and amp16: conv3x3 +
    the fp32 LDS-window DCN"""
    B, H, W = shape

    def call(inp):
        y = lib.mdcn(*inp, dtype=mode, flags=flags, route=route)
        census = lib.mdcn_census(B, 67, H, W, dtype=mode, flags=flags, device=DEV)
        if far and census[0] is not None and can_leave_window(H, W):   # +-7 px against a window of +-2: taps 2, 5 and 8 leave it
            assert census[0]["fixup_wave_taps"] > 0 and census[0]["samples_outside_window"] > 0, census
        return {"y": y, "census": census}
    run_case(monkeypatch, f"mdcn {mode} {route} flags {flags} {shape} far {far}", call, mdcn_case(H * W + int(far), B, H, W, far))


@pytest.mark.parametrize("C", [67, 11])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_deform_conv2d(mode, C, monkeypatch):
    """lib.deform_conv2d at (1, 9, 33): C = 67 - the LDS-window kernels (fp32: deform_f32w, bf16: the pack layout with offsets read from
    memory), less than a tile high, two tiles and one column wide; C = 11 - the global-gather kernel.  Offsets up to +-6 px: beyond the
    window and beyond the image"""
    g = torch.Generator().manual_seed(900 + C)
    B, H, W = 1, 9, 33
    inp = [torch.randn(B, C, H, W, generator=g), (torch.rand(B, 18, H, W, generator=g) * 2 - 1) * 6.0, torch.rand(B, 9, H, W, generator=g),
           torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9), torch.randn(C, generator=g) * 0.1]
    run_case(monkeypatch, f"deform_conv2d {mode} C {C}", lambda t: lib.deform_conv2d(*t, dtype=mode), inp)


# one or two cases per family of tests/test_gpu_conv_rounding_model.py, each at a shape with tile or strip remainders
CONV_CASES = {
    "tile": [({}, 11, 27, 1, (5, 7), "none"), ({}, 8, 16, 2, (33, 47), "relu")],
    "persist16": [({}, 64, 32, 1, (17, 33), "relu"), (NO_RING, 64, 40, 1, (17, 33), "none")],
    "persist32": [(OLD32, 64, 32, 1, (17, 33), "relu"), ({}, 67, 27, 1, (33, 47), "none")],
    "ring2": [({}, 64, 64, 1, (17, 125), "relu"), ({}, 64, 33, 1, (3, 61), "none")],
    "ring3": [({}, 67, 64, 1, (17, 125), "relu"), ({}, 65, 64, 1, (2, 124), "none")],
    "s2ring": [({}, 64, 128, 2, (37, 53), "relu"), ({}, 64, 100, 2, (1, 7), "none")],
    "wreg": [({}, 128, 256, 2, (19, 67), "relu"), ({}, 192, 250, 1, (1, 5), "none")],
    "light": [({}, 32, 3, 1, (21, 45), "tanh01")],
}
ACT = {"none": lib.ACT_NONE, "relu": lib.ACT_RELU, "tanh01": lib.ACT_TANH01}


@pytest.mark.parametrize("family,mode", [(f, d) for f in CONV_CASES for d in FAMILIES[f][0]])
def test_conv3x3(family, mode, monkeypatch):
    """lib.conv3x3, B = 2, per kernel family (asserted with family_of, as the rounding-model tests do)"""
    assert set(ALL_SWITCHES) >= {k for env, *_ in CONV_CASES[family] for k in env}
    for env, cin, cout, stride, (H, W), act in CONV_CASES[family]:
        set_env(monkeypatch, env)
        expect_family(family, cin, cout, stride, mode, env, act)
        g = torch.Generator().manual_seed(cin * 131 + cout)
        inp = [torch.randn(2, cin, H, W, generator=g)] + conv_params(g, ((cout, cin),))
        run_case(monkeypatch, f"conv3x3 {family} {mode} {cin}->{cout} s{stride} {act} 2x{H}x{W}",
                 lambda t: lib.conv3x3(*t, stride=stride, act=ACT[act], dtype=mode), inp)


@pytest.mark.parametrize("shape", [(2, 3, 9, 37), (1, 3, 8, 40)], ids=lambda s: "x".join(map(str, s)))
def test_warp(shape, monkeypatch):
    """lib.warp takes no workspace: guarded inputs and output only.  W % 4 != 0 (one pixel per thread) and W % 4 == 0 (four); flows of
    up to +-60 px leave the frame on every side (finite flows: the result is finite)"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(W)
    inp = [torch.randn(B, C, H, W, generator=g), (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 60.0]
    run_case(monkeypatch, f"warp {shape}", lambda t: lib.warp(t[0], t[1]), inp, has_workspace=False)


def test_frame_metrics(monkeypatch):
    """lib.frame_metrics_u8 at 12 x 60 x 3: 2 x 50 windows, two tiles of 32 windows across per channel - the per-tile partial sums in
    the workspace (96 bytes)"""
    g = torch.Generator().manual_seed(12)
    a = torch.randint(0, 256, (1, 12, 60, 3), generator=g, dtype=torch.uint8)
    b = (a.int() + torch.randint(-9, 10, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    assert lib.load().emavfi_frame_metrics_workspace_bytes(1, 12, 60, 3) == 3 * 2 * 16
    run_case(monkeypatch, "frame_metrics_u8 1x12x60x3", lambda t: lib.frame_metrics_u8(t[0], t[1]), [a, b])
