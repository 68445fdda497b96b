"""Every compute entry, captured into a graph once and replayed, gives what the eager call gives.

The statement is the same for every case and has no tolerance (tests/graph_harness.py, replay_case): after one warm-up the entry is
captured with torch.cuda.graph on a side stream - one linear sequence, model.pipeline = 1, no queue or graph setting - and replayed
four times: on the captured content with the stream's whole workspace filled with 0xFF and every returned tensor with a sentinel, on
new content over a workspace of 0x7B, once more with nothing touched, and on the first content again.  Every replay equals the eager
call on the same content bit for bit in every output and tap, and word for word in every census row and route; the capture is handed
no workspace the warm-up had not made.  What tests/test_gpu_workspace.py says about an eager call - independent of what the workspace
held - is said here about a replay, where the entry's own clears are nodes of the graph and not calls; the third replay is the one
that sees a counter that was not cleared.

The cases are test_gpu_workspace.py's builders at the smallest of its shapes that still reach the paths named there; content B is the
same builder with another seed.  All frames and weights are synthetic; nothing is read from the reference."""
import math

import pytest
import torch

import test_gpu_workspace as tw
from emavfi import lib
from graph_harness import GraphHooks, replay_case
from test_gpu_conv_rounding_model import ALL_SWITCHES, FAMILIES, expect_family, set_env
from test_gpu_pack_adapt import block1_scaled, routed, same
from test_gpu_pack_adapt import frames as adapt_frames
from test_gpu_parity import make_model
from test_gpu_workspace import (ACT, CONV_CASES, MDCN_CASES, MODES, SWITCHES, can_leave_window, conv_params, forward_census, forward_enqueue,
                                frames, leaves, mdcn_case, model_of)
from workspace_harness import DEV, _snapshot, bits, debug_switch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 23, 37), (1, 17, 125)]   # odd at every pyramid level, scalar warp, pack-tile remainders | two strips and a column, a row beyond a tile
SEED_B = 29                            # content B of the forward cases (content A: test_gpu_workspace.frames' 17)
ids = lambda s: "x".join(map(str, s))


def forward_case(label, model, shape, kind):
    replay_case(label, forward_enqueue(model), frames(*shape, kind), frames(*shape, kind, seed=SEED_B),
                read_after=forward_census(model, leaves(kind, shape)))


@pytest.mark.parametrize("kind", ["natural", "stress"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("mode", MODES)
def test_forward(mode, shape, kind, monkeypatch):
    """EMA_VFI(mid_channels = 64)(f1, f2, return_taps=True): out, feat, ctx, flow, warped, fused_0..2 and pack_census().  stress: every
    block with a census counted fix-up wave-taps and samples outside the window in every read - an accumulating census of zeros
    would pass"""
    set_env(monkeypatch, {})
    forward_case(f"forward {mode} {shape} {kind}", model_of(64, mode, kind), shape, kind)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_forward_gather_route(mode, shape, monkeypatch):
    """pack_policy = "gather": the window-free kernel in every block, stress weights"""
    set_env(monkeypatch, {})
    model = model_of(64, mode, "stress")
    model.pack_policy = "gather"
    try:
        forward_case(f"forward {mode} gather {shape} stress", model, shape, "stress")
    finally:
        model.pack_policy = "window"


def fresh_model(mid, mode, kind):
    """model_of's model, but nobody else's: an adaptive forward keeps a route state per stream"""
    key = (mid, mode, kind)
    tw._models.pop(key, None)
    model = model_of(mid, mode, kind)
    tw._models.pop(key)
    return model


class EagerTwin:
    """The reference of an adaptive case: a second model with the same weights and the same warm-up history (one forward on content A),
    stepped eagerly through the contents the replays see, on the default stream - its own workspace and its own route state"""

    def __init__(self, model, warm_up, leaves_window):
        self.model, self.warm_up, self.steps = model, warm_up, []
        self.enqueue, self.read = forward_enqueue(model), adaptive_read(model, leaves_window)

    def __call__(self, step, inputs):
        if not self.steps:
            self.enqueue([t.clone() for t in self.warm_up])
        res = _snapshot(self.enqueue([t.clone() for t in inputs]))
        torch.cuda.synchronize()
        res.update(self.read())
        self.steps.append(res)
        return res


def adaptive_read(model, leaves_window):
    census = forward_census(model, leaves_window)
    return lambda: {**census(), "routes": model.pack_routes()}


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_forward_adaptive_route(mode, shape, monkeypatch):
    """pack_adapt = (0.75, 0.65), stress weights: the routed pack reads its route word on the device and route_select writes the next
    one from this forward's census, so a replay's result depends on the replays before it.  After every replay the frames and taps,
    pack_routes() and pack_census() equal those of the eager twin after the same sequence of contents"""
    set_env(monkeypatch, {})
    replayed, twin = fresh_model(64, mode, "stress"), fresh_model(64, mode, "stress")
    for m in (replayed, twin):
        m.pack_adapt = (0.75, 0.65)
    a, b = [t.to(DEV) for t in frames(*shape, "stress")], [t.to(DEV) for t in frames(*shape, "stress", seed=SEED_B)]
    reference = EagerTwin(twin, a, leaves("stress", shape))
    replay_case(f"forward {mode} adapt {shape} stress", forward_enqueue(replayed), a, b, read_after=adaptive_read(replayed, leaves("stress", shape)),
                reference=reference)
    ra, rb = reference.steps[0], reference.steps[1]
    assert all(not torch.equal(bits(ra[k]), bits(rb[k])) for k in ra if torch.is_tensor(ra[k])), "the two contents give the same tap"
    assert all(r is not None for r in ra["routes"]), ra["routes"]


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_forward_unfused_launches(name, monkeypatch):
    """(2, 23, 37) in bf16, stress, with one debug switch set: the launches test_gpu_workspace.test_forward_unfused_launches names"""
    set_env(monkeypatch, {})
    launches = lambda: [n for n, _, _ in lib.forward_launches(3, 64, 3, 2, 23, 37, "bf16")]
    default = launches()
    with debug_switch(SWITCHES[name]):
        assert launches() != default, f"{name} selects no other launch at (2, 23, 37) in bf16: {default}"
        forward_case(f"forward bf16 {name} stress", model_of(64, "bf16", "stress"), (2, 23, 37), "stress")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_forward_mid8(mode, monkeypatch):
    """mid_channels = 8 at (2, 23, 37): the generic tile kernels, conv3x3 + the global-gather DCN per attention block"""
    set_env(monkeypatch, {})
    forward_case(f"forward mid 8 {mode}", model_of(8, mode, "natural"), (2, 23, 37), "natural")


def test_adaptive_threshold_is_not_crossed_by_replays(monkeypatch):
    """The one case with a number.  block1_scaled(8.0) on frames(32, 2, 64, 96) in bf16: block 1's fix-up share s is measured eagerly with
    pack_adapt = (1.0, 0.99), as test_gpu_pack_adapt.test_hysteresis_and_reset does, and must lie in 0.05 < s < 0.6 above the other
    blocks' (measured on an MI355X: s = 0.25347, the others 0.00231 and 0; the threshold is then 0.38021).  With pack_adapt = (min(0.95, 1.5 s), 0.0) captured and replayed four times on the same content, after
    EVERY replay block 1 ran and will run the window route with no switch, its share is s to 1e-5 (that file's figure) and the frame is
    emavfi_forward_routed's with mask 0.  A census that accumulated over replays would read 2 s > 1.5 s after the second."""
    set_env(monkeypatch, {})
    sd = block1_scaled(8.0)
    f1, f2 = adapt_frames(32, 2, 64, 96)
    probe = make_model(sd, dtype="bf16")
    probe.pack_adapt = (1.0, 0.99)   # nothing can switch: a probe of the shares
    with torch.no_grad():
        probe(f1, f2)
    shares = [r["fixup_share"] for r in probe.pack_routes()]
    s = shares[1]
    print(f"fix-up shares {shares}")
    assert 0.05 < s < 0.6 and max(shares[0], shares[2]) < s, shares
    m = make_model(sd, dtype="bf16")
    m.pipeline = 1
    m.pack_adapt = (min(0.95, 1.5 * s), 0.0)
    window = routed(m, f1, f2, "bf16", 0)
    h = GraphHooks()
    with h.on_stream():
        m(f1, f2)                    # the warm-up: weights packed, the route state of the capture stream made
    h.synchronize()
    g, out = h.capture(lambda: m(f1, f2))
    for k in range(4):
        h.replay(g)
        h.synchronize()
        with h.on_stream():
            r = m.pack_routes()[1]
        print(f"replay {k + 1}: block 1 {r}")
        assert r["ran"] == "window" and r["next"] == "window" and r["switches"] == 0, (k, r)
        assert abs(r["fixup_share"] - s) < 1e-5, (k, r, s)
        assert same(out, window), k


# ------------------------------------------------------------------------------------------------ stage entries
def seeded(build):
    """contents A and B of a builder that takes a torch generator"""
    return build(torch.Generator().manual_seed(101)), build(torch.Generator().manual_seed(202))


@pytest.mark.parametrize("pool", ["poolfuse", "no_poolfuse"])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "amp16"])
def test_context(mode, pool, monkeypatch):
    """lib.context at mid_channels 64, (2, 37, 53): the per-call blob and the zero weights of the folded context half are cleared by the entry"""
    set_env(monkeypatch, {})
    build = lambda g: [torch.randn(2, 64, 37, 53, generator=g).relu()] + conv_params(g, ((128, 64), (256, 128), (256, 256))) \
        + [torch.randn(64, 256, generator=g) / 16, torch.randn(64, generator=g) * 0.1]
    with debug_switch(lib.SW_NO_POOLFUSE, pool == "no_poolfuse"):
        replay_case(f"context {mode} {pool}", lambda inp: lib.context(inp[0], inp[1:], dtype=mode), *seeded(build))


@pytest.mark.parametrize("tail", ["tailfuse", "no_tailfuse"])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16", "amp16"])
def test_reconstruct(mode, tail, monkeypatch):
    """lib.reconstruct at mid_channels 64, (1, 17, 125): two strips and one column"""
    set_env(monkeypatch, {})
    build = lambda g: [torch.randn(1, 67, 17, 125, generator=g)] + conv_params(g, ((64, 67), (32, 64), (3, 32)))
    with debug_switch(lib.SW_NO_TAILFUSE, tail == "no_tailfuse"):
        replay_case(f"reconstruct {mode} {tail}", lambda inp: lib.reconstruct(inp[0], inp[1:], dtype=mode), *seeded(build))


@pytest.mark.parametrize("far", [0.0, 7.0], ids=["inside", "beyond"])
@pytest.mark.parametrize("mode,route,flags", MDCN_CASES)
def test_mdcn(mode, route, flags, far):
    """lib.mdcn at C = 67, (1, 17, 33), and lib.mdcn_census read after every replay: the per-call blob and its census block"""
    B, H, W = 1, 17, 33

    def read():
        census = lib.mdcn_census(B, 67, H, W, dtype=mode, flags=flags, device=DEV)
        if far and census[0] is not None and can_leave_window(H, W):   # +-7 px against a window of +-2: taps 2, 5 and 8 leave it
            assert census[0]["fixup_wave_taps"] > 0 and census[0]["samples_outside_window"] > 0, census
        return {"census": census}
    replay_case(f"mdcn {mode} {route} flags {flags} far {far}", lambda inp: {"y": lib.mdcn(*inp, dtype=mode, flags=flags, route=route)},
                mdcn_case(H * W + int(far), B, H, W, far), mdcn_case(7 * H * W + int(far), B, H, W, far), read_after=read)


@pytest.mark.parametrize("C", [67, 11])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_deform_conv2d(mode, C):
    """lib.deform_conv2d at (1, 9, 33), offsets up to +-6 px - beyond the window and beyond the image: the zero page"""
    build = lambda g: [torch.randn(1, C, 9, 33, generator=g), (torch.rand(1, 18, 9, 33, generator=g) * 2 - 1) * 6.0, torch.rand(1, 9, 9, 33, generator=g),
                       torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9), torch.randn(C, generator=g) * 0.1]
    replay_case(f"deform_conv2d {mode} C {C}", lambda t: lib.deform_conv2d(*t, dtype=mode), *seeded(build))


@pytest.mark.parametrize("family,mode", [(f, d) for f in CONV_CASES for d in FAMILIES[f][0]])
def test_conv3x3(family, mode, monkeypatch):
    """lib.conv3x3, B = 2: the first case of the family in test_gpu_workspace.CONV_CASES, the family asserted as there"""
    env, cin, cout, stride, (H, W), act = CONV_CASES[family][0]
    assert set(ALL_SWITCHES) >= set(env)
    set_env(monkeypatch, env)
    expect_family(family, cin, cout, stride, mode, env, act)
    build = lambda g: [torch.randn(2, cin, H, W, generator=g)] + conv_params(g, ((cout, cin),))
    replay_case(f"conv3x3 {family} {mode} {cin}->{cout} s{stride} {act} 2x{H}x{W}",
                lambda t: lib.conv3x3(*t, stride=stride, act=ACT[act], dtype=mode), *seeded(build))


@pytest.mark.parametrize("shape", [(2, 3, 9, 37), (1, 3, 8, 40)], ids=ids)
def test_warp(shape):
    """lib.warp takes no workspace: the outputs' sentinel and the new content only.  W % 4 != 0 and W % 4 == 0"""
    B, C, H, W = shape
    build = lambda g: [torch.randn(B, C, H, W, generator=g), (torch.rand(B, 2, H, W, generator=g) * 2 - 1) * 60.0]
    replay_case(f"warp {shape}", lambda t: lib.warp(t[0], t[1]), *seeded(build))


def byte_pair(g, shape, spread=9):
    a = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return [a, (a.int() + torch.randint(-spread, spread + 1, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)]


def test_frame_metrics():
    """lib.frame_metrics_u8 at 12 x 60 x 3: the per-tile partial sums in the workspace"""
    replay_case("frame_metrics_u8 1x12x60x3", lambda t: lib.frame_metrics_u8(t[0], t[1]), *seeded(lambda g: byte_pair(g, (1, 12, 60, 3))))


# ------------------------------------------------------------------------------------------------ counters and extremes kept on the device
def test_static_guard_counts():
    """lib.static_guard_frames with counts, 2 x 40 x 56 x 3, radius 1, tol 2: the counts start from zero in every replay.  The guard
    writes into its destination, so the call copies a static destination first"""
    def build(g):
        srcs = torch.randint(0, 256, (3, 40, 56, 3), generator=g, dtype=torch.uint8)
        srcs[1], srcs[2] = srcs[0], srcs[0]
        srcs[1, 5:22, 9:41] = torch.randint(0, 256, (17, 32, 3), generator=g, dtype=torch.uint8)     # what moved between the sources
        srcs[2, 18:37, 3:30] = torch.randint(0, 256, (19, 27, 3), generator=g, dtype=torch.uint8)
        return [torch.randint(0, 256, (2, 40, 56, 3), generator=g, dtype=torch.uint8), srcs]

    def call(inp):
        dst, counts = inp[0].clone(), torch.empty(2, dtype=torch.int32, device=inp[0].device)
        lib.static_guard_frames(dst, inp[1], [(0, 1), (1, 2)], (40, 56), C=3, radius=1, tol=2, counts=counts)
        return {"dst": dst, "counts": counts}
    a, b = seeded(build)
    b[1][1, 5:30, 9:41] = 255 - b[1][0, 5:30, 9:41]   # another area moves in content B: other counts
    replay_case("static_guard_frames counts", call, a, b)


def test_agreement_guard_counts():
    """lib.agreement_guard_f32 with counts at (2, 3, 23, 37), radius 1"""
    def build(g):
        u = torch.rand(2, 3, 23, 37, generator=g)
        v = u + (torch.rand(2, 3, 23, 37, generator=g) < 0.05) * 0.3 + (torch.rand(2, 3, 23, 37, generator=g) - 0.5) * 0.01
        return [u, v, torch.randn(2, 3, 23, 37, generator=g), torch.randn(2, 3, 23, 37, generator=g)]

    def call(inp):
        counts = torch.empty(2, dtype=torch.int32, device=inp[0].device)
        return {"out": lib.agreement_guard_f32(*inp, 0.05, 1, counts=counts), "counts": counts}
    replay_case("agreement_guard_f32 counts", call, *seeded(build))


def test_active_bounds():
    """lib.active_bounds at 2 x 23 x 37 x 3: the four extremes of a frame are folded by atomics onto words an init launch wrote"""
    def build(g):
        img = torch.zeros(2, 23, 37, 3, dtype=torch.uint8)
        for k in range(2):
            t, l = (int(v) for v in torch.randint(1, 8, (2,), generator=g))
            hh, ww = (int(v) for v in torch.randint(3, 12, (2,), generator=g))
            img[k, t:t + hh, l:l + ww] = torch.randint(40, 256, (hh, ww, 3), generator=g, dtype=torch.uint8)
        return [img]
    replay_case("active_bounds", lambda t: lib.active_bounds(t[0], level=16), *seeded(build))


def test_frame_diff_cells():
    """lib.frame_diff_cells at 2 x 40 x 56 x 3: cells of the 32 x 32 grid with partial rows and columns"""
    replay_case("frame_diff_cells", lambda t: lib.frame_diff_cells(t[0], t[1]), *seeded(lambda g: byte_pair(g, (2, 40, 56, 3), 40)))


def test_luma_signature():
    """lib.luma_signature_u8 at 2 x 40 x 56 x 3"""
    build = lambda g: [torch.randint(0, 256, (2, 40, 56, 3), generator=g, dtype=torch.uint8)]
    replay_case("luma_signature_u8", lambda t: lib.luma_signature_u8(t[0]), *seeded(build))


def test_align_search():
    """lib.align_search over the signatures of 2 x 3 x 32 x 48 frames, 4 cells of radius: a second witness of the clearing launch the
    entry was given (profiles/r28_align.md) - the sums of one replay must not show in the next"""
    def build(g, pans):
        picture = torch.rand(2, 3, 64, 80, generator=g)
        crop = lambda k, dy, dx: picture[k, :, 16 + dy:48 + dy, 16 + dx:64 + dx]
        return [torch.stack([crop(k, 0, 0) for k in range(2)]).contiguous(), torch.stack([crop(k, *pans[k]) for k in range(2)]).contiguous()]

    def call(inp):
        return lib.align_search(lib.align_signature_f32(inp[0]), lib.align_signature_f32(inp[1]), 4, 512)
    replay_case("align_search", call, build(torch.Generator().manual_seed(101), ((8, -12), (-4, 16))),
                build(torch.Generator().manual_seed(202), ((-12, 4), (16, -8))))
