"""The adaptive per-block route of the 16-bit attention blocks (include/emavfi.h, emavfi_forward_adaptive; EMA_VFI.pack_adapt): the
routed pack (deform_route3.inl) reads its block's route word on the device, and route_select writes the next forward's route from this
forward's census.  Where the window route has a fix-up the two routes' frames differ in low bits, so bit-identity with
emavfi_forward_routed under a given mask says which kernel body ran."""
import pytest
import torch

from emavfi import lib, synth
from test_gpu_mdcn import DEV
from test_gpu_parity import load_golden, make_model, psnr

pytestmark = pytest.mark.gpu


def routed(m, f1, f2, dtype, mask):
    """emavfi_forward_routed with `mask` on the current stream (the reference frames of each route)"""
    L, dt = lib.load(), lib.dtype_code(dtype)
    B, C, H, W = f1.shape
    packed = m.packed_weights(dt, f1.device)
    nws = L.emavfi_workspace_bytes(3, 64, 3, B, H, W, dt)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(f1)
    lib.check(L.emavfi_forward_routed(3, 64, 3, packed.data_ptr(), packed.numel(), f1.data_ptr(), f2.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                      nws, B, H, W, dt, None, None, None, 0, mask, lib._stream()), "emavfi_forward_routed")
    torch.cuda.synchronize()
    return out


def block1_scaled(s_px):
    """default synthetic weights, attention block 1's offset_conv from the recipe at about +-s_px"""
    sd = synth.synthetic_state_dict(seed=0)
    big = synth.synthetic_state_dict(seed=0, offset_std=0.5 * s_px, offset_bias=0.5 * s_px)
    for k in ("weight", "bias"):
        sd[f"attention_blocks.1.offset_conv.{k}"] = big[f"attention_blocks.1.offset_conv.{k}"]
    return sd


def frames(seed, B, H, W):
    return tuple(t.to(DEV) for t in synth.synthetic_frames(seed, B, H, W, "natural"))


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_small_offsets_stay_on_the_window_and_equal_emavfi_forward(dtype):
    m = make_model(synth.synthetic_state_dict(seed=0), dtype=dtype)
    plain = make_model(synth.synthetic_state_dict(seed=0), dtype=dtype)
    m.pack_adapt = (0.75, 0.65)
    for k, (B, H, W) in enumerate(((1, 37, 53), (2, 64, 96), (1, 17, 130))):
        f1, f2 = frames(20 + k, B, H, W)
        with torch.no_grad():
            for _ in range(2):
                a = m(f1, f2)
                b = plain(f1, f2)
                torch.cuda.synchronize()
                assert same(a, b), (dtype, B, H, W)
        rows = m.pack_routes()
        assert all(r["ran"] == "window" and r["next"] == "window" and r["switches"] == 0 for r in rows), rows
        assert all(r["route"] == "window" for r in m.pack_census())


LARGE = 30.0   # px: block 1's offsets leave the window almost everywhere


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_large_offsets_on_one_block_switch_it_to_gather(dtype):
    sd = block1_scaled(LARGE)
    f1, f2 = frames(31, 2, 64, 96)
    probe = make_model(sd, dtype=dtype)
    with torch.no_grad():
        probe(f1, f2)
    shares = [r["fixup_share"] for r in probe.pack_census()]
    assert shares[1] >= 0.85 and shares[0] < 0.65 and shares[2] < 0.65, shares
    m = make_model(sd, dtype=dtype)
    m.pack_adapt = (0.75, 0.65)
    w0, w2 = routed(m, f1, f2, dtype, 0), routed(m, f1, f2, dtype, 0b010)
    assert not same(w0, w2)   # the routes differ where the window has a fix-up: the comparisons below see which one ran
    with torch.no_grad():
        a1 = m(f1, f2).clone()
        r1 = m.pack_routes()
        c1 = m.pack_census()
        a2 = m(f1, f2).clone()
        r2 = m.pack_routes()
        c2 = m.pack_census()
    torch.cuda.synchronize()
    assert same(a1, w0) and same(a2, w2)
    assert [r["ran"] for r in r1] == ["window"] * 3 and [r["next"] for r in r1] == ["window", "gather", "window"], r1
    assert [r["ran"] for r in r2] == ["window", "gather", "window"] and [r["next"] for r in r2] == ["window", "gather", "window"], r2
    assert [r["switches"] for r in r2] == [0, 1, 0]
    assert abs(r1[1]["fixup_share"] - shares[1]) < 1e-5 and abs(r2[1]["fixup_share"] - shares[1]) < 1e-5
    assert [r["route"] for r in c1] == ["window"] * 3 and [r["route"] for r in c2] == ["window", "gather", "window"]


def test_hysteresis_and_reset():
    sd = block1_scaled(8.0)
    f1, f2 = frames(32, 2, 64, 96)
    m = make_model(sd, dtype="bf16")
    m.pack_adapt = (1.0, 0.99)   # nothing can switch: a probe of the shares
    with torch.no_grad():
        m(f1, f2)
    s = [r["fixup_share"] for r in m.pack_routes()]
    print("shares", s)
    assert s[1] - max(s[0], s[2]) > 0.1 and 0.05 < s[1] < 0.85, s
    lo = max(s[0], s[2])

    def step(enter, leave):
        m.pack_adapt = (enter, leave)   # (new thresholds keep the state)
        with torch.no_grad():
            m(f1, f2)
        return m.pack_routes()

    r = step((lo + s[1]) / 2, lo / 2 if lo > 0 else 0.0)            # share >= enter on the window: to gather
    assert [x["next"] for x in r] == ["window", "gather", "window"] and r[1]["switches"] == 1, r
    r = step(min(1.0, s[1] + 0.1), max(0.0, s[1] - 0.05))          # leave < share < enter: keeps gather
    assert r[1]["ran"] == "gather" and r[1]["next"] == "gather" and r[1]["switches"] == 1, r
    r = step(min(1.0, s[1] + 0.1), s[1])                            # share <= leave on gather: back to the window
    assert r[1]["ran"] == "gather" and r[1]["next"] == "window" and r[1]["switches"] == 2, r
    r = step(min(1.0, s[1] + 0.1), max(0.0, s[1] - 0.05))          # between again, now on the window: keeps the window
    assert r[1]["ran"] == "window" and r[1]["next"] == "window" and r[1]["switches"] == 2, r
    assert [x["switches"] for x in r] == [0, 2, 0]
    m.pack_adapt = ((lo + s[1]) / 2, 0.0)
    with torch.no_grad():
        m(f1, f2)
    assert m.pack_routes()[1]["next"] == "gather"
    m.load_state_dict(sd)   # the state goes back to the starting route (pack_policy "window")
    r = m.pack_routes()
    assert all(x["next"] == "window" and x["switches"] == 0 and x["ran"] == "window" for x in r), r
    m.pack_policy = "gather"   # a new starting route resets as well
    r = m.pack_routes()
    assert all(x["next"] == "gather" and x["switches"] == 0 for x in r), r


def test_graph_capture_adapts_on_replay():
    sd_big = block1_scaled(LARGE)
    f1, f2 = frames(33, 2, 64, 96)
    m = make_model(synth.synthetic_state_dict(seed=0), dtype="bf16")
    m.pack_adapt = (0.75, 0.65)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            m(f1, f2)
    torch.cuda.current_stream().wait_stream(s)
    m.load_state_dict(sd_big)   # large offsets; the state of `s` back to the window route
    m.packed_weights(lib.BF16, f1.device)
    torch.cuda.synchronize()
    w0, w2 = routed(m, f1, f2, "bf16", 0), routed(m, f1, f2, "bf16", 0b010)
    assert not same(w0, w2)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, stream=s):
        out = m(f1, f2)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, w0)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, w2)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, w2)


def test_capture_without_a_state_asks_for_a_warm_up():
    f1, f2 = frames(34, 1, 32, 48)
    m = make_model(synth.synthetic_state_dict(seed=0), dtype="bf16")
    m.packed_weights(lib.BF16, f1.device)
    m.pack_adapt = (0.75, 0.65)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="warm-up"):
        with torch.no_grad(), torch.cuda.graph(g, stream=s):
            m(f1, f2)


@pytest.mark.parametrize("dtype", ["fp32", "amp16", "fp32x3"])
def test_modes_without_a_gather_route_run_their_plain_forward(dtype):
    sd = block1_scaled(LARGE)
    f1, f2 = frames(35, 1, 48, 64)
    m, plain = make_model(sd, dtype=dtype), make_model(sd, dtype=dtype)
    m.pack_adapt = (0.75, 0.65)
    with torch.no_grad():
        for _ in range(2):
            a, b = m(f1, f2), plain(f1, f2)
            torch.cuda.synchronize()
            assert torch.equal(a, b)
    assert m.pack_routes() == [None] * 3
    st = next(iter(m._route_states.values())).cpu()
    assert int(st[4]) == 0 and int(st[3]) == 0   # no selector ran: no forward counted


def test_independent_streams_and_pipeline():
    sd = block1_scaled(LARGE)
    f1, f2 = frames(36, 4, 64, 96)
    m = make_model(sd, dtype="bf16")
    m.pack_adapt = (0.75, 0.65)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(s1):
            m(f1, f2)
            m(f1, f2)
            r1 = m.pack_routes()
        with torch.cuda.stream(s2):
            m(f1, f2)
            r2 = m.pack_routes()
    assert r1[1]["ran"] == "gather" and r1[1]["switches"] == 1
    assert r2[1]["ran"] == "window" and r2[1]["next"] == "gather" and r2[1]["switches"] == 1
    # pipeline = 2 under adaptation is one sequence: the same frames as pipeline = 1, forward by forward
    one, two = make_model(sd, dtype="bf16"), make_model(sd, dtype="bf16")
    for x in (one, two):
        x.pack_adapt = (0.75, 0.65)
    two.pipeline = 2
    with torch.no_grad():
        for _ in range(3):
            a, b = one(f1, f2), two(f1, f2)
            torch.cuda.synchronize()
            assert same(a, b)
    assert two.pack_routes() == one.pack_routes()


def test_forward_adaptive_refuses_a_state_of_another_model():
    L = lib.load()
    st = torch.zeros(L.emavfi_route_state_bytes() // 4, dtype=torch.int32, device=DEV)
    lib.check(L.emavfi_route_state_init(st.data_ptr(), 2, 0, lib._stream()), "emavfi_route_state_init")
    torch.cuda.synchronize()
    w = st.cpu()
    assert int(w[0]) & 0xffffffff == 0x52544531 and int(w[1]) == 2 and int(w[4]) == 0
    rc = L.emavfi_forward_adaptive(3, 64, 3, None, 0, None, None, None, None, 0, 1, 32, 32, lib.BF16, None, None, None, 0, st.data_ptr(),
                                   0.75, 0.65, None)
    assert rc == -1 and "num_blocks" in lib.last_error()


@pytest.mark.parametrize("adapt", [(0.75, 0.65), (0.5, 0.4)])
def test_adaptive_forward_vs_reference_run_large_offsets(adapt):
    """test_gpu_parity's gates for the window route on large_offsets16.npz, for the adaptive bf16 forward (its first three forwards).
    Its blocks' fix-up shares are about 0.55: the default thresholds keep the window, (0.5, 0.4) move every block to gather."""
    g = load_golden("large_offsets16.npz")
    B, H, W, seed, kind = (int(v) for v in g["off16.meta"])
    std, bias = (float(v) for v in g["off16.recipe"])
    sd = synth.synthetic_state_dict(seed=0, offset_std=std, offset_bias=bias)
    f1, f2 = synth.synthetic_frames(seed, B, H, W, "natural")
    m = make_model(sd, dtype="bf16")
    m.pack_adapt = adapt
    ref = torch.from_numpy(g["off16.val.out"])
    for k in range(3):
        with torch.no_grad():
            out = m(f1.to(DEV), f2.to(DEV))
        got = out.contiguous().view(-1).cpu()[torch.from_numpy(g["off16.pos.out"])]
        p, err = psnr(got, ref), (got - ref).abs().max().item()
        routes = m.pack_routes()
        print(f"adaptive {adapt} forward {k}, large offsets: PSNR {p:.1f} dB, max-abs {err:.3e}; routes {routes}")
        assert p >= 52.0 and err <= 2.5e-2
    want = "window" if adapt[0] > 0.6 else "gather"
    assert all(r["ran"] == want for r in routes), routes
