"""The coarse flow on the device (include/emavfi.h, "COARSE FLOW DEFINITION"): emavfi_downscale_f32 and emavfi_upsample_flow_f32 against the
numpy oracle (tests/coarse_flow_oracle.py) bit for bit, on every access width and between guard words, and past 2^32 bytes; the forward split
at its flow (emavfi_forward_flow, emavfi_forward_given_flow) against the plain forward and its taps, bit for bit, in every mode and on both
pack routes; EMA_VFI.flow_scale against the four entries composed by hand, plain, ensembled and bordered; the two workspace entries under
the workspace contract; the fp32 coarse forward against the CPU oracle's stages at the frame gate; the harness and the command line.
Every comparison but the one against the CPU oracle is an equality of 32-bit words or of bytes."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
from oracle import emavfi_oracle
import coarse_flow_oracle as oracle
from workspace_harness import run_case

pytestmark = pytest.mark.gpu

GUARD = 64                      # words of guard on either side: 256 bytes, so the band keeps the tensor's 16-byte alignment
GUARD_WORD = 0x7B7B7B7B
UNWRITTEN = 0x55AA55AA          # what a destination holds before a call: no generated word equals it
PLANES = 3                      # generated planes differ from one another
# wide path; scalar path with clamped edges; smaller than s = 4 and 8; the smallest; one row; one column of blocks at s = 8 beside wide loads
SHAPES = [(24, 40), (23, 37), (3, 5), (1, 1), (1, 16), (16, 8)]
MODES = ("fp32", "bf16", "fp16", "amp16", "fp32x3")


def words(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "words differ")


def placed(shape, off, values=None):
    """(buffer, view): a float32 view of `shape` inside a device word buffer between guard words, starting `off` words behind a 16-byte
    boundary; filled with `values` or, for a destination, with UNWRITTEN"""
    count = int(np.prod(shape))
    host = np.full(count + 2 * GUARD + off, GUARD_WORD, np.uint32)
    host[GUARD + off:GUARD + off + count] = UNWRITTEN if values is None else words(values).reshape(-1)
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    view = buf[GUARD + off:GUARD + off + count].view(torch.float32).view(shape)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return buf, view


def written_and_guarded(buf, view, what):
    torch.cuda.synchronize()
    w = words(buf.view(torch.float32))
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    rest = np.concatenate([w[:lo], w[lo + view.numel():]])
    assert rest.size >= 2 * GUARD and (rest == GUARD_WORD).all(), (what, "a guard word was written")
    assert not (w[lo:lo + view.numel()] == UNWRITTEN).any(), (what, "a word of the destination was not written")


# ---------------------------------------------------------------- 1. the two kernels against the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("s", oracle.SCALES)
def test_down_and_up_are_the_oracle_bit_for_bit(s, shape):
    H, W = shape
    Hs, Ws = oracle.coarse_size(H, W, s)
    assert lib.coarse_size(H, W, s) == (Hs, Ws)
    x = oracle.generated(H * 100 + W, PLANES * H * W).reshape(PLANES, H, W)
    p = oracle.generated(H * 100 + W + 1, PLANES * Hs * Ws).reshape(PLANES, Hs, Ws)
    assert not np.array_equal(x[0], x[1]) or H * W == 1
    want_down, want_up = oracle.down(x, s), oracle.up(p, (H, W), s)
    # (source offset, destination offset) in words behind a 16-byte boundary: dense; the plane base 4 bytes in on both; on either alone
    for soff, doff in ((0, 0), (1, 1), (1, 0), (0, 1)):
        what = (s, shape, soff, doff)
        _, xv = placed(x.shape, soff, x)
        dbuf, dv = placed(want_down.shape, doff)
        assert lib.downscale_f32(xv, s, out=dv) is dv
        written_and_guarded(dbuf, dv, what)
        same_words(dv, want_down, (what, "down"))
        _, pv = placed(p.shape, soff, p)
        ubuf, uv = placed(want_up.shape, doff)
        assert lib.upsample_flow_f32(pv, (H, W), s, out=uv) is uv
        written_and_guarded(ubuf, uv, what)
        same_words(uv, want_up, (what, "up"))
        same_words(xv, x, "the source is left as it was")
    # out allocated by the wrapper, over leading dimensions of any count
    same_words(lib.downscale_f32(torch.from_numpy(x).cuda().view(1, PLANES, 1, H, W), s), want_down.reshape(1, PLANES, 1, Hs, Ws), (s, shape))
    same_words(lib.upsample_flow_f32(torch.from_numpy(p).cuda()[1], (H, W), s), want_up[1], (s, shape))
    # the closed forms, on the device: a constant stays, a constant flow is scaled
    c = torch.full((2, H, W), 0.1, device="cuda")
    same_words(lib.downscale_f32(c, s), np.full((2, Hs, Ws), 0.1, np.float32), (s, shape, "down of a constant"))
    f = torch.full((2, Hs, Ws), -2.25, device="cuda")
    same_words(lib.upsample_flow_f32(f, (H, W), s), np.full((2, H, W), -2.25 * s, np.float32), (s, shape, "up of a constant"))


def test_tensors_past_2_pow_32_bytes():
    """flow [17][8190][8192] is 4.56e9 bytes: plane 16 straddles 2^32.  up writes it from a coarse tensor at s = 8, down reads it back at
    s = 8; sampled rows of sampled planes against the oracle"""
    planes, H, W, s = 17, 8190, 8192, 8
    Hs, Ws = oracle.coarse_size(H, W, s)
    assert planes * H * W * 4 > 1 << 32 and (1 << 32) // (H * W * 4) == 16 and (Hs, Ws) == (1024, 1024) and H % s != 0
    g = torch.Generator(device="cuda").manual_seed(5)
    p = torch.randn(planes, Hs, Ws, device="cuda", generator=g)
    flow = lib.upsample_flow_f32(p, (H, W), s)
    assert flow.shape == (planes, H, W)
    rows = np.array([0, 1, 3, 4, 5, 4099, 4100, H - 5, H - 4, H - 1])
    for pl in (0, 15, 16):
        want = oracle.up(p[pl].cpu().numpy(), (H, W), s, rows=rows)
        same_words(flow[pl][torch.from_numpy(rows).cuda()], want, ("up", pl))
    low = lib.downscale_f32(flow, s)
    assert low.shape == (planes, Hs, Ws)
    for pl in (0, 15, 16):
        for i0, i1 in ((0, 2), (511, 513), (Hs - 2, Hs)):                   # coarse rows [i0, i1): the last one is the clamped edge block
            slab = flow[pl, s * i0:min(s * i1, H)].cpu().numpy()
            same_words(low[pl, i0:i1], oracle.down(slab, s), ("down", pl, i0))


# ---------------------------------------------------------------- 2. the forward split at its flow
def build_model(mid, dtype, cls=EMA_VFI, seed=0):
    m = cls(mid_channels=mid, compute_dtype=dtype).cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=seed, mid_channels=mid), strict=True)
    m.pipeline = 1
    return m


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(mid, dtype):
        if (mid, dtype) not in cache:
            cache[(mid, dtype)] = build_model(mid, dtype)
        m = cache[(mid, dtype)]
        m.pack_policy, m.pack_adapt, m.flow_scale, m.ensemble, m.border = "window", None, None, None, None
        return m
    return get


def frames(B, H, W, seed=3):
    a, b = synth.synthetic_frames(seed, B, H, W, "natural")
    return a.contiguous().cuda(), b.contiguous().cuda()


def run(model, a, b, **kw):
    with torch.no_grad():
        return model(a, b, **kw)


def blob(model):
    dt = model._resolve_dtype()
    return model.packed_weights(dt, torch.device("cuda", torch.cuda.current_device())), dt


CASES = [(8, 24, 40), (8, 23, 37), (64, 40, 56)]


def stored_as(t, dtype):
    """what the `warped` tap can hold of fp32 values t: the tail of the fusion tensor is fp32 in the fp32-family modes and 16-bit in the
    16-bit ones (a bf16 model keeps it in f16 where its first pack is the one-launch kernel: either rounding is accepted)"""
    if dtype in ("fp32", "amp16", "fp32x3"):
        return [t]
    return [t.to(torch.float16).float()] + ([t.to(torch.bfloat16).float()] if dtype == "bf16" else [])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_flow_is_the_flow_tap(models, dtype, case):
    mid, H, W = case
    model = models(mid, dtype)
    a, b = frames(2, H, W)
    _, taps = run(model, a, b, return_taps=True)
    packed, dt = blob(model)
    flow = lib.forward_flow(packed, a, b, mid, 3, dt)
    assert flow.shape == (2, 2, H, W) and flow.dtype == torch.float32
    same_words(flow, taps["flow"], (dtype, case))
    out = torch.full((2, 2, H, W), float("nan"), device="cuda")
    assert lib.forward_flow(packed, a, b, mid, 3, dt, out=out) is out
    same_words(out, taps["flow"], (dtype, case, "into out"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", MODES)
def test_forward_given_its_own_flow_is_the_plain_forward(models, dtype, case):
    mid, H, W = case
    model = models(mid, dtype)
    a, b = frames(2, H, W)
    packed, dt = blob(model)
    routes = ("window", "gather") if mid == 64 and dtype in ("bf16", "fp16") else ("window",)     # where the gather route exists
    for route in routes:
        model.pack_policy = route
        gmask = 0b111 if route == "gather" else 0
        plain, taps = run(model, a, b, return_taps=True)
        if route == "gather":
            assert any(n.startswith("deform_gather") for n, _, _ in lib.forward_launches(3, mid, 3, 2, H, W, dtype, gather_blocks=gmask, flow="given"))
        out, mine = lib.forward_given_flow(packed, a, b, taps["flow"], mid, 3, dt, return_taps=True, gather_blocks=gmask)
        same_words(out, plain.float(), (dtype, case, route, "out"))
        assert list(mine) == ["feat", "warped", "fused_0", "fused_1", "fused_2"]
        for k, v in mine.items():
            same_words(v, taps[k], (dtype, case, route, k))
        same_words(lib.forward_given_flow(packed, a, b, taps["flow"], mid, 3, dt, gather_blocks=gmask), plain.float(), (dtype, case, route, "no taps"))
        # a given flow is what the warp reads: with a zero flow `warped` is emavfi_warp(frame2, 0), in the storage type of the warped tail
        # (test_a_zero_flow_returns_frame2 has the sizes at which that is frame2 itself)
        zeros = torch.zeros(2, 2, H, W, device="cuda")
        _, zero = lib.forward_given_flow(packed, a, b, zeros, mid, 3, dt, return_taps=True, gather_blocks=gmask)
        assert any(torch.equal(zero["warped"], v) for v in stored_as(lib.warp(b, zeros), dtype)), (dtype, case, route, "zero flow")
    model.pack_policy = "window"
    with pytest.raises(RuntimeError, match=r"\(-1\).*taps\[1\]"):
        ptrs = [None, a.data_ptr(), None, None, None, None, None, None]
        import ctypes
        arr = ctypes.cast((ctypes.c_void_p * 8)(*ptrs), ctypes.POINTER(ctypes.c_void_p))
        ws = lib.workspace(lib.load().emavfi_workspace_bytes(3, mid, 3, 2, H, W, dt), a.device)
        lib.check(lib.load().emavfi_forward_given_flow(3, mid, 3, packed.data_ptr(), packed.numel(), a.data_ptr(), b.data_ptr(), taps["flow"].data_ptr(),
                                                       plain.data_ptr(), ws.data_ptr(), ws.numel(), 2, H, W, dt, arr, None, None, 0, 0, None),
                  "emavfi_forward_given_flow")


@pytest.mark.parametrize("dtype", MODES)
def test_a_zero_flow_returns_frame2(models, dtype):
    """17 x 33: H - 1 and W - 1 are powers of two, so the warp's normalise / un-normalise round trip (2 x / (W - 1) - 1 and back, the
    reference's operation order) is exact and a zero flow samples every pixel at its own centre with weights 1, 0, 0, 0.  At other sizes
    the round trip rounds and the sample is a pixel's ulp-neighbourhood blend: there the statement is the one about emavfi_warp above."""
    model = models(8, dtype)
    a, b = frames(2, 17, 33, seed=9)
    packed, dt = blob(model)
    _, taps = lib.forward_given_flow(packed, a, b, torch.zeros(2, 2, 17, 33, device="cuda"), 8, 3, dt, return_taps=True)
    assert any(torch.equal(taps["warped"], v) for v in stored_as(b, dtype)), dtype
    if dtype in ("fp32", "amp16", "fp32x3"):
        same_words(taps["warped"], b, dtype)


# ---------------------------------------------------------------- 3. EMA_VFI.flow_scale is the composition
def by_hand(model, a, b, s, gmask=0):
    """F_s from the four entries, one call each"""
    packed, dt = blob(model)
    mid = model.mid_channels
    a_s, b_s = lib.downscale_f32(a, s), lib.downscale_f32(b, s)
    flow_s = lib.forward_flow(packed, a_s, b_s, mid, 3, dt)
    flow = lib.upsample_flow_f32(flow_s, a.shape[-2:], s)
    return lib.forward_given_flow(packed, a, b, flow, mid, 3, dt, gather_blocks=gmask)


@pytest.mark.parametrize("size", [(24, 40), (23, 37)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_coarse_forward_is_the_composition(models, dtype, size):
    model = models(8, dtype)
    a, b = frames(2, *size)
    plain = run(model, a, b)
    same_words(run(model, a, b, flow_scale=None), plain, "flow_scale=None is the plain call")
    for s in oracle.SCALES:
        what = (dtype, size, s)
        want = by_hand(model, a, b, s)
        got = run(model, a, b, flow_scale=s)
        assert got.dtype == torch.float32 and got.shape == a.shape
        same_words(got, want, what)
        assert not torch.equal(got, plain), (what, "the coarse forward must differ from the plain one")
        model.flow_scale = s
        try:
            same_words(run(model, a, b), want, (what, "through the attribute"))
            same_words(run(model, a, b, flow_scale=None), plain, (what, "the per-call None over the attribute"))
        finally:
            model.flow_scale = None
        # under "reverse": the tree mean of F_s(a, b) and F_s(b, a)
        ens = run(model, a, b, flow_scale=s, ensemble="reverse")
        same_words(ens, lib.ensemble_mean_f32([want, by_hand(model, b, a, s)], [0, 0]), (what, "reverse"))
        same_words(run(model, b, a, flow_scale=s, ensemble="reverse"), ens, (what, "reverse is symmetric in time"))
        # under a border: the padded pair is what is reduced
        pa, pb = lib.border_pad_f32(a, 4, "replicate"), lib.border_pad_f32(b, 4, "replicate")
        same_words(run(model, a, b, flow_scale=s, border=4), lib.border_crop_f32(by_hand(model, pa, pb, s), 4), (what, "border"))
    same_words(run(model, a, b), plain, "the plain forward is what it was")
    with pytest.raises(ValueError, match="return_taps=True with a flow scale"):
        run(model, a, b, flow_scale=2, return_taps=True)
    model.pack_adapt = (0.75, 0.65)
    try:
        with pytest.raises(ValueError, match="flow_scale with pack_adapt"):
            run(model, a, b, flow_scale=2)
    finally:
        model.pack_adapt = None


def test_the_gather_policy_and_amp16_under_a_flow_scale(models):
    a, b = frames(2, 40, 56)
    model = models(64, "bf16")
    model.pack_policy = "gather"
    try:
        same_words(run(model, a, b, flow_scale=2), by_hand(model, a, b, 2, gmask=0b111), "gather")
        census = model.pack_census()
        assert all(r is not None and r["route"] == "gather" for r in census)
    finally:
        model.pack_policy = "window"
    amp = models(8, "amp16")
    got = run(amp, a, b, flow_scale=4)
    assert got.dtype == torch.float16 and torch.equal(got, by_hand(amp, a, b, 4).half())


# ---------------------------------------------------------------- 4. the workspace contract
@pytest.mark.parametrize("shape", [(2, 23, 37), (1, 48, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", MODES)
def test_workspace_contract_of_the_two_entries(models, dtype, shape, monkeypatch):
    """emavfi_forward_flow and emavfi_forward_given_flow in exactly-sized, guard-banded workspaces pre-filled with 0x00, 0xFF and 0x7B
    (tests/workspace_harness.py): the given flow is an input like the frames - guarded, compared afterwards"""
    model = models(64, dtype)
    packed, dt = blob(model)
    a, b = frames(*shape, seed=17)
    flow = lib.forward_flow(packed, a, b, 64, 3, dt)

    def flow_call(inp):
        return {"flow": lib.forward_flow(packed, inp[0], inp[1], 64, 3, dt)}

    def given_call(inp):
        out, taps = lib.forward_given_flow(packed, inp[0], inp[1], inp[2], 64, 3, dt, return_taps=True)
        return dict(taps, out=out)
    run_case(monkeypatch, f"forward_flow {dtype} {shape}", flow_call, [a, b])
    run_case(monkeypatch, f"forward_given_flow {dtype} {shape}", given_call, [a, b, flow])


# ---------------------------------------------------------------- 5. against the CPU oracle
_oracle_outputs = {}


def oracle_coarse_forward(name, s):
    """F_s from oracle/emavfi_oracle.py's stage functions and the numpy oracle of steps 1 and 3, computed once per (fixture, s)"""
    if (name, s) not in _oracle_outputs:
        g = load_golden(name)
        sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
        a, b = torch.from_numpy(g["frame1"]), torch.from_numpy(g["frame2"])
        with torch.no_grad():
            a_s, b_s = (torch.from_numpy(oracle.down(t.numpy(), s)) for t in (a, b))
            feat_s = emavfi_oracle.feature_extraction(sd, a_s, b_s)
            flow_s = emavfi_oracle.motion_estimation(sd, feat_s, emavfi_oracle.context_encoding(sd, feat_s))
            flow = torch.from_numpy(oracle.up(flow_s.numpy(), a.shape[-2:], s))
            feat = emavfi_oracle.feature_extraction(sd, a, b)
            warped = emavfi_oracle.warp(b, flow)
            fused = torch.cat([feat, warped], dim=1)
            for i in range(3):
                fused = emavfi_oracle.attention_block(sd, i, fused)
            out = emavfi_oracle.reconstruction(sd, fused)
        _oracle_outputs[(name, s)] = (sd, a, b, dict(flow_s=flow_s, flow=flow, warped=warped, out=out))
    return _oracle_outputs[(name, s)]


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["tiny_mid8_24x40.npz", "tiny_mid8_23x37.npz"])
def test_fp32_coarse_forward_against_the_cpu_oracle(name, s):
    """the project's frame gate, 1e-3 max-abs.  The figures per stage are printed before the assertion (profiles/r24_flow_scale.md holds
    the measured ones)."""
    sd, a, b, ref = oracle_coarse_forward(name, s)
    model = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    model.load_state_dict(sd, strict=True)
    ad, bd = a.cuda(), b.cuda()
    got = run(model, ad, bd, flow_scale=s)
    packed, dt = blob(model)
    flow_s = lib.forward_flow(packed, lib.downscale_f32(ad, s), lib.downscale_f32(bd, s), 8, 3, dt)
    flow = lib.upsample_flow_f32(flow_s, a.shape[-2:], s)
    _, taps = lib.forward_given_flow(packed, ad, bd, flow, 8, 3, dt, return_taps=True)
    err = {"flow_s": (flow_s.cpu() - ref["flow_s"]).abs().max().item(), "flow": (flow.cpu() - ref["flow"]).abs().max().item(),
           "warped": (taps["warped"].cpu() - ref["warped"]).abs().max().item(), "out": (got.cpu() - ref["out"]).abs().max().item()}
    print(f"coarse forward vs CPU oracle, {name} s={s}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["out"] <= 1e-3, err


# ---------------------------------------------------------------- 6. the harness and the command line
FH, FW = 48, 64


class ByHand(EMA_VFI):
    """every forward with flow_scale=2 given by hand: what the harness must issue"""

    def forward(self, a, b, **kw):
        assert "flow_scale" not in kw
        return EMA_VFI.forward(self, a, b, flow_scale=2, **kw)


@pytest.fixture(scope="module")
def harness_models():
    return build_model(8, "fp32"), build_model(8, "fp32", ByHand)


def same_frames(got, want, what):
    assert len(got) == len(want) > 0, (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


HOW = {"reference": dict(), "recursive3": dict(mode="recursive", interpolation_factor=3),
       "reverse_border": dict(ensemble="reverse", border=4)}


@pytest.mark.parametrize("how", list(HOW))
def test_harness_equals_the_forwards_by_hand(harness_models, how):
    model, by_hand_model = harness_models
    rng = np.random.default_rng(1)
    clip = [(rng.uniform(0, 1, (FH, FW, 3)) * 255).astype(np.uint8) for _ in range(5)]
    kw = dict(batch_pairs=2, reference_quirks=False, **HOW[how])
    plain = list(FrameInterpolator(model, **kw).run(clip))
    want = list(FrameInterpolator(by_hand_model, **kw).run(clip))
    got = list(FrameInterpolator(model, flow_scale=2, **kw).run(clip))
    assert model.flow_scale is None                                         # the harness's value rides on each call
    same_frames(got, want, how)
    assert any(not np.array_equal(x, y) for x, y in zip(got, plain)), (how, "the flow scale must show")
    if how == "reference":
        ev = FrameInterpolator(model, flow_scale=2, **kw).evaluate(clip, every=2)
        ev_want = FrameInterpolator(by_hand_model, **kw).evaluate(clip, every=2)
        assert [(t.t, t.sse, t.ssimq) for t in ev] == [(t.t, t.sse, t.ssimq) for t in ev_want]
        assert [t.sse for t in ev] != [t.sse for t in FrameInterpolator(model, **kw).evaluate(clip, every=2)]


def test_command_line_flow_scale(harness_models, tmp_path, capsys):
    model, _ = harness_models
    clip = [(np.random.default_rng(k).uniform(0, 1, (FH * 3 // 2, FW)) * 219 + 16).astype(np.uint8) for k in range(4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(FW, FH, 24, 1, colorspace="420jpeg")) as w:
        for f in clip:
            w.write(f)
    base = [str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1"]
    rc = cli.main(base + ["--flow-scale", "2"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "flow scale 2" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format="yuv420p8")
    same_frames(got, list(FrameInterpolator(model, flow_scale=2, **kw).run(clip)), "cli")      # seed 0, 8 channels, fp32: the fixture's model
    assert not np.array_equal(got[0], list(FrameInterpolator(model, **kw).run(clip))[0])
    assert cli.main(base[:1] + base[2:] + ["--evaluate", "--flow-scale", "4"]) == 0
    assert "psnr" in capsys.readouterr().out.lower()
