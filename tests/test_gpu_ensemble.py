"""Test-time ensembling on the device (include/emavfi.h, "ENSEMBLE DEFINITION"): emavfi_flip_f32 and emavfi_ensemble_mean_f32 against the numpy
oracle (tests/ensemble_oracle.py) bit for bit, on both access widths and inside guard bands; EMA_VFI.ensemble against the composition of
plain forwards it is defined as; the two properties the definition buys - exact symmetry in time, exact equivariance under flips - which
the plain forward has not; the harness and the command line."""
import ctypes

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import ensemble_oracle as oracle

pytestmark = pytest.mark.gpu

SHAPES = [(6, 23, 37), (3, 24, 40), (2, 5, 8), (1, 1, 1), (2, 1, 9), (2, 9, 1), (1, 3, 4)]
GUARD = 64                      # floats of guard band on either side: 256 bytes, so the band keeps the tensor's 16-byte alignment
SENTINEL = -12345.678


def ibits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what):
    got, want = (torch.as_tensor(v).cpu().contiguous() for v in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    assert torch.equal(ibits(got), ibits(want)), (what, int((ibits(got) != ibits(want)).sum()))


def placed(values, off):
    """(buffer, view): `values` on the device inside sentinel guard bands, the view starting `off` floats behind a 16-byte boundary"""
    values = torch.as_tensor(values)
    buf = torch.full((values.numel() + 2 * GUARD + off,), SENTINEL, device="cuda")
    view = buf[GUARD + off:GUARD + off + values.numel()].view(values.shape)
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return buf, view


def bands_intact(buf, view, what):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    rest = torch.cat([buf[:lo], buf[lo + view.numel():]])
    assert rest.numel() >= 2 * GUARD and bool((rest == SENTINEL).all()), what


def members_np(shape, n, seed=0):
    count = int(np.prod(shape))
    return [oracle.generated(seed + k, count).reshape(shape) for k in range(n)]


# ---------------------------------------------------------------- the entries
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entries_are_the_oracle_bit_for_bit(shape, off):
    mem = members_np(shape, 8)
    dev = [placed(m, off) for m in mem]
    for f in range(4):
        buf, out = placed(np.zeros(shape, np.float32), off)
        assert lib.flip_f32(dev[0][1], f, out=out) is out
        same_bits(out, oracle.flip(mem[0], f), ("flip", shape, off, f))
        bands_intact(buf, out, ("flip", shape, off, f))
    for n in (1, 2, 4, 8):
        for base in (0, n):
            flips = [(3 * k + base) & 3 for k in range(n)]
            buf, out = placed(np.zeros(shape, np.float32), off)
            lib.ensemble_mean_f32([v for _, v in dev[:n]], flips, out=out)
            same_bits(out, oracle.mean(mem[:n], flips), ("mean", shape, off, n, flips))
            bands_intact(buf, out, ("mean", shape, off, n, flips))
    for (b, v), m in zip(dev, mem):
        bands_intact(b, v, "a member")                                   # nothing but out is written
        same_bits(v, m, "a member is left as it was")
    # out allocated by the wrapper
    same_bits(lib.flip_f32(dev[1][1], 3), oracle.flip(mem[1], 3), ("flip, own out", shape))
    same_bits(lib.ensemble_mean_f32([v for _, v in dev[:4]], oracle.FLIPS), oracle.mean(mem[:4], oracle.FLIPS), ("mean, own out", shape))


def test_wide_path_equals_scalar_path():
    shape = (3, 24, 40)
    mem = members_np(shape, 8, seed=20)
    wide, scalar = [placed(m, 0)[1] for m in mem], [placed(m, 1)[1] for m in mem]
    for f in range(4):
        same_bits(lib.flip_f32(wide[0], f), lib.flip_f32(scalar[0], f, out=placed(np.zeros(shape, np.float32), 1)[1]), ("flip", f))
    for n in (1, 2, 4, 8):
        flips = [(k + 1) & 3 for k in range(n)]
        a = lib.ensemble_mean_f32(wide[:n], flips)
        b = lib.ensemble_mean_f32(scalar[:n], flips, out=placed(np.zeros(shape, np.float32), 1)[1])
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
        same_bits(a, b, ("mean", n))
    # one misaligned member among aligned ones takes the whole call to the scalar path: same bits again
    mixed = wide[:3] + [scalar[3]]
    same_bits(lib.ensemble_mean_f32(mixed, oracle.FLIPS), lib.ensemble_mean_f32(wide[:4], oracle.FLIPS), "mixed alignment")


def test_members_in_pinned_host_memory():
    """the entries take device pointers or pinned (device-mapped) host memory, as the header says"""
    shape = (2, 24, 40)
    mem = members_np(shape, 4, seed=30)
    pinned = [torch.from_numpy(m.copy()).pin_memory() for m in mem]
    same_bits(lib.ensemble_mean_f32(pinned, oracle.FLIPS), oracle.mean(mem, oracle.FLIPS), "pinned members")
    out = torch.zeros(shape).pin_memory()
    lib.flip_f32(pinned[0], 1, out=out)
    torch.cuda.synchronize()
    same_bits(out, oracle.flip(mem[0], 1), "pinned src and dst")
    with pytest.raises(RuntimeError, match="PINNED"):
        lib.flip_f32(torch.from_numpy(mem[0].copy()), 1)                  # pageable host memory is refused by the wrapper


def test_a_nan_in_any_member_gives_nan_and_the_tree_order_is_the_definitions():
    shape = (1, 3, 4)
    mem = members_np(shape, 8, seed=40)
    for n in (2, 4, 8):
        for k in range(n):
            bad = [m.copy() for m in mem[:n]]
            bad[k][0, 1, 2] = np.nan
            out = lib.ensemble_mean_f32([torch.from_numpy(m).cuda() for m in bad], [0] * n).cpu().numpy()
            want = oracle.mean(bad, [0] * n)
            assert np.isnan(out[0, 1, 2]) and np.array_equal(np.isnan(out), np.isnan(want)), (n, k)
    m = [torch.full((1, 1, 1), v, device="cuda") for v in (2.0 ** 24, 1.0, 1.0, 1.0)]
    assert lib.ensemble_mean_f32(m, [0] * 4).item() == 4194304.5           # the running sum gives 4194304.0


def test_refusals_are_codes_not_aborts():
    L = lib.load()
    shape = (3, 8, 16)
    t = [torch.zeros(shape, device="cuda") for _ in range(5)]
    S, D = t[0].data_ptr(), t[1].data_ptr()
    nbytes = t[0].numel() * 4
    big = torch.zeros(2 * t[0].numel(), device="cuda")

    def flip(src=S, dst=D, planes=3, H=8, W=16, f=1):
        return L.emavfi_flip_f32(src, dst, planes, H, W, f, None), lib.last_error()
    for kw, word in ((dict(src=None), "null pointer src"), (dict(dst=None), "null pointer dst"), (dict(planes=0), "planes"), (dict(H=0), ">= 1"),
                     (dict(W=16385), "16384"), (dict(f=4), "flip = 4"), (dict(src=S + 2), "4-byte"), (dict(dst=D + 1), "4-byte"),
                     (dict(planes=1 << 63, H=16384, W=16384), "overflows"), (dict(dst=S), "dst overlaps src"),
                     (dict(src=big.data_ptr(), dst=big.data_ptr() + nbytes - 4), "dst overlaps src")):
        rc, msg = flip(**kw)
        assert rc == -1 and "flip_f32" in msg and word in msg, (kw, rc, msg)

    def mean(members, flips, n=None, out=D, planes=3, H=8, W=16):
        mp = (ctypes.c_void_p * len(members))(*members)
        fp = (ctypes.c_int * len(flips))(*flips)
        return L.emavfi_ensemble_mean_f32(ctypes.cast(mp, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(fp, ctypes.POINTER(ctypes.c_int)),
                                          len(members) if n is None else n, out, planes, H, W, None), lib.last_error()
    M = [v.data_ptr() for v in t[1:]]                                      # four members; t[0] is out
    for args, kw, word in ([((M + M, [0] * 8), dict(n=n, out=S), f"n = {n}") for n in (0, 3, 5, 6, 7, 9)]
                           + [((M, [0, 1, 2, 4]), dict(out=S), "flips[3] = 4"), ((M, [0] * 4), dict(out=None), "null pointer out"),
                              ((M, [0] * 4), dict(out=S, planes=0), "planes"), ((M, [0] * 4), dict(out=S, W=0), ">= 1"),
                              ((M[:2] + [None, M[3]], [0] * 4), dict(out=S), "null pointer members[2]"),
                              ((M[:3] + [M[3] + 1], [0] * 4), dict(out=S), "4-byte"), ((M, [0] * 4), dict(out=S + 2), "4-byte"),
                              ((M, [0] * 4), dict(out=M[2]), "out overlaps members[2]"),
                              (([big.data_ptr()], [0]), dict(out=big.data_ptr() + nbytes - 4), "out overlaps members[0]"),
                              ((M[:2], [0, 3]), dict(out=M[1] + 0), "out overlaps members[1]")]):
        rc, msg = mean(*args, **kw)
        assert rc == -1 and "ensemble_mean_f32" in msg and word in msg, (kw, rc, msg)
    # the wrappers raise with the library's message, and the process goes on: a good call after all of that
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        lib.flip_f32(t[0], 1, out=t[0])
    with pytest.raises(RuntimeError, match="out overlaps members"):
        lib.ensemble_mean_f32([t[1], t[2]], [0, 0], out=t[2])
    with pytest.raises(RuntimeError, match="n = 3"):
        lib.ensemble_mean_f32(t[:3], [0, 0, 0])
    x = torch.from_numpy(members_np(shape, 1)[0]).cuda()
    same_bits(lib.flip_f32(x, 2), torch.flip(x, [1]), "a good call after the refusals")


def test_more_planes_than_grid_rows_and_a_tensor_past_2_pow_32_bytes():
    # 70000 planes of 3 x 4: a workgroup walks the planes beyond the grid's 65535 rows
    x = torch.arange(70000 * 12, device="cuda", dtype=torch.float32).view(70000, 3, 4)
    assert torch.equal(lib.flip_f32(x, 3), torch.flip(x, [1, 2]))
    y = x + 0.5
    assert torch.equal(lib.ensemble_mean_f32([x, y], [1, 2]), (torch.flip(x, [2]) + torch.flip(y, [1])) * 0.5)
    # 5 planes of 16384 x 16384: 5 * 2^30 bytes, plane offsets pass 2^32 bytes and the element index 2^30
    free, _ = torch.cuda.mem_get_info()
    if free < 28 << 30:
        pytest.skip("needs 28 GiB of free device memory")
    big = torch.arange(5 << 28, device="cuda", dtype=torch.int32).view(5, 16384, 16384).view(torch.float32)   # element i holds the bits of i
    out = lib.flip_f32(big, 3)
    assert torch.equal(ibits(out), torch.flip(ibits(big), [1, 2]))


# ---------------------------------------------------------------- the model
CASES = {"mid8_fp32_23x37": (8, "fp32", 23, 37), "mid64_bf16_24x40": (64, "bf16", 24, 40)}


def build_model(mid, dtype):
    m = EMA_VFI(mid_channels=mid, compute_dtype=dtype).cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=mid), strict=True)
    return m


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    """(model, a, b) with ensemble None; every test leaves the attribute None again"""
    mid, dtype, H, W = CASES[request.param]
    a, b = synth.synthetic_frames(3, 2, H, W, "natural")
    return build_model(mid, dtype), a.cuda(), b.cuda()


def phi(t, f):
    dims = [d for d, bit in ((3, lib.FLIP_H), (2, lib.FLIP_V)) if f & bit]
    return torch.flip(t, dims).contiguous() if dims else t


def run(model, a, b, ensemble=None):
    model.ensemble = ensemble
    try:
        with torch.no_grad():
            return model(a, b)
    finally:
        model.ensemble = None


def composed(model, a, b, ensemble):
    """the ensemble from plain forwards, torch.flip and the mean entry: section by section what the definition says"""
    mem, codes = [], []
    for reverse, f in oracle.members_of(ensemble):
        x, y = (b, a) if reverse else (a, b)
        mem.append(run(model, phi(x, f), phi(y, f)).float().contiguous())
        codes.append(f)
    return lib.ensemble_mean_f32(mem, codes)


@pytest.mark.parametrize("ensemble", ["reverse", "flip", "full"])
def test_forward_is_the_composition_bit_for_bit(case, ensemble):
    model, a, b = case
    got = run(model, a, b, ensemble)
    assert got.dtype == torch.float32 and got.shape == a.shape
    same_bits(got, composed(model, a, b, ensemble), ensemble)
    assert not torch.equal(got, run(model, a, b)), "the ensemble must differ from the plain forward"
    with torch.no_grad():
        same_bits(model(a, b, ensemble=ensemble), got, "the per-call argument")
    assert model.ensemble is None


def test_amp16_converts_after_the_mean():
    model = build_model(8, "amp16")
    a, b = (t.cuda() for t in synth.synthetic_frames(3, 2, 23, 37, "natural"))
    got = run(model, a, b, "flip")
    assert got.dtype == torch.float16
    want = composed(model, a, b, "flip")                                   # fp32 mean of the fp16-valued members
    assert torch.equal(got, want.half())


@pytest.mark.parametrize("ensemble", ["reverse", "full"])
def test_time_symmetry(case, ensemble):
    model, a, b = case
    same_bits(run(model, a, b, ensemble), run(model, b, a, ensemble), ensemble)
    assert not torch.equal(run(model, a, b), run(model, b, a)), "the plain forward is not symmetric in time"


@pytest.mark.parametrize("ensemble", ["flip", "full"])
def test_flip_equivariance(case, ensemble):
    model, a, b = case
    base = run(model, a, b, ensemble)
    plain = run(model, a, b)
    for g in (1, 2, 3):
        same_bits(run(model, phi(a, g), phi(b, g), ensemble), phi(base, g), (ensemble, g))
        if a.shape[-2:] == (23, 37):
            assert not torch.equal(run(model, phi(a, g), phi(b, g)), phi(plain, g)), ("the plain forward is not equivariant", g)


def test_under_pack_adapt_the_forward_matches_the_composition_from_the_same_state():
    model = build_model(64, "bf16")
    sd = synth.synthetic_state_dict(seed=0, mid_channels=64)
    a, b = (t.cuda() for t in synth.synthetic_frames(3, 2, 24, 40, "natural"))
    model.pack_adapt = (0.75, 0.65)
    run(model, a, b)                                                       # creates the stream's route state
    model.load_state_dict(sd, strict=True)                                 # back to the starting route
    want = composed(model, a, b, "flip")
    model.load_state_dict(sd, strict=True)
    same_bits(run(model, a, b, "flip"), want, "pack_adapt")


def test_return_taps_is_refused_and_none_is_the_untouched_forward(case):
    model, a, b = case
    for how in (dict(), dict(ensemble="reverse")):
        model.ensemble = None if how else "flip"
        try:
            with pytest.raises(ValueError, match="return_taps"), torch.no_grad():
                model(a, b, return_taps=True, **how)
        finally:
            model.ensemble = None
    mid, dtype = model.mid_channels, model.compute_dtype
    fresh = build_model(mid, dtype)                                        # never had the attribute touched
    with torch.no_grad():
        same_bits(run(model, a, b), fresh(a, b), "ensemble=None")
        out, taps = model(a, b, return_taps=True)
    same_bits(out, run(model, a, b), "return_taps with ensemble None still works")
    assert "feat" in taps


# ---------------------------------------------------------------- the harness and the command line
H, W = 24, 40


@pytest.fixture(scope="module")
def model():
    return build_model(8, "fp32")


def clip(fmt, n, seed=1):
    rng = np.random.default_rng(seed)
    if fmt == "bgr24":
        return [(rng.uniform(0, 1, (H, W, 3)) * 255).astype(np.uint8) for _ in range(n)]
    return [(rng.uniform(0, 1, (H * 3 // 2, W)) * 876 + 64).astype(np.uint16) for _ in range(n)]


def same_frames(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


def interpolator(model, fmt, **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, pixel_format=fmt, **kw)


@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p10"])
def test_harness_reversed_clip_gives_reversed_predictions(model, fmt):
    frames = clip(fmt, 5)
    kw = dict(mode="recursive", interpolation_factor=1)
    fwd = list(interpolator(model, fmt, ensemble="reverse", **kw).run(frames))
    bwd = list(interpolator(model, fmt, ensemble="reverse", **kw).run(frames[::-1]))
    plan = FrameInterpolator.emission_plan(5, 1, 1, reference_quirks=False)      # each pair's prediction, then its earlier frame; the tail
    assert len(fwd) == len(bwd) == len(plan) == 9

    def preds(out):
        return [o for item, o in zip(plan, out) if item[0] == "pred"]

    def sources(out):
        return [o for item, o in zip(plan, out) if item[0] != "pred"]
    assert len(preds(fwd)) == 4
    same_frames(preds(bwd), preds(fwd)[::-1], (fmt, "the interpolated frames"))
    same_frames(sources(bwd), sources(fwd)[::-1], (fmt, "the source frames"))
    plain_f, plain_b = (list(interpolator(model, fmt, **kw).run(f)) for f in (frames, frames[::-1]))
    assert all(not np.array_equal(x, y) for x, y in zip(preds(plain_b), preds(plain_f)[::-1])), "without the ensemble the two differ"
    assert all(not np.array_equal(x, y) for x, y in zip(preds(fwd), preds(plain_f)))


def test_harness_precedence(model):
    frames = clip("bgr24", 5, seed=2)
    for kw in (dict(), dict(mode="recursive", interpolation_factor=3),
               dict(mode="resample", rate_in=24, rate_out=60, resample_depth=2), dict(static_guard=1, scene_threshold=0.9)):
        assert model.ensemble is None
        by_harness = list(interpolator(model, "bgr24", ensemble="flip", **kw).run(frames))
        assert model.ensemble is None                                     # the harness's value rides on each call
        plain = list(interpolator(model, "bgr24", **kw).run(frames))
        model.ensemble = "flip"
        try:
            by_model = list(interpolator(model, "bgr24", **kw).run(frames))
            assert model.ensemble == "flip"
            by_both = list(interpolator(model, "bgr24", ensemble="reverse", **kw).run(frames)) if not kw else None   # the harness's value wins
        finally:
            model.ensemble = None
        same_frames(by_harness, by_model, kw)
        assert any(not np.array_equal(x, y) for x, y in zip(by_harness, plain)), kw
        if by_both is not None:
            same_frames(by_both, list(interpolator(model, "bgr24", ensemble="reverse").run(frames)), "harness over model")
    # evaluate() issues its forwards the same way
    ev_h = interpolator(model, "bgr24", ensemble="flip").evaluate(frames)
    model.ensemble = "flip"
    try:
        ev_m = interpolator(model, "bgr24").evaluate(frames)
    finally:
        model.ensemble = None
    ev_p = interpolator(model, "bgr24").evaluate(frames)
    assert len(ev_h) == 3 and [s.sse for s in ev_h] == [s.sse for s in ev_m] != [s.sse for s in ev_p]


def test_command_line_ensemble(model, tmp_path, capsys):
    frames = [(np.random.default_rng(k).uniform(0, 1, (H * 3 // 2, W)) * 219 + 16).astype(np.uint8) for k in range(4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 24, 1, colorspace="420jpeg")) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1",
                   "--ensemble", "reverse"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "ensemble reverse" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    same_frames(got, list(interpolator(model, "yuv420p8", ensemble="reverse").run(frames)), "cli")   # seed 0, 8 channels, fp32: the fixture's model
    assert not np.array_equal(got[0], list(interpolator(model, "yuv420p8").run(frames))[0])   # the first pair's prediction comes first
    assert cli.main([str(src), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--evaluate", "--ensemble", "full"]) == 0
    assert "psnr" in capsys.readouterr().out.lower()
