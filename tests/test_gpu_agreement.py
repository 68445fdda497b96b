"""The agreement guard on the device (include/emavfi.h, "AGREEMENT GUARD DEFINITION"): emavfi_agreement_guard_f32 against the numpy oracle
(tests/agreement_oracle.py) bit for bit, on both access widths, inside guard bands, with and without counts; EMA_VFI.agreement against the
oracle applied to the plain forwards it is defined on; the symmetries the definition keeps; the harness, evaluate() and the command line.

Every tolerance of the model-level tests is picked from the ORACLE's disagreement of the plain forwards (pick_tol), never from a guarded
output.  The entry tests run the cases of agreement_oracle.RANDOM_CASES, whose held shares tests/test_agreement_cpu.py pins to [0.1, 0.9]."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import agreement_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of guard band on either side: 256 bytes, so the band keeps the tensor's 16-byte alignment
SENTINEL = -12345.678
F32 = np.float32
TOL = float(oracle.TOL)


def ibits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what):
    got, want = (torch.as_tensor(v).cpu().contiguous() for v in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = ibits(got) != ibits(want)
    assert not bool(diff.any()), (what, int(diff.sum()), diff.nonzero()[:4].tolist())


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


def check_entry(inputs, r, tol, off, what, mean=None, std=None):
    """the entry on `inputs` = (u, v, a, b) placed `off` floats off alignment, with counts pre-filled with garbage and with counts NULL:
    out and counts are the oracle's, nothing outside out is written, the inputs are left as they were"""
    B, C = inputs[0].shape[:2]
    m, s = oracle.stats(C, mean, std)
    want, hold, counts = oracle.guard(*inputs, tol, r, m, s)
    dev = [placed(t, off) for t in inputs]
    kw = dict(mean=tuple(float(x) for x in m), std=tuple(float(x) for x in s))
    buf, out = placed(np.full(inputs[0].shape, 7.0, F32), off)
    got_counts = torch.full((B + 2,), -559038737, dtype=torch.int32, device="cuda")          # garbage, and a word on either side
    assert lib.agreement_guard_f32(*(v for _, v in dev), tol, r, out=out, counts=got_counts[1:B + 1], **kw) is out
    same_bits(out, want, (what, "with counts"))
    bands_intact(buf, out, what)
    assert got_counts.tolist() == [-559038737] + [int(c) for c in counts] + [-559038737], (what, got_counts.tolist(), counts.tolist())
    buf2, out2 = placed(np.full(inputs[0].shape, -3.0, F32), off)
    lib.agreement_guard_f32(*(v for _, v in dev), tol, r, out=out2, **kw)                     # counts NULL
    same_bits(out2, want, (what, "counts NULL"))
    bands_intact(buf2, out2, what)
    for (b, v), t in zip(dev, inputs):
        bands_intact(b, v, (what, "an input's bands"))
        assert torch.equal(ibits(v.cpu()), ibits(torch.from_numpy(t))), (what, "an input is left as it was")
    return want, hold, counts


# ---------------------------------------------------------------- the entry
RANDOM = [(s, r, seed, off) for s, r, seed in oracle.RANDOM_CASES for off in ((0, 1) if s == (1, 4, 33, 64) else (0,))]


@pytest.mark.parametrize("shape,r,seed,off", RANDOM, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_entry_is_the_oracle_bit_for_bit_on_random_flags(shape, r, seed, off):
    """u, v on the 2^-10 grid: d == tol exactly at some samples (not flagged), one ulp or one grid step above at others (flagged)"""
    inputs = oracle.random_case(shape, r, seed)
    _, hold, _ = check_entry(inputs, r, TOL, off, (shape, r, off))
    assert 0.1 <= hold.mean() <= 0.9


def test_wide_path_equals_scalar_path():
    shape, r = (1, 4, 33, 64), 3
    inputs = oracle.random_case(shape, r, 5)
    wide, scalar = [placed(t, 0)[1] for t in inputs], [placed(t, 1)[1] for t in inputs]
    kw = dict(mean=(0.5, 0.25, 0.375, 0.625), std=(0.25, 0.5, 0.125, 0.375))
    a = lib.agreement_guard_f32(*wide, TOL, r, **kw)
    b = lib.agreement_guard_f32(*scalar, TOL, r, out=placed(np.zeros(shape, F32), 1)[1], **kw)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
    same_bits(a, b, "wide against scalar")
    # one misaligned input among aligned ones takes the whole call to the scalar path: same bits again
    for k in range(4):
        mixed = wide[:k] + [scalar[k]] + wide[k + 1:]
        same_bits(lib.agreement_guard_f32(*mixed, TOL, r, **kw), a, ("mixed alignment", k))


@pytest.mark.parametrize("shape", [(2, 3, 23, 37), (1, 3, 70, 140), (1, 1, 1, 1), (2, 3, 1, 9), (2, 3, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_one_flagged_pixel_at_each_corner_and_at_the_centre(shape):
    """radii 0, 1, 3 and 16, r larger than H or W included: a (2 r + 1)^2 square clipped at the frame, counted per sample"""
    B, C, H, W = shape
    for where in ("tl", "tr", "bl", "br", "centre"):
        inputs = oracle.single_case(shape, where)
        y, x = {"centre": (H // 2, W // 2), "tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}[where]
        for r in (0, 1, 3, 16):
            _, hold, counts = check_entry(inputs, r, TOL, 0, (shape, where, r))
            side = lambda p, n: min(n - 1, p + r) - max(0, p - r) + 1
            assert counts.tolist() == [side(y, H) * side(x, W)] * B and hold[:, y, x].all()
    _, hold, counts = check_entry(oracle.single_case(shape, None), 16, TOL, 0, (shape, "nothing flagged"))
    assert not hold.any() and not counts.any()


def test_nans_flag_and_pass_as_the_definition_says():
    shape = (2, 3, 23, 37)
    u, v, a, b = oracle.single_case(shape, None)
    u[0, 0, 4, 6] = np.nan                       # held at any tolerance, the output there is the finite blend
    v[1, 2, 22, 36] = np.nan
    a[0, 2, 4, 7] = np.nan                       # a source NaN inside the held window stays a NaN, in its channel alone
    b[1, 1, 0, 0] = np.nan                       # and one at a pixel that is not held is never read
    for r, tol in ((0, 1.0), (1, 1.0), (3, TOL)):
        want, hold, counts = check_entry((u, v, a, b), r, tol, 0, ("nan", r))
        assert hold[0, 4, 6] and hold[1, 22, 36] and not hold[1, 0, 0]
        assert np.isnan(want).sum() == (1 if r else 0) and bool(np.isnan(want[0, 2, 4, 7])) == bool(r)
        assert np.isfinite(want[0, :, 4, 6]).all()
    # infinities of one sign: inf - inf is a NaN, flagged
    u[0, 1, 10, 10] = v[0, 1, 10, 10] = np.inf
    _, hold, _ = check_entry((u, v, a, b), 0, 1.0, 0, "inf - inf")
    assert hold[0, 10, 10]


def test_tol_one_holds_nothing_and_tol_zero_holds_every_difference():
    shape = (2, 3, 23, 37)
    rng = np.random.default_rng(3)
    u, v = (rng.uniform(0, 1, shape).astype(F32) for _ in range(2))
    u[0, 0, 0, 0], v[0, 0, 0, 0] = 0, 1           # d == 1 == tol
    v[1, :, 5:9, 7:30] = u[1, :, 5:9, 7:30]       # a region of exact agreement
    a, b = oracle.sources(shape, 3)
    want, hold, counts = check_entry((u, v, a, b), 16, 1.0, 0, "tol 1")
    assert not hold.any() and np.array_equal(want.view(np.uint32), ((u + v) * F32(0.5)).view(np.uint32))
    _, hold, counts = check_entry((u, v, a, b), 0, 0.0, 0, "tol 0")
    assert counts.tolist() == [23 * 37, 23 * 37 - 4 * 23] and not hold[1, 5:9, 7:30].any()
    # monotone in r and in tol, on the device's own counts
    prev = None
    for r in (0, 1, 3, 16):
        c = torch.zeros(2, dtype=torch.int32, device="cuda")
        lib.agreement_guard_f32(*(torch.from_numpy(t).cuda() for t in (u, v, a, b)), 0.9, r, counts=c)
        assert prev is None or all(x >= y for x, y in zip(c.tolist(), prev))
        prev = c.tolist()
    for tol in (0.92, 0.95, 1.0):
        c = torch.zeros(2, dtype=torch.int32, device="cuda")
        lib.agreement_guard_f32(*(torch.from_numpy(t).cuda() for t in (u, v, a, b)), tol, 16, counts=c)
        assert all(x <= y for x, y in zip(c.tolist(), prev))
        prev = c.tolist()


def test_inputs_in_pinned_host_memory():
    """the entry takes device pointers or pinned (device-mapped) host memory, as the header says"""
    shape, r = (2, 3, 23, 37), 1
    inputs = oracle.random_case(shape, r, 1)
    want, _, counts = oracle.guard(*inputs, TOL, r)
    pinned = [torch.from_numpy(t.copy()).pin_memory() for t in inputs]
    c = torch.full((2,), 99, dtype=torch.int32, device="cuda")
    same_bits(lib.agreement_guard_f32(*pinned, TOL, r, counts=c), want, "pinned inputs")
    assert c.tolist() == counts.tolist()
    out = torch.zeros(shape).pin_memory()
    lib.agreement_guard_f32(*pinned, TOL, r, out=out)
    torch.cuda.synchronize()
    same_bits(out, want, "pinned inputs and out")
    with pytest.raises(RuntimeError, match="PINNED"):
        lib.agreement_guard_f32(torch.from_numpy(inputs[0].copy()), *pinned[1:], TOL, r)   # pageable host memory is refused by the wrapper


def test_refusals_are_codes_not_aborts():
    L = lib.load()
    shape = (2, 3, 8, 16)
    t = [torch.zeros(shape, device="cuda") for _ in range(5)]
    big = torch.zeros(2 * t[0].numel(), device="cuda")
    nbytes = t[0].numel() * 4
    import ctypes
    m, s = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)

    def call(ptrs=None, out=None, r=1, tol=0.1, B=2):
        p = [v.data_ptr() for v in t[:4]] if ptrs is None else ptrs
        return L.emavfi_agreement_guard_f32(*p, t[4].data_ptr() if out is None else out, B, 3, 8, 16, r, tol, m, s, None, None), lib.last_error()
    for kw, word in ((dict(r=17), "radius = 17"), (dict(tol=float("nan")), "tol = nan"), (dict(B=0), "B = 0"), (dict(out=t[2].data_ptr()), "out overlaps a"),
                     (dict(ptrs=[big.data_ptr()] * 4, out=big.data_ptr() + nbytes - 4), "out overlaps u"), (dict(out=t[4].data_ptr() + 2), "4-byte")):
        rc, msg = call(**kw)
        assert rc == -1 and "agreement_guard_f32" in msg and word in msg, (kw, rc, msg)
    with pytest.raises(RuntimeError, match="out overlaps v"):
        lib.agreement_guard_f32(t[0], t[1], t[2], t[3], 0.1, out=t[1])
    with pytest.raises(ValueError, match="one shape"):
        lib.agreement_guard_f32(t[0], t[1], t[2], torch.zeros(2, 3, 8, 12, device="cuda"), 0.1)
    with pytest.raises(ValueError, match="counts must be"):
        lib.agreement_guard_f32(*t[:4], 0.1, counts=torch.zeros(3, dtype=torch.int32, device="cuda"))
    # the process goes on: a good call after all of that, with every input the same tensor (inputs may alias one another)
    x = torch.from_numpy(oracle.agreeing(shape, 1)[0]).cuda()
    same_bits(lib.agreement_guard_f32(x, x, x, x, 0.0), x, "u == v: (u + u) * 0.5f == u, nothing held")


# ---------------------------------------------------------------- the model
CASES = {"mid8_fp32_23x37": (8, "fp32", 23, 37), "mid64_bf16_24x40": (64, "bf16", 24, 40)}
RADII = (0, 1, 3)


def build_model(mid, dtype):
    m = EMA_VFI(mid_channels=mid, compute_dtype=dtype).cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=mid), strict=True)
    return m


def phi(t, f):
    dims = [d for d, bit in ((3, lib.FLIP_H), (2, lib.FLIP_V)) if f & bit]
    return torch.flip(t, dims).contiguous() if dims else t


def run(model, a, b, **kw):
    with torch.no_grad():
        return model(a, b, **kw)


def halves(model, a, b, ensemble):
    """(u, v) of the definition's composition from forwards WITHOUT the guard: plain forwards for "reverse", "flip" ensembles for "full" """
    inner = None if ensemble == "reverse" else "flip"
    return (run(model, a, b, ensemble=inner).float().cpu().numpy(), run(model, b, a, ensemble=inner).float().cpu().numpy())


def pick_tol(u, v, r):
    """a tolerance at which the ORACLE holds about half the pixels at radius r: the quantile of the oracle's own per-pixel disagreement
    whose dilated share lies nearest one half.  Nothing here looks at a guarded output."""
    d = oracle.disagreement(u, v).max(axis=1)
    best = None
    for q in (0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.999):
        tol = F32(np.quantile(d, q))
        share = oracle.held(u, v, tol, r).mean()
        if best is None or abs(share - 0.5) < abs(best[1] - 0.5):
            best = (tol, share)
    assert 0.1 <= best[1] <= 0.9 and 0 <= best[0] <= 1, best
    return float(best[0])


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    """(model, a, b, {ensemble: (u, v)}): the halves are computed once and shared, unchanged, by the tests below"""
    mid, dtype, H, W = CASES[request.param]
    a, b = (t.cuda() for t in synth.synthetic_frames(3, 2, H, W, "natural"))
    model = build_model(mid, dtype)
    return model, a, b, {e: halves(model, a, b, e) for e in ("reverse", "full")}


@pytest.mark.parametrize("ensemble", ["reverse", "full"])
def test_forward_is_the_oracle_on_the_two_halves(case, ensemble):
    model, a, b, hv = case
    u, v = hv[ensemble]
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    assert not np.array_equal(u, v), "the two time directions must differ somewhere"
    for r in RADII:
        tol = pick_tol(u, v, r)
        want, hold, counts = oracle.guard(u, v, an, bn, tol, r)
        got = run(model, a, b, ensemble=ensemble, agreement=(tol, r))
        assert got.dtype == torch.float32 and got.shape == a.shape
        same_bits(got, want, (ensemble, r, tol))
        assert model.agreement_counts.dtype == torch.int32 and model.agreement_counts.tolist() == counts.tolist()
        assert 0.1 <= hold.mean() <= 0.9
        assert not torch.equal(got, run(model, a, b, ensemble=ensemble)), "something held must show"
    # the attribute does what the per-call argument does, and is left alone by it
    tol = pick_tol(u, v, 1)
    model.ensemble, model.agreement = ensemble, (tol, 1)
    try:
        same_bits(run(model, a, b), run(model, a, b, ensemble=ensemble, agreement=(tol, 1)), "attribute against argument")
        same_bits(run(model, a, b, agreement=None), run(model, a, b, ensemble=ensemble, agreement=None), "agreement=None for one call")
        assert model.agreement == (tol, 1)
    finally:
        model.ensemble, model.agreement = None, None


@pytest.mark.parametrize("ensemble", ["reverse", "full"])
def test_tol_one_gives_the_ensembles_bits(case, ensemble):
    """required for "reverse" (the same two operations); expected for "full", where the halves are scaled by 1 / 4 before they are added
    instead of 1 / 8 after - exact unless an intermediate is subnormal, which a frame's values are far from"""
    model, a, b, _ = case
    for r in (0, 16):
        same_bits(run(model, a, b, ensemble=ensemble, agreement=(1.0, r)), run(model, a, b, ensemble=ensemble), (ensemble, r))
        assert model.agreement_counts.tolist() == [0, 0]


@pytest.mark.parametrize("ensemble", ["reverse", "full"])
def test_time_symmetry(case, ensemble):
    model, a, b, hv = case
    for r in RADII:
        tol = pick_tol(*hv[ensemble], r)
        fwd = run(model, a, b, ensemble=ensemble, agreement=(tol, r))
        cf = model.agreement_counts.tolist()
        same_bits(fwd, run(model, b, a, ensemble=ensemble, agreement=(tol, r)), (ensemble, r))
        assert model.agreement_counts.tolist() == cf and 0 < sum(cf) < 2 * a.shape[2] * a.shape[3]


def test_flip_equivariance_under_full(case):
    model, a, b, hv = case
    tol = pick_tol(*hv["full"], 1)
    base = run(model, a, b, ensemble="full", agreement=(tol, 1))
    counts = model.agreement_counts.tolist()
    for g in (1, 2, 3):
        same_bits(run(model, phi(a, g), phi(b, g), ensemble="full", agreement=(tol, 1)), phi(base, g), g)
        assert model.agreement_counts.tolist() == counts


@pytest.mark.parametrize("border", [(4, "replicate"), (3, "reflect")], ids=lambda v: f"{v[0]}_{v[1]}")
def test_with_a_border_the_result_is_the_composition_written_out(case, border):
    """pad, the two forwards at the padded size, crop u and v, then the guard on the picture with the UNPADDED sources"""
    model, a, b, _ = case
    N, mode = border
    pa, pb = (lib.border_pad_f32(t.float().contiguous(), N, mode) for t in (a, b))
    u = lib.border_crop_f32(run(model, pa, pb).float().contiguous(), N).cpu().numpy()
    v = lib.border_crop_f32(run(model, pb, pa).float().contiguous(), N).cpu().numpy()
    tol = pick_tol(u, v, 3)
    want, hold, counts = oracle.guard(u, v, a.cpu().numpy(), b.cpu().numpy(), tol, 3)
    got = run(model, a, b, ensemble="reverse", border=border, agreement=(tol, 3))
    same_bits(got, want, border)
    assert model.agreement_counts.tolist() == counts.tolist() and got.shape == a.shape
    same_bits(got, run(model, b, a, ensemble="reverse", border=border, agreement=(tol, 3)), "symmetric with a border too")


def test_amp16_converts_after_the_guard():
    model = build_model(8, "amp16")
    a, b = (t.cuda() for t in synth.synthetic_frames(3, 2, 23, 37, "natural"))
    u, v = halves(model, a, b, "reverse")                                  # fp16-valued fp32
    tol = pick_tol(u, v, 1)
    want, hold, counts = oracle.guard(u, v, a.cpu().numpy(), b.cpu().numpy(), tol, 1)
    got = run(model, a, b, ensemble="reverse", agreement=(tol, 1))
    assert got.dtype == torch.float16 and torch.equal(got.cpu(), torch.from_numpy(want).half())
    assert model.agreement_counts.tolist() == counts.tolist() and hold.any()
    assert not torch.equal(torch.from_numpy(want).half().float(), torch.from_numpy(want)), "the fp32 guard result is not fp16-valued everywhere"


def test_refusals(case):
    model, a, b, _ = case
    for kw in (dict(agreement=0.1), dict(agreement=0.1, ensemble="flip"), dict(agreement=(0.1, 2), ensemble=None)):
        with pytest.raises(ValueError, match="needs an ensemble that runs both"):
            run(model, a, b, **kw)
    with pytest.raises(ValueError, match="return_taps"):
        run(model, a, b, ensemble="reverse", agreement=0.1, return_taps=True)
    with pytest.raises(ValueError, match="EMA_VFI.agreement must be None"):
        run(model, a, b, ensemble="reverse", agreement=(0.1, 17))
    fresh = build_model(model.mid_channels, model.compute_dtype)           # never had the attribute touched
    same_bits(run(model, a, b, ensemble="reverse"), run(fresh, a, b, ensemble="reverse"), "agreement None is the untouched ensemble")
    out, taps = run(model, a, b, return_taps=True)
    assert "feat" in taps


# ---------------------------------------------------------------- the harness, evaluate() and the command line
H, W = 24, 40


@pytest.fixture(scope="module")
def model():
    return build_model(8, "fp32")


def clip(fmt, n, seed=1):
    rng = np.random.default_rng(seed)
    if fmt == "bgr24":
        return [(rng.uniform(0, 1, (H, W, 3)) * 255).astype(np.uint8) for _ in range(n)]
    return [(rng.uniform(0, 1, (H * 3 // 2, W)) * 876 + 64).astype(np.uint16) for _ in range(n)]


def interpolator(model, fmt, **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, pixel_format=fmt, **kw)


def staged(fi, frames):
    """the normalised fp32 batch of a clip as the harness's preprocess kernel makes it"""
    host = np.stack([f.view(np.uint8) if f.dtype == np.uint16 else f for f in frames])
    return fi._pre_kernel(torch.from_numpy(host).cuda())


def clip_tol(model, x, pairs, r):
    u = np.concatenate([run(model, x[i:i + 1], x[j:j + 1]).cpu().numpy() for i, j in pairs])
    v = np.concatenate([run(model, x[j:j + 1], x[i:i + 1]).cpu().numpy() for i, j in pairs])
    return pick_tol(u, v, r)


@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p10"])
def test_harness_emits_the_postprocessed_model_result_and_its_shares(model, fmt):
    frames, r = clip(fmt, 5), 1
    plain = interpolator(model, fmt, ensemble="reverse")
    x = staged(plain, frames)
    pairs = [(k, k + 1) for k in range(4)]
    tol = clip_tol(model, x, pairs, r)
    fi = interpolator(model, fmt, ensemble="reverse", agreement=tol, agreement_radius=r)
    got = list(fi.run(frames))
    plan = FrameInterpolator.emission_plan(5, 1, 1, reference_quirks=False)
    preds = [o for item, o in zip(plan, got) if item[0] == "pred"]
    assert len(got) == len(plan) == 9 and len(preds) == 4 and len(fi.agreement_share) == 4 and model.agreement is None
    want, shares = [], []
    for k in (0, 2):                                                      # the harness's batches: two pairs each
        out = run(model, x[k:k + 2], x[k + 1:k + 3], ensemble="reverse", agreement=(tol, r))
        shares += [c / (H * W) for c in model.agreement_counts.tolist()]
        b = plain._post_kernel(out, False).cpu().numpy()
        want += [f.view(np.uint16) if fmt != "bgr24" else f for f in b]
    for k, (g, w) in enumerate(zip(preds, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (fmt, k, int((g != w).sum()))
    assert fi.agreement_share == shares and all(0 < s < 1 for s in shares)
    unguarded = [o for item, o in zip(plan, plain.run(frames)) if item[0] == "pred"]
    assert all(not np.array_equal(x_, y_) for x_, y_ in zip(preds, unguarded)) and plain.agreement_share == []
    # the model's own attributes serve a harness that was given neither, and the harness's values win over the model's
    model.ensemble, model.agreement = "reverse", (tol, r)
    try:
        by_model = list(interpolator(model, fmt).run(frames))
        assert all(np.array_equal(x_, y_) for x_, y_ in zip(by_model, got)) and len(by_model) == len(got)
    finally:
        model.ensemble, model.agreement = None, None


def test_harness_recursive_and_resample_shares_follow_their_frames(model):
    frames, r = clip("bgr24", 4, seed=3), 1
    x = staged(interpolator(model, "bgr24"), frames)
    tol = clip_tol(model, x, [(0, 1), (1, 2), (2, 3)], r)
    kw = dict(ensemble="reverse", agreement=tol, agreement_radius=r)
    fi = interpolator(model, "bgr24", mode="recursive", interpolation_factor=3, **kw)
    got = list(fi.run(frames))
    assert len(got) == 3 * 4 + 1 and len(fi.agreement_share) == 9 and all(0 <= s <= 1 for s in fi.agreement_share)
    # the middle prediction of each pair is the guarded midpoint of its two sources: the share the one-level harness reports
    one = interpolator(model, "bgr24", mode="recursive", interpolation_factor=1, **kw)
    mids = list(one.run(frames))
    assert [fi.agreement_share[3 * k + 1] for k in range(3)] == one.agreement_share
    assert all(np.array_equal(got[4 * k + 1], mids[2 * k]) for k in range(3))
    rs = interpolator(model, "bgr24", mode="resample", rate_in=24, rate_out=48, resample_depth=1, **kw)
    out = list(rs.run(frames))
    assert len(out) == 7 and rs.agreement_share == one.agreement_share     # every second output is a node frame: the same midpoints
    assert all(np.array_equal(out[2 * k + 1], mids[2 * k]) for k in range(3))


def test_evaluate_scores_the_guarded_prediction(model):
    frames, r = clip("bgr24", 5, seed=4), 1
    fi0 = interpolator(model, "bgr24", ensemble="reverse")
    x = staged(fi0, frames)
    tol = clip_tol(model, x, [(0, 2), (1, 3), (2, 4)], r)
    ev = interpolator(model, "bgr24", ensemble="reverse", agreement=tol, agreement_radius=r).evaluate(frames)
    ev0 = fi0.evaluate(frames)
    assert len(ev) == len(ev0) == 3 and all(s.sse != s0.sse for s, s0 in zip(ev, ev0))
    truth = torch.from_numpy(np.stack(frames)).cuda()
    by_hand = []
    for ia, ib in (([0, 1], [2, 3]), ([2], [4])):                          # evaluate()'s batches: two targets, then one
        pred = run(model, x[ia[0]:ia[-1] + 1], x[ib[0]:ib[-1] + 1], ensemble="reverse", agreement=(tol, r))
        assert all(0 < c < H * W for c in model.agreement_counts.tolist())
        words = lib.frame_metrics_u8(lib.postprocess_u8(pred, denormalize=False), truth[ia[0] + 1:ia[-1] + 2])
        by_hand += [tuple(int(w[0]) for w in ws) for ws in words.cpu().tolist()]
    assert [tuple(s.sse) for s in ev] == by_hand


def test_command_line_agreement(model, tmp_path, capsys):
    frames = [(np.random.default_rng(k).uniform(0, 1, (H * 3 // 2, W)) * 219 + 16).astype(np.uint8) for k in range(4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 24, 1, colorspace="420jpeg")) as w:
        for f in frames:
            w.write(f)
    x = staged(interpolator(model, "yuv420p8"), frames)
    tol = clip_tol(model, x, [(0, 1), (1, 2), (2, 3)], 2)
    base = [str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1"]
    rc = cli.main(base + ["--ensemble", "reverse", "--agreement", repr(tol), "--agreement-radius", "2"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "ensemble reverse" in err and "agreement guard held" in err, err
    with y4m.Y4MReader(str(dst)) as rd:
        got = list(rd)
    fi = interpolator(model, "yuv420p8", ensemble="reverse", agreement=tol, agreement_radius=2)   # seed 0, 8 channels, fp32: the fixture's model
    want = list(fi.run(frames))
    assert len(got) == len(want) == 7 and all(np.array_equal(g, w_) for g, w_ in zip(got, want))
    assert all(0 < s < 1 for s in fi.agreement_share)
    assert not np.array_equal(got[0], list(interpolator(model, "yuv420p8", ensemble="reverse").run(frames))[0])
    held = 100.0 * sum(fi.agreement_share) / len(fi.agreement_share)
    assert f"agreement guard held {held:.2f} %" in err
    assert cli.main([str(src), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--evaluate", "--ensemble", "full",
                     "--agreement", repr(tol)]) == 0
    assert "psnr" in capsys.readouterr().out.lower()
    assert cli.main(base + ["--agreement", repr(tol)]) != 0 and "--agreement needs --ensemble" in capsys.readouterr().err
