"""Global motion on the device (include/emavfi.h, "ALIGN DEFINITION"): emavfi_align_signature_f32, emavfi_align_search and emavfi_shift_f32
against the numpy oracle (tests/align_oracle.py) bit for bit, on every access width and between guard words; a planted pan end to end;
EMA_VFI.align against the composition model(a', b') it is defined as - plain, ensembled, bordered, coarse and guarded - with the
ensemble's exact time symmetry carried over; the harness against a stand-in model that moves the frames by indexing; the command line.
Every comparison is an equality of words or of bytes."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import align_oracle as oracle

pytestmark = pytest.mark.gpu

GUARD = 64                      # words of guard on either side: 256 bytes, so the band keeps the tensor's 16-byte alignment
GUARD_WORD = 0x7B7B7B7B
UNWRITTEN = 0x55AA55AA          # what a destination holds before a call


def words(t):
    """the 32-bit words of a float32 / int32 tensor or array, as a numpy uint32 array on the host"""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "words differ")


def placed(shape, off, values=None, dtype=torch.float32):
    """(buffer, view): a view of `shape` and `dtype` (4 or 2 bytes wide) inside a word buffer between guard words, starting `off` words
    behind a 16-byte boundary; filled with the words of `values` or, for a destination, with UNWRITTEN"""
    per = 4 // torch.empty(0, dtype=dtype).element_size()
    count = (int(np.prod(shape)) + per - 1) // per
    host = np.full(count + 2 * GUARD + off, GUARD_WORD, np.uint32)
    body = host[GUARD + off:GUARD + off + count]
    body[:] = UNWRITTEN
    if values is not None:
        raw = np.ascontiguousarray(values).reshape(-1).view(np.uint8)
        body.view(np.uint8)[:raw.size] = raw
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    view = buf[GUARD + off:GUARD + off + count].view(dtype)[:int(np.prod(shape))].view(shape)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return buf, view


def guards_intact(buf, view, what):
    torch.cuda.synchronize()
    w = words(buf)
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    n = (view.numel() * view.element_size() + 3) // 4
    rest = np.concatenate([w[:lo], w[lo + n:]])
    assert rest.size >= 2 * GUARD and (rest == GUARD_WORD).all(), (what, "a guard word was written")


@pytest.fixture(scope="module")
def picture():
    return synth.synthetic_frames(3, 1, 160, 224)[0][0].numpy().astype(np.float32)


# ---------------------------------------------------------------- 1. the signature
@pytest.mark.parametrize("size", [(8, 8), (9, 13), (24, 40), (23, 37)], ids=lambda s: "x".join(map(str, s)))
def test_signature_is_the_oracle_bit_for_bit(size):
    H, W = size
    rng = np.random.default_rng(H * 100 + W)
    x = rng.normal(0.0, 2.5, (2, 3, H, W)).astype(np.float32)                    # |t| passes 512 for a good share of the pixels
    xw = x.view(np.uint32)
    for k, word in enumerate((0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x7149F2CA, 0xF149F2CA)):   # NaN, +-inf, -0.0, +-1e30
        xw[k % 2, k % 3, (3 * k) % (H // 4 * 4), (5 * k + 1) % (W // 4 * 4)] = word
    want = oracle.signature(x)
    assert 0 < (oracle.quantise(x) == 0).mean() < 0.5 and 0 < (oracle.quantise(x) == 1023).mean() < 0.5
    poisoned = x.copy()
    poisoned[:, :, H // 4 * 4:, :] = np.nan                                       # the remainder rows and columns are not looked at
    poisoned[:, :, :, W // 4 * 4:] = -1e30
    for off in (0, 1):                                                            # 16-byte aligned: 16-byte loads where W % 4 == 0; 4 bytes in: scalar
        for src in (x, poisoned):
            _, xv = placed(x.shape, off, src)
            gbuf, gv = placed(want.shape, 0, None, torch.int16)
            assert lib.align_signature_f32(xv, out=gv) is gv
            guards_intact(gbuf, gv, (size, off))
            assert np.array_equal(gv.cpu().numpy().view(np.uint16), want), (size, off, "poisoned" if src is poisoned else "plain")
    got = lib.align_signature_f32(torch.from_numpy(x).cuda())
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy().view(np.uint16), want)


# ---------------------------------------------------------------- 2. the search
def device_search(ga, gb, R, ratio, prefill=None):
    """the device's records for two uint16 [B, Hc, Wc] arrays, between guard words; `prefill`: the byte the workspace holds before"""
    B = ga.shape[0]
    da, db = (torch.from_numpy(g.view(np.int16)).cuda() for g in (ga, gb))
    sbuf, sv = placed((B, 4), 0, None, torch.int32)
    ws = None
    if prefill is not None:
        ws = torch.full((lib.load().emavfi_align_workspace_bytes(B, R),), prefill, dtype=torch.uint8, device="cuda")
    assert lib.align_search(da, db, R, ratio, out=sv, workspace_=ws) is sv
    guards_intact(sbuf, sv, (ga.shape, R, ratio))
    return sv.cpu().numpy()


def check_search(ga, gb, R, ratio, what):
    want = oracle.search(ga, gb, R, ratio)
    got = device_search(ga, gb, R, ratio)
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())
    assert np.array_equal(device_search(ga, gb, R, ratio, prefill=0xFF), want), (what, "the workspace's earlier content shows")
    back = device_search(gb, ga, R, ratio)
    assert np.array_equal(back, want * np.array([-1, -1, 1, 1], np.int32)), (what, "the exchanged pair must give the negated shift")
    return want


# (B, Hc, Wc, R, top): the smallest grid; odd sizes at R = 2, 3; the largest radius; several samples, two row tiles; two column tiles;
# signatures' own range
GRIDS = [(1, 2, 2, 1, 65536), (2, 5, 9, 2, 65536), (1, 6, 10, 3, 65536), (1, 64, 64, 32, 65536), (3, 45, 80, 16, 65536), (1, 34, 131, 9, 65536),
         (2, 12, 20, 6, 16369)]


@pytest.mark.parametrize("case", GRIDS, ids=lambda c: "x".join(map(str, c)))
def test_search_is_the_oracle_bit_for_bit_on_random_grids(case):
    B, Hc, Wc, R, top = case
    rng = np.random.default_rng(Hc * 1000 + Wc)
    ga, gb = (rng.integers(0, top, (B, Hc, Wc)).astype(np.uint16) for _ in range(2))
    for ratio in (1024, 1000):
        check_search(ga, gb, R, ratio, (case, ratio))
    # the same content moved inside the grid: a real minimum instead of noise
    d = (min(R, (Hc - 1) // 2), -min(R, (Wc - 1) // 2))                          # below half the grid: np.roll's wrap-around matches nothing
    moved = np.roll(ga, d, axis=(1, 2))
    want = check_search(ga, moved, R, 512, (case, "moved"))
    assert (want[:, :2] == 4 * np.array(d)).all()


def test_search_finds_the_planted_pans_and_gives_zero_on_flat_and_striped_grids(picture):
    for (H, W), R, d in (((32, 48), 4, (8, -12)), ((24, 40), 3, (-12, 4)), ((32, 48), 4, (16, 16)), ((64, 96), 8, (-28, 32)), ((33, 50), 4, (4, 0))):
        a, b = oracle.planted(picture, H, W, *d)
        want = check_search(oracle.signature(a), oracle.signature(b), R, 512, (H, W, d))
        assert tuple(want[0, :3]) == (*d, 0)
    flat = np.full((1, 8, 12), 4000, np.uint16)
    assert check_search(flat, flat, 4, 1024, "flat").tolist() == [[0, 0, 0, 0]]
    assert check_search(flat, flat + np.uint16(7), 4, 1024, "two levels").tolist() == [[0, 0, 7 * 256, 7 * 256]]
    stripes = np.tile(np.array([0, 16368], np.uint16), (1, 8, 6))                  # period 2 cells: +1 and -1 cell match alike
    want = check_search(stripes, np.roll(stripes, 1, axis=2), 4, 1024, "stripes")
    assert tuple(want[0, :2]) == (0, 0) and want[0, 2] == want[0, 3] == 16368 * 256
    noise = np.random.default_rng(1).integers(0, 65536, (1, 8, 8)).astype(np.uint16)
    want = check_search(noise, np.roll(noise, 4, axis=2), 4, 1024, "half a period")   # a wrap by half the grid: (0, 4) and (0, -4) both match
    assert tuple(want[0, :2]) == (0, 0) and want[0, 2] == want[0, 3] > 0


def test_the_acceptance_boundary():
    """one feature of 23 at (3, 3) of a, of 9 at (3, 4) of b, 8 x 8 cells, R = 1: SAD(0, 1) = 14 over 56 cells, m = 64; SAD(0) = 32 over
    64 cells, m = 128; every other candidate has SAD 32 over at most 56 cells.  64 * 1024 == 128 * 512: ratio 512 accepts, 511 rejects"""
    ga, gb = np.zeros((1, 8, 8), np.uint16), np.zeros((1, 8, 8), np.uint16)
    ga[0, 3, 3], gb[0, 3, 4] = 23, 9
    assert check_search(ga, gb, 1, 512, "at the boundary").tolist() == [[0, 4, 64, 128]]
    assert check_search(ga, gb, 1, 511, "one below").tolist() == [[0, 0, 128, 128]]
    assert check_search(ga, gb, 1, 1024, "wide open").tolist() == [[0, 4, 64, 128]]
    assert check_search(ga, gb, 1, 0, "closed").tolist() == [[0, 0, 128, 128]]


# ---------------------------------------------------------------- 3. the shift
@pytest.mark.parametrize("size", [(12, 20), (5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_shift_is_clamp_indexing_bit_for_bit(size):
    H, W = size
    # no move; even halves that are no multiple of 4 (8-byte loads); every index clamps; odd halves (scalar loads); multiples of 4 (16-byte loads)
    rec = np.array([[0, 0, 1, 2], [8, -4, -1, 0x7FFFFFFF], [-32768, 32768, -2 ** 31, 5], [6, 2, 0, 0], [-8, 16, 77, -77]], np.int32)
    B, C = rec.shape[0], 3
    x = oracle.generated(2, B * C * H * W).reshape(B, C, H, W).copy()
    xw = x.view(np.uint32)
    for k, word in enumerate((0x7FC12345, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000001)):
        xw[k, k % C, k % H, (2 * k) % W] = word
    clean = rec.copy()
    clean[:, 2:] = 0
    for sign in (1, -1):
        want = oracle.shift(x, rec, sign)
        assert np.array_equal(words(want), words(oracle.shift(x, clean, sign)))
        for so, do in ((0, 0), (1, 1), (1, 0), (0, 1)):
            _, xv = placed(x.shape, so, x)
            dbuf, dv = placed(x.shape, do)
            sbuf, sv = placed(rec.shape, 0, rec, torch.int32)
            assert lib.shift_f32(xv, sv, sign, out=dv) is dv
            guards_intact(dbuf, dv, (size, sign, so, do))
            guards_intact(sbuf, sv, "shifts are read only")
            same_words(dv, want, (size, sign, so, do))
            same_words(sv, rec, "shifts are read only")
    full = oracle.shift(x, rec, 1)
    assert (words(full)[2] == words(x)[2][:, -1:, :1]).all()                       # (-16384, 16384): every word is the bottom-left one
    same_words(lib.shift_f32(torch.from_numpy(x).cuda(), torch.from_numpy(rec).cuda(), 1), full, "allocating form")


# ---------------------------------------------------------------- 4. a planted pan, end to end
def moved(x, shifts, sign):
    """step 4 by torch indexing from records on the host: out[b][c][y][x] = x[b][c][cy(y - sign hy)][cx(x - sign hx)]"""
    H, W = x.shape[-2:]
    out = torch.empty_like(x)
    for b, rec in enumerate(shifts.tolist()):
        iy = (torch.arange(H, device=x.device) - sign * oracle.half(rec[0])).clamp(0, H - 1)
        ix = (torch.arange(W, device=x.device) - sign * oracle.half(rec[1])).clamp(0, W - 1)
        out[b] = x[b][:, iy][:, :, ix]
    return out


def test_align_pair_finds_a_planted_pan_and_makes_the_interiors_equal(picture):
    a, b = oracle.planted(picture, 32, 48, 8, -12)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    a2, b2, sh = lib.align_pair_f32(ad, bd, 16, 0.5)
    wa, wb, want = oracle.align_pair(a, b, 16, 512)
    assert sh.dtype == torch.int32 and sh.cpu().numpy().tolist() == want.tolist() and tuple(want[0, :3]) == (8, -12, 0)
    same_words(a2, wa, "a'")
    same_words(b2, wb, "b'")
    same_words(a2, moved(ad, sh.cpu(), 1), "a' by indexing")
    same_words(b2, moved(bd, sh.cpu(), -1), "b' by indexing")
    ys, xs = oracle.interior(32, 48, want[0])
    assert np.array_equal(words(a2)[..., ys, xs], words(b2)[..., ys, xs]) and not torch.equal(a2, b2)
    b3, a3, back = lib.align_pair_f32(bd, ad, 16, 0.5)
    assert back.cpu().numpy().tolist() == [[-8, 12, 0, int(want[0, 3])]] and torch.equal(a3, a2) and torch.equal(b3, b2)
    with pytest.raises(ValueError, match="needs frames of at least 80 x 80"):
        lib.align_pair_f32(ad, bd, 40, 0.5)


# ---------------------------------------------------------------- 5. the model
def build_model(mid, dtype, cls=EMA_VFI):
    m = cls(mid_channels=mid, compute_dtype=dtype).cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=mid), strict=True)
    return m


@pytest.fixture(scope="module")
def models():
    return {dt: build_model(8, dt) for dt in ("fp32", "bf16", "amp16")}


def pans(picture, H, W, shifts):
    """a batch of planted pairs, one per shift, on the device"""
    pairs = [oracle.planted(picture, H, W, *d, top=48 + 3 * k, left=64 + 5 * k) for k, d in enumerate(shifts)]
    return tuple(torch.from_numpy(np.concatenate([p[i] for p in pairs])).cuda() for i in (0, 1))


def run(model, a, b, **kw):
    with torch.no_grad():
        return model(a, b, **kw)


def composed(model, a, b, align, **kw):
    """model(a', b') with a' and b' made by torch indexing from the device's own records"""
    R, units = lib.align_args(*align, "test")
    sh = lib.align_search(lib.align_signature_f32(a), lib.align_signature_f32(b), R, units).cpu()
    return run(model, moved(a, sh, 1), moved(b, sh, -1), align=None, **kw), sh


@pytest.mark.parametrize("size,align,shifts", [((32, 48), (16, 0.5), ((8, -12), (-4, 16))), ((24, 40), (12, 0.5), ((-12, 4), (0, 8)))],
                         ids=["32x48", "24x40"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_aligned_forward_is_the_composition(models, picture, dtype, size, align, shifts):
    model = models[dtype]
    a, b = pans(picture, *size, shifts)
    plain = run(model, a, b)
    same_words(run(model, a, b, align=None), plain, "align=None is the plain call")
    want, sh = composed(model, a, b, align)
    assert [tuple(r[:2]) for r in sh.tolist()] == list(shifts)
    got = run(model, a, b, align=align)
    assert got.dtype == torch.float32 and got.shape == a.shape
    same_words(got, want, (dtype, size))
    assert torch.equal(model.align_shifts.cpu(), sh) and not torch.equal(got, plain)
    model.align = align
    try:
        same_words(run(model, a, b), want, "through the attribute")
        same_words(run(model, a, b, align=None), plain, "the per-call None over the attribute")
    finally:
        model.align = None
    # with the other options: M(a', b') with (a', b') in every role
    cases = [dict(ensemble="reverse"), dict(border=4), dict(flow_scale=2), dict(ensemble="reverse", agreement=(0.1, 1))]
    for kw in cases if size == (32, 48) else cases[:2]:
        same_words(run(model, a, b, align=align, **kw), composed(model, a, b, align, **kw)[0], (dtype, size, kw))
    # the exact time symmetry of the reversed ensemble survives: d*(b, a) = -d*(a, b), forward(b, a) runs on (b', a')
    sym = run(model, a, b, align=align, ensemble="reverse")
    same_words(run(model, b, a, align=align, ensemble="reverse"), sym, "ens(b, a) == ens(a, b)")
    assert (model.align_shifts.cpu()[:, :2] == -sh[:, :2]).all() and not torch.equal(sym, run(model, a, b, ensemble="reverse"))
    with pytest.raises(ValueError, match="return_taps=True with align"):
        run(model, a, b, align=align, return_taps=True)
    with pytest.raises(ValueError, match="a radius of 128 pixels needs frames of at least 256 x 256"):
        run(model, a, b, align=(128, 0.5))


def test_batch_of_one_an_odd_size_and_amp16(models, picture):
    for dtype, size, B in (("fp32", (33, 50), 1), ("bf16", (33, 50), 2), ("amp16", (32, 48), 2), ("bf16", (32, 48), 1)):
        model = models[dtype]
        a, b = pans(picture, *size, ((4, -8), (-8, 4))[:B])
        got = run(model, a, b, align=(16, 0.5))
        want, sh = composed(model, a, b, (16, 0.5))
        assert got.dtype == want.dtype == (torch.float16 if dtype == "amp16" else torch.float32)
        assert [tuple(r[:2]) for r in sh.tolist()] == [(4, -8), (-8, 4)][:B]
        assert torch.equal(got, want) and not torch.equal(got, run(model, a, b)), (dtype, size, B)


def test_a_rejected_pair_is_the_plain_forward_byte_for_byte(models, picture):
    model = models["bf16"]
    a, b = pans(picture, 32, 48, ((8, -12), (-4, 16)))
    noisy = b + torch.from_numpy(np.random.default_rng(0).normal(0, 0.02, tuple(b.shape)).astype(np.float32)).cuda()
    for x1, x2, align, what in ((a, a.clone(), (16, 1.0), "b = a"), (a, noisy, (16, 0.0), "ratio 0")):
        plain = run(model, x1, x2)
        got = run(model, x1, x2, align=align)
        assert (model.align_shifts.cpu()[:, :2] == 0).all(), what
        same_words(got, plain, what)
    assert (run(model, a, noisy, align=(16, 0.5)) != run(model, a, noisy)).any() and (model.align_shifts.cpu()[:, :2] != 0).any()


def test_stream_capture_replays_the_decision_of_the_new_content(models, picture):
    """nothing waits on the host: a captured aligned forward decides again, on the device, for whatever the static inputs hold"""
    model = models["fp32"]
    a, b = pans(picture, 32, 48, ((8, -12),))
    a2, b2 = pans(picture, 32, 48, ((-4, 16),))
    sa, sb = a.clone(), b.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(model, sa, sb, align=(16, 0.5))                                        # warm-up: weights packed, workspaces allocated
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = run(model, sa, sb, align=(16, 0.5))
    shifts = model.align_shifts
    for x1, x2, d in ((a, b, (8, -12)), (a2, b2, (-4, 16))):
        sa.copy_(x1)
        sb.copy_(x2)
        g.replay()
        torch.cuda.synchronize()
        assert tuple(shifts.cpu()[0, :2].tolist()) == d
        same_words(out, run(model, x1, x2, align=(16, 0.5)), ("replay", d))


# ---------------------------------------------------------------- 6. the harness
FH, FW = 48, 64
ALIGN = (16, 0.5)


class StandIn(EMA_VFI):
    """finds the shifts with the device's search, moves both frames by torch indexing, runs the parent's plain forward"""

    def forward(self, a, b):
        a, b = lib._f32c(a), lib._f32c(b)
        R, units = lib.align_args(*ALIGN, "stand-in")
        sh = lib.align_search(lib.align_signature_f32(a), lib.align_signature_f32(b), R, units).cpu()
        self.seen.append([tuple(r[:2]) for r in sh.tolist()])
        return EMA_VFI.forward(self, moved(a, sh, 1), moved(b, sh, -1), align=None)


@pytest.fixture(scope="module")
def harness_models():
    return build_model(8, "fp32"), build_model(8, "fp32", StandIn)


def clip(fmt, n, step=(4, -8)):
    """n frames of a camera moving by `step` pixels a frame over one picture: the content moves by -step"""
    pic = synth.synthetic_frames(9, 1, FH + 96, FW + 96)[0][0].numpy()
    pic = np.clip(pic * 0.22 + 0.5, 0.0, 1.0)
    out = []
    for k in range(n):
        top, left = 48 + step[0] * k, 48 + step[1] * k
        if fmt == "bgr24":
            out.append(np.ascontiguousarray((pic[:, top:top + FH, left:left + FW] * 255).astype(np.uint8).transpose(1, 2, 0)))
            continue
        peak, base, dt = (219, 16, np.uint8) if fmt == "yuv420p8" else (876, 64, np.uint16)
        y = (pic[0, top:top + FH, left:left + FW] * peak + base).astype(dt)
        u, v = ((pic[c, ::2, ::2][top // 2:(top + FH) // 2, left // 2:(left + FW) // 2] * peak * 0.5 + base + peak // 4).astype(dt) for c in (1, 2))
        out.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(FH * 3 // 2, FW))
    return out


def same_frames(got, want, what):
    assert len(got) == len(want) > 0, (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


MODES = {"reference": dict(), "recursive3": dict(mode="recursive", interpolation_factor=3),
         "resample": dict(mode="resample", rate_in=24, rate_out=60, resample_depth=2, static_guard=1, scene_threshold=0.9)}


@pytest.mark.parametrize("how", list(MODES))
@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p10"])
def test_harness_equals_a_stand_in_that_moves_by_indexing(harness_models, fmt, how):
    model, standin = harness_models
    frames_ = clip(fmt, 5)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format=fmt, **MODES[how])
    if fmt != "bgr24":
        kw.pop("scene_threshold", None)                                     # 16-bit frames are not scanned for cuts: the harness refuses the pair
    plain = list(FrameInterpolator(model, **kw).run(frames_))
    standin.seen = []
    want = list(FrameInterpolator(standin, **kw).run(frames_))
    fi = FrameInterpolator(model, align=ALIGN[0], align_ratio=ALIGN[1], **kw)
    got = list(fi.run(frames_))
    assert model.align is None                                                  # the harness's value rides on each call
    same_frames(got, want, (fmt, how))
    assert any(not np.array_equal(x, y) for x, y in zip(got, plain)), (fmt, how, "the alignment must show")
    # the report: one (dy, dx) per emitted prediction, in the order of the predictions
    if how == "resample":
        # per emitted frame made of node frames, the shift of the first node frame it names: every one of them some forward's
        assert 0 < len(fi.align_shifts) < len(got) and set(fi.align_shifts) <= {d for batch in standin.seen for d in batch}
        assert any(d != (0, 0) for d in fi.align_shifts)
        return
    if how == "reference":
        listed = [d for batch in standin.seen for d in batch]
        assert listed == [(-4, 8)] * 4                                            # the content moves against the camera
    else:
        listed = []
        for mid, left, right in zip(standin.seen[0::3], standin.seen[1::3], standin.seen[2::3]):     # per batch: the midpoint first
            listed += [d for k in range(len(mid)) for d in (left[k], mid[k], right[k])]
        assert listed[1::3] == [(-4, 8)] * 4
    assert fi.align_shifts == listed and len(listed) == sum(1 for f in got) - len(frames_)


@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p8"])      # the metric kernel reads bytes: evaluate() refuses the 16-bit formats
def test_evaluate_equals_the_stand_in(harness_models, fmt):
    model, standin = harness_models
    frames_ = clip(fmt, 7, step=(2, -4))                     # a target's neighbours are two frames apart
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format=fmt)
    plain = FrameInterpolator(model, **kw).evaluate(frames_, every=2)
    standin.seen = []
    want = FrameInterpolator(standin, **kw).evaluate(frames_, every=2)
    got = FrameInterpolator(model, align=ALIGN[0], align_ratio=ALIGN[1], **kw).evaluate(frames_, every=2)
    assert (got.size, got.channels) == (want.size, want.channels) and len(got.targets) == len(want.targets) == 3
    assert [(s.t, s.sse, s.ssimq) for s in got] == [(s.t, s.sse, s.ssimq) for s in want], fmt
    assert [s.sse for s in got] != [s.sse for s in plain] and [d for batch in standin.seen for d in batch] == [(-4, 8)] * 3


# ---------------------------------------------------------------- 7. the command line
def test_command_line_align(harness_models, tmp_path, capsys):
    model, _ = harness_models
    frames_ = clip("yuv420p8", 4)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(FW, FH, 24, 1, colorspace="420jpeg")) as w:
        for f in frames_:
            w.write(f)
    base = [str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1"]
    assert cli.main(base + ["--align", "16"]) != 0
    assert "belong together" in capsys.readouterr().err and not dst.exists()
    rc = cli.main(base + ["--align", "16", "--align-ratio", "0.5"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "align 16 px at ratio 0.5 shifted 100.00 % of the predictions" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format="yuv420p8")
    same_frames(got, list(FrameInterpolator(model, align=16, align_ratio=0.5, **kw).run(frames_)), "cli")   # seed 0, 8 channels, fp32: the fixture's model
    assert not np.array_equal(got[0], list(FrameInterpolator(model, **kw).run(frames_))[0])                 # the first pair's prediction comes first
    assert cli.main(base[:1] + base[2:] + ["--evaluate", "--align", "16", "--align-ratio", "0.5"]) == 0
    assert "psnr" in capsys.readouterr().out.lower()
