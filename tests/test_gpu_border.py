"""Frame borders on the device (include/emavfi.h, "BORDER DEFINITION"): emavfi_border_pad_f32 and emavfi_border_crop_f32 against the numpy
oracle (tests/border_oracle.py) bit for bit, on every access width and between guard words; past 2^32 bytes; EMA_VFI.border against the
composition crop(forward(pad a, pad b)) it is defined as, plain and ensembled, with the ensemble's two exact symmetries carried over; the
harness against a stand-in model that pads by indexing; the command line.  Every comparison is an equality of 32-bit words or of bytes."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import border_oracle as oracle
import ensemble_oracle

pytestmark = pytest.mark.gpu

GUARD = 64                      # words of guard on either side: 256 bytes, so the band keeps the tensor's 16-byte alignment
GUARD_WORD = 0x7B7B7B7B
UNWRITTEN = 0x55AA55AA          # what dst holds before a call: no generated or planted word equals it
PLANES = 3
# (H, W, N): smallest frame; H = 1; W = 1; scalar path; scalar path with several reflections; wide stores with aligned interior loads; wide
# stores with a misaligned interior; a padded row of 8 from an odd-quarter W; N at its maximum; a typical test frame; the copy
CASES = [(1, 1, 1), (1, 7, 3), (5, 1, 2), (5, 7, 1), (5, 7, 9), (8, 16, 4), (8, 16, 2), (6, 6, 1), (12, 20, 64), (24, 40, 16), (8, 16, 0)]


def words(t):
    """the 32-bit words of a float32 tensor or array, as a numpy uint32 array on the host"""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "words differ")


def picture(shape, seed):
    """generated values with -0.0, both infinities and NaNs with payloads planted"""
    t = oracle.generated(seed, int(np.prod(shape))).copy()
    w = t.view(np.uint32)
    assert not (w == UNWRITTEN).any() and not (w == GUARD_WORD).any()
    for k, word in enumerate((0x80000000, 0x7F800000, 0x7FC12345, 0xFF800000, 0xFFC00001, 0x00000001)):
        w[(k * 7) % w.size] = word
    return t.reshape(shape)


def placed(shape, off, values=None, pinned=False):
    """(buffer, view): a float32 view of `shape` inside a word buffer between guard words, starting `off` words behind a 16-byte boundary;
    filled with `values` or, for a destination, with UNWRITTEN"""
    count = int(np.prod(shape))
    host = np.full(count + 2 * GUARD + off, GUARD_WORD, np.uint32)
    host[GUARD + off:GUARD + off + count] = UNWRITTEN if values is None else words(values).reshape(-1)
    buf = torch.from_numpy(host.view(np.int32))
    buf = buf.pin_memory() if pinned else buf.cuda()
    view = buf[GUARD + off:GUARD + off + count].view(torch.float32).view(shape)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * (GUARD + off)
    return buf, view


def guards_intact(buf, view, what):
    torch.cuda.synchronize()
    w = words(buf.view(torch.float32))
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    rest = np.concatenate([w[:lo], w[lo + view.numel():]])
    assert rest.size >= 2 * GUARD and (rest == GUARD_WORD).all(), (what, "a guard word was written")


# the placements of (src, dst): (src offset in words, dst offset in words, dst in pinned host memory)
PLACEMENTS = {"dense": (0, 0, False), "both_4_bytes_in": (1, 1, False), "src_4_bytes_in": (1, 0, False), "pinned_dst": (0, 0, True)}


# ---------------------------------------------------------------- 1. the entries against the oracle
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_entries_are_the_oracle_bit_for_bit(case):
    H, W, N = case
    Hp, Wp = H + 2 * N, W + 2 * N
    assert lib.border_padded_size(H, W, N) == (Hp, Wp)
    src = picture((PLANES, H, W), seed=H * 100 + W)
    big = picture((PLANES, Hp, Wp), seed=H * 100 + W + 1)                  # an arbitrary tensor of the padded size, to crop
    for name, (soff, doff, pinned) in PLACEMENTS.items():
        sbuf, sview = placed(src.shape, soff, src)
        bbuf, bview = placed(big.shape, soff, big)
        for mode in oracle.MODES:
            what = (case, name, mode)
            want = oracle.pad(src, N, mode)
            dbuf, dview = placed(want.shape, doff, pinned=pinned)
            assert lib.border_pad_f32(sview, N, mode, out=dview) is dview
            guards_intact(dbuf, dview, what)
            got = words(dview)
            assert not (got == UNWRITTEN).any(), (what, "a word of dst was not written")
            same_words(dview, want, what)
            # crop(pad(x)) is x: from the padded tensor just written, when it is on the device, into a fresh destination
            if not pinned:
                cbuf, cview = placed(src.shape, doff)
                assert lib.border_crop_f32(dview, N, out=cview) is cview
                guards_intact(cbuf, cview, what)
                same_words(cview, src, (what, "crop(pad(x))"))
            if mode == "reflect":
                same_words(lib.border_pad_f32(sview, N, lib.BORDER_REFLECT), want, (what, "by code, own out"))
        # crop of an arbitrary tensor is the slice
        cbuf, cview = placed(src.shape, doff, pinned=pinned)
        lib.border_crop_f32(bview, N, out=cview)
        guards_intact(cbuf, cview, (case, name, "crop"))
        assert not (words(cview) == UNWRITTEN).any()
        same_words(cview, oracle.crop(big, N), (case, name, "crop"))
        same_words(cview, big[:, N:N + H, N:N + W], (case, name, "crop is the slice"))
        for b, v, orig in ((sbuf, sview, src), (bbuf, bview, big)):
            guards_intact(b, v, "a source")                                 # nothing but dst is written
            same_words(v, orig, "a source is left as it was")
    # out allocated by the wrapper, over leading dimensions of any count
    x = torch.from_numpy(src).cuda()
    same_words(lib.border_pad_f32(x.view(1, PLANES, 1, H, W), N, "replicate"), oracle.pad(src, N, "replicate").reshape(1, PLANES, 1, Hp, Wp), case)
    same_words(lib.border_crop_f32(torch.from_numpy(big).cuda()[0], N), oracle.crop(big, N)[0], case)


def test_wide_and_scalar_paths_agree_and_refusals_are_codes():
    src = picture((PLANES, 24, 40), seed=77)
    for N in (2, 4, 16):
        for mode in oracle.MODES:
            a = lib.border_pad_f32(placed(src.shape, 0, src)[1], N, mode)
            b = lib.border_pad_f32(placed(src.shape, 1, src)[1], N, mode, out=placed(a.shape, 1)[1])
            assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
            same_words(a, b, (N, mode))
    x = torch.from_numpy(src).cuda()
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        lib.border_pad_f32(x, 0, out=x)
    both = torch.zeros(3 * x.numel(), device="cuda")
    with pytest.raises(RuntimeError, match="dst overlaps src"):
        lib.border_crop_f32(both[:PLANES * 26 * 42].view(PLANES, 26, 42), 1, out=both[PLANES * 26 * 42 - 1:PLANES * 26 * 42 - 1 + x.numel()].view(x.shape))
    with pytest.raises(RuntimeError, match="PINNED"):
        lib.border_pad_f32(torch.from_numpy(src), 1)
    L = lib.load()
    assert L.emavfi_border_pad_f32(x.data_ptr(), both.data_ptr(), PLANES, 24, 40, 65, 0, None) == -1 and "N = 65" in lib.last_error()
    assert L.emavfi_border_pad_f32(x.data_ptr(), both.data_ptr(), PLANES, 24, 40, 1, 2, None) == -1 and "mode = 2" in lib.last_error()
    assert L.emavfi_border_crop_f32(x.data_ptr(), both.data_ptr(), PLANES, 24, 16384, 1, None) == -1 and "padded" in lib.last_error()
    same_words(lib.border_pad_f32(x, 3, "reflect"), oracle.pad(src, 3, "reflect"), "a good call after the refusals")


# ---------------------------------------------------------------- 2. past 2^32 bytes
def test_a_tensor_past_2_pow_32_bytes():
    planes, H, W, N = 68, 4096, 4096, 4
    Hp, Wp = H + 2 * N, W + 2 * N
    assert planes * H * W * 4 > 1 << 32
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory")
    src = torch.arange(planes * H * W, device="cuda", dtype=torch.int32).view(planes, H, W)     # word i holds i: every word differs
    at = planes * H * W * 4 // 2 // (H * W * 4)                                                  # a plane in the middle, for good measure
    first = (1 << 32) // (Hp * Wp * 4)                                                           # the padded plane that straddles 2^32 bytes
    assert (1 << 32) // (H * W * 4) == 64 and first == 63
    check = sorted({0, planes - 1, 62, 63, 64, 65, at})
    for mode in oracle.MODES:
        iy = torch.from_numpy(oracle.indices(H, N, mode)).cuda()
        ix = torch.from_numpy(oracle.indices(W, N, mode)).cuda()
        out = lib.border_pad_f32(src.view(torch.float32), N, mode).view(torch.int32)
        assert out.shape == (planes, Hp, Wp)
        for p in check:
            assert torch.equal(out[p], src[p][iy][:, ix]), (mode, p)
        back = lib.border_crop_f32(out.view(torch.float32), N).view(torch.int32)
        for p in check:
            assert torch.equal(back[p], src[p]), (mode, p, "crop")
        del out, back


# ---------------------------------------------------------------- 3 - 6. the model
def build_model(mid, dtype, cls=EMA_VFI):
    m = cls(mid_channels=mid, compute_dtype=dtype).cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=mid), strict=True)
    return m


@pytest.fixture(scope="module")
def models():
    return {dt: build_model(8, dt) for dt in ("fp32", "bf16", "amp16")}


def frames(B, H, W, seed=3):
    a, b = synth.synthetic_frames(seed, B, H, W, "natural")
    return a.contiguous(), b.contiguous()


def run(model, a, b, **kw):
    with torch.no_grad():
        return model(a, b, **kw)


def composed(model, a, b, N, mode, **kw):
    """crop(G(pad a, pad b)) with pad and crop done by the oracle on the host; G is the model's forward at the padded size"""
    pa, pb = (torch.from_numpy(oracle.pad(t.numpy(), N, mode)).cuda() for t in (a, b))
    out = run(model, pa, pb, border=None, **kw)
    return oracle.crop(out.float().cpu().numpy(), N), out.dtype


@pytest.mark.parametrize("size", [(24, 40), (23, 37)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_bordered_forward_is_the_composition(models, dtype, size):
    model = models[dtype]
    a, b = frames(2, *size)
    ad, bd = a.cuda(), b.cuda()
    plain = run(model, ad, bd)
    same_words(run(model, ad, bd, border=None), plain, "border=None is the plain call")
    for N in (1, 4, 16):
        for mode in oracle.MODES:
            what = (dtype, size, N, mode)
            want, _ = composed(model, a, b, N, mode)
            got = run(model, ad, bd, border=(N, mode))
            assert got.dtype == torch.float32 and got.shape == ad.shape
            same_words(got, want, what)
            assert not torch.equal(got, plain), (what, "the bordered forward must differ from the plain one")
            model.border = (N, mode)
            try:
                same_words(run(model, ad, bd), want, (what, "through the attribute"))
                same_words(run(model, ad, bd, border=None), plain, (what, "the per-call None over the attribute"))
            finally:
                model.border = None
    same_words(run(model, ad, bd, border=4), composed(model, a, b, 4, "replicate")[0], "an int is replicate")
    with pytest.raises(ValueError, match="return_taps=True with a border"):
        run(model, ad, bd, border=4, return_taps=True)
    out, taps = run(model, ad, bd, return_taps=True)
    same_words(out, plain, "return_taps without a border still works")
    assert model.border is None and "feat" in taps


def test_amp16_converts_after_the_crop(models):
    model = models["amp16"]
    a, b = frames(2, 23, 37)
    for N, mode in ((4, "reflect"), (1, "replicate")):
        got = run(model, a.cuda(), b.cuda(), border=(N, mode))
        want, dt = composed(model, a, b, N, mode)
        assert got.dtype == dt == torch.float16 and got.shape == a.shape
        assert torch.equal(got.cpu(), torch.from_numpy(want).half())
        assert not torch.equal(got, run(model, a.cuda(), b.cuda()))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_of_one_and_an_odd_sample_size(models, dtype):
    """B = 1 and 3 * 23 * 37 odd: the forward runs as one sequence of launches, not pipelined over two streams"""
    model = models[dtype]
    for size in ((23, 37), (24, 40)):
        a, b = frames(1, *size, seed=5)
        plain = run(model, a.cuda(), b.cuda())
        for N, mode in ((1, "reflect"), (4, "replicate"), (16, "reflect")):
            got = run(model, a.cuda(), b.cuda(), border=(N, mode))
            same_words(got, composed(model, a, b, N, mode)[0], (dtype, size, N, mode))
            assert not torch.equal(got, plain)


def test_ensemble_with_a_border_is_the_composition_and_keeps_its_symmetries(models):
    model = models["fp32"]                                                 # fp32: the route is fixed
    a, b = frames(2, 23, 37, seed=7)
    ad, bd = a.cuda(), b.cuda()
    kw = dict(ensemble="full", border=(4, "reflect"))
    base = run(model, ad, bd, **kw)
    same_words(base, composed(model, a, b, 4, "reflect", ensemble="full")[0], "crop(ens(pad a, pad b))")
    assert not torch.equal(base, run(model, ad, bd, ensemble="full")) and not torch.equal(base, run(model, ad, bd, border=(4, "reflect")))
    # exact symmetry in time and exact flip equivariance carry over, bit for bit
    same_words(run(model, bd, ad, **kw), base, "ens(b, a) == ens(a, b)")

    def phi(t, g):
        return torch.from_numpy(ensemble_oracle.flip(t.cpu().numpy(), g)).cuda()
    for g in (1, 2, 3):
        same_words(run(model, phi(a, g), phi(b, g), **kw), phi(base, g), ("ens(phi a, phi b) == phi ens(a, b)", g))
    # neither holds for the bordered plain forward: the properties are the ensemble's
    assert not torch.equal(run(model, bd, ad, border=(4, "reflect")), run(model, ad, bd, border=(4, "reflect")))


# ---------------------------------------------------------------- 7. the harness
FH, FW = 48, 64


class StandIn(EMA_VFI):
    """pads by torch indexing from the oracle's index vectors, runs the parent's plain forward, slices"""
    pad_n, pad_mode = 8, "replicate"

    def forward(self, a, b):
        N = self.pad_n
        iy = torch.from_numpy(oracle.indices(a.shape[-2], N, self.pad_mode)).to(a.device)
        ix = torch.from_numpy(oracle.indices(a.shape[-1], N, self.pad_mode)).to(a.device)
        pa, pb = (t[..., iy, :][..., :, ix].contiguous() for t in (a, b))
        out = EMA_VFI.forward(self, pa, pb, ensemble=None, border=None)
        return out[..., N:N + a.shape[-2], N:N + a.shape[-1]].contiguous()


@pytest.fixture(scope="module")
def harness_models():
    return build_model(8, "fp32"), build_model(8, "fp32", StandIn)


def clip(fmt, n, seed=1):
    rng = np.random.default_rng(seed)
    if fmt == "bgr24":
        return [(rng.uniform(0, 1, (FH, FW, 3)) * 255).astype(np.uint8) for _ in range(n)]
    if fmt == "yuv420p8":
        return [(rng.uniform(0, 1, (FH * 3 // 2, FW)) * 219 + 16).astype(np.uint8) for _ in range(n)]
    return [(rng.uniform(0, 1, (FH * 3 // 2, FW)) * 876 + 64).astype(np.uint16) for _ in range(n)]


def same_frames(got, want, what):
    assert len(got) == len(want) > 0, (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, int((g != w).sum()))


MODES = {"reference": dict(), "recursive3": dict(mode="recursive", interpolation_factor=3),
         "resample": dict(mode="resample", rate_in=24, rate_out=60, resample_depth=2, static_guard=1, scene_threshold=0.9)}


@pytest.mark.parametrize("how", list(MODES))
@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p10"])
def test_harness_equals_a_stand_in_that_pads_by_indexing(harness_models, fmt, how):
    model, standin = harness_models
    frames_ = clip(fmt, 5)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format=fmt, **MODES[how])
    if fmt != "bgr24":
        kw.pop("scene_threshold", None)                                     # 16-bit frames are not scanned for cuts: the harness refuses the pair
    plain = list(FrameInterpolator(model, **kw).run(frames_))
    for mode in oracle.MODES:
        standin.pad_mode = mode
        want = list(FrameInterpolator(standin, **kw).run(frames_))
        got = list(FrameInterpolator(model, border=8, border_mode=mode, **kw).run(frames_))
        assert model.border is None                                         # the harness's value rides on each call
        same_frames(got, want, (fmt, how, mode))
        assert any(not np.array_equal(x, y) for x, y in zip(got, plain)), (fmt, how, mode, "the border must show")
    standin.pad_mode = "replicate"


@pytest.mark.parametrize("fmt", ["bgr24", "yuv420p8"])      # the metric kernel reads bytes: evaluate() refuses the 16-bit formats
def test_evaluate_equals_the_stand_in(harness_models, fmt):
    model, standin = harness_models
    frames_ = clip(fmt, 7, seed=2)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format=fmt)
    plain = FrameInterpolator(model, **kw).evaluate(frames_, every=2)
    for mode in oracle.MODES:
        standin.pad_mode = mode
        want = FrameInterpolator(standin, **kw).evaluate(frames_, every=2)
        got = FrameInterpolator(model, border=8, border_mode=mode, **kw).evaluate(frames_, every=2)
        assert (got.size, got.channels) == (want.size, want.channels) and len(got.targets) == len(want.targets) == 3
        assert [(s.t, s.sse, s.ssimq) for s in got] == [(s.t, s.sse, s.ssimq) for s in want], (fmt, mode)
        assert [s.sse for s in got] != [s.sse for s in plain]
    standin.pad_mode = "replicate"


# ---------------------------------------------------------------- 8. the command line
def test_command_line_border(harness_models, tmp_path, capsys):
    model, _ = harness_models
    frames_ = [(np.random.default_rng(k).uniform(0, 1, (FH * 3 // 2, FW)) * 219 + 16).astype(np.uint8) for k in range(4)]
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(FW, FH, 24, 1, colorspace="420jpeg")) as w:
        for f in frames_:
            w.write(f)
    base = [str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2", "--factor", "1"]
    assert cli.main(base + ["--border-mode", "reflect"]) != 0
    assert "--border-mode needs --border" in capsys.readouterr().err and not dst.exists()
    rc = cli.main(base + ["--border", "8", "--border-mode", "reflect"])
    err = capsys.readouterr().err
    assert rc == 0 and "7 frames out" in err and "border 8 reflect" in err, err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    kw = dict(batch_pairs=2, reference_quirks=False, pixel_format="yuv420p8")
    same_frames(got, list(FrameInterpolator(model, border=8, border_mode="reflect", **kw).run(frames_)), "cli")   # seed 0, 8 channels, fp32: the fixture's model
    assert not np.array_equal(got[0], list(FrameInterpolator(model, **kw).run(frames_))[0])                       # the first pair's prediction comes first
    assert cli.main(base[:1] + base[2:] + ["--evaluate", "--border", "4"]) == 0
    assert "psnr" in capsys.readouterr().out.lower()
