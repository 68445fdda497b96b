"""Linear light on the GPU: emavfi_accumulate_frames_linear against the numpy restatement of the linear light definition
(tests/linear_light_oracle.py) and against emavfi_accumulate_frames, and the harness's ``light=`` under a shutter and under the blend against
the oracle's accumulation of the frames mode "recursive" yields.  Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import linear_light_oracle as oracle
import scene_oracle
import shutter_oracle

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
NODES = lib.RESAMPLE_NODES
N_SRCS, N_NODES = 3, 31
TOP = (1985,) * 32 + (2015,)                                         # 33 weights that sum to 65535
FORMATS5 = [(1, 8, 0), (2, 10, 6), (2, 10, 0), (2, 12, 4), (2, 12, 0)]


def up(v, m):
    return (v + m - 1) // m * m


def pool(data, stride):
    """frames `data` [n, fb] on the device, `stride` bytes apart, in an allocation of exactly (n - 1) stride + fb bytes"""
    n, fb = data.shape
    raw = torch.full(((n - 1) * stride + fb,), 0x3C, dtype=torch.uint8, device="cuda")
    view = raw.as_strided((n, fb), (stride, 1))
    view.copy_(torch.from_numpy(data))
    return view


def device_table(lin):
    """the bits of a uint32 table as the int32 device tensor the wrapper takes"""
    return torch.from_numpy(np.ascontiguousarray(lin, dtype=np.uint32).view(np.int32)).cuda()


def table(flags_on):
    """the 9 entries of tests/test_gpu_shutter.py, so two launches: n = 1, 2, 3 and 33, both pools, the largest weight sum, an entry whose
    flag is clear and one whose flag is set, and the (256 - w, w) of a blend in the second launch"""
    every = (0, *(NODES | i for i in range(N_NODES)), 1)              # 33 taps: source 0, every node, source 1
    return [((1,), (7,), 0, 0), ((NODES | 0, NODES | 1), (1, 1), 0, 0), ((0, NODES | 0, NODES | 1), (1, 2, 1), 0, 0), (every, TOP, 0, 0),
            ((NODES | 3, NODES | 4, NODES | 5), (5, 6, 1), 1 if flags_on else 0, 1), ((2, NODES | 30), (65534, 1), 0, 0),
            (every, (1,) * 33, 2 if flags_on else 0, 2),
            ((NODES | 7,), (1,), 0, 0), ((1, 2), (192, 64), 0, 0)]


def pools(samples, sb, seed):
    fb = samples * sb
    rng = np.random.default_rng(seed)
    srcs = rng.integers(0, 256, (N_SRCS, fb), dtype=np.uint8)        # at 2 bytes per sample: whole words, bits outside the sample included
    nodes = rng.integers(0, 256, (N_NODES, fb), dtype=np.uint8)
    for p in (srcs, nodes):
        p[:, :32 * sb], p[:, 32 * sb:64 * sb] = 255, 0
    return fb, srcs, nodes


_tables = {}


def built_in(name, depth, full):
    if (name, depth, full) not in _tables:
        lin = lib.transfer_table(name, depth, full)
        lib.transfer_table_check(lin, depth)
        _tables[name, depth, full] = (lin, device_table(lin))
    return _tables[name, depth, full]


@pytest.mark.parametrize("name,full", [("bt709", False), ("hlg", True)])
@pytest.mark.parametrize("sb,depth,shift", FORMATS5)
@pytest.mark.parametrize("samples", [9 * 11 * 3, 24 * 40 * 3])
def test_entry_is_the_oracle_byte_for_byte(samples, sb, depth, shift, name, full):
    """frames of 9 x 11 x 3 samples (297 bytes, 594 as words: no multiple of 16, so dense frames after the first are misaligned and go by bytes
    or words) and of 24 x 40 x 3 (aligned); dense pools, a stride that breaks the alignment and the next multiple of 16 (16-byte accesses and
    a byte / word tail); linear_bytes of 0, of 99 samples (inside a 16-byte piece: both halves of it follow their own rule), of 96 samples
    and of the whole frame.  The first samples of every frame are all ones, the next all zeros: with the weights that sum to 65535 the
    largest intermediate of the definition, 65535 * lin[2^depth - 1] + 32767, occurs."""
    fb, srcs, nodes = pools(samples, sb, samples + 16 * depth + shift)
    lin, d_lin = built_in(name, depth, full)
    for stride, fl in ((fb, None), (fb + 6, (0, 1)), (up(fb, 16), (0, 1))):
        tab = table(fl is not None)
        d_s, d_n = pool(srcs, stride), pool(nodes, stride + (16 if stride % 16 == 0 else 2))
        flags = torch.tensor(fl, dtype=torch.int32, device="cuda") if fl is not None else None
        for lb in (0, 99 * sb, 96 * sb, fb):
            raw = torch.full(((len(tab) - 1) * stride + fb + GUARD,), POISON, dtype=torch.uint8, device="cuda")
            dst = raw.as_strided((len(tab), fb), (stride, 1))
            want = np.full(raw.shape, POISON, np.uint8)
            out = oracle.accumulate(srcs, nodes, tab, fl, lin, lb, sb, depth, shift)
            for k in range(len(tab)):
                want[k * stride:k * stride + fb] = out[k]
            assert lib.accumulate_frames_linear(dst, d_s, d_n, tab, d_lin, lb, flags, sb, depth, shift).data_ptr() == dst.data_ptr()
            got = raw.cpu().numpy()
            assert np.array_equal(got, want), ("frames / stride gaps / the bytes after the last frame", fb, stride, fl, depth, shift, lb,
                                               [k for k in range(len(tab)) if not np.array_equal(got[k * stride:k * stride + fb], out[k])])
            # what the table is meant to reach
            full_code = (255 if sb == 1 else ((1 << depth) - 1) << shift)
            top = np.frombuffer(out[3].tobytes(), "<u2" if sb == 2 else np.uint8)
            assert (top[:32] == full_code).all() and (top[32:64] == 0).all()
            if fl is not None:
                assert np.array_equal(out[6], srcs[2]) and not np.array_equal(out[4], srcs[1])  # the set flag holds, the clear one does not
        assert np.array_equal(d_s.cpu().numpy(), srcs) and np.array_equal(d_n.cpu().numpy(), nodes)
        assert np.array_equal(d_lin.cpu().numpy().view(np.uint32), lin)


@pytest.mark.parametrize("sb,depth,shift", FORMATS5)
def test_no_linear_bytes_and_the_affine_table_are_the_coded_entry(sb, depth, shift):
    fb, srcs, nodes = pools(24 * 40 * 3 + 5, sb, depth + shift)
    d_s, d_n = torch.from_numpy(srcs).cuda(), torch.from_numpy(nodes).cuda()
    tab = table(True)
    flags = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    coded, a, b = (torch.full((len(tab), fb), POISON, dtype=torch.uint8, device="cuda") for _ in range(3))
    lib.accumulate_frames(coded, d_s, d_n, tab, flags, sb, depth, shift)
    lib.accumulate_frames_linear(a, d_s, d_n, tab, built_in("hlg", depth, True)[1], 0, flags, sb, depth, shift)
    assert torch.equal(a, coded)
    affine = oracle.affine(depth)
    lib.transfer_table_check(affine, depth)
    lib.accumulate_frames_linear(b, d_s, d_n, tab, device_table(affine), fb, flags, sb, depth, shift)
    assert torch.equal(b, coded)
    assert np.array_equal(coded.cpu().numpy(), shutter_oracle.accumulate(srcs, nodes, tab, [0, 1], sb, depth, shift))


@pytest.mark.parametrize("sb,depth,shift", FORMATS5)
def test_a_constant_clip_stays_constant(sb, depth, shift):
    rng = np.random.default_rng(3 * depth + shift)
    fb = (24 * 40 * 3 + 3) * sb
    frame = rng.integers(0, 256, fb, dtype=np.uint8)
    if sb == 2:                                                       # only the sample's bits: the other bits of a word are written as zero
        frame = (frame.view("<u2") & (((1 << depth) - 1) << shift)).astype("<u2").view(np.uint8)
    d_s, d_n = torch.from_numpy(np.stack([frame] * N_SRCS)).cuda(), torch.from_numpy(np.stack([frame] * N_NODES)).cuda()
    tab = table(False)
    for name, full in (("srgb", True), ("bt709", False), ("hlg", False)):
        dst = torch.full((len(tab), fb), POISON, dtype=torch.uint8, device="cuda")
        lib.accumulate_frames_linear(dst, d_s, d_n, tab, built_in(name, depth, full)[1], fb, None, sb, depth, shift)
        assert np.array_equal(dst.cpu().numpy(), np.stack([frame] * len(tab))), (name, full)


@pytest.mark.parametrize("sb,depth,shift", FORMATS5)
def test_a_table_that_is_not_valid_gives_codes_and_touches_nothing_else(sb, depth, shift):
    """the contract is that the table passed the check; the kernel is memory-safe all the same: the decode index is masked to the table and
    the search is bounded to it, so all zeros and random words give SOME code per sample, the guard bytes stay, the pools stay"""
    fb, srcs, nodes = pools(24 * 40 * 3 + 5, sb, 7)
    d_s, d_n = torch.from_numpy(srcs).cuda(), torch.from_numpy(nodes).cuda()
    tab = table(False)
    rng = np.random.default_rng(depth)
    for junk in (np.zeros(1 << depth, np.uint32), rng.integers(0, 1 << 32, 1 << depth, dtype=np.uint64).astype(np.uint32)):
        assert not oracle.valid(junk)
        raw = torch.full((len(tab) * fb + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        dst = raw[:len(tab) * fb].view(len(tab), fb)
        lib.accumulate_frames_linear(dst, d_s, d_n, tab, device_table(junk), fb, None, sb, depth, shift)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        assert (got[len(tab) * fb:] == POISON).all()
        mixed = got[:len(tab) * fb].reshape(len(tab), fb)[[1, 2, 3, 4, 5, 6, 8]]
        if sb == 2:
            assert (mixed.view("<u2") & ~np.uint16(((1 << depth) - 1) << shift) == 0).all()
        assert np.array_equal(got[:fb], srcs[1]) and np.array_equal(got[7 * fb:8 * fb], nodes[7])     # the copies do not look at the table
        assert np.array_equal(d_s.cpu().numpy(), srcs) and np.array_equal(d_n.cpu().numpy(), nodes)


# ---------------------------------------------------------------- the harness
H, W, NF, D, G = 24, 40, 5, 2, 4
FORMATS = ["bgr24", "nv12", "p010", "yuv420p10"]


class Counting(EMA_VFI):
    """the model, counting the pairs it is given"""
    def forward(self, a, b, *args, **kw):
        self.rows.append(a.shape[0])
        return EMA_VFI.forward(self, a, b, *args, **kw)


@pytest.fixture(scope="module")
def model():
    m = Counting(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
    m.rows = []
    return m


def clip(fmt, n=NF, h=H, w=W, seed=1):
    rng = np.random.default_rng(seed)
    if fmt == "bgr24":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    if fmt in ("nv12", "yuv420p8"):
        return [rng.integers(16, 236, (h * 3 // 2, w), dtype=np.uint8) for _ in range(n)]
    depth = lib.DEPTHS.get(fmt) or lib.PLANAR_DEPTHS[fmt]
    shift = 16 - depth if fmt in lib.DEPTHS else 0
    return [(rng.integers(64, 940, (h * 3 // 2, w)) << (depth - 10 + shift)).astype(np.uint16) for _ in range(n)]


_recursive = {}


def recursive(model, fmt, frames=None, key="clip", **kw):
    """(sources, nodes): sources[s] as emitted and nodes[s][j - 1], j = 1 .. G - 1, of mode "recursive" with factor G - 1 - computed once per
    configuration and left unchanged"""
    k = (fmt, key, tuple(sorted(kw.items())))
    if k not in _recursive:
        if frames is None:
            frames = clip(fmt)
        out = list(FrameInterpolator(model, G - 1, 1, batch_pairs=2, reference_quirks=False, mode="recursive", pixel_format=fmt, **kw).run(frames))
        assert len(out) == (len(frames) - 1) * G + 1
        srcs = [out[s * G + G - 1] for s in range(len(frames) - 1)] + [out[-1]]
        _recursive[k] = (srcs, [out[s * G:s * G + G - 1] for s in range(len(frames) - 1)])
    return _recursive[k]


def luma_bytes(fmt, frame):
    """linear_bytes of the harness: the whole bgr24 frame, the Y plane of a 4:2:0 frame"""
    return frame.nbytes if fmt == "bgr24" else frame.nbytes * 2 // 3


def mix(fmt, frames, weights, lin):
    """the oracle's mean of emitted frames: in light below linear_bytes, coded above"""
    sb, depth, shift = lib.resample_sample_format(fmt)
    fr = [np.ascontiguousarray(f).view(np.uint8).reshape(-1) for f in frames]
    lb = luma_bytes(fmt, frames[0])
    out = shutter_oracle.mean(fr, weights, sb, depth, shift)
    out[:lb] = oracle.mean([f[:lb] for f in fr], weights, lin, sb, depth, shift)
    return out.view(frames[0].dtype).reshape(frames[0].shape)


def harness_table(fmt, name, full_range=False):
    depth = lib.resample_sample_format(fmt)[1]
    return lib.transfer_table(name, depth, True if fmt == "bgr24" else full_range)


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k)


def chroma_same_luma_differs(fmt, got, plain):
    assert len(got) == len(plain)
    if fmt != "bgr24":
        rows = got[0].shape[0] * 2 // 3
        assert all(np.array_equal(g[rows:], p[rows:]) for g, p in zip(got, plain)), "chroma stays coded"
        assert any(not np.array_equal(g[:rows], p[:rows]) for g, p in zip(got, plain)), "luma is mixed in light"
    else:
        assert any(not np.array_equal(g, p) for g, p in zip(got, plain))


@pytest.mark.parametrize("fmt", FORMATS)
def test_shutter_in_light_is_the_oracles_accumulation_of_the_recursive_nodes(model, fmt):
    srcs, nodes = recursive(model, fmt)
    plan = FrameInterpolator.shutter_plan(NF, 15, 15, D, 180)
    kw = dict(batch_pairs=2, reference_quirks=False, mode="resample", pixel_format=fmt, rate_in=15, rate_out=15, resample_depth=D, shutter=180)
    frames = clip(fmt)
    model.rows.clear()
    plain = list(FrameInterpolator(model, **kw).run(frames))
    rows_plain = list(model.rows)
    model.rows.clear()
    fi = FrameInterpolator(model, light="bt709", **kw)
    got = list(fi.run(frames))
    assert list(model.rows) == rows_plain and sum(rows_plain) == plan.forwards       # the same forwards, batch for batch
    lin = harness_table(fmt, "bt709")
    node = lambda s, j: srcs[s + (j == G)] if j in (0, G) else nodes[s][j - 1]
    want = [srcs[s] if len(taps) == 1 else mix(fmt, [node(s, j) for j, _ in taps], [w for _, w in taps], lin) for _, s, taps in plan.outputs]
    same(got, want, (fmt, "shutter"))
    chroma_same_luma_differs(fmt, got, plain)
    assert fi.light == "bt709" and np.array_equal(fi._lin.cpu().numpy().view(np.uint32), lin)
    same(list(fi.run_chunked(iter(frames), chunk_pairs=2)), got, "run_chunked")


@pytest.mark.parametrize("fmt", FORMATS)
def test_blend_in_light_is_the_oracles_mix_of_the_recursive_nodes(model, fmt):
    srcs, nodes = recursive(model, fmt)
    plan = FrameInterpolator.resample_plan(NF, 24, 60, D, "blend")
    kw = dict(batch_pairs=2, reference_quirks=False, mode="resample", pixel_format=fmt, rate_in=24, rate_out=60, resample_depth=D,
              resample_method="blend")
    frames = clip(fmt)
    model.rows.clear()
    plain = list(FrameInterpolator(model, **kw).run(frames))
    rows_plain = list(model.rows)
    model.rows.clear()
    got = list(FrameInterpolator(model, light="srgb", **kw).run(frames))
    assert list(model.rows) == rows_plain and sum(rows_plain) == plan.forwards
    lin = harness_table(fmt, "srgb")
    node = lambda s, j: srcs[s + (j == G)] if j in (0, G) else nodes[s][j - 1]
    want = []
    for _, s, j0, j1, w in plan.outputs:
        want.append(node(s, j0) if w == 0 else node(s, j1) if w == 256 else mix(fmt, [node(s, j0), node(s, j1)], [256 - w, w], lin))
    assert any(0 < o[-1] < 256 for o in plan.outputs)
    same(got, want, (fmt, "blend"))
    chroma_same_luma_differs(fmt, got, plain)


def test_guards_and_dedup_keep_their_books_on_the_converted_entries(model):
    """the static guard, the agreement guard and dedup's blends with light: the outputs are the light=None run's wherever nothing is mixed,
    the reports (shares, duplicates) are identical"""
    frames = clip("bgr24", n=6, seed=2)
    frames[3] = frames[2].copy()                                       # a duplicate: the gap (2, 4) is blended across
    for f in frames[1:]:
        f[:6] = frames[0][:6]                                          # a static band
    kw = dict(batch_pairs=2, reference_quirks=False, mode="resample", pixel_format="bgr24", rate_in=24, rate_out=60, resample_depth=D,
              resample_method="blend", static_guard=1, dedup_threshold=0.0, ensemble="reverse", agreement=0.05)
    a = FrameInterpolator(model, **kw)
    plain = list(a.run(frames))
    b = FrameInterpolator(model, light="srgb", **kw)
    got = list(b.run(frames))
    assert len(got) == len(plain) and a.duplicates == b.duplicates and len(a.duplicates) == 1
    assert a.static_share == b.static_share and len(a.static_share) > 0 and a.agreement_share == b.agreement_share and len(a.agreement_share) > 0
    assert any(not np.array_equal(g, p) for g, p in zip(got, plain))
    assert all(np.array_equal(g[:5], p[:5]) for g, p in zip(got, plain))          # the held band (its core at radius 1): equal samples mix to themselves


def test_scene_cuts_hold_the_earlier_frame(model):
    rng = np.random.default_rng(8)
    base = synth.synthetic_frames(9, 1, H, W, "natural")[0][0].numpy().transpose(1, 2, 0)
    frames = [(np.clip(np.roll(base, 2 * i, axis=1) * 0.2 + (0.15 if i <= 2 else 0.70) + rng.normal(0, 0.01, (H, W, 3)), 0, 1) * 255).astype(np.uint8)
              for i in range(NF)]
    cut = (2, 3)
    sig = scene_oracle.signature(np.stack(frames), "bgr")
    scores = {(i, i + 1): int(scene_oracle.score(sig[i], sig[i + 1], H, W)) for i in range(NF - 1)}
    rest = max(v for k, v in scores.items() if k != cut)
    fraction = (scores[cut] + rest) / 2 / (4080 * scene_oracle.cells(H, W))
    assert scores[cut] > 4 * rest > 0
    for ratio, shutter in ((1, 360), (2, 180)):                        # at 360 degrees the window of the flagged pair reaches the next shot
        kw = dict(batch_pairs=2, reference_quirks=False, mode="resample", rate_in=15, rate_out=15 * ratio, resample_depth=D, shutter=shutter)
        fi = FrameInterpolator(model, light="srgb", scene_threshold=fraction, **kw)
        got = list(fi.run(frames))
        free = list(FrameInterpolator(model, light="srgb", **kw).run(frames))
        assert all(np.array_equal(got[cut[0] * ratio + r], frames[cut[0]]) for r in range(ratio))
        assert not np.array_equal(free[cut[0] * ratio], frames[cut[0]])
        same([g for k, g in enumerate(got) if k // ratio != cut[0]], [g for k, g in enumerate(free) if k // ratio != cut[0]], "the other pairs")
        assert fi.scene_cuts == [(*cut, scores[cut])]


def test_command_line_light(model, tmp_path, capsys):
    frames = clip("yuv420p8")
    src, dst = tmp_path / "in15.y4m", tmp_path / "out15.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 15, 1)) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2",
                   "--chunk-pairs", "2", "--output-fps", "15", "--shutter", "180", "--resample-depth", str(D), "--light", "bt709"])
    assert rc == 0, capsys.readouterr().err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    kw = dict(batch_pairs=2, reference_quirks=False, mode="resample", pixel_format="yuv420p8", rate_in=15, rate_out=15, resample_depth=D, shutter=180)
    same(got, list(FrameInterpolator(model, light="bt709", **kw).run(frames)), "cli")   # the fixture's model is the command line's
    assert any(not np.array_equal(g, p) for g, p in zip(got, FrameInterpolator(model, **kw).run(frames)))
