"""Motion blur from a shutter angle on the GPU: emavfi_accumulate_frames against the numpy restatement of the shutter definition
(tests/shutter_oracle.py) and against emavfi_resample_frames' blend, and the harness's ``shutter=`` against the oracle's accumulation of the
frames mode "recursive" yields.  Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import resample_oracle
import scene_oracle
import shutter_oracle as oracle

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
NODES = lib.RESAMPLE_NODES
N_SRCS, N_NODES = 3, 31
TOP = (1985,) * 32 + (2015,)                                         # 33 weights that sum to 65535


def up(v, m):
    return (v + m - 1) // m * m


def pool(data, stride):
    """frames `data` [n, fb] on the device, `stride` bytes apart, in an allocation of exactly (n - 1) stride + fb bytes"""
    n, fb = data.shape
    raw = torch.full(((n - 1) * stride + fb,), 0x3C, dtype=torch.uint8, device="cuda")
    view = raw.as_strided((n, fb), (stride, 1))
    view.copy_(torch.from_numpy(data))
    return view


def table(flags_on):
    """9 entries, so two launches: n = 1, 2, 3 and 33, both pools, the largest weight sum, an entry whose flag is clear and one whose flag is
    set, and the (256 - w, w) of a blend in the second launch"""
    every = (0, *(NODES | i for i in range(N_NODES)), 1)              # 33 taps: source 0, every node, source 1
    return [((1,), (7,), 0, 0), ((NODES | 0, NODES | 1), (1, 1), 0, 0), ((0, NODES | 0, NODES | 1), (1, 2, 1), 0, 0), (every, TOP, 0, 0),
            ((NODES | 3, NODES | 4, NODES | 5), (5, 6, 1), 1 if flags_on else 0, 1), ((2, NODES | 30), (65534, 1), 0, 0),
            (every, (1,) * 33, 2 if flags_on else 0, 2),
            ((NODES | 7,), (1,), 0, 0), ((1, 2), (192, 64), 0, 0)]


@pytest.mark.parametrize("sb,depth,shift", [(1, 8, 0), (2, 10, 6), (2, 10, 0), (2, 16, 0)])
@pytest.mark.parametrize("samples", [9 * 11 * 3, 24 * 40 * 3])
def test_entry_is_the_oracle_byte_for_byte(samples, sb, depth, shift):
    """frames of 9 x 11 x 3 samples (297 bytes, 594 as words: no multiple of 16, so dense frames after the first are misaligned and go by bytes
    or words) and of 24 x 40 x 3 (2880 / 5760 bytes: aligned); dense pools, a stride that breaks the alignment and the next multiple of 16
    (16-byte accesses and a byte / word tail).  The first samples of every frame are all ones, the next all zeros: with the weights that
    sum to 65535 the largest intermediate of the definition, 65535 * 65535 + 32767, occurs at depth 16."""
    fb = samples * sb
    rng = np.random.default_rng(samples + 16 * depth + shift)
    srcs = rng.integers(0, 256, (N_SRCS, fb), dtype=np.uint8)        # at 2 bytes per sample: whole words, bits outside the sample included
    nodes = rng.integers(0, 256, (N_NODES, fb), dtype=np.uint8)
    for p in (srcs, nodes):
        p[:, :32 * sb], p[:, 32 * sb:64 * sb] = 255, 0
    for stride, fl in ((fb, None), (fb + 6, (0, 1)), (up(fb, 16), (0, 1))):
        tab = table(fl is not None)
        d_s, d_n = pool(srcs, stride), pool(nodes, stride + (16 if stride % 16 == 0 else 2))
        raw = torch.full(((len(tab) - 1) * stride + fb + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        dst = raw.as_strided((len(tab), fb), (stride, 1))
        want = np.full(raw.shape, POISON, np.uint8)
        out = oracle.accumulate(srcs, nodes, tab, fl, sb, depth, shift)
        for k in range(len(tab)):
            want[k * stride:k * stride + fb] = out[k]
        flags = torch.tensor(fl, dtype=torch.int32, device="cuda") if fl is not None else None
        assert lib.accumulate_frames(dst, d_s, d_n, tab, flags, sb, depth, shift).data_ptr() == dst.data_ptr()
        got = raw.cpu().numpy()
        assert np.array_equal(got, want), ("frames / stride gaps / the bytes after the last frame", fb, stride, fl, depth, shift,
                                           [k for k in range(len(tab)) if not np.array_equal(got[k * stride:k * stride + fb], out[k])])
        assert np.array_equal(d_s.cpu().numpy(), srcs) and np.array_equal(d_n.cpu().numpy(), nodes)
        # what the table is meant to reach
        full = (255 if sb == 1 else ((1 << depth) - 1) << shift)
        top = np.frombuffer(out[3].tobytes(), "<u2" if sb == 2 else np.uint8)
        assert (top[:32] == full).all() and (top[32:64] == 0).all()
        if fl is not None:
            assert np.array_equal(out[6], srcs[2]) and not np.array_equal(out[4], srcs[1])      # the set flag holds, the clear one does not


@pytest.mark.parametrize("sb,depth,shift", [(1, 8, 0), (2, 10, 6)])
def test_weights_256_minus_w_and_w_are_the_resample_blend(sb, depth, shift):
    rng = np.random.default_rng(11)
    fb = 2880 * sb
    srcs = torch.from_numpy(rng.integers(0, 256, (2, fb), dtype=np.uint8)).cuda()
    ws = (1, 64, 128, 255)
    a, b = (torch.full((len(ws), fb), POISON, dtype=torch.uint8, device="cuda") for _ in range(2))
    lib.accumulate_frames(a, srcs, None, [((0, 1), (256 - w, w), 0, 0) for w in ws], None, sb, depth, shift)
    lib.resample_frames(b, srcs, None, [(0, 1, w, 0, 0) for w in ws], None, sb, depth, shift)
    assert torch.equal(a, b)
    want = [resample_oracle.blend(*srcs.cpu().numpy(), w, sb, depth, shift) for w in ws]
    assert np.array_equal(a.cpu().numpy(), np.stack(want))


@pytest.mark.parametrize("n,stride", [(2, (1 << 32) + 4096), (3, (1 << 31) + 64)])
def test_frame_strides_beyond_the_lines(n, stride):
    """dst, srcs and nodes pools of dense 34 x 70 x 3 frames whose frame strides pass 2^31 and 2^32: a frame address computed in 32 bits
    would land in another frame or in the gap.  Means over both pools and a held entry, byte for byte the oracle's; every byte between the
    frames unchanged."""
    fb, last = 34 * 70 * 3, n - 1
    rng = np.random.default_rng(n)
    srcs, nodes = (rng.integers(0, 256, (n, fb), dtype=np.uint8) for _ in range(2))
    bufs = [torch.full(((n - 1) * stride + fb,), POISON, dtype=torch.uint8, device="cuda") for _ in range(3)]
    dst, d_s, d_n = (b.as_strided((n, fb), (stride, 1)) for b in bufs)
    d_s.copy_(torch.from_numpy(srcs))
    d_n.copy_(torch.from_numpy(nodes))
    tab = [((0, NODES | last, last), (1, 2, 1), 0, 0), ((NODES | 0, last), (3, 1), 1, last), ((last, NODES | last), (1, 1), 0, 0)][:n]
    lib.accumulate_frames(dst, d_s, d_n, tab, torch.tensor([1], dtype=torch.int32, device="cuda"))
    want = oracle.accumulate(srcs, nodes, tab, [1])
    assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(want[1], srcs[last])
    assert np.array_equal(d_s.cpu().numpy(), srcs) and np.array_equal(d_n.cpu().numpy(), nodes)
    for b in bufs:
        assert all(bool((b[k * stride + fb:(k + 1) * stride] == POISON).all()) for k in range(n - 1))


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
            frames = clip(fmt, **({"h": 2 * H, "w": 2 * W} if "scale" in kw else {}))
        out = list(FrameInterpolator(model, G - 1, 1, batch_pairs=2, reference_quirks=False, mode="recursive", pixel_format=fmt, **kw).run(frames))
        assert len(out) == (len(frames) - 1) * G + 1
        srcs = [out[s * G + G - 1] for s in range(len(frames) - 1)] + [out[-1]]
        _recursive[k] = (srcs, [out[s * G:s * G + G - 1] for s in range(len(frames) - 1)])
    return _recursive[k]


def blurred(model, fmt, ratio, shutter, **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, mode="resample", pixel_format=fmt, rate_in=15, rate_out=15 * ratio,
                             resample_depth=D, shutter=shutter, **kw)


def expected(fmt, plan, srcs, nodes, held=()):
    """the plan's outputs accumulated by the oracle from mode "recursive"'s frames"""
    sb, depth, shift = lib.resample_sample_format(fmt)
    node = lambda s, j: srcs[s + (j == G)] if j in (0, G) else nodes[s][j - 1]
    out = []
    for k, s, taps in plan.outputs:
        if s in held or len(taps) == 1:
            out.append(srcs[s])
        else:
            fr = [node(s, j) for j, _ in taps]
            out.append(oracle.mean([f.view(np.uint8) for f in fr], [w for _, w in taps], sb, depth, shift).view(fr[0].dtype))
    return out


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k)


@pytest.mark.parametrize("ratio,shutter", [(1, 180), (1, 360), (2, 180), (2, 360)])
def test_bgr24_is_the_oracles_accumulation_of_the_recursive_nodes(model, ratio, shutter):
    srcs, nodes = recursive(model, "bgr24")
    plan = FrameInterpolator.shutter_plan(NF, 15, 15 * ratio, D, shutter)
    fi = blurred(model, "bgr24", ratio, shutter)
    model.rows.clear()
    got = list(fi.run(clip("bgr24")))
    rows = list(model.rows)
    same(got, expected("bgr24", plan, srcs, nodes), (ratio, shutter))
    assert len(got) == fi.count_outputs(NF) == (NF - 1) * ratio + 1 and np.array_equal(got[-1], srcs[-1])
    assert any(not np.array_equal(g, srcs[k // ratio]) for k, g in enumerate(got[:-1]))
    # the forwards issued are the plan's: 180 degrees at ratio 1 taps nodes 0 .. 2 and never computes node 3
    assert sum(rows) == plan.forwards == (NF - 1) * {(1, 180): 2, (1, 360): 3, (2, 180): 3, (2, 360): 3}[ratio, shutter]
    assert len(rows) <= D * 2                                          # level by level over the pairs of a batch


@pytest.mark.parametrize("fmt", FORMATS[1:])
def test_every_format_goes_through_the_same_arithmetic(model, fmt):
    srcs, nodes = recursive(model, fmt)
    plan = FrameInterpolator.shutter_plan(NF, 15, 15, D, 180)
    same(list(blurred(model, fmt, 1, 180).run(clip(fmt))), expected(fmt, plan, srcs, nodes), fmt)


def test_scale_resizes_sources_and_nodes_alike(model):
    srcs, nodes = recursive(model, "bgr24", scale=0.5)
    assert srcs[0].shape == (H, W, 3)
    plan = FrameInterpolator.shutter_plan(NF, 15, 15, D, 360)
    same(list(blurred(model, "bgr24", 1, 360, scale=0.5).run(clip("bgr24", h=2 * H, w=2 * W))), expected("bgr24", plan, srcs, nodes), "scale=0.5")


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
    assert scores[cut] > 4 * rest > 0 and rest < lib.scene_threshold_units(fraction, H, W) <= scores[cut]
    srcs, nodes = recursive(model, "bgr24", frames, key="cut")
    for ratio, shutter in ((1, 360), (2, 180)):                        # at 360 degrees the window of the flagged pair reaches the next shot
        plan = FrameInterpolator.shutter_plan(NF, 15, 15 * ratio, D, shutter)
        fi = blurred(model, "bgr24", ratio, shutter, scene_threshold=fraction)
        got = list(fi.run(frames))
        same(got, expected("bgr24", plan, srcs, nodes, held={cut[0]}), ("cut", ratio, shutter))
        assert all(np.array_equal(got[cut[0] * ratio + r], frames[cut[0]]) for r in range(ratio))
        assert not np.array_equal(expected("bgr24", plan, srcs, nodes)[cut[0] * ratio], frames[cut[0]])
        assert fi.scene_cuts == [(*cut, scores[cut])]
        same(list(fi.run_chunked(iter(frames), chunk_pairs=2)), got, "run_chunked with cuts")


def test_static_guard_accumulates_the_guarded_nodes(model):
    frames = clip("bgr24", seed=2)
    for f in frames[1:]:                                               # a static band: the guard has something to hold
        f[:6] = frames[0][:6]
    srcs, nodes = recursive(model, "bgr24", frames, key="static", static_guard=1)
    plain = recursive(model, "bgr24", frames, key="static")[1]
    assert any(not np.array_equal(a, b) for a, b in zip(nodes[0], plain[0]))
    plan = FrameInterpolator.shutter_plan(NF, 15, 15, D, 360)
    fi = blurred(model, "bgr24", 1, 360, static_guard=1)
    same(list(fi.run(frames)), expected("bgr24", plan, srcs, nodes), "static_guard=1")
    assert len(fi.static_share) == NF - 1 and all(0 < s < 1 for s in fi.static_share)


def test_chunks_and_ranks_concatenate_to_the_whole(model):
    frames = clip("bgr24", n=6, seed=3)
    whole = list(blurred(model, "bgr24", 2, 360).run(frames))
    assert len(whole) == 11
    same(list(blurred(model, "bgr24", 2, 360).run_chunked(iter(frames), chunk_pairs=2)), whole, "run_chunked(chunk_pairs=2)")
    same(list(blurred(model, "bgr24", 2, 360).run_chunked(iter(frames[:5]), chunk_pairs=2)), whole[:8] + [frames[4]], "a clip that ends on a chunk boundary")
    fi = blurred(model, "bgr24", 2, 360)
    parts = [list(fi.run(frames, rank=rank, world=2)) for rank in range(2)]
    assert [len(p) for p in parts] == [6, 5]
    same(parts[0] + parts[1], whole, "ranks 0 and 1 of world 2")
    with pytest.raises(ValueError, match="evaluate\\(\\) with a shutter"):
        fi.evaluate(frames)


def test_command_line_shutter(model, tmp_path, capsys):
    frames = clip("yuv420p8")
    src, dst = tmp_path / "in15.y4m", tmp_path / "out15.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 15, 1)) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2",
                   "--chunk-pairs", "2", "--output-fps", "15", "--shutter", "180", "--resample-depth", str(D)])
    assert rc == 0, capsys.readouterr().err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
        assert (r.header.fps_num, r.header.fps_den, r.header.width, r.header.height) == (15, 1, W, H)
    same(got, list(blurred(model, "yuv420p8", 1, 180).run(frames)), "cli")      # the fixture's model is the command line's: seed 0, 8 channels, fp32
    assert not np.array_equal(got[0], frames[0])
