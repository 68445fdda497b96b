"""Frame-rate conversion on the GPU: emavfi_resample_frames against the numpy restatement of the temporal resample definition
(tests/resample_oracle.py) and the harness's mode "resample" against the frames mode "recursive" yields.  Every comparison is bit-exact."""
import itertools

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, FrameInterpolator, cli, lib, synth, y4m
import resample_oracle as oracle
import scene_oracle

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
CAP = lib.RESAMPLE_LAUNCH_CAP
WEIGHTS = (0, 1, 127, 128, 255, 256)
N_SRCS, N_NODES = 3, 4


def up(v, m):
    return (v + m - 1) // m * m


def pool(data, stride):
    """frames `data` [n, fb] on the device, `stride` bytes apart, in an allocation of exactly (n - 1) stride + fb bytes"""
    n, fb = data.shape
    raw = torch.full(((n - 1) * stride + fb,), 0x3C, dtype=torch.uint8, device="cuda")
    view = raw.as_strided((n, fb), (stride, 1))
    view.copy_(torch.from_numpy(data))
    return view


def table_for(n_out, flags_on):
    """every weight, both pools on either side, both frames of a blend from one pool and from two; with flags: every third entry may be held"""
    t = []
    for k in range(n_out):
        a = (k % N_SRCS) if k % 2 else lib.RESAMPLE_NODES | (k % N_NODES)
        b = lib.RESAMPLE_NODES | ((k + 1) % N_NODES) if k % 3 else (k + 1) % N_SRCS
        t.append((a, b, WEIGHTS[(k + k // 6) % 6], (k % 5) + 1 if (flags_on and k % 3 == 0) else 0, (k + 2) % N_SRCS))
    return t


def check_entry(fb, strides, n_outs, sample_bytes=1, depth=8, shift=0, seed=0):
    rng = np.random.default_rng(seed + fb)
    srcs = rng.integers(0, 256, (N_SRCS, fb), dtype=np.uint8)         # at 2 bytes per sample: whole words, bits outside the sample included
    nodes = rng.integers(0, 256, (N_NODES, fb), dtype=np.uint8)
    for stride, n_out, fl in itertools.product(strides, n_outs, (None, (0, 0, 0, 0, 0), (1, 0, 7, 0, -1))):
        d_s, d_n = pool(srcs, stride), pool(nodes, stride + (16 if stride % 16 == 0 else 2))
        raw = torch.full(((n_out - 1) * stride + fb + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        dst = raw.as_strided((n_out, fb), (stride, 1))
        table = table_for(n_out, fl is not None)
        want = np.full(raw.shape, POISON, np.uint8)
        out = oracle.assemble(srcs, nodes, table, fl, sample_bytes, depth, shift)
        for k in range(n_out):
            want[k * stride:k * stride + fb] = out[k]
        flags = torch.tensor(fl, dtype=torch.int32, device="cuda") if fl is not None else None
        assert lib.resample_frames(dst, d_s, d_n, table, flags, sample_bytes, depth, shift).data_ptr() == dst.data_ptr()
        assert np.array_equal(raw.cpu().numpy(), want), ("frames / stride gaps / the bytes after the last frame", fb, stride, n_out, fl, depth, shift)
        assert np.array_equal(d_s.cpu().numpy(), srcs) and np.array_equal(d_n.cpu().numpy(), nodes)


@pytest.mark.parametrize("fb", [1, 15, 16, 17, 48, 4099])
def test_entry_is_the_oracle_byte_for_byte(fb):
    """dense frames, an odd stride (byte accesses throughout) and the next multiple of 16 (16-byte accesses and a byte tail); one launch, and
    one entry more than a launch holds"""
    check_entry(fb, (fb, fb + 5, up(fb, 16)), (1, 7, CAP + 1))


@pytest.mark.parametrize("depth,shift", [(10, 0), (10, 6), (12, 0), (12, 4), (16, 0)])
def test_entry_blends_the_samples_of_16_bit_words(depth, shift):
    """4098 bytes: 256 16-byte units and one word of tail; a stride has to be even here, so the scalar path's is frame_bytes + 6"""
    check_entry(4098, (4098, 4098 + 6, up(4098, 16)), (1, 7, CAP + 1), 2, depth, shift, seed=depth * 16 + shift)


def test_entry_properties_and_single_pool():
    rng = np.random.default_rng(3)
    for fb, off in ((4099, 0), (4099, 1), (777, 16)):
        a, b = (rng.integers(0, 256, (1, fb), dtype=np.uint8) for _ in range(2))
        raw = torch.zeros(2 * fb + 64, dtype=torch.uint8, device="cuda")
        srcs = raw[off:off + 2 * fb].view(2, fb)
        srcs.copy_(torch.from_numpy(np.concatenate([a, b])))
        dst = torch.full((8, fb), POISON, dtype=torch.uint8, device="cuda")
        # no node pool at all; w = 128 is the rounded mean; a frame blended with itself stays what it is at every weight
        lib.resample_frames(dst, srcs, None, [(0, 1, 128, 0, 0), (1, 0, 128, 0, 0)] + [(1, 1, w, 0, 0) for w in WEIGHTS])
        got = dst.cpu().numpy()
        mean = ((a[0].astype(int) + b[0] + 1) >> 1).astype(np.uint8)
        assert np.array_equal(got[0], mean) and np.array_equal(got[1], mean) and all(np.array_equal(got[k], b[0]) for k in range(2, 8))
    # pinned destination: the kernel writes host memory in place
    d = torch.zeros(2, 23, 37, 3, dtype=torch.uint8).pin_memory()
    s = torch.from_numpy(rng.integers(0, 256, (2, 23, 37, 3), dtype=np.uint8)).cuda()
    lib.resample_frames(d, s, None, [(1, 0, 0, 0, 0), (0, 1, 77, 0, 0)])
    torch.cuda.synchronize()
    assert torch.equal(d[0], s[1].cpu()) and np.array_equal(d[1].numpy(), oracle.blend(s[0].cpu().numpy(), s[1].cpu().numpy(), 77))


# ---------------------------------------------------------------- the harness
H, W, NF, D, G = 24, 40, 6, 3, 8
FORMATS = ["bgr24", "nv12", "p010", "yuv420p10"]


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
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


def recursive(model, fmt, factor, frames_key="clip", **kw):
    """(sources, nodes): sources[s] and nodes[s][j - 1] of mode "recursive" at `factor` on the shared clip - computed once per configuration"""
    key = (fmt, factor, frames_key, tuple(sorted(kw.items())))
    if key not in _recursive:
        frames = clip(fmt, **({"h": 2 * H, "w": 2 * W} if "scale" in kw else {}))
        out = list(FrameInterpolator(model, factor, 1, batch_pairs=2, reference_quirks=False, mode="recursive", pixel_format=fmt, **kw).run(frames))
        assert len(out) == (NF - 1) * (factor + 1) + 1
        srcs = [out[s * (factor + 1) + factor] for s in range(NF - 1)] + [out[-1]]
        _recursive[key] = (srcs, [out[s * (factor + 1):s * (factor + 1) + factor] for s in range(NF - 1)])
    return _recursive[key]


def resampler(model, fmt, rate_in, rate_out, method="nearest", **kw):
    return FrameInterpolator(model, batch_pairs=2, reference_quirks=False, mode="resample", pixel_format=fmt, rate_in=rate_in, rate_out=rate_out,
                             resample_depth=D, resample_method=method, **kw)


def expected(fmt, plan, srcs, nodes, factor=G - 1, held=()):
    """the plan's outputs assembled by the oracle from mode "recursive"'s frames; node j of depth D is prediction j (factor + 1) / G of `factor`"""
    sb, depth, shift = lib.resample_sample_format(fmt)

    def node(s, j):
        if j in (0, G):
            return srcs[s + (j == G)]
        assert j * (factor + 1) % G == 0
        return nodes[s][j * (factor + 1) // G - 1]

    out = []
    for k, s, j0, j1, w in plan.outputs:
        if s in held and k * plan.P - s * plan.Q > 0:
            out.append(srcs[s])
        elif w == 0:
            out.append(node(s, j0))
        else:
            a, b = node(s, j0), node(s, j1)
            out.append(oracle.blend(a.view(np.uint8), b.view(np.uint8), w, sb, depth, shift).view(a.dtype))
    return out


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_ratios_2_and_4_are_the_recursive_stream_in_temporal_order(model, fmt):
    for ratio, factor in ((2, 1), (4, 3)):
        srcs, nodes = recursive(model, fmt, factor)
        fi = resampler(model, fmt, 15, 15 * ratio)
        got = list(fi.run(clip(fmt)))
        want = [f for s in range(NF - 1) for f in [srcs[s], *nodes[s]]] + [srcs[-1]]
        same(got, want, (fmt, ratio))
        assert len(got) == fi.count_outputs(NF) == (NF - 1) * ratio + 1


@pytest.mark.parametrize("fmt,method", [("bgr24", "nearest"), ("bgr24", "blend"), ("nv12", "blend"), ("p010", "blend"), ("yuv420p10", "blend")])
def test_24_to_60_is_the_oracles_selection_or_blend_of_the_full_tree(model, fmt, method):
    """also pins that the nodes of a pruned tree are the nodes of the full one"""
    srcs, nodes = recursive(model, fmt, G - 1)
    plan = FrameInterpolator.resample_plan(NF, 24, 60, D, method)
    assert len(plan.outputs) == 13 and plan.outputs[10][1:] == (4, 0, 0, 0) and plan.outputs[-1][:2] == (12, 4)   # k = 10 is not the last output; none falls on frame 5
    fi = resampler(model, fmt, 24, 60, method)
    same(list(fi.run(clip(fmt))), expected(fmt, plan, srcs, nodes), (fmt, method))
    if method == "blend":
        assert any(0 < o[4] < 256 for o in plan.outputs)


@pytest.mark.parametrize("rates,method", [((24, 60), "nearest"), ((24, 60), "blend"), ((30, 60), "blend"), ((30, 30), "nearest")])
def test_the_forwards_issued_are_the_plans(model, rates, method):
    rows, inner = [], model.forward

    def counting(x1, x2, *a, **kw):
        rows.append(x1.shape[0])
        return inner(x1, x2, *a, **kw)

    model.forward = counting
    try:
        got = list(resampler(model, "bgr24", *rates, method).run(clip("bgr24")))
    finally:
        del model.forward
    plan = FrameInterpolator.resample_plan(NF, *rates, D, method)
    assert sum(rows) == plan.forwards == {((24, 60), "nearest"): 20, ((24, 60), "blend"): 25, ((30, 60), "blend"): 5, ((30, 30), "nearest"): 0}[rates, method]
    assert len(got) == len(plan.outputs)
    # level by level over the pairs of a batch: at most `depth` calls per batch of two pairs
    assert len(rows) <= D * 3


@pytest.mark.parametrize("method", ["nearest", "blend"])
def test_chunks_and_ranks_concatenate_to_the_whole(model, method):
    frames = clip("bgr24", n=7)
    whole = list(resampler(model, "bgr24", 24, 60, method).run(frames))
    assert len(whole) == 16
    same(list(resampler(model, "bgr24", 24, 60, method).run_chunked(iter(frames), chunk_pairs=2)), whole, "run_chunked(chunk_pairs=2)")
    same(list(resampler(model, "bgr24", 24, 60, method).run_chunked(iter(frames[:5]), chunk_pairs=2)),
         list(resampler(model, "bgr24", 24, 60, method).run(frames[:5])), "a clip that ends on a chunk boundary")
    fi = resampler(model, "bgr24", 24, 60, method)
    parts = [list(fi.run(frames, rank=rank, world=2)) for rank in range(2)]
    assert [len(p) for p in parts] == [8, 8]
    same(parts[0] + parts[1], whole, "ranks 0 and 1 of world 2")


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
    for method in ("nearest", "blend"):
        plain = list(resampler(model, "bgr24", 24, 60, method).run(frames))
        fi = resampler(model, "bgr24", 24, 60, method, scene_threshold=fraction)
        got = list(fi.run(frames))
        plan = FrameInterpolator.resample_plan(NF, 24, 60, D, method)
        assert len(got) == len(plain) == len(plan.outputs)
        held = 0
        for (k, s, *_), g, p in zip(plan.outputs, got, plain):
            if s == cut[0] and k * plan.P - s * plan.Q > 0:
                assert np.array_equal(g, frames[s]) and not np.array_equal(g, p), ("held output", k)
                held += 1
            else:
                assert np.array_equal(g, p), ("untouched output", k)
        assert held == 2
        assert fi.scene_cuts == [(*cut, scores[cut])] and fi.scene_scores == [(i, i + 1, scores[(i, i + 1)]) for i in range(NF - 1)]
        # chunks report the same cuts with global indices
        same(list(fi.run_chunked(iter(frames), chunk_pairs=2)), got, "run_chunked with cuts")
        assert fi.scene_cuts == [(*cut, scores[cut])]


def test_scale_resizes_sources_and_nodes_alike(model):
    srcs, nodes = recursive(model, "bgr24", G - 1, scale=0.5)
    assert srcs[0].shape == (H, W, 3)
    for method in ("nearest", "blend"):
        plan = FrameInterpolator.resample_plan(NF, 24, 60, D, method)
        got = list(resampler(model, "bgr24", 24, 60, method, scale=0.5).run(clip("bgr24", h=2 * H, w=2 * W)))
        same(got, expected("bgr24", plan, srcs, nodes), ("scale=0.5", method))


def test_command_line_output_fps(model, tmp_path, capsys):
    frames = clip("yuv420p8")
    src, dst = tmp_path / "in24.y4m", tmp_path / "out60.y4m"
    with y4m.Y4MWriter(str(src), y4m.Y4MHeader(W, H, 24, 1)) as w:
        for f in frames:
            w.write(f)
    rc = cli.main([str(src), str(dst), "--synthetic-weights", "0", "--mid-channels", "8", "--dtype", "fp32", "--batch-pairs", "2",
                   "--chunk-pairs", "2", "--output-fps", "60"])
    assert rc == 0, capsys.readouterr().err
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
        assert (r.header.fps_num, r.header.fps_den, r.header.width, r.header.height) == (60, 1, W, H)
    assert len(got) == ((NF - 1) * 5) // 2 + 1 == 13
    srcs, nodes = recursive(model, "yuv420p8", G - 1)             # the fixture's model is the command line's: seed 0, 8 channels, fp32
    same(got, expected("yuv420p8", FrameInterpolator.resample_plan(NF, 24, 60, D, "nearest"), srcs, nodes), "cli")
