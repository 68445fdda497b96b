#!/usr/bin/env python3
"""What do planar 4:2:0 frames and the chunked run cost (round 15)?
  (1) At 9 frames x 1280 x 720, resident in HBM, in one process, interleaved a-b-a-b: the kernel times of emavfi_preprocess_yuv420p /
      _postprocess_yuv420p at depth 8 beside emavfi_preprocess_nv12 / _postprocess_nv12 and at depth 10 beside emavfi_preprocess_p010 /
      _postprocess_p010 - the same samples, the same bytes moved (13.5 B/px at depth 8, 15 above), only the chroma planes apart instead
      of interleaved.  HIP events, warm-up, the median of N >= 20 and the spread (min .. max, and the shift of the median between the
      first and the second half of the samples).  All eight are instantiations of one kernel pair (misc_kernels.hip, preprocess_yuv420_kernel).  There is no
      pass / fail time; the ratios are recorded, and a planar kernel slower than its counterpart by more than that counterpart's own
      spread is flagged: the explanation is written by hand under the file's "## Notes" heading, which the tool keeps when it rewrites
      the file.  --ab-lib PATH times the same eight entries of a second build of the library (`make -C video-frame-interpolation_amd/csrc
      TAG=_other`, in a checkout of another commit or with EXTRA flags) in the same process and the same interleaved loop, on the same
      buffers, and asserts that both builds write identical frames; both builds are then called through ctypes directly, without lib's wrappers.
  (2) run_chunked beside run on 65 frames of 1280 x 720 (64 pairs), batch_pairs 8, bf16, pixel_format="yuv420p8", alternating: what
      cutting the stream into chunks of --chunk-pairs pairs (bounded memory) costs in rate.
Writes a markdown note (default profiles/r15_yuv420p_y4m.md); --vgprs puts the code object's register counts into it."""
import argparse, os, platform, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, formats, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_yuv420p_y4m.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--chunk-pairs", type=int, nargs="+", default=[16, 64])
ap.add_argument("--skip-harness", action="store_true")
ap.add_argument("--ab-lib", default="", help="a second build of libemavfi.so whose eight entries are timed beside the loaded one's")
ap.add_argument("--vgprs", default="", help="text for the note: VGPR counts of the planar kernels read from the gfx950 code object")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
B, H, W, NFRAMES = 9, 720, 1280, 65
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def encode_host(bgr):
    """a plain float BT.601 limited-range encode on the host - content for the benchmark only (the kernels' own definition is integer)"""
    b, g, r = (bgr[..., c].astype(np.float32) for c in range(3))
    y = np.clip(16 + 0.2568 * r + 0.5041 * g + 0.0979 * b + 0.5, 0, 255).astype(np.uint8)
    m = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
    u = np.clip(128 - 0.1482 * m(r) - 0.2910 * m(g) + 0.4392 * m(b) + 0.5, 0, 255).astype(np.uint8)
    v = np.clip(128 + 0.4392 * m(r) - 0.3678 * m(g) - 0.0714 * m(b) + 0.5, 0, 255).astype(np.uint8)
    return y, u, v


def halves(t):
    return statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])


f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
yuv = [encode_host(np.roll(f1[0], 3 * i, axis=1)) for i in range(NFRAMES)]
planar8 = [np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(H * 3 // 2, W) for y, u, v in yuv]
nv12 = [np.concatenate([y, np.stack([u, v], axis=-1).reshape(H // 2, W)]) for y, u, v in yuv]
wide = lambda f: (f.astype(np.uint16) << 2 | f >> 6)                  # byte -> 10-bit sample (bit replication)
planar10 = [wide(f) for f in planar8[:B]]                            # the sample in the word's low bits
p010 = [wide(f) << 6 for f in nv12[:B]]                              # ... in its top bits

say("# Planar 4:2:0 frames in and out, and the chunked run: kernel times and harness rate (tools/bench_yuv420p.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
if args.vgprs:
    say()
    say(f"gfx950 code object, planar kernels: {args.vgprs}.")
say()


def planes3(buf, words):
    """the harness's own views (emavfi.formats) of planar frames held as bytes or as words"""
    return formats.FORMATS["yuv420p10" if words else "yuv420p8"].planes(buf.view(torch.uint8))


def planes2(buf):
    return formats.FORMATS["p010" if buf.element_size() == 2 else "nv12"].planes(buf.view(torch.uint8))


# ---------------------------------------------------------------- (1) kernels, resident frames
d_pl8, d_nv = torch.from_numpy(np.stack(planar8[:B])).to(dev), torch.from_numpy(np.stack(nv12[:B])).to(dev)
d_pl10, d_p010 = torch.from_numpy(np.stack(planar10).view(np.int16)).to(dev), torch.from_numpy(np.stack(p010).view(np.int16)).to(dev)
x = torch.empty(B, 3, H, W, device=dev)
pred = torch.rand(B, 3, H, W, device=dev)
o_pl8, o_nv = torch.empty_like(d_pl8), torch.empty_like(d_nv)
o_pl10, o_p010 = torch.empty_like(d_pl10), torch.empty_like(d_p010)
kernels = {
    "preprocess_nv12": (lambda: lib.preprocess_nv12(*planes2(d_nv), out=x), 13.5),
    "preprocess_yuv420p d=8": (lambda: lib.preprocess_yuv420p(*planes3(d_pl8, False), 8, out=x), 13.5),
    "preprocess_p010": (lambda: lib.preprocess_p010(*planes2(d_p010), 10, out=x), 15.0),
    "preprocess_yuv420p d=10": (lambda: lib.preprocess_yuv420p(*planes3(d_pl10, True), 10, out=x), 15.0),
    "postprocess_nv12": (lambda: lib.postprocess_nv12(pred, denormalize=True, out=planes2(o_nv)), 13.5),
    "postprocess_yuv420p d=8": (lambda: lib.postprocess_yuv420p(pred, 8, denormalize=True, out=planes3(o_pl8, False)), 13.5),
    "postprocess_p010": (lambda: lib.postprocess_p010(pred, 10, denormalize=True, out=planes2(o_p010)), 15.0),
    "postprocess_yuv420p d=10": (lambda: lib.postprocess_yuv420p(pred, 10, denormalize=True, out=planes3(o_pl10, True)), 15.0),
}
if args.ab_lib:
    import ctypes
    AB = ctypes.CDLL(os.path.abspath(args.ab_lib))
    for sym in ("emavfi_preprocess_nv12", "emavfi_postprocess_nv12", "emavfi_preprocess_p010", "emavfi_postprocess_p010",
                "emavfi_preprocess_yuv420p", "emavfi_postprocess_yuv420p"):
        getattr(AB, sym).restype, getattr(AB, sym).argtypes = lib._PROTOTYPES[sym]
    m32, s32 = lib._stats(lib.IMAGENET_MEAN, lib.IMAGENET_STD, 3)
    m64, s64 = lib._stats(lib.IMAGENET_MEAN, lib.IMAGENET_STD, 3, ctypes.c_double)

    def semi_args(buf, depth):
        """(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride) and the depth argument, if the entry takes one"""
        y, uv = planes2(buf)
        _, _, _, yp, ybs, uvp, uvbs = (lib._nv12_planes if depth == 8 else lib._p010_planes)(y, uv, "ab")
        return (y.data_ptr(), yp, ybs, uv.data_ptr(), uvp, uvbs), (() if depth == 8 else (depth,))

    def ab_pre(L, buf, depth, planar):
        """a call of the build's preprocess entry on `buf`, arguments worked out once"""
        if planar:
            fn, args = L.emavfi_preprocess_yuv420p, (*lib._yuv420p_planes(*planes3(buf, depth > 8), depth, "ab")[3], x.data_ptr(), B, H, W, depth)
        else:
            pl, d = semi_args(buf, depth)
            fn, args = (L.emavfi_preprocess_nv12 if depth == 8 else L.emavfi_preprocess_p010), (*pl, x.data_ptr(), B, H, W, *d)

        def call():
            assert fn(*args, 0, 0, m32, s32, lib._stream()) == 0
        return call

    def ab_post(L, buf, depth, planar):
        if planar:
            fn, args = L.emavfi_postprocess_yuv420p, (pred.data_ptr(), *lib._yuv420p_planes(*planes3(buf, depth > 8), depth, "ab")[3], B, H, W, depth)
        else:
            pl, d = semi_args(buf, depth)
            fn, args = (L.emavfi_postprocess_nv12 if depth == 8 else L.emavfi_postprocess_p010), (pred.data_ptr(), *pl, B, H, W, *d)

        def call():
            assert fn(*args, 0, 0, m64, s64, 1, lib._stream()) == 0
        return call

    ab8, ab10, ab_nv, ab_p010 = torch.empty_like(d_pl8), torch.empty_like(d_pl10), torch.empty_like(d_nv), torch.empty_like(d_p010)
    # both builds through the same direct calls: lib's wrappers cost a few microseconds of host time in front of a launch, which HIP events
    # around a 40 - 80 us kernel on an idle queue would count against the loaded library alone
    def eight(L, tag, out_nv, out8, out_p010, out10):
        return {
            "preprocess_nv12" + tag: (ab_pre(L, d_nv, 8, False), 13.5),
            "preprocess_yuv420p d=8" + tag: (ab_pre(L, d_pl8, 8, True), 13.5),
            "preprocess_p010" + tag: (ab_pre(L, d_p010, 10, False), 15.0),
            "preprocess_yuv420p d=10" + tag: (ab_pre(L, d_pl10, 10, True), 15.0),
            "postprocess_nv12" + tag: (ab_post(L, out_nv, 8, False), 13.5),
            "postprocess_yuv420p d=8" + tag: (ab_post(L, out8, 8, True), 13.5),
            "postprocess_p010" + tag: (ab_post(L, out_p010, 10, False), 15.0),
            "postprocess_yuv420p d=10" + tag: (ab_post(L, out10, 10, True), 15.0),
        }

    kernels = {**eight(lib.load(), "", o_nv, o_pl8, o_p010, o_pl10), **eight(AB, ", second build", ab_nv, ab8, ab_p010, ab10)}
times = {k: [] for k in kernels}
for name, (fn, _) in kernels.items():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
# the planar results are the interleaved results: checked here once, on the benchmark's own frames
assert torch.equal(planes3(o_pl8, False)[1], planes2(o_nv)[1][..., 0]) and torch.equal(planes3(o_pl8, False)[0], planes2(o_nv)[0])
if args.ab_lib:                              # both builds write the same frames
    assert torch.equal(ab8, o_pl8) and torch.equal(ab10, o_pl10) and torch.equal(ab_nv, o_nv) and torch.equal(ab_p010, o_p010)
    ref = torch.empty_like(x)
    for buf, depth, planar in ((d_nv, 8, False), (d_pl8, 8, True), (d_p010, 10, False), (d_pl10, 10, True)):
        ab_pre(lib.load(), buf, depth, planar)()
        ref.copy_(x)
        ab_pre(AB, buf, depth, planar)()
        assert torch.equal(ref.view(torch.int32), x.view(torch.int32))
u16 = lambda t: t.to(torch.int32).bitwise_and(0xffff)
assert torch.equal(u16(planes3(o_pl10, True)[2]), u16(planes2(o_p010)[1][..., 1]) >> 6)
for _ in range(max(20, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved: every round times each kernel once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
n = len(times["preprocess_nv12"])
say(f"## Kernels on {B} resident frames of {W} x {H} (us per call; HIP events, 5 warm-up calls, {n} interleaved samples)")
say()
say("| kernel | median | min | max | median, first half / second half | algorithmic B/px | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
med = {}
for name, (_, bpp) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = halves(t)
    bw = bpp * B * H * W / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {bpp} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
for a, b in (("preprocess_yuv420p d=8", "preprocess_nv12"), ("preprocess_yuv420p d=10", "preprocess_p010"),
             ("postprocess_yuv420p d=8", "postprocess_nv12"), ("postprocess_yuv420p d=10", "postprocess_p010")):
    spread = max(times[b]) - min(times[b])
    verdict = ("within the counterpart's spread" if med[a] <= med[b] + spread else
               "SLOWER than the counterpart by more than its spread: the reason belongs under \"## Notes\" at the end of this file, by hand")
    say(f"- {a} {med[a]:.1f} us vs {b} {med[b]:.1f} us: ratio {med[a] / med[b]:.3f}; {b}'s own min..max spread {spread:.1f} us: {verdict}.")
if args.ab_lib:
    say()
    say(f"Second build ({os.path.basename(args.ab_lib)}) beside the loaded library, same loop, same buffers; ratio of medians loaded / second:")
    say()
    for a in [k for k in kernels if not k.endswith(", second build")]:
        c = a + ", second build"
        say(f"- {a}: loaded {med[a]:.1f} us, second build {med[c]:.1f} us: {med[a] / med[c]:.3f}.")
say()

# ---------------------------------------------------------------- (2) run_chunked beside run, host frames in and out
if not args.skip_harness:
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    make = lambda: FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, pixel_format="yuv420p8", copy_out=False)
    runs = {"run": lambda fi: fi.run(planar8)}
    for k in args.chunk_pairs:
        runs[f"run_chunked, chunk_pairs={k}"] = lambda fi, k=k: fi.run_chunked(iter(planar8), chunk_pairs=k)
    rate = {k: [] for k in runs}
    sum(1 for _ in make().run(planar8[:17]))   # warm-up
    for _ in range(args.rounds):
        for name, go in runs.items():          # alternating
            fi = make()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            nout = sum(1 for _ in go(fi))
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            assert nout == 2 * (NFRAMES - 1) + 1
            rate[name].append((NFRAMES - 1) / dt)
    say(f"## run_chunked beside run ({NFRAMES} frames = {NFRAMES - 1} pairs of {W} x {H}, yuv420p8, batch 8, bf16, factor 1, copy_out off; "
        f"{args.rounds} alternating runs each)")
    say()
    say("| call | interpolated frames/s: median | min | max | source frames held at most |")
    say("|---|---|---|---|---|")
    for name in runs:
        r = rate[name]
        held = NFRAMES if name == "run" else min(NFRAMES, int(name.split("=")[1]) + 1)
        say(f"| {name} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} | {held} |")
    say()
    base = statistics.median(rate["run"])
    for name in list(runs)[1:]:
        say(f"- {name}: {statistics.median(rate[name]) / base:.3f} of run()'s rate (run()'s own min..max spread: {max(rate['run']) - min(rate['run']):.1f} frames/s).  "
            "Every chunk drains its last batch before the next one stages its first: the pipeline empties once per chunk.")
# what was written by hand under "## Notes" survives a re-run; a new file gets the heading and a placeholder
NOTES = "## Notes (written by hand; the tool keeps everything from this heading on when it rewrites the file)"
notes = NOTES + "\n\n(none yet: explain here every kernel flagged SLOWER above)\n"
if os.path.exists(args.out):
    old = open(args.out).read()
    if NOTES in old:
        notes = old[old.index(NOTES):]
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n\n" + notes)
