#!/usr/bin/env python3
"""What does motion blur from a shutter angle cost (round 23)?  One process, one box:
  (a) emavfi_accumulate_frames on resident 1280 x 720 frames, bgr24 (bytes) and p010 (16-bit words, sample in the top 10 bits), 8 output
      frames per call - one launch - at n = 3, 5 and 9 taps per output, interleaved with emavfi_resample_frames' blend (n = 2) in the same
      run.  Every entry of every call reads frames of its own: the calls of all forms walk one pool of 96 frames (265 MB, above the
      Infinity Cache), each starting where the one before it ended, so no form finds its frames where its own last call left them.  Timed
      with HIP events around 10 calls enqueued behind a few ms of matrix products (device time alone: no wrapper, no launch latency of an
      idle queue), `--samples` interleaved samples; median, min .. max and the median of either half of the samples (the run-to-run spread
      the comparison has to clear).  Reported as a fraction of the HBM peak on the algorithmic bytes, (n + 1) frame_bytes per output.
  (b) the harness's PCIe-inclusive output rate, host frames in and out (`--pairs` pairs of 720p bgr24, batch 8, bf16, copy_out=False; the
      median of three runs of the stream): shutter=180 at ratio 1 and depth 3 (4 of the tree's 7 forwards, one frame per pair back over
      PCIe) beside mode "recursive" at factor 7 (the 7 forwards and 8 frames per pair a host-side accumulation would need) and beside the
      plain resample run at ratio 1 (no forward at all: the transport alone), alternating, `--rounds` times each.
Nothing here is a gate.  Writes a markdown note (default profiles/r23_shutter.md)."""
import argparse, os, platform, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_shutter.md"))
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
H, W, N, POOL, REP = 720, 1280, 8, 96, 10
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say("# Motion blur from a shutter angle: the accumulation kernel and the harness (tools/bench_shutter.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
say()

# ---------------------------------------------------------------- (a) the kernel, resident frames
rng = np.random.default_rng(0)
cursor = 0


def walk(n):
    """the next N * n frames of the pool, as N tap lists"""
    global cursor
    taps = [[lib.RESAMPLE_NODES | ((cursor + k * n + i) % POOL) for i in range(n)] for k in range(N)]
    cursor = (cursor + N * n) % POOL
    return taps


kernels = {}
for fmt, shape in (("bgr24", (H, W, 3)), ("p010", (H * 3 // 2, 2 * W))):       # frames as their bytes
    fb = int(np.prod(shape))
    one = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).to(dev)
    nodes = torch.stack([one.roll(k, 0) for k in range(POOL)])
    srcs, dst = nodes[:1], torch.empty(N, *shape, dtype=torch.uint8, device=dev)
    sf = lib.resample_sample_format(fmt)

    def blend(d=dst, s=srcs, p=nodes, sf=sf):
        lib.resample_frames(d, s, p, [(a, b, 102, 0, 0) for a, b in walk(2)], None, *sf)

    kernels[f"{fmt} resample_frames, blend (n = 2)"] = (blend, 3.0 * N * fb)
    for n in (3, 5, 9):
        def accumulate(d=dst, s=srcs, p=nodes, sf=sf, n=n):
            lib.accumulate_frames(d, s, p, [(t, [1, 2] + [2] * (n - 3) + [1], 0, 0) for t in walk(n)], None, *sf)
        kernels[f"{fmt} accumulate_frames, n = {n}"] = (accumulate, (n + 1.0) * N * fb)
for fn, _ in kernels.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
plug = torch.randn(4096, 4096, device=dev)
times = {k: [] for k in kernels}
for _ in range(max(10, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved: every round times each form once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(6):
            plug @ plug
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / REP)
n_s = len(next(iter(times.values())))
say(f"## (a) The kernel on resident {W} x {H} frames, {N} output frames per call ({REP} calls behind a few ms of matrix products between two HIP "
    f"events: device time; 5 warm-up calls, {n_s} interleaved samples; every call reads the next frames of a pool of {POOL})")
say()
say("| launch | us per call: median | min | max | median, first half / second half | MB read + written (algorithmic) | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
share = {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    m = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    share[name] = {k: nbytes / (v * 1e-6) / HBM_PEAK for k, v in (("med", m), ("lo", max(t)), ("hi", min(t)), ("h1", h1), ("h2", h2))}
    say(f"| {name} | {m:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {nbytes / (m * 1e-6) / 1e9:.0f} | {100 * share[name]['med']:.1f} % |")
say()
say("The expectation to check (no gate): the accumulation moves its algorithmic bytes at the blend's fraction of the HBM peak, within the spread "
    "of the samples.")
say()
for fmt in ("bgr24", "p010"):
    b = share[f"{fmt} resample_frames, blend (n = 2)"]
    for n in (3, 5, 9):
        a = share[f"{fmt} accumulate_frames, n = {n}"]
        spread = max(abs(b["h1"] - b["h2"]), abs(a["h1"] - a["h2"]))
        say(f"- {fmt}, n = {n}: {100 * a['med']:.1f} % against the blend's {100 * b['med']:.1f} % ({a['med'] / b['med']:.2f} x); the medians of the two "
            f"halves of the samples differ by up to {100 * spread:.1f} points, the samples span {100 * a['lo']:.1f} .. {100 * a['hi']:.1f} % and "
            f"{100 * b['lo']:.1f} .. {100 * b['hi']:.1f} %.")
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
if not args.skip_harness:
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    frames = [np.roll(u8[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    common = dict(batch_pairs=8, copy_out=False, reference_quirks=False)
    fis = {"shutter 180, ratio 1, depth 3": FrameInterpolator(model, mode="resample", rate_in=24, rate_out=24, shutter=180, **common),
           "recursive, factor 7": FrameInterpolator(model, 7, mode="recursive", **common),
           "resample, ratio 1 (no forwards)": FrameInterpolator(model, mode="resample", rate_in=24, rate_out=24, **common)}
    fwd = {"shutter 180, ratio 1, depth 3": FrameInterpolator.shutter_plan(args.pairs + 1, 24, 24, 3, 180).forwards / args.pairs,
           "recursive, factor 7": 7.0, "resample, ratio 1 (no forwards)": 0.0}
    secs, count = {k: [] for k in fis}, {}

    def stream(fi):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            count[fi] = sum(1 for _ in fi.run(frames))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    for fi in fis.values():
        sum(1 for _ in fi.run(frames[:17]))                   # warm-up
    for _ in range(args.rounds):
        for name, fi in fis.items():                          # alternating
            secs[name].append(stream(fi))
    say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} bgr24, batch 8, bf16, copy_out=False; each figure the median of three "
        f"runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | frames back over PCIe per run | forwards per pair | source pairs/s: median of the rounds | min | max | forwards/s at the median |")
    say("|---|---|---|---|---|---|---|")
    for name, fi in fis.items():
        r = [args.pairs / s for s in secs[name]]
        m = statistics.median(r)
        say(f"| {name} | {count[fi]} | {fwd[name]:.2f} | {m:.1f} | {min(r):.1f} | {max(r):.1f} | {m * fwd[name]:.1f} |")
    say()
    say("Source pairs/s is the rate at which the clip is consumed: at ratio 1 it is the output frame rate of the blurred stream.  The recursive "
        "row is what a host-side accumulation of the full tree would have to run first (its own summing not included).")
    say()
say("## Not measured")
say()
say("Counters (achieved HBM traffic, L2 / Infinity Cache hit rates) were not collected: the fractions above are algorithmic bytes over event "
    "time.  Other frame sizes, other depths and ratios above 1, the 16-bit planar formats, more than one GPU, and the idle-queue latency of "
    "a single call were not measured.  bench.py, the flagship measurement, does not run this path and is unchanged.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
