#!/usr/bin/env python3
"""What does frame-rate conversion cost (round 16)?  One process, one box:
  (a) emavfi_resample_frames on resident 1280 x 720 frames, bgr24 (bytes) and yuv420p10 (16-bit words, sample in the low 10 bits), 8 output
      frames per call: copy entries (w = 0) and blend entries (w = 102) separately, per output frame (HIP events, warm-up, N >= 20 interleaved
      samples; median, min .. max and the median's shift between the two halves of the samples).  The yardstick is emavfi_hold_frames_u8
      copying the same bytes (8 pairs, all flagged) in the same run.  A blend moves three frames' bytes where a copy moves two.  Each launch
      is timed twice: one call on an idle queue (wrapper and launch latency included), and ten calls behind a few ms of matrix products
      (device time alone).
  (b) the harness's PCIe-inclusive output rate, host frames in and out (`--pairs` pairs of 720p, batch 8, bf16, copy_out=False; the median
      of three runs of the stream): mode "resample" 24 -> 60 at depth 3, nearest and blend, beside mode "recursive" at factor 3 and at
      factor 7 in the same process, alternating, `--rounds` times each; forwards per pair from resample_plan stand beside the rates.
Nothing here is a gate.  Writes a markdown note (default profiles/r16_resample.md)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_resample.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
H, W, N = 720, 1280, 8
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Frame-rate conversion: the assembly kernel and the harness (tools/bench_resample.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()

# ---------------------------------------------------------------- (a) the kernel, resident frames
rng = np.random.default_rng(0)
kernels = {}
ones = torch.ones(N, dtype=torch.int32, device=dev)
for fmt, shape in (("bgr24", (H, W, 3)), ("yuv420p10", (H * 3 // 2, 2 * W))):       # frames as their bytes
    fb = int(np.prod(shape))
    srcs = torch.from_numpy(rng.integers(0, 4 if fmt != "bgr24" else 256, (N + 1, *shape), dtype=np.uint8)).to(dev)
    nodes = torch.from_numpy(rng.integers(0, 4 if fmt != "bgr24" else 256, (N + 1, *shape), dtype=np.uint8)).to(dev)
    dst = torch.empty(N, *shape, dtype=torch.uint8, device=dev)
    sf = lib.resample_sample_format(fmt)
    copy = [(lib.RESAMPLE_NODES | k, lib.RESAMPLE_NODES | (k + 1), 0, 0, 0) for k in range(N)]
    blend = [(lib.RESAMPLE_NODES | k, lib.RESAMPLE_NODES | (k + 1), 102, 0, 0) for k in range(N)]
    kernels[f"{fmt} resample_frames, {N} copy entries"] = (lambda d=dst, s=srcs, n=nodes, t=copy, sf=sf: lib.resample_frames(d, s, n, t, None, *sf), 2.0 * N * fb)
    kernels[f"{fmt} resample_frames, {N} blend entries"] = (lambda d=dst, s=srcs, n=nodes, t=blend, sf=sf: lib.resample_frames(d, s, n, t, None, *sf), 3.0 * N * fb)
    kernels[f"{fmt} hold_frames_u8, {N} pairs, all flagged (yardstick)"] = (lambda d=dst, s=srcs: lib.hold_frames_u8(d, s[:N], ones), 2.0 * N * fb)
times = {k: [] for k in kernels}
for name, (fn, _) in kernels.items():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
for _ in range(max(20, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved: every round times each form once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
# the same launches with the queue kept full: a few ms of matrix products go first, so the host enqueues REP calls while the device is still
# busy and the events bracket device time alone - no wrapper, no launch latency of an idle queue
REP = 10
plug = torch.randn(4096, 4096, device=dev)
full = {k: [] for k in kernels}
for _ in range(max(10, args.samples // 2)):
    for name, (fn, _) in kernels.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):
            plug @ plug
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        e1.synchronize()
        full[name].append(e0.elapsed_time(e1) * 1e3 / REP)
n = len(next(iter(times.values())))
say(f"## (a) The kernel on resident {W} x {H} frames, {N} output frames per call (HIP events around the call, 5 warm-up calls, {n} interleaved samples)")
say()
say("| launch | us per call: median | min | max | median, first half / second half | us per output frame | MB read + written | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|---|")
med, fmed = {}, {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    bw = nbytes / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {med[name] / N:.2f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
say("One call between two events on an idle queue: the times include the Python wrapper (the resample wrapper also builds the ctypes table of its "
    "entries on every call) and the launch latency.")
say()
say(f"The same launches with the queue kept full ({REP} calls enqueued behind a few ms of matrix products, so the events bracket device time alone; "
    f"{len(next(iter(full.values())))} interleaved samples):")
say()
say("| launch | us per call: median | min | max | us per output frame | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|")
for name, (_, nbytes) in kernels.items():
    t = full[name]
    fmed[name] = statistics.median(t)
    bw = nbytes / (fmed[name] * 1e-6)
    say(f"| {name} | {fmed[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {fmed[name] / N:.2f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
for what, m in (("idle queue", med), ("queue kept full", fmed)):
    for fmt in ("bgr24", "yuv420p10"):
        y = m[f"{fmt} hold_frames_u8, {N} pairs, all flagged (yardstick)"]
        c, b = m[f"{fmt} resample_frames, {N} copy entries"], m[f"{fmt} resample_frames, {N} blend entries"]
        say(f"- {what}, {fmt}: copy entries take {c / y:.2f} x the yardstick's time, blend entries {b / y:.2f} x (3 / 2 = 1.50 x by the bytes moved); "
            f"blend / copy {b / c:.2f} x.")
say()
say("No gate: the ratios are recorded.")
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
if not args.skip_harness:
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    frames = [np.roll(u8[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    common = dict(batch_pairs=8, copy_out=False, reference_quirks=False)
    fis = {"resample 24 -> 60, nearest, depth 3": FrameInterpolator(model, mode="resample", rate_in=24, rate_out=60, resample_method="nearest", **common),
           "resample 24 -> 60, blend, depth 3": FrameInterpolator(model, mode="resample", rate_in=24, rate_out=60, resample_method="blend", **common),
           "recursive, factor 3": FrameInterpolator(model, 3, mode="recursive", **common),
           "recursive, factor 7": FrameInterpolator(model, 7, mode="recursive", **common)}
    fwd = {"resample 24 -> 60, nearest, depth 3": FrameInterpolator.resample_plan(args.pairs + 1, 24, 60, 3, "nearest").forwards / args.pairs,
           "resample 24 -> 60, blend, depth 3": FrameInterpolator.resample_plan(args.pairs + 1, 24, 60, 3, "blend").forwards / args.pairs,
           "recursive, factor 3": 3.0, "recursive, factor 7": 7.0}
    rate, count = {k: [] for k in fis}, {}

    def stream(fi):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            count[fi] = sum(1 for _ in fi.run(frames))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return count[fi] / statistics.median(ts)

    for fi in fis.values():
        sum(1 for _ in fi.run(frames[:25]))                   # warm-up
    for _ in range(args.rounds):
        for name, fi in fis.items():                          # alternating
            rate[name].append(stream(fi))
    say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} bgr24, batch 8, bf16, copy_out=False; each figure the median of three "
        f"runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | output frames per run | forwards per pair | output frames/s: median of the rounds | min | max | forwards/s at the median |")
    say("|---|---|---|---|---|---|---|")
    for name, fi in fis.items():
        r = rate[name]
        m = statistics.median(r)
        say(f"| {name} | {count[fi]} | {fwd[name]:.2f} | {m:.1f} | {min(r):.1f} | {max(r):.1f} | {m / count[fi] * fwd[name] * args.pairs:.1f} |")
    say()
    say("Output frames/s counts every frame the harness yields, source frames included.  The forwards decide the rate: a mode's output rate "
        "follows its forwards per pair, and the forwards/s column is the same model at the same size in every row.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
