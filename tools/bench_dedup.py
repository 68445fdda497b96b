#!/usr/bin/env python3
"""What does finding duplicate frames on the device cost (round 17)?  One process, one box:
  (a) emavfi_frame_diff_cells on 9 resident frames (8 consecutive pairs from one buffer, b = a + batch stride) of 1280 x 720 and of 1920 x 1080:
      a Y plane of bytes, interleaved BGR bytes and a Y plane of 10-bit words, beside emavfi_luma_signature_u8 over the same 9 frames in the
      same run, and emavfi_duplicate_flags over the 8 pairs' cells.  HIP events, warm-up, N >= 20 interleaved samples; median, min .. max and
      the median's shift between the two halves of the samples.  Each launch is timed twice: one call on an idle queue (wrapper and launch
      latency included), and ten calls behind a few ms of matrix products (device time alone).  The rate is on the bytes a launch asks for:
      the diff kernel reads 16 frames' worth where the signature reads 9, so equal bytes per second is the expectation to confirm or explain.
  (b) the harness's PCIe-inclusive output rate, host frames in and out (`--pairs` pairs of 1280 x 720 yuv420p8, 24 -> 60, nearest, depth 3,
      batch 8, bf16, copy_out=False; the median of three runs of the stream): dedup off (the path of the commit before) against
      dedup_threshold=0 on a clip without copies - the difference is the pre-pass, its second upload and its one host wait -, and the same
      clip with every fifth frame a copy of the frame before it, dedup off and on; alternating, `--rounds` times each; forwards per output
      frame are counted at the model.
Nothing here is a gate.  Writes a markdown note (default profiles/r17_dedup.md)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_dedup.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
B = 9
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Duplicate frames found on the device: kernel rates and harness cost (tools/bench_dedup.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_dedup.py --samples {args.samples} --pairs {args.pairs} --rounds {args.rounds}"
    + (" --skip-harness" if args.skip_harness else "") + "`")
say()

# ---------------------------------------------------------------- (a) kernels, resident frames
rng = np.random.default_rng(0)
kernels = {}
for H, W in ((720, 1280), (1080, 1920)):
    tag = f"{W} x {H}"
    d_y = torch.from_numpy(rng.integers(0, 256, (B, H, W, 1), dtype=np.uint8)).to(dev)
    d_c = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    d_w = torch.from_numpy(rng.integers(0, 1024, (B, H, W), dtype=np.int16)).to(dev)
    sig = torch.empty(B, 1024, dtype=torch.int32, device=dev)
    cells = torch.empty(B - 1, 1024, dtype=torch.int32, device=dev)
    flags, scores = torch.zeros(B - 1, dtype=torch.int32, device=dev), torch.zeros(B - 1, dtype=torch.int32, device=dev)
    px = float(H * W)
    kernels[f"{tag} Y bytes: frame_diff_cells, 8 pairs"] = (lambda d=d_y, c=cells: lib.frame_diff_cells(d[:-1], d[1:], out=c), 16 * px)
    kernels[f"{tag} Y bytes: luma_signature_u8, 9 frames"] = (lambda d=d_y, s=sig: lib.luma_signature_u8(d, out=s), 9 * px)
    kernels[f"{tag} BGR bytes: frame_diff_cells, 8 pairs"] = (lambda d=d_c, c=cells: lib.frame_diff_cells(d[:-1], d[1:], out=c), 48 * px)
    kernels[f"{tag} BGR bytes: luma_signature_u8, 9 frames"] = (lambda d=d_c, s=sig: lib.luma_signature_u8(d, out=s), 27 * px)
    kernels[f"{tag} Y 10-bit words: frame_diff_cells, 8 pairs"] = (lambda d=d_w, c=cells: lib.frame_diff_cells(d[:-1], d[1:], depth=10, out=c), 32 * px)
    kernels[f"{tag} duplicate_flags, 8 pairs"] = (lambda c=cells, f=flags, s=scores: lib.duplicate_flags(c, 0, flags=f, scores=s), 8 * 4096.0)
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
med, fmed = {}, {}
for title, data, store in ((f"one call on an idle queue (HIP events around the call, 5 warm-up calls, {len(next(iter(times.values())))} interleaved samples; "
                            "the Python wrapper and the launch latency are inside)", times, med),
                           (f"the queue kept full ({REP} calls enqueued behind a few ms of matrix products, so the events bracket device time alone; "
                            f"{len(next(iter(full.values())))} interleaved samples)", full, fmed)):
    say(f"## (a) Kernels on {B} resident frames: {title}")
    say()
    say("| launch | us per call: median | min | max | median, first half / second half | MB asked for | GB/s | of 8.0 TB/s HBM peak |")
    say("|---|---|---|---|---|---|---|---|")
    for name, (_, nbytes) in kernels.items():
        t = data[name]
        store[name] = statistics.median(t)
        h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
        bw = nbytes / (store[name] * 1e-6)
        say(f"| {name} | {store[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
    say()
for what, m in (("idle queue", med), ("queue kept full", fmed)):
    for tag in ("1280 x 720", "1920 x 1080"):
        for kind, nd, ns in (("Y bytes", 16, 9), ("BGR bytes", 48, 27)):
            d, s = m[f"{tag} {kind}: frame_diff_cells, 8 pairs"], m[f"{tag} {kind}: luma_signature_u8, 9 frames"]
            say(f"- {what}, {tag} {kind}: frame_diff_cells takes {d / s:.2f} x the signature's time for {nd / ns:.2f} x its bytes: "
                f"{(nd / d) / (ns / s):.2f} x its bytes per second.")
say()
say("The diff kernel asks for every frame but the first and the last twice (frame k is b of pair k - 1 and a of pair k); the nine frames fit the "
    "256 MB of last-level cache, so the second read need not come from HBM, and the rates above are on the bytes ASKED FOR.  No gate: the ratios "
    "are recorded.")
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
if not args.skip_harness:
    H, W = 720, 1280
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    chroma = np.full((H // 2, W), 128, np.uint8)
    clean = [np.concatenate([np.ascontiguousarray(np.roll(u8[0][..., 1], 3 * i, axis=1)), chroma]) for i in range(args.pairs + 1)]
    fifth = [clean[i - 1] if i % 5 == 4 else f for i, f in enumerate(clean)]          # every fifth frame copies the frame before it
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    rows, inner = [], model.forward

    def counting(x1, x2, *a, **kw):
        rows.append(x1.shape[0])
        return inner(x1, x2, *a, **kw)

    model.forward = counting
    common = dict(batch_pairs=8, copy_out=False, reference_quirks=False, mode="resample", rate_in=24, rate_out=60, pixel_format="yuv420p8")
    runs = {"no copies in the clip, dedup off (the path before this change)": (clean, {}),
            "no copies in the clip, dedup_threshold=0": (clean, dict(dedup_threshold=0)),
            "every fifth frame a copy, dedup off": (fifth, {}),
            "every fifth frame a copy, dedup_threshold=0": (fifth, dict(dedup_threshold=0))}
    fis = {name: FrameInterpolator(model, **common, **kw) for name, (_, kw) in runs.items()}
    rate, count, fwd, dropped = {k: [] for k in runs}, {}, {}, {}

    def stream(name):
        fi, fr = fis[name], runs[name][0]
        ts = []
        for _ in range(3):
            del rows[:]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            count[name] = sum(1 for _ in fi.run(fr))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            fwd[name], dropped[name] = sum(rows), len(fi.duplicates)
        return count[name] / statistics.median(ts)

    for name in runs:
        sum(1 for _ in fis[name].run(runs[name][0][:25]))     # warm-up
    for _ in range(args.rounds):
        for name in runs:                                     # alternating
            rate[name].append(stream(name))
    say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} yuv420p8, 24 -> 60, nearest, depth 3, batch 8, bf16, copy_out=False; each "
        f"figure the median of three runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | output frames per run | frames dropped | forwards per run | forwards per output frame | output frames/s: median of the rounds | min | max |")
    say("|---|---|---|---|---|---|---|---|")
    for name in runs:
        r = rate[name]
        say(f"| {name} | {count[name]} | {dropped[name]} | {fwd[name]} | {fwd[name] / count[name]:.3f} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} |")
    say()
    off, on = rate["no copies in the clip, dedup off (the path before this change)"], rate["no copies in the clip, dedup_threshold=0"]
    diff, spread = statistics.median(on) - statistics.median(off), max(off) - min(off)
    say(f"- clip without copies, dedup on minus off: {diff:+.1f} output frames/s ({100 * diff / statistics.median(off):+.2f} %); spread of the off rounds "
        f"(max - min): {spread:.1f} frames/s.  " + ("The on rate lies inside that spread: no cost resolved." if min(off) <= statistics.median(on) <= max(off)
        else "That is the price of the pre-pass: a second upload of every source frame, one frame_diff_cells and one duplicate_flags per slot-sized "
             "batch, and one host wait per run() before the first forward is enqueued."))
    say("- every output frame is counted, source frames included; a dropped copy costs the forwards of a deeper tree (a gap of two source "
        "intervals has four levels at depth 3), which is why forwards per output frame rise with dedup on.")
say()
say("Not measured: coded material (every clip here is synthetic, and its copies are bit-identical), any threshold above 0, other frame sizes and pixel formats in the harness, and `run_chunked`, which pays the wait once per chunk.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
