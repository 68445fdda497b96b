#!/usr/bin/env python3
"""What does a frame border cost (round 21)?  One process, one box, the headline configuration: B = 8 x 1280 x 720, bf16, synthetic weights.
  (a) `model(a, b)` with border None / 8 / 16 / 32 (replicate), alternating in one process with the plain forward AT THE PADDED SIZE (inputs
      padded beforehand: what the extra pixels cost) and the plain forward at 720p: HIP events around each, after warm-up, `--samples`
      samples each; median, min .. max.  The remainder - the bordered step minus the plain forward at the padded size - is what pad and
      crop cost.
  (b) the two kernels alone on resident tensors of the step's shape ([8, 3, 720, 1280] fp32 and its extension), both modes, N = 8 / 16 /
      32 and the misaligned N = 2, beside emavfi_flip_f32 (flip 0: the reference streaming copy) on the same tensors in the same run, each
      `--samples` times behind a few ms of matrix products (device time alone), HIP events; rate on the algorithmic bytes (one read of
      the source, one write of the destination; the flip: of the picture both ways) and the ratio to the flip's.
  (c) the streaming harness (tools/bench_stream.py's path: 64 pairs of 720p uint8 host frames in and out, batch 8, PCIe included) with
      border=16 against without, alternating, `--stream-runs` runs each: the spread.
`--trace-run` issues three steps of each border and leaves: the workload of a `rocprofv3 --kernel-trace --stats` run of its own.
Nothing here is a gate.  Writes a markdown note (default profiles/r21_border.md; --append keeps what the file holds)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np
import torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_border.md"))
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--stream-runs", type=int, default=5)
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--trace-run", action="store_true", help="three steps of each border and leave (rocprofv3 --kernel-trace --stats -- python "
                "tools/bench_border.py --trace-run); writes no note")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
B, H, W = 8, 720, 1280
BORDERS = (8, 16, 32)
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0), strict=True)
a, b = synth.fast_frames(0, B, H, W, device=dev)


def step(border, x=a, y=b):
    with torch.no_grad():
        return model(x, y, border=border)


if args.trace_run:
    for N in BORDERS:
        for mode in lib.BORDER_MODES:
            for _ in range(3):
                step((N, mode))
    for _ in range(3):
        step((2, "reflect"))            # the misaligned interior
        lib.flip_f32(a, 0)              # the reference streaming kernel on the same tensor
    torch.cuda.synchronize()
    sys.exit(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Frame borders: what the extra pixels cost, what pad and crop cost, and the two kernels' rates (tools/bench_border.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_border.py --samples {args.samples} --warmup {args.warmup} --stream-runs {args.stream_runs}`")
say()

# ---------------------------------------------------------------- (a) the bordered step against the plain forward at the padded size
say(f"## (a) `model(a, b)` at B = {B} x {W} x {H}, bf16, border replicate: bordered step, plain forward at the padded size, plain forward, alternating")
say()
padded = {N: tuple(lib.border_pad_f32(t, N, "replicate") for t in (a, b)) for N in BORDERS}
for _ in range(args.warmup):
    step(None)
    for N in BORDERS:
        step(N)
        step(None, *padded[N])
torch.cuda.synchronize()
say("| border N | padded size | pixels | bordered step | plain forward at the padded size | plain forward at 720p | the extra pixels | pad and crop | share of the step |")
say("|---|---|---|---|---|---|---|---|---|")
for N in BORDERS:
    bord, big, plain = [], [], []
    for _ in range(args.samples):
        bord.append(timed(lambda: step(N)))
        big.append(timed(lambda: step(None, *padded[N])))
        plain.append(timed(lambda: step(None)))
    mb, mg, mp = (statistics.median(v) for v in (bord, big, plain))
    Hp, Wp = lib.border_padded_size(H, W, N)
    say(f"| {N} | {Wp} x {Hp} | {100.0 * (Hp * Wp / (H * W) - 1):+.2f} % | {stats(bord)} | {stats(big)} | {stats(plain)} | "
        f"{mg - mp:+.3f} ms ({100.0 * (mg / mp - 1):+.2f} %) | {mb - mg:+.3f} ms | {100.0 * (mb - mg) / mb:+.2f} % |")
say()
del padded

# ---------------------------------------------------------------- (b) the two kernels alone, beside the flip
say(f"## (b) the kernels on resident [{B}, 3, {H}, {W}] fp32 tensors, behind a few ms of matrix products (device time alone)")
say()
x = torch.randn(B, 3, H, W, device=dev)
y = torch.empty_like(x)
g = torch.randn(4096, 4096, device=dev)
nbytes = x.numel() * 4
cases = [("flip_f32, flip 0 (the reference streaming copy)", (lambda: lib.flip_f32(x, 0, out=y)), 2 * nbytes)]
keep = []
for N in (8, 16, 32, 2):
    Hp, Wp = lib.border_padded_size(H, W, N)
    big = torch.randn(B, 3, Hp, Wp, device=dev)
    keep.append(big)
    by = nbytes + big.numel() * 4
    for mode in lib.BORDER_MODES:
        cases.append((f"border_pad_f32, N = {N}, {mode}", (lambda N=N, mode=mode, big=big: lib.border_pad_f32(x, N, mode, out=big)), by))
    cases.append((f"border_crop_f32, N = {N}", (lambda N=N, big=big: lib.border_crop_f32(big, N, out=y)), by))
say("| launch | algorithmic bytes | device time | rate | of the HBM peak (8 TB/s) | of the flip's rate |")
say("|---|---|---|---|---|---|")
rates = {}
for label, fn, by in cases:
    fn()
    v = []
    for _ in range(args.samples):
        for _ in range(4):
            g @ g                                   # the queue stays busy: the events below bracket device time, not launch latency
        v.append(timed(fn))
    med = statistics.median(v)
    rates[label] = by / (med * 1e-3)
    flip = next(iter(rates.values()))
    say(f"| {label} | {by / 1e6:.1f} MB | {stats(v)} | {rates[label] / 1e9:.0f} GB/s | {100.0 * rates[label] / HBM_PEAK:.1f} % | {rates[label] / flip:.2f} |")
say()
flip = next(iter(rates.values()))
worst = min((r, k) for k, r in rates.items() if k.startswith("border"))
say(f"The slowest border launch ({worst[1]}) runs at {worst[0] / flip:.2f} of the flip's rate.")
say()
del keep, x, y

# ---------------------------------------------------------------- (c) the streaming harness
say(f"## (c) streaming harness (tools/bench_stream.py's path): 64 pairs of 720p uint8 host frames in and out, batch 8, PCIe included, alternating")
say()
f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
frames = [np.roll(f1[0], 3 * i, axis=1) for i in range(65)]
fis = {"no border": FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, reference_quirks=False),
       "border=16 replicate": FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, reference_quirks=False, border=16)}
for fi in fis.values():
    sum(1 for _ in fi.run(frames[:17]))             # warm-up
got = {k: [] for k in fis}
for _ in range(args.stream_runs):
    for k, fi in fis.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sum(1 for _ in fi.run(frames))
        torch.cuda.synchronize()
        got[k].append((len(frames) - 1) / (time.perf_counter() - t0))
say("| harness | interpolated frames/s: median (min .. max) |")
say("|---|---|")
for k, v in got.items():
    say(f"| {k} | {statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f}) |")
m0, m1 = (statistics.median(got[k]) for k in fis)
say()
say(f"border=16 runs at {m1 / m0:.3f} of the rate without ({100.0 * (m0 / m1 - 1):+.2f} % time per frame).")
say()
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
