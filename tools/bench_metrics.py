#!/usr/bin/env python3
"""What does scoring interpolated frames on the device cost (round 13)?  One process, one box:
  (1) the kernel on B = 8 resident 720p BGR pairs (HIP events, warm-up, N >= 20 interleaved samples; median, min .. max and the median's
      shift between the two halves of the samples): frame_metrics_u8 (both launches of the entry), beside postprocess_u8 over the same
      eight frames in the same run - the other kernel of the post lane - and the same pairs as Y planes (C = 1).  The achieved rate is quoted
      on the algorithmic bytes 2 * B * H * W * C (each image read once), and the time beside the forward's step at B = 8 x 720p;
  (2) the rate of evaluate() on a 64-target 720p clip against run() doing the same number of forwards on the same box in the same
      session (64 pairs, batch 8, bf16, factor 1, copy_out=False: bench.py's also_stream_pcie form), alternating, `--rounds` times each,
      the median of three runs per figure.  run() is the yardstick: it moves every frame back to the host, evaluate() moves none.
Writes a markdown note (default profiles/r13_frame_metrics.md)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_frame_metrics.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--targets", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--forward-ms", type=float, default=8.6, help="the forward's step at B = 8 x 720p bf16 the kernel time is set beside")
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
B, H, W = 8, 720, 1280
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Held-out PSNR / SSIM scored on the device: kernel time and evaluate() beside run() (tools/bench_metrics.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()

# ---------------------------------------------------------------- (1) the kernel, resident frames
rng = np.random.default_rng(0)
f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
a = torch.from_numpy(np.stack([np.roll(f1[0], 5 * i, axis=1) for i in range(B)])).to(dev)
b = torch.from_numpy(np.clip(a.cpu().numpy().astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)).to(dev)
ya, yb = a[..., :1].contiguous(), b[..., :1].contiguous()
x = torch.rand(B, 3, H, W, device=dev)
out3, out1 = torch.empty(B, 3, 2, dtype=torch.int64, device=dev), torch.empty(B, 1, 2, dtype=torch.int64, device=dev)
pred = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
px = float(B * H * W)
kernels = {
    "frame_metrics_u8, 8 BGR pairs (C = 3)": (lambda: lib.frame_metrics_u8(a, b, out=out3), 2 * 3 * px),
    "frame_metrics_u8, 8 Y-plane pairs (C = 1)": (lambda: lib.frame_metrics_u8(ya, yb, out=out1), 2 * px),
    "postprocess_u8(denormalize=False), the same 8 frames": (lambda: lib.postprocess_u8(x, denormalize=False, out=pred), 15 * px),
}
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
n = len(next(iter(times.values())))
w = out3.cpu().numpy()
say(f"## The kernel on {B} resident {W} x {H} pairs (us per call; HIP events around the call, 5 warm-up calls, {n} interleaved samples)")
say()
say("| launch | median | min | max | median, first half / second half | algorithmic MB | GB/s on them | of 8.0 TB/s HBM peak | of the forward's step |")
say("|---|---|---|---|---|---|---|---|---|")
med = {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    bw = nbytes / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.2f} % | "
        f"{100 * med[name] * 1e-3 / args.forward_ms:.1f} % |")
say()
say(f"The algorithmic bytes of the metric are 2 * B * H * W * C: each image read once (what it writes is {B * 3 * 16} bytes); a tile of 32 x 32 windows "
    "stages 42 x 42 pixels, so the kernel asks the caches for (42 / 32)^2 = 1.72 times that and is bound by its arithmetic (per pixel and channel 55 "
    "integer multiply-adds in the row pass at 42 / 32 rows per row used, 55 64-bit ones in the column pass, and a double-precision tail with a "
    f"division), not by memory.  postprocess_u8 reads 12 B and writes 3 B per pixel.  The forward's step is taken as {args.forward_ms} ms (B = 8 x 720p, bf16).  "
    f"Scores of the pairs measured (the second image is the first +- 3 counts of noise): PSNR {lib.psnr(int(w[..., 0].sum()), B * H * W * 3):.2f} dB, "
    f"SSIM {sum(lib.ssim(int(v), H, W) for v in w[..., 1].reshape(-1)) / (B * 3):.5f}.  Times include the Python wrappers' launch overhead.")
say()

# ---------------------------------------------------------------- (2) the harness: evaluate() beside run()
if not args.skip_harness:
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    nt = args.targets
    clip = [np.roll(u8[0], 3 * i, axis=1) for i in range(nt + 2)]       # nt targets: frames 1 .. nt
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    fi = {"run": FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, copy_out=False),
          "evaluate": FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, copy_out=False)}
    work = {"run": lambda: sum(1 for _ in fi["run"].run(clip[:nt + 1])),       # nt pairs: nt forwards, 2 nt + 1 frames back to the host
            "evaluate": lambda: len(fi["evaluate"].evaluate(clip))}           # nt targets: nt forwards, nt * 48 bytes back to the host
    rate = {k: [] for k in work}

    def stream(fn):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return nt / statistics.median(ts)

    for fn in work.values():
        fn()                                                  # warm-up: buffers, workspaces, the half-size first batch of run()
    for _ in range(args.rounds):
        for name, fn in work.items():                         # alternating
            rate[name].append(stream(fn))
    ev = fi["evaluate"].evaluate(clip)
    say(f"## Harness ({nt} forwards on {W} x {H} host frames, batch 8, bf16; each figure the median of three runs, {args.rounds} alternating rounds)")
    say()
    say("| harness | forwards/s: median of the rounds | min | max |")
    say("|---|---|---|---|")
    for name in work:
        r = rate[name]
        say(f"| {name}() | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} |")
    say()
    ratio = statistics.median(rate["evaluate"]) / statistics.median(rate["run"])
    say(f"- evaluate() / run(): {ratio:.3f} of run()'s forward rate (spread of the run() rounds, max - min: {max(rate['run']) - min(rate['run']):.1f}/s).  "
        "evaluate() stages three frames per target where run() stages the two of a pair (with every=1: n + 2 frames for n targets against n + 1), "
        "normalises all of them, and returns 48 bytes per target instead of two frames."
        + ("" if ratio >= 0.9 else "  BELOW 0.9: the lane ordering is the place to look (the metric kernel runs on the post lane beside the next "
           "batch's convolutions)."))
    say(f"- the clip's scores (synthetic weights, so the figures mean nothing as quality): {ev!r}")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
KEEP = "## Without a GPU"        # the hand-written section of the note survives a rewrite
if os.path.exists(args.out):
    old = open(args.out).read()
    if KEEP in old:
        lines += ["", old[old.index(KEEP):].rstrip("\n")]
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
