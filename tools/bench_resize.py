#!/usr/bin/env python3
"""What does resizing on the device cost (round 11)?  At 9 frames, 2560 x 1440 -> 1280 x 720 (the reference's default --scale 0.5):
  (1) kernel times, frames resident in HBM, in one process, interleaved a-b-a-b (HIP events, warm-up, the median of N >= 20 and the spread:
      min .. max and the median's shift between the first and the second half of the samples):
        fused u8     emavfi_preprocess_u8_resized            one launch            against   resize_u8 + preprocess_u8              two launches
        fused nv12   emavfi_preprocess_nv12_resized          one launch            against   resize_u8 (Y) + resize_u8 (UV) + preprocess_nv12
      and each as a rate on its ALGORITHMIC bytes: the source bytes once plus 12 B of fp32 per destination pixel.
  (2) the harness rate of FrameInterpolator(scale=0.5) on 1440p host frames against the same harness fed pre-resized 720p host frames
      (host frames in, host frames out, batch 8, bf16, alternating).  The H2D leg of the first carries four times the bytes.
Writes a markdown note (default profiles/r11_resize_io.md)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_resize_io.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
B, Hs, Ws, Hd, Wd = 9, 1440, 2560, 720, 1280
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Frames resized on the device: kernel times and harness rate (tools/bench_resize.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()

# ---------------------------------------------------------------- (1) kernels, resident frames
f1, _ = synth.synthetic_frames_u8(3, 1, Hs, Ws, "natural")
rng = np.random.default_rng(0)
d_u8 = torch.from_numpy(np.stack([np.roll(f1[0], 5 * i, axis=1) for i in range(B)])).to(dev)
d_nv = torch.from_numpy(rng.integers(0, 256, (B, Hs * 3 // 2, Ws), dtype=np.uint8)).to(dev)
d_y, d_uv = d_nv[:, :Hs], d_nv[:, Hs:].unflatten(2, (Ws // 2, 2))
x = torch.empty(B, 3, Hd, Wd, device=dev)
r_u8 = torch.empty(B, Hd, Wd, 3, dtype=torch.uint8, device=dev)
r_nv = torch.empty(B, Hd * 3 // 2, Wd, dtype=torch.uint8, device=dev)
r_y, r_uv = r_nv[:, :Hd], r_nv[:, Hd:].unflatten(2, (Wd // 2, 2))


def two_u8():
    lib.resize_u8(d_u8, (Hd, Wd), out=r_u8)
    lib.preprocess_u8(r_u8, out=x)


def two_nv12():
    lib.resize_u8(d_y.unsqueeze(-1), (Hd, Wd), out=r_y.unsqueeze(-1))
    lib.resize_u8(d_uv, (Hd // 2, Wd // 2), out=r_uv)
    lib.preprocess_nv12(r_y, r_uv, out=x)


src_u8, src_nv, dst = 3.0 * B * Hs * Ws, 1.5 * B * Hs * Ws, 12.0 * B * Hd * Wd
kernels = {
    "u8 fused (1 launch)": (lambda: lib.preprocess_u8(d_u8, out=x, size=(Hd, Wd)), src_u8 + dst),
    "u8 fused + resized bytes out": (lambda: lib.preprocess_u8(d_u8, out=x, size=(Hd, Wd), resized_out=r_u8), src_u8 + dst),
    "u8 composition (2 launches)": (two_u8, src_u8 + dst),
    "nv12 fused (1 launch)": (lambda: lib.preprocess_nv12(d_y, d_uv, out=x, size=(Hd, Wd)), src_nv + dst),
    "nv12 fused + resized planes out": (lambda: lib.preprocess_nv12(d_y, d_uv, out=x, size=(Hd, Wd), resized_out=(r_y, r_uv)), src_nv + dst),
    "nv12 composition (3 launches)": (two_nv12, src_nv + dst),
    "resize_u8 alone (C = 3)": (lambda: lib.resize_u8(d_u8, (Hd, Wd), out=r_u8), src_u8 + 3.0 * B * Hd * Wd),
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
say(f"## Kernels on {B} resident frames, {Ws} x {Hs} -> {Wd} x {Hd} (us per call; HIP events around the call, 5 warm-up calls, {n} interleaved samples)")
say()
say("| form | median | min | max | median, first half / second half | algorithmic MB | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
med, shift = {}, {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    shift[name] = abs(h1 - h2)
    bw = nbytes / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
say("The composition's rate is on the same algorithmic bytes as the fused form's; the bytes it really moves are more (the resized bytes are "
    "written and read back).  Times include the Python wrappers' launch overhead, the same for every launch.")
say()
for a, b in (("u8 fused (1 launch)", "u8 composition (2 launches)"), ("nv12 fused (1 launch)", "nv12 composition (3 launches)")):
    spread = max(shift[a], shift[b])
    verdict = "no slower" if med[a] <= med[b] + spread else "SLOWER"
    say(f"- {a} {med[a]:.1f} us vs {b} {med[b]:.1f} us (run-to-run shift of the medians {spread:.1f} us): {verdict} "
        f"(expectation: no slower - it moves strictly fewer bytes).")
say()

# ---------------------------------------------------------------- (2) harness, host frames in and out
if not args.skip_harness:
    big = [np.roll(f1[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
    small = [lib.resize_u8(torch.from_numpy(f).unsqueeze(0).to(dev), (Hd, Wd)).cpu().numpy()[0] for f in big]
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    runs = {"pre-resized 720p frames": (small, {}), "1440p frames, scale=0.5": (big, {"scale": 0.5})}
    rate = {k: [] for k in runs}
    for name, (frames, kw) in runs.items():
        sum(1 for _ in FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, **kw).run(frames[:17]))   # warm-up
    for _ in range(args.rounds):
        for name, (frames, kw) in runs.items():      # alternating
            fi = FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sum(1 for _ in fi.run(frames))
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            rate[name].append(args.pairs / dt)
    say(f"## Harness, host frames in and out ({args.pairs} pairs, model at {Wd} x {Hd}, batch 8, bf16, factor 1, reference_quirks on; {args.rounds} alternating runs each)")
    say()
    say("| input | interpolated frames/s: median | min | max | bytes per frame host -> device |")
    say("|---|---|---|---|---|")
    for name, (frames, _) in runs.items():
        r = rate[name]
        say(f"| {name} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} | {frames[0].nbytes / 1e6:.2f} MB |")
    say()
    a, b = statistics.median(rate["1440p frames, scale=0.5"]), statistics.median(rate["pre-resized 720p frames"])
    say(f"- scale=0.5 on 1440p sources runs at {100 * a / b:.1f} % of the rate on pre-resized 720p frames ({a:.1f} vs {b:.1f} frames/s).  A drop is "
        "expected: the host stages and the H2D leg copies four times the bytes.  The pre-resized run is the path the parent commit has: "
        "without scale / size the harness enqueues the same kernels with the same arguments.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
