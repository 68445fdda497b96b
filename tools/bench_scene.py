#!/usr/bin/env python3
"""What does deciding and applying scene cuts on the device cost (round 12)?  One process, one box:
  (1) kernel times on 9 resident frames at 720p and 1440p, BGR and NV12 (HIP events, warm-up, N >= 20 interleaved samples; median, min .. max
      and the median's shift between the two halves of the samples):
        luma_signature_u8    the pass that touches every byte, as a rate on the bytes it reads (BGR: 3 B/px; NV12: the Y plane, 1 B/px)
        preprocess_u8 / preprocess_nv12 over the same frames in the same run - the comparison point: a kernel that reads the same bytes
                             (and writes 12 B of fp32 per pixel on top)
        scene_flags (8 pairs) and hold_frames_u8 (8 pairs x 720p / 1440p BGR frames; none flagged / all flagged)
  (2) the harness's PCIe-inclusive rate as bench.py's also_stream_pcie measures it (64 pairs of 720p, batch 8, bf16, factor 1, copy_out=False;
      the median of three runs of the stream) with scene_threshold unset and set, alternating, `--rounds` times each: the spread of the
      "unset" medians stands beside the difference.  The frames hold no cut, so "set" pays for the decision and an empty hold launch; a
      third row puts a cut into every eighth pair.
Writes a markdown note (default profiles/r12_scene_cuts.md)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_scene_cuts.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=64)
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
say("# Scene cuts decided and applied on the device: kernel times and harness rate (tools/bench_scene.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()

# ---------------------------------------------------------------- (1) kernels, resident frames
rng = np.random.default_rng(0)
kernels = {}
for H, W in ((720, 1280), (1440, 2560)):
    tag = f"{H}p"
    f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    d_u8 = torch.from_numpy(np.stack([np.roll(f1[0], 5 * i, axis=1) for i in range(B)])).to(dev)
    d_nv = torch.from_numpy(rng.integers(0, 256, (B, H * 3 // 2, W), dtype=np.uint8)).to(dev)
    d_y, d_uv = d_nv[:, :H], d_nv[:, H:].unflatten(2, (W // 2, 2))
    x = torch.empty(B, 3, H, W, device=dev)
    sig = torch.empty(B, 1024, dtype=torch.int32, device=dev)
    flags, scores = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    ones = torch.ones(8, dtype=torch.int32, device=dev)
    pred = torch.empty(8, H, W, 3, dtype=torch.uint8, device=dev)
    px = float(B * H * W)
    kernels[f"{tag} BGR luma_signature_u8"] = (lambda d=d_u8, s=sig: lib.luma_signature_u8(d, out=s), 3 * px)
    kernels[f"{tag} BGR preprocess_u8 (same bytes read)"] = (lambda d=d_u8, o=x: lib.preprocess_u8(d, out=o), 3 * px)
    kernels[f"{tag} NV12 luma_signature_u8 (Y plane)"] = (lambda y=d_y, s=sig: lib.luma_signature_u8(y.unsqueeze(-1), out=s), px)
    kernels[f"{tag} NV12 preprocess_nv12 (Y and UV read)"] = (lambda y=d_y, uv=d_uv, o=x: lib.preprocess_nv12(y, uv, out=o), 1.5 * px)
    kernels[f"{tag} scene_flags, 8 pairs"] = (lambda s=sig, f=flags, c=scores, hw=(H, W): lib.scene_flags(s[:8], s[1:], hw, 1000, flags=f, scores=c), 2 * 8 * 4096.0)
    kernels[f"{tag} BGR hold_frames_u8, 8 pairs, none flagged"] = (lambda p=pred, a=d_u8, f=flags: lib.hold_frames_u8(p, a[:8], f), 0.0)
    kernels[f"{tag} BGR hold_frames_u8, 8 pairs, all flagged"] = (lambda p=pred, a=d_u8, f=ones: lib.hold_frames_u8(p, a[:8], f), 2 * 8 * 3.0 * H * W)
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
say(f"## Kernels on {B} resident frames (us per call; HIP events around the call, 5 warm-up calls, {n} interleaved samples)")
say()
say("| launch | median | min | max | median, first half / second half | MB read (+ written) | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
med = {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    bw = nbytes / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
say("The rates are on the bytes a launch READS (the hold: read + written); the preprocess kernels also write 12 B of fp32 per pixel, which their "
    "rate leaves out - they are the comparison point for a pass over the same bytes, not a like-for-like kernel.  Times include the Python "
    "wrappers' launch overhead, the same for every launch; the small launches (scene_flags, an unflagged hold) measure little else.")
say()

# ---------------------------------------------------------------- (2) harness, host frames in and out
if not args.skip_harness:
    H, W = 720, 1280
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    frames = [np.roll(u8[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
    cuts = [f if (i // 8) % 2 == 0 else (255 - f[::-1]) for i, f in enumerate(frames)]      # a new shot every 8 frames
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    runs = {"scene_threshold unset": (frames, {}), "scene_threshold=0.1, no cut in the stream": (frames, {"scene_threshold": 0.1}),
            "scene_threshold=0.1, a cut every 8 frames": (cuts, {"scene_threshold": 0.1})}
    rate, found = {k: [] for k in runs}, {}

    def stream(fi, fr):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sum(1 for _ in fi.run(fr))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return args.pairs / statistics.median(ts)

    fis = {name: FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, copy_out=False, **kw) for name, (_, kw) in runs.items()}
    for name, (fr, _) in runs.items():
        sum(1 for _ in fis[name].run(fr[:25]))                # warm-up long enough to take the half-size first batch once
    for _ in range(args.rounds):
        for name, (fr, _) in runs.items():                    # alternating
            rate[name].append(stream(fis[name], fr))
            found[name] = len(fis[name].scene_cuts)
    say(f"## Harness, host frames in and out ({args.pairs} pairs of {W} x {H}, batch 8, bf16, factor 1, copy_out=False; each figure the median of three "
        f"runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | interpolated frames/s: median of the rounds | min | max | pairs flagged |")
    say("|---|---|---|---|---|")
    for name in runs:
        r = rate[name]
        say(f"| {name} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} | {found[name]} |")
    say()
    un, st = rate["scene_threshold unset"], rate["scene_threshold=0.1, no cut in the stream"]
    diff, spread = statistics.median(st) - statistics.median(un), max(un) - min(un)
    inside = min(un) <= statistics.median(st) <= max(un)
    say(f"- set minus unset: {diff:+.1f} frames/s ({100 * diff / statistics.median(un):+.2f} %); spread of the unset rounds (max - min): {spread:.1f} frames/s.  "
        + ("The set rate lies inside that spread: no cost resolved." if inside or diff > 0 else
           "The set rate falls below that spread.  Per batch the feature adds the launches timed above: one luma_signature_u8 over 9 frames, one "
           f"scene_flags, one hold_frames_u8 and a 64-byte copy ({med['720p BGR luma_signature_u8']:.0f} + {med['720p scene_flags, 8 pairs']:.0f} + "
           f"{med['720p BGR hold_frames_u8, 8 pairs, none flagged']:.0f} us by the table above), and it moves the HBM -> pinned copy of the "
           "predictions behind the hold on the post lane."))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
