#!/usr/bin/env python3
"""What does NV12 in / out cost or save (round 10)?  At 9 frames x 1280 x 720:
  (1) kernel times of emavfi_preprocess_nv12 / _postprocess_nv12 against emavfi_preprocess_u8 / _postprocess_u8 on the same frames
      (the NV12 frames are the encode of the u8 ones), resident in HBM, in one process, interleaved a-b-a-b: HIP events, warm-up, the
      median of N >= 20 and the spread (min .. max, and the median's shift between the first and the second half of the samples).
      Each also as a fraction of the HBM peak on its algorithmic bytes: 13.5 B/px for NV12 (1.5 byte side + 12 fp32 side), 15 for u8.
      The u8 kernels are the ones this library had before NV12 existed: the change did not touch them.
  (2) the harness rate with pixel_format="nv12" against "bgr24": host frames in, host frames out, B = 8 x 720p, bf16, alternating.
Writes a markdown note (default profiles/r10_nv12_io.md)."""
import argparse, os, platform, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_nv12_io.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
B, H, W = 9, 720, 1280
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
    return np.concatenate([y, np.stack([u, v], axis=-1).reshape(y.shape[0] // 2, y.shape[1])], axis=0)


f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
u8_frames = [np.roll(f1[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
nv_frames = [encode_host(f) for f in u8_frames]

say("# NV12 frames in and out: kernel times and harness rate (tools/bench_nv12.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
say()

# ---------------------------------------------------------------- (1) kernels, resident frames
d_u8 = torch.from_numpy(np.stack(u8_frames[:B])).to(dev)
d_nv = torch.from_numpy(np.stack(nv_frames[:B])).to(dev)
d_y, d_uv = d_nv[:, :H], d_nv[:, H:].unflatten(2, (W // 2, 2))
x = torch.empty(B, 3, H, W, device=dev)
pred = torch.rand(B, 3, H, W, device=dev)
o_u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
o_nv = torch.empty(B, H * 3 // 2, W, dtype=torch.uint8, device=dev)
o_y, o_uv = o_nv[:, :H], o_nv[:, H:].unflatten(2, (W // 2, 2))
kernels = {
    "preprocess_u8": (lambda: lib.preprocess_u8(d_u8, out=x), 15.0),
    "preprocess_nv12": (lambda: lib.preprocess_nv12(d_y, d_uv, out=x), 13.5),
    "postprocess_u8": (lambda: lib.postprocess_u8(pred, denormalize=True, out=o_u8), 15.0),
    "postprocess_nv12": (lambda: lib.postprocess_nv12(pred, denormalize=True, out=(o_y, o_uv)), 13.5),
}
times = {k: [] for k in kernels}
for name, (fn, _) in kernels.items():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
for _ in range(max(20, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved: every round times each kernel once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
say(f"## Kernels on {B} resident frames of {W} x {H} (us per call; HIP events, 5 warm-up calls, {len(times['preprocess_u8'])} interleaved samples)")
say()
say("| kernel | median | min | max | median, first half / second half | algorithmic B/px | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
med = {}
for name, (_, bpp) in kernels.items():
    t = times[name]
    med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    bw = bpp * B * H * W / (med[name] * 1e-6)
    say(f"| {name} | {med[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {bpp} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
say()
for a, b in (("preprocess_nv12", "preprocess_u8"), ("postprocess_nv12", "postprocess_u8")):
    spread = max(abs(statistics.median(times[k][:len(times[k]) // 2]) - statistics.median(times[k][len(times[k]) // 2:])) for k in (a, b))
    verdict = "no slower" if med[a] <= med[b] + spread else "SLOWER"
    say(f"- {a} {med[a]:.1f} us vs {b} {med[b]:.1f} us (run-to-run shift of the medians {spread:.1f} us): {verdict} "
        f"(expectation: no slower - same fp32 bytes, half the byte side).")
say()

# ---------------------------------------------------------------- (2) harness, host frames in and out
if not args.skip_harness:
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    runs = {"bgr24": u8_frames, "nv12": nv_frames}
    rate = {k: [] for k in runs}
    for fmt, frames in runs.items():
        fi = FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, pixel_format=fmt)
        sum(1 for _ in fi.run(frames[:17]))   # warm-up
    for _ in range(args.rounds):
        for fmt, frames in runs.items():      # alternating
            fi = FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, pixel_format=fmt)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            n = sum(1 for _ in fi.run(frames))
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            rate[fmt].append(args.pairs / dt)
    say(f"## Harness, host frames in and out ({args.pairs} pairs of {W} x {H}, batch 8, bf16, factor 1, reference_quirks on; {args.rounds} alternating runs each)")
    say()
    say("| pixel_format | interpolated frames/s: median | min | max | bytes per frame over PCIe, each way |")
    say("|---|---|---|---|---|")
    for fmt in runs:
        r = rate[fmt]
        say(f"| {fmt} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} | {(3 if fmt == 'bgr24' else 1.5) * H * W / 1e6:.2f} MB |")
    say()
    spread = max(max(r) - min(r) for r in rate.values())
    a, b = statistics.median(rate["nv12"]), statistics.median(rate["bgr24"])
    say(f"- nv12 {a:.1f} vs bgr24 {b:.1f} frames/s (widest min..max spread of either {spread:.1f}): "
        f"{'no slower' if a >= b - spread else 'SLOWER'} (expectation: no slower).")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
