#!/usr/bin/env python3
"""What do 16-bit frames in / out cost (round 14)?  At 9 frames x 1280 x 720:
  (1) kernel times of emavfi_preprocess_p010 / _postprocess_p010 against emavfi_preprocess_nv12 / _postprocess_nv12 on the same content
      (the P010 frames are the NV12 ones with every byte widened to a 10-bit sample), resident in HBM, in one process, interleaved
      a-b-a-b: HIP events, warm-up, the median of N >= 20 and the spread (min .. max, and the median's shift between the first and the
      second half of the samples).  Each also as a fraction of the HBM peak on its algorithmic bytes: 15 B/px for P010 (3 byte side + 12
      fp32 side), 13.5 for NV12.  The NV12 kernels are the ones this library had before the 16-bit formats existed: the change did not
      touch them.  Expectation: a P010 kernel costs at most 15 / 13.5 of its NV12 sibling's time plus the spread the run shows.
  (2) the harness rate with pixel_format="p010" against "nv12": host frames in, host frames out, B = 8 x 720p, bf16, alternating.
Writes a markdown note (default profiles/r14_p010_io.md); --vgprs "pre / post" puts the code object's register counts into it."""
import argparse, os, platform, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_p010_io.md"))
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--skip-harness", action="store_true")
ap.add_argument("--vgprs", default="", help="text for the note: VGPR counts of the two kernels read from the gfx950 code object")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
RATIO = 15.0 / 13.5
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


def halves(t):
    return statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])


f1, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
nv_frames = [encode_host(np.roll(f1[0], 3 * i, axis=1)) for i in range(args.pairs + 1)]
p10_frames = [(f.astype(np.uint16) << 2 | f >> 6) << 6 for f in nv_frames]   # byte -> 10-bit sample (bit replication) -> the word's top bits

say("# 16-bit frames (P010) in and out: kernel times and harness rate (tools/bench_p010.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
if args.vgprs:
    say()
    say(f"gfx950 code object, preprocess_yuv420_kernel<Yuv16<true>> / postprocess_yuv420_kernel<Yuv16<true>>: {args.vgprs}.")
say()

# ---------------------------------------------------------------- (1) kernels, resident frames
d_nv = torch.from_numpy(np.stack(nv_frames[:B])).to(dev)
d_y, d_uv = d_nv[:, :H], d_nv[:, H:].unflatten(2, (W // 2, 2))
d_p = torch.from_numpy(np.stack(p10_frames[:B]).view(np.int16)).to(dev)
d_py, d_puv = d_p[:, :H], d_p[:, H:].unflatten(2, (W // 2, 2))
x = torch.empty(B, 3, H, W, device=dev)
pred = torch.rand(B, 3, H, W, device=dev)
o_nv = torch.empty(B, H * 3 // 2, W, dtype=torch.uint8, device=dev)
o_y, o_uv = o_nv[:, :H], o_nv[:, H:].unflatten(2, (W // 2, 2))
o_p = torch.empty(B, H * 3 // 2, W, dtype=torch.int16, device=dev)
o_py, o_puv = o_p[:, :H], o_p[:, H:].unflatten(2, (W // 2, 2))
kernels = {
    "preprocess_nv12": (lambda: lib.preprocess_nv12(d_y, d_uv, out=x), 13.5),
    "preprocess_p010": (lambda: lib.preprocess_p010(d_py, d_puv, 10, out=x), 15.0),
    "postprocess_nv12": (lambda: lib.postprocess_nv12(pred, denormalize=True, out=(o_y, o_uv)), 13.5),
    "postprocess_p010": (lambda: lib.postprocess_p010(pred, 10, denormalize=True, out=(o_py, o_puv)), 15.0),
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
say(f"## Kernels on {B} resident frames of {W} x {H} (us per call; HIP events, 5 warm-up calls, {len(times['preprocess_nv12'])} interleaved samples)")
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
for a, b in (("preprocess_p010", "preprocess_nv12"), ("postprocess_p010", "postprocess_nv12")):
    spread = max(abs(halves(times[k])[0] - halves(times[k])[1]) for k in (a, b))
    bound = RATIO * med[b] + spread
    say(f"- {a} {med[a]:.1f} us vs {b} {med[b]:.1f} us: ratio {med[a] / med[b]:.3f}; bound 15 / 13.5 x {med[b]:.1f} + {spread:.1f} "
        f"(shift of the medians between the halves) = {bound:.1f} us: expectation {'CONFIRMED' if med[a] <= bound else 'REFUTED'}.")
say()

# ---------------------------------------------------------------- (2) harness, host frames in and out
if not args.skip_harness:
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    runs = {"nv12": nv_frames, "p010": p10_frames}
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
        say(f"| {fmt} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} | {(1.5 if fmt == 'nv12' else 3) * H * W / 1e6:.2f} MB |")
    say()
    spread = max(max(r) - min(r) for r in rate.values())
    a, b = statistics.median(rate["p010"]), statistics.median(rate["nv12"])
    say(f"- p010 {a:.1f} vs nv12 {b:.1f} frames/s (widest min..max spread of either {spread:.1f}): ratio {a / b:.3f}.  P010 moves twice "
        f"NV12's bytes over PCIe and through the staging copies, the same as bgr24.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
