#!/usr/bin/env python3
"""What does a flow scale cost or save (round 24)?  One process, one box, the headline configuration: B = 8 x 1280 x 720, bf16, synthetic
weights.
  (a) `model(a, b)` with flow_scale None / 2 / 4 / 8, alternating in one process: HIP events around each, after warm-up, `--samples`
      samples each; median, min .. max, and the ratio to the plain forward beside the algorithmic expectation (SURVEY.md section 2.2 with
      the folded context: context encoding + motion estimation are 148 608 of 490 590 MAC/px, the coarse front adds 262 656 / s^2).
  (b) the four steps of the coarse forward one by one at each s (down x 2, the flow's forward at the reduced size, up, the forward with
      the given flow), the same way: where the step's time goes.
  (c) the two bandwidth kernels alone on resident tensors of the step's shapes ([8, 3, 720, 1280] frames down, [8, 2, 720, 1280] flow up),
      beside emavfi_flip_f32 (flip 0: the reference streaming copy) on the frames in the same run, each `--samples` times behind a few ms
      of matrix products (device time alone), HIP events; rate on the algorithmic bytes (one read of the source, one write of the
      destination).
The whole run ends itself after `--time-limit` seconds (SIGALRM), whatever it is doing.  Nothing here is a gate; nothing outside the
tree is read.  Writes a markdown note (default profiles/r24_flow_scale.md; --append keeps what the file holds)."""
import argparse, os, platform, signal, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import torch
from emavfi import EMA_VFI, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_flow_scale.md"))
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the process ends itself")
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
args = ap.parse_args()
signal.alarm(args.time_limit)
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
B, H, W = 8, 720, 1280
SCALES = lib.FLOW_SCALES
MAC_ALL, MAC_FLOW_ONLY, MAC_FRONT = 490590, 148608, 262656      # per pixel: the forward; context + motion estimation; features + those
if not torch.cuda.is_available():
    sys.exit("bench_flow_scale: no ROCm device (this tool measures; it has no CPU path)")
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f})"


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0), strict=True)
a, b = synth.fast_frames(0, B, H, W, device=dev)
dt = model._resolve_dtype()
packed = model.packed_weights(dt, dev)
mid, nb = model.mid_channels, model.num_blocks


def step(s):
    with torch.no_grad():
        return model(a, b, flow_scale=s)


say("# Flow scale: the coarse forward's step time, where it goes, and the two kernels' rates (tools/bench_flow_scale.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
say()
say(f"Command line: `python tools/bench_flow_scale.py --samples {args.samples} --warmup {args.warmup}`")
say()

# ---------------------------------------------------------------- (a) the step
say(f"## (a) `model(a, b, flow_scale=s)` at B = {B} x {W} x {H}, bf16 (pipeline = {model.pipeline}: the plain forward as the model runs it), alternating")
say()
for _ in range(args.warmup):
    for s in (None,) + SCALES:
        step(s)
torch.cuda.synchronize()
got = {s: [] for s in (None,) + SCALES}
for _ in range(args.samples):
    for s in got:
        got[s].append(timed(lambda: step(s)))
plain = statistics.median(got[None])
say("| flow_scale | step | of the plain forward | algorithmic MACs of the plain forward's |")
say("|---|---|---|---|")
for s, v in got.items():
    expect = 1.0 if s is None else (MAC_ALL - MAC_FLOW_ONLY + MAC_FRONT / (s * s)) / MAC_ALL
    say(f"| {s} | {stats(v)} | {statistics.median(v) / plain:.3f} | {expect:.3f} |")
say()

# ---------------------------------------------------------------- (b) the four steps one by one
say("## (b) the steps of the coarse forward, one by one (same process, HIP events around each call)")
say()
say("| s | down (both frames) | flow at the reduced size | up | forward with the given flow | sum |")
say("|---|---|---|---|---|---|")
for s in SCALES:
    a_s, b_s = lib.downscale_f32(a, s), lib.downscale_f32(b, s)
    flow_s = lib.forward_flow(packed, a_s, b_s, mid, nb, dt)
    flow = lib.upsample_flow_f32(flow_s, (H, W), s)
    out = torch.empty_like(a)
    parts = {"down": (lambda: (lib.downscale_f32(a, s, out=a_s), lib.downscale_f32(b, s, out=b_s))),
             "flow": (lambda: lib.forward_flow(packed, a_s, b_s, mid, nb, dt, out=flow_s)),
             "up": (lambda: lib.upsample_flow_f32(flow_s, (H, W), s, out=flow)),
             "given": (lambda: lib.forward_given_flow(packed, a, b, flow, mid, nb, dt, out=out))}
    t = {k: [] for k in parts}
    for k, fn in parts.items():
        fn()
    for _ in range(args.samples):
        for k, fn in parts.items():
            t[k].append(timed(fn))
    say(f"| {s} | " + " | ".join(stats(t[k]) for k in parts) + f" | {sum(statistics.median(v) for v in t.values()):.3f} ms |")
say()

# ---------------------------------------------------------------- (c) the two kernels alone, beside the flip
say(f"## (c) the kernels on resident tensors of the step's shapes, behind a few ms of matrix products (device time alone)")
say()
x = torch.randn(B, 3, H, W, device=dev)
y = torch.empty_like(x)
fl = torch.empty(B, 2, H, W, device=dev)
g = torch.randn(4096, 4096, device=dev)
cases = [("flip_f32, flip 0 (the reference streaming copy)", (lambda: lib.flip_f32(x, 0, out=y)), 2 * x.numel() * 4)]
keep = []
for s in SCALES:
    Hs, Ws = lib.coarse_size(H, W, s)
    lo, fs = torch.empty(B, 3, Hs, Ws, device=dev), torch.randn(B, 2, Hs, Ws, device=dev)
    keep += [lo, fs]
    cases.append((f"downscale_f32, s = {s}, [8, 3, 720, 1280] -> {Hs} x {Ws}", (lambda s=s, lo=lo: lib.downscale_f32(x, s, out=lo)), (x.numel() + lo.numel()) * 4))
    cases.append((f"upsample_flow_f32, s = {s}, {Hs} x {Ws} -> [8, 2, 720, 1280]", (lambda s=s, fs=fs: lib.upsample_flow_f32(fs, (H, W), s, out=fl)),
                  (fl.numel() + fs.numel()) * 4))
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
    say(f"| {label} | {by / 1e6:.1f} MB | {stats(v)} | {rates[label] / 1e12:.2f} TB/s | {100.0 * rates[label] / HBM_PEAK:.1f} % | {rates[label] / flip:.2f} |")
say()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
