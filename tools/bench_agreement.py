#!/usr/bin/env python3
"""What does the agreement guard cost (round 22)?  One process, one box, the headline configuration: B = 8 x 1280 x 720, bf16, synthetic
weights.
  (a) `model(a, b, ensemble="reverse")` with and without `agreement=(tol, r)`, alternating in one process: HIP events around each, after
      warm-up, `--samples` samples each; median, min .. max.  The guard REPLACES the ensemble's mean launch, so the overhead is the
      difference of the medians, as a share of the guarded step.  tol is picked from the two plain forwards so that about a tenth of
      the pixels is flagged (the share actually held is printed: the model's own count).
  (b) the guard launch alone on resident tensors of the step's shape ([8, 3, 720, 1280] fp32), radius 0, 2 and 16, with nothing, about a
      tenth and everything held, each `--samples` times behind a few ms of matrix products (device time alone), HIP events; rate on the
      algorithmic bytes (u and v read, out written, a and b read where held - from the launch's own count) beside the HBM peak.
`--trace-run` issues three guarded steps per radius and leaves: the workload of a `rocprofv3 --kernel-trace --stats` run of its own.
Nothing here is a gate.  Writes a markdown note (default profiles/r22_agreement_guard.md; --append keeps what the file holds)."""
import argparse, os, platform, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import torch
from emavfi import EMA_VFI, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_agreement_guard.md"))
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--trace-run", action="store_true", help="three guarded steps per radius and leave (rocprofv3 --kernel-trace --stats -- python "
                "tools/bench_agreement.py --trace-run); writes no note")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
B, H, W = 8, 720, 1280
RADII = (0, 2, 16)
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0), strict=True)
a, b = synth.fast_frames(0, B, H, W, device=dev)
with torch.no_grad():
    u0, v0 = model(a, b).float(), model(b, a).float()
# about a tenth of the pixels flagged: the 0.9 quantile of the per-pixel disagreement of the two plain forwards (a strided sample of it)
d = (u0 - v0).abs().amax(dim=1).flatten()[::97]
TOL = min(1.0, float(torch.quantile(d, 0.9)))


def step(agreement):
    with torch.no_grad():
        return model(a, b, ensemble="reverse", agreement=agreement)


if args.trace_run:
    for r in RADII:
        for _ in range(3):
            step((TOL, r))
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
say("# Agreement guard: cost beside the \"reverse\" ensemble and the launch's rate (tools/bench_agreement.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_agreement.py --samples {args.samples} --warmup {args.warmup}`")
say()

# ---------------------------------------------------------------- (a) the guarded step against the plain "reverse" ensemble
say(f"## (a) `model(a, b, ensemble=\"reverse\")` at B = {B} x {W} x {H}, bf16: with the guard against without, alternating")
say()
say(f"tol = {TOL:.6g} (the 0.9 quantile of the two plain forwards' per-pixel disagreement).")
say()
for _ in range(args.warmup):
    step(None)
    for r in RADII:
        step((TOL, r))
torch.cuda.synchronize()
say("| radius | held share | guarded step | plain \"reverse\" step | guard beyond the mean it replaces | share of the step |")
say("|---|---|---|---|---|---|")
for r in RADII:
    g, p = [], []
    for _ in range(args.samples):
        g.append(timed(lambda: step((TOL, r))))
        p.append(timed(lambda: step(None)))
    held = model.agreement_counts.sum().item() / (B * H * W)
    over = statistics.median(g) - statistics.median(p)
    say(f"| {r} | {100.0 * held:.1f} % | {stats(g)} | {stats(p)} | {over:+.3f} ms | {100.0 * over / statistics.median(g):+.2f} % |")
say()

# ---------------------------------------------------------------- (b) the launch alone
say(f"## (b) the launch on resident [{B}, 3, {H}, {W}] fp32 tensors, behind a few ms of matrix products (device time alone)")
say()
u = torch.rand(B, 3, H, W, device=dev)
noise = torch.rand(B, 1, H, W, device=dev)
x = [torch.randn(B, 3, H, W, device=dev) for _ in range(2)]
out, counts = torch.empty_like(u), torch.zeros(B, dtype=torch.int32, device=dev)
nbytes = u.numel() * 4
g2 = torch.randn(4096, 4096, device=dev)
say("| radius | flagged pixels | held share | algorithmic bytes | device time | rate | of the HBM peak (8 TB/s) |")
say("|---|---|---|---|---|---|---|")
for r in RADII:
    for label, p_flag in (("none", 0.0), ("a tenth held", 1.0 - 0.9 ** (1.0 / (2 * r + 1) ** 2)), ("all", 1.0)):
        v = torch.where(noise < p_flag, (u + 0.5) % 1.0, u).contiguous()      # flagged pixels differ by 0.5 in every channel
        fn = lambda: lib.agreement_guard_f32(u, v, x[0], x[1], 0.25, r, out=out, counts=counts)
        fn()
        held = counts.sum().item() / (B * H * W)
        by = 3 * nbytes + 2 * held * nbytes
        t = []
        for _ in range(args.samples):
            for _ in range(4):
                g2 @ g2                                 # the queue stays busy: the events below bracket device time, not launch latency
            t.append(timed(fn))
        rate = by / (statistics.median(t) * 1e-3)
        say(f"| {r} | {label} | {100.0 * held:.1f} % | {by / 1e6:.1f} MB | {stats(t)} | {rate / 1e9:.0f} GB/s | {100.0 * rate / HBM_PEAK:.1f} % |")
say()
say("The event timings include the counts' clearing launch and the launch gap behind the matrix products.")
say()
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
