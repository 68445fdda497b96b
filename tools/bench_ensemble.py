#!/usr/bin/env python3
"""What does test-time ensembling cost beyond its forwards (round 20)?  One process, one box, the headline configuration: B = 8 x 1280 x 720,
bf16, synthetic weights.
  (a) `model(a, b)` with ensemble "reverse" / "flip" / "full" against n x the plain forward (n = 2 / 4 / 8 plain forwards issued back to
      back), alternating in one process: HIP events around each, after warm-up, `--samples` samples each; median, min .. max.  The
      overhead beyond n forwards is the difference of the medians, as a share of the ensembled step.
  (b) the two kernels alone on resident tensors of the step's shape ([8, 3, 720, 1280] fp32): emavfi_flip_f32 per flip code and
      emavfi_ensemble_mean_f32 at n = 2, 4, 8 with the ensembles' flips, each `--samples` times behind a few ms of matrix products (device
      time alone), HIP events; rate on the algorithmic bytes (flip: one read and one write; mean: n reads and one write) beside the HBM peak.
`--trace-run` issues three steps of each ensemble and leaves: the workload of a `rocprofv3 --kernel-trace --stats` run of its own.
Nothing here is a gate.  Writes a markdown note (default profiles/r20_ensemble.md; --append keeps what the file holds)."""
import argparse, os, platform, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import torch
from emavfi import EMA_VFI, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_ensemble.md"))
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--trace-run", action="store_true", help="three steps of each ensemble and leave (rocprofv3 --kernel-trace --stats -- python "
                "tools/bench_ensemble.py --trace-run); writes no note")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
B, H, W = 8, 720, 1280
N_OF = {"reverse": 2, "flip": 4, "full": 8}
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0), strict=True)
a, b = synth.fast_frames(0, B, H, W, device=dev)


def step(ensemble, n=1):
    with torch.no_grad():
        for _ in range(n):
            out = model(a, b, ensemble=ensemble)
    return out


if args.trace_run:
    for name in N_OF:
        for _ in range(3):
            step(name)
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
say("# Test-time ensembling: cost beyond the forwards and the two kernels' rates (tools/bench_ensemble.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_ensemble.py --samples {args.samples} --warmup {args.warmup}`")
say()

# ---------------------------------------------------------------- (a) the ensembled step against n plain forwards
say(f"## (a) `model(a, b)` at B = {B} x {W} x {H}, bf16: ensemble against n x the plain forward, alternating")
say()
for _ in range(args.warmup):
    step(None)
    for name in N_OF:
        step(name)
torch.cuda.synchronize()
plain = [timed(lambda: step(None)) for _ in range(args.samples)]
say(f"plain forward: {stats(plain)}")
say()
say("| ensemble | n | ensembled step | n plain forwards | beyond n forwards | share of the step |")
say("|---|---|---|---|---|---|")
for name, n in N_OF.items():
    ens, ref = [], []
    for _ in range(args.samples):
        ens.append(timed(lambda: step(name)))
        ref.append(timed(lambda: step(None, n)))
    over = statistics.median(ens) - statistics.median(ref)
    say(f"| {name} | {n} | {stats(ens)} | {stats(ref)} | {over:+.3f} ms | {100.0 * over / statistics.median(ens):+.2f} % |")
say()

# ---------------------------------------------------------------- (b) the two kernels alone
say(f"## (b) the kernels on resident [{B}, 3, {H}, {W}] fp32 tensors, behind a few ms of matrix products (device time alone)")
say()
x = [torch.randn(B, 3, H, W, device=dev) for _ in range(8)]
out = torch.empty_like(x[0])
nbytes = x[0].numel() * 4
g = torch.randn(4096, 4096, device=dev)
cases = [(f"flip_f32, flip {f}", (lambda f=f: lib.flip_f32(x[0], f, out=out)), 2 * nbytes) for f in range(4)]
for name, n in N_OF.items():
    flips = [0, 0] if name == "reverse" else list(lib.ENSEMBLE_FLIPS) * (n // 4)
    cases.append((f"ensemble_mean_f32, n = {n} (\"{name}\")", (lambda n=n, flips=flips: lib.ensemble_mean_f32(x[:n], flips, out=out)), (n + 1) * nbytes))
say("| launch | algorithmic bytes | device time | rate | of the HBM peak (8 TB/s) |")
say("|---|---|---|---|---|")
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
    say(f"| {label} | {by / 1e6:.1f} MB | {stats(v)} | {rates[label] / 1e9:.0f} GB/s | {100.0 * rates[label] / HBM_PEAK:.1f} % |")
say()
fl, mn = [r for k, r in rates.items() if k.startswith("flip")], [r for k, r in rates.items() if k.startswith("ensemble")]
say(f"flip_f32 reaches {min(fl) / 1e9:.0f} .. {max(fl) / 1e9:.0f} GB/s, ensemble_mean_f32 {min(mn) / 1e9:.0f} .. {max(mn) / 1e9:.0f} GB/s: "
    f"the slower of the two runs at {min(min(fl), min(mn)) / max(max(fl), max(mn)):.2f} x the faster.")
say()
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
