#!/usr/bin/env python3
"""What does global motion compensation cost (round 28)?  One process, one box, synthetic weights.
  (a) the three kernels alone on resident tensors, at B = 8 x 1280 x 720 and B = 2 x 3840 x 2160 with a radius of 64 and of 128 pixels:
      emavfi_align_signature_f32, emavfi_align_search (its clear, search and finish launches together) and emavfi_shift_f32 - by a record
      whose halves are multiples of 4 (16-byte loads), by one whose halves are even only (8-byte loads) and by the zero record - beside
      emavfi_flip_f32 (flip 0: the reference streaming copy) on the same tensors in the same run, each `--samples` times behind a few ms
      of matrix products (device time alone), HIP events; signature and shift: the rate on their algorithmic bytes (one read of the
      frames and one write of the grid; one read and one write of the tensor), the shift's also as a share of the flip's.
  (b) `model(a, b)` at B = 8 x 1280 x 720, bf16, with align=(64, 0.5) and align=(128, 0.5) against the plain step, alternating in one
      process, HIP events around each, after warm-up, `--samples` samples each; median, min .. max; the overhead in microseconds and
      percent.  The pair is a planted pan of (-8, 24) pixels, so the shift is taken and the 8-byte loads run.
`--trace-run` issues three aligned steps and leaves: the workload of a `rocprofv3 --kernel-trace --stats` run of its own.
Nothing here is a gate.  Writes a markdown note (default profiles/r28_align.md; --append keeps what the file holds)."""
import argparse, os, platform, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import torch
from emavfi import EMA_VFI, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_align.md"))
ap.add_argument("--samples", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--trace-run", action="store_true", help="three aligned steps and leave (rocprofv3 --kernel-trace --stats -- python "
                "tools/bench_align.py --trace-run); writes no note")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
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


def pan(B, H, W, dy, dx):
    """a pair whose content moves by (dy, dx) pixels: two windows of one larger batch of frames"""
    big, _ = synth.fast_frames(0, B, H + 64, W + 64, device=dev)
    return big[:, :, 32:32 + H, 32:32 + W].contiguous(), big[:, :, 32 - dy:32 - dy + H, 32 - dx:32 - dx + W].contiguous()


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0), strict=True)
B, H, W = 8, 720, 1280
a, b = pan(B, H, W, -8, 24)


def step(align):
    with torch.no_grad():
        return model(a, b, align=align)


if args.trace_run:
    for _ in range(3):
        step((64, 0.5))
        step((128, 0.5))
    torch.cuda.synchronize()
    sys.exit(0)

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Global motion compensation: the three kernels' times and rates, and what an aligned step costs (tools/bench_align.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_align.py --samples {args.samples} --warmup {args.warmup}`")
say()

# ---------------------------------------------------------------- (a) the kernels alone, beside the flip
g = torch.randn(4096, 4096, device=dev)


def device_time(fn):
    fn()
    v = []
    for _ in range(args.samples):
        for _ in range(4):
            g @ g                                   # the queue stays busy: the events below bracket device time, not launch latency
        v.append(timed(fn))
    return v


for (kb, kh, kw) in ((8, 720, 1280), (2, 2160, 3840)):
    say(f"## (a) the kernels on resident [{kb}, 3, {kh}, {kw}] fp32 tensors, behind a few ms of matrix products (device time alone)")
    say()
    x, x2 = pan(kb, kh, kw, -8, 24)
    y = torch.empty_like(x)
    nbytes = x.numel() * 4
    sa, sb = lib.align_signature_f32(x), lib.align_signature_f32(x2)
    say("| launch | algorithmic bytes | device time | rate | of the HBM peak (8 TB/s) | of the flip's rate |")
    say("|---|---|---|---|---|---|")
    v = device_time(lambda: lib.flip_f32(x, 0, out=y))
    flip = 2 * nbytes / (statistics.median(v) * 1e-3)
    say(f"| flip_f32, flip 0 (the reference streaming copy) | {2 * nbytes / 1e6:.1f} MB | {stats(v)} | {flip / 1e9:.0f} GB/s | {100.0 * flip / HBM_PEAK:.1f} % | 1.00 |")
    v = device_time(lambda: lib.align_signature_f32(x, out=sa))
    by = nbytes + sa.numel() * 2
    rate = by / (statistics.median(v) * 1e-3)
    say(f"| align_signature_f32 | {by / 1e6:.1f} MB | {stats(v)} | {rate / 1e9:.0f} GB/s | {100.0 * rate / HBM_PEAK:.1f} % | {rate / flip:.2f} |")
    for label, rec in (("halves multiples of 4: (8, -16) pixels", (8, -16)), ("halves even: (-4, 12) pixels", (-4, 12)), ("the zero record", (0, 0))):
        sh = torch.tensor([[rec[0], rec[1], 0, 0]] * kb, dtype=torch.int32, device=dev)
        v = device_time(lambda: lib.shift_f32(x, sh, 1, out=y))
        rate = 2 * nbytes / (statistics.median(v) * 1e-3)
        say(f"| shift_f32, {label} | {2 * nbytes / 1e6:.1f} MB | {stats(v)} | {rate / 1e9:.0f} GB/s | {100.0 * rate / HBM_PEAK:.1f} % | {rate / flip:.2f} |")
    for R_px in (64, 128):
        R = R_px // lib.ALIGN_CELL
        out = torch.empty(kb, 4, dtype=torch.int32, device=dev)
        v = device_time(lambda: lib.align_search(sa, sb, R, 512, out=out))
        diffs = kb * sa.shape[1] * sa.shape[2] * (2 * R + 1) ** 2
        say(f"| align_search, R = {R_px} pixels ({R} cells; clear + search + finish) -> {out[0, :2].tolist()} | {diffs / 1e6:.0f} M differences | {stats(v)} | "
            f"{diffs / (statistics.median(v) * 1e-3) / 1e9:.0f} G differences/s | | |")
    say()
    del x, x2, y, sa, sb

# ---------------------------------------------------------------- (b) the aligned step against the plain step
say(f"## (b) `model(a, b)` at B = {B} x {W} x {H}, bf16: aligned step against the plain step, alternating (a planted pan of (-8, 24) pixels)")
say()
ALIGNS = ((64, 0.5), (128, 0.5))
for _ in range(args.warmup):
    step(None)
    for al in ALIGNS:
        step(al)
torch.cuda.synchronize()
say("| align | shifts found | aligned step | plain step | overhead |")
say("|---|---|---|---|---|")
for al in ALIGNS:
    al_t, plain = [], []
    for _ in range(args.samples):
        al_t.append(timed(lambda: step(al)))
        plain.append(timed(lambda: step(None)))
    ma, mp = statistics.median(al_t), statistics.median(plain)
    found = sorted(set(tuple(r[:2]) for r in model.align_shifts.cpu().tolist()))
    say(f"| {al} | {found} | {stats(al_t)} | {stats(plain)} | {1e3 * (ma - mp):+.0f} us ({100.0 * (ma / mp - 1):+.2f} %) |")
say()
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
