#!/usr/bin/env python3
"""What does holding static regions on the device cost (round 19)?  One process, one box:
  (a) emavfi_static_guard_frames on 8 resident prediction frames against 9 resident source frames (pair k = frames k, k + 1) of 1280 x 720
      and of 1920 x 1080, as bgr24, nv12 and p010, at radius 0, 4 and 16, with NOTHING static (the sources are unrelated noise: every
      comparison fails, nothing is stored) and with EVERYTHING static (frame k + 1 is frame k: every sample of d is replaced), beside
      emavfi_hold_frames_u8 over the same 8 frames (every pair flagged: a plain copy, the rate to compare with) and the format's postprocess
      kernel over the 8 predictions, in the same run.  HIP events, warm-up, N >= 20 interleaved samples; median, min .. max and the median's
      shift between the two halves of the samples.  Each launch is timed twice: one call on an idle queue (wrapper, the count-clearing launch
      and launch latency included), and ten calls behind a few ms of matrix products (device time alone).  The rate is on the bytes the
      DEFINITION obliges: a and b read once, d written where core - the halo a tile reads beyond itself and the second read of a's tile
      ahead of the stores are not counted, so they show as a lower rate.
  (b) the harness's PCIe-inclusive output rate, host frames in and out (`--pairs` pairs of 1280 x 720 yuv420p8, factor 1, batch 8, bf16,
      copy_out=False, reference_quirks=False; the median of three runs of the stream): static_guard off against static_guard=4 on a clip with
      letterbox bars, alternating, `--rounds` times each.  Recorded, not gated.
`--pmc-run` launches the r = 4 cases alone, for a counter run.  Nothing here is a gate.  Writes a markdown note (default profiles/r19_static_guard.md, section by section; --append keeps what the file holds)."""
import argparse, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, formats, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_static_guard.md"))
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
ap.add_argument("--pmc-run", action="store_true", help="only launch the r = 4 guard cases and the hold copy five times each and leave: the "
                "workload of a counter run (rocprofv3 --pmc ... -- python tools/bench_static.py --pmc-run); writes no note")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
N = 8
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# Static regions held on the device: kernel rates and harness cost (tools/bench_static.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_static.py --samples {args.samples} --pairs {args.pairs} --rounds {args.rounds}"
    + (" --skip-harness" if args.skip_harness else "") + "`")
say()

# ---------------------------------------------------------------- (a) kernels, resident frames
rng = np.random.default_rng(0)
kernels = {}
for H, W in ((720, 1280), (1080, 1920)):
    x = torch.rand(N, 3, H, W, device=dev)
    for fmt in ("bgr24", "nv12", "p010"):
        layout, C, sb, depth, shift = lib.static_frame_format(fmt)
        shape = (H, W, 3) if fmt == "bgr24" else (H * 3 // 2, W * sb)
        fb = int(np.prod(shape))
        tag = f"{W} x {H} {fmt}"
        noise = torch.from_numpy(rng.integers(0, 256, (N + 1, *shape), dtype=np.uint8)).to(dev)
        still = noise[:1].expand(N + 1, *shape).contiguous()
        d = torch.empty(N, *shape, dtype=torch.uint8, device=dev)
        counts = torch.zeros(N, dtype=torch.int32, device=dev)
        flags = torch.ones(N, dtype=torch.int32, device=dev)
        table = [(k, k + 1) for k in range(N)]
        for what, srcs, wr in (("nothing static", noise, 0), ("everything static", still, 1)):
            for r in (0, 4, 16):
                kernels[f"{tag}: static_guard_frames, r = {r}, {what}"] = (
                    lambda d=d, s=srcs, r=r, c=counts, f=(layout, C, sb, depth, shift), hw=(H, W), table=table: lib.static_guard_frames(
                        d, s, table, hw, layout=f[0], C=f[1], sample_bytes=f[2], depth=f[3], shift=f[4], radius=r, tol=0, counts=c),
                    float((2 + wr) * N * fb))
        kernels[f"{tag}: hold_frames_u8, 8 frames copied"] = (lambda d=d, s=noise, f=flags: lib.hold_frames_u8(d, s[:N], f), float(2 * N * fb))
        if fmt == "bgr24":
            post = lambda x=x, d=d: lib.postprocess_u8(x, denormalize=False, out=d)
        elif fmt == "nv12":
            post = lambda x=x, d=d: lib.postprocess_nv12(x, denormalize=False, out=formats.FORMATS["nv12"].planes(d))
        else:
            post = lambda x=x, d=d: lib.postprocess_p010(x, 10, denormalize=False, out=formats.FORMATS["p010"].planes(d))
        kernels[f"{tag}: postprocess, 8 frames"] = (post, float(N * (12 * H * W + fb)))
if args.pmc_run:
    for name, (fn, _) in kernels.items():
        if "r = 4" in name or "hold_frames" in name:
            for _ in range(5):
                fn()
    torch.cuda.synchronize()
    sys.exit(0)
times = {k: [] for k in kernels}
for name, (fn, _) in kernels.items():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
for _ in range(max(20, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved: every round times each form once
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
# the same launches with the queue kept full: a few ms of matrix products go first, so the host enqueues REP calls while the device is still
# busy and the events bracket device time alone - no wrapper, no launch latency of an idle queue
REP = 10
plug = torch.randn(4096, 4096, device=dev)
full = {k: [] for k in kernels}
for _ in range(max(10, args.samples // 2)):
    for name, (fn, _) in kernels.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(4):
            plug @ plug
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        e1.synchronize()
        full[name].append(e0.elapsed_time(e1) * 1e3 / REP)
med, fmed = {}, {}
for title, data, store in ((f"one call on an idle queue (HIP events around the call, 3 warm-up calls, {len(next(iter(times.values())))} interleaved samples; "
                            "the Python wrapper, the count-clearing launch and the launch latency are inside)", times, med),
                           (f"the queue kept full ({REP} calls enqueued behind a few ms of matrix products, so the events bracket device time alone; "
                            f"{len(next(iter(full.values())))} interleaved samples)", full, fmed)):
    say(f"## (a) Kernels on {N} resident frames: {title}")
    say()
    say("| launch | us per call: median | min | max | median, first half / second half | MB the definition obliges | GB/s | of 8.0 TB/s HBM peak |")
    say("|---|---|---|---|---|---|---|---|")
    for name, (_, nbytes) in kernels.items():
        t = data[name]
        store[name] = statistics.median(t)
        h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
        bw = nbytes / (store[name] * 1e-6)
        say(f"| {name} | {store[name]:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % |")
    say()
say("## (a) The guard at r = 4 beside the hold kernel's copy, bytes per second (queue kept full)")
say()
for tag in [k.split(":")[0] for k in kernels if "hold_frames_u8" in k]:
    hold_t, hold_b = fmed[f"{tag}: hold_frames_u8, 8 frames copied"], kernels[f"{tag}: hold_frames_u8, 8 frames copied"][1]
    for what in ("nothing static", "everything static"):
        name = f"{tag}: static_guard_frames, r = 4, {what}"
        ratio = (kernels[name][1] / fmed[name]) / (hold_b / hold_t)
        say(f"- {tag}, {what}: {kernels[name][1] / fmed[name] / 1e3:.0f} GB/s against the copy's {hold_b / hold_t / 1e3:.0f} GB/s: {ratio:.2f} x"
            + ("  (below half: see the note's explanation)" if ratio < 0.5 else ""))
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
if not args.skip_harness:
    H, W = 720, 1280
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    chroma = np.full((H // 2, W), 128, np.uint8)
    clip = []
    for i in range(args.pairs + 1):
        y = np.ascontiguousarray(np.roll(u8[0][..., 1], 3 * i, axis=1))
        y[:90] = 16
        y[-90:] = 16                              # letterbox bars: 25 % of the frame is static
        clip.append(np.concatenate([y, chroma]))
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    common = dict(batch_pairs=8, copy_out=False, reference_quirks=False, pixel_format="yuv420p8")
    fis = {"static_guard off (the path before this change)": FrameInterpolator(model, **common),
           "static_guard=4": FrameInterpolator(model, **common, static_guard=4)}
    rate, count = {k: [] for k in fis}, {}

    def stream(name):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            count[name] = sum(1 for _ in fis[name].run(clip))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return count[name] / statistics.median(ts)

    for name in fis:
        sum(1 for _ in fis[name].run(clip[:17]))     # warm-up
    for _ in range(args.rounds):
        for name in fis:                              # alternating
            rate[name].append(stream(name))
    say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} yuv420p8 with letterbox bars, factor 1, batch 8, bf16, copy_out=False; each "
        f"figure the median of three runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | output frames per run | mean held share | output frames/s: median of the rounds | min | max |")
    say("|---|---|---|---|---|---|")
    for name, fi in fis.items():
        r = rate[name]
        share = f"{100 * sum(fi.static_share) / len(fi.static_share):.1f} %" if fi.static_share else "-"
        say(f"| {name} | {count[name]} | {share} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} |")
    say()
    off, on = rate["static_guard off (the path before this change)"], rate["static_guard=4"]
    diff, spread = statistics.median(on) - statistics.median(off), max(off) - min(off)
    say(f"- guard on minus off: {diff:+.1f} output frames/s ({100 * diff / statistics.median(off):+.2f} %); spread of the off rounds (max - min): "
        f"{spread:.1f} frames/s.  " + ("The on rate lies inside that spread: no cost resolved." if min(off) <= statistics.median(on) <= max(off)
        else "That is the price of one guard launch per batch on the post lane.") + "  Recorded, not gated.")
say()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
