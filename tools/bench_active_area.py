#!/usr/bin/env python3
"""What does running the forward on the active picture only buy, and what do its kernels cost (round 27)?  One process, one box:
  (a) the STEP: the forward alone on a batch of 8 pairs of 1280 x 720 bf16 against the same batch cut to its 1280 x 544 picture (a 2.35:1
      film in a 16:9 frame: 0.756 of the pixels), HIP events, warm-up, N interleaved samples; the expectation the ratio is held against is the
      pixel share itself.  Recorded, not gated.
  (b) the harness's PCIe-inclusive output rate, host frames in and out (`--pairs` pairs of 1280 x 720 yuv420p8 with black bars above and below
      a 1280 x 544 picture, factor 1, batch 8, bf16, copy_out=False, reference_quirks=False; the median of three runs of the stream): plain,
      with the explicit rectangle, with active_area="auto", alternating, `--rounds` times each.  `--parent DIR` (a built checkout of the parent
      commit) adds the parent's plain figure, measured by a child process of this script in the same call, in the same alternation.
  (c) emavfi_active_bounds on 9 resident frames of 1280 x 720 and emavfi_fill_outside_frames on 8 of them (rectangle 88, 0, 544, 1280), as
      bgr24, nv12 and p010: one call on an idle queue and ten calls behind a few ms of matrix products (device time alone), with the bytes
      the definition obliges - the image read once; the bars read and written once - and the rate on them.
  (d) the pre-pass of active_area="auto" alone: staging, upload, scan and its ONE host wait for the clip of (b), in milliseconds.
Nothing here is a gate.  Writes a markdown note (default profiles/r27_active_area.md)."""
import argparse, json, os, platform, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_active_area.md"))
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its plain harness rate and forward time go beside this tree's")
ap.add_argument("--tree", default=ROOT, help="the checkout whose emavfi package is measured (what --parent hands the child process)")
ap.add_argument("--plain-json", action="store_true", help="measure the plain harness rounds and the plain forward alone and print them as one JSON line")
args = ap.parse_args()
sys.path.insert(0, os.path.join(args.tree, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
H, W, RECT = 720, 1280, (88, 0, 544, 1280)
SHARE = RECT[2] * RECT[3] / float(H * W)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_clip(n):
    """n frames of 1280 x 720 yuv420p8: a moving natural picture in rows 88 .. 632, black bars (Y = 16) above and below, grey chroma"""
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    chroma = np.full((H // 2, W), 128, np.uint8)
    clip = []
    for i in range(n):
        y = np.ascontiguousarray(np.roll(u8[0][..., 1], 3 * i, axis=1))
        y = np.maximum(y, 17)                         # every sample of the picture is above black
        y[:RECT[0]] = 16
        y[RECT[0] + RECT[2]:] = 16
        clip.append(np.concatenate([y, chroma]))
    return clip


def forward_times(model, samples):
    """median ms of the forward alone on 8 pairs: {whole frame, the picture alone}, interleaved"""
    xs = {"plain": [torch.randn(8, 3, H, W, device=dev) for _ in range(2)], "cropped": [torch.randn(8, 3, RECT[2], RECT[3], device=dev) for _ in range(2)]}
    ts = {k: [] for k in xs}
    with torch.no_grad():
        for k, (a, b) in xs.items():
            for _ in range(3):
                model(a, b)
        torch.cuda.synchronize()
        for _ in range(samples):
            for k, (a, b) in xs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); model(a, b); e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1))
    return ts


def stream_rate(fi, clip):
    ts, n = [], 0
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = sum(1 for _ in fi.run(clip))
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return n / statistics.median(ts), n


model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0))
common = dict(batch_pairs=8, copy_out=False, reference_quirks=False, pixel_format="yuv420p8")
clip = make_clip(args.pairs + 1)

if args.plain_json:
    # the child process of --parent: one plain round per line read from stdin, so that the rounds of the two trees alternate
    fi = FrameInterpolator(model, **common)
    sum(1 for _ in fi.run(clip[:17]))
    fwd = forward_times(model, max(10, args.samples // 2))
    print(json.dumps({"forward_ms": {k: statistics.median(v) for k, v in fwd.items()}}), flush=True)
    for _ in sys.stdin:
        print(json.dumps({"rate": stream_rate(fi, clip)[0]}), flush=True)
    sys.exit(0)

try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
say("# The forward on the active picture only: the step, the harness and the kernels (tools/bench_active_area.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.  Parent commit of the tree measured: {commit}.")
say()
say(f"Command line: `python tools/bench_active_area.py --samples {args.samples} --pairs {args.pairs} --rounds {args.rounds}"
    + (" --parent <a built checkout of the parent commit>" if args.parent else "") + "`")
say()

child = None
if args.parent:
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--tree", args.parent, "--plain-json", "--pairs", str(args.pairs),
                              "--samples", str(args.samples)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    parent_fwd = json.loads(child.stdout.readline())["forward_ms"]

# ---------------------------------------------------------------- (a) the step
fwd = forward_times(model, max(20, args.samples))
say(f"## (a) The step: the forward alone, 8 pairs of {W} x {H} bf16 against the same batch cut to {RECT[3]} x {RECT[2]} (share {SHARE:.3f})")
say()
say(f"HIP events around one call of the model, 3 warm-up calls, {len(fwd['plain'])} interleaved samples.")
say()
say("| forward | ms per call: median | min | max | median, first half / second half |")
say("|---|---|---|---|---|")
for k, t in fwd.items():
    say(f"| {k} | {statistics.median(t):.3f} | {min(t):.3f} | {max(t):.3f} | {statistics.median(t[:len(t) // 2]):.3f} / {statistics.median(t[len(t) // 2:]):.3f} |")
if child is not None:
    say(f"| plain, the parent commit's tree (its own process, measured before this table) | {parent_fwd['plain']:.3f} | | | |")
ratio = statistics.median(fwd["cropped"]) / statistics.median(fwd["plain"])
say()
say(f"- cropped / plain = {ratio:.3f} against the pixel share {SHARE:.3f}: " + ("within share + 0.05." if ratio <= SHARE + 0.05 else
    "ABOVE share + 0.05: see the per-kernel list below."))
say()

# which launches do not scale: HIP events around every launch of the forward (the launch list names them), at both sizes
import ctypes
rt = lib.hip().rt
rt.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
rt.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
rt.hipEventDestroy.argtypes = [ctypes.c_void_p]


def per_launch_us(hw, steps=10):
    """{kernel name: mean us per forward, summed over its launches} of the bf16 forward on 8 pairs of hw, by events around every launch"""
    launches = lib.forward_launches(3, 64, 3, 8, hw[0], hw[1], "bf16")
    nl = len(launches)
    ev = (ctypes.c_void_p * (2 * nl))()
    for i in range(2 * nl):
        e = ctypes.c_void_p()
        if rt.hipEventCreate(ctypes.byref(e)) != 0:
            raise RuntimeError("hipEventCreate failed")
        ev[i] = e
    a, b = (torch.randn(8, 3, hw[0], hw[1], device=dev) for _ in range(2))
    agg = {}
    with torch.no_grad():
        model(a, b)
        for _ in range(steps):
            model(a, b, _events=(ctypes.cast(ev, ctypes.c_void_p), 2 * nl))
            torch.cuda.synchronize()
            for j, (name, _, _) in enumerate(launches):
                ms = ctypes.c_float()
                if rt.hipEventElapsedTime(ctypes.byref(ms), ev[2 * j], ev[2 * j + 1]) != 0:
                    raise RuntimeError("hipEventElapsedTime failed")
                agg[name.split(" ")[0]] = agg.get(name.split(" ")[0], 0.0) + ms.value * 1e3 / steps
    for e in ev:
        rt.hipEventDestroy(e)
    return agg


whole, cut = per_launch_us((H, W)), per_launch_us(RECT[2:])
say(f"Per kernel, the sum over its launches in one forward (HIP events around every launch, the mean of 10 forwards; a `*` marks a kernel "
    f"whose time shrinks by less than the share + 0.05 = {SHARE + 0.05:.3f} and takes at least 1 % of the plain forward):")
say()
say("| kernel | plain us | cropped us | cropped / plain | |")
say("|---|---|---|---|---|")
total = sum(whole.values())
for name, us in sorted(whole.items(), key=lambda kv: -kv[1]):
    c = cut.get(name, 0.0)
    say(f"| {name} | {us:.1f} | {c:.1f} | {c / us:.3f} | {'*' if (c / us > SHARE + 0.05 and us >= 0.01 * total) else ''} |")
say(f"| sum | {total:.1f} | {sum(cut.values()):.1f} | {sum(cut.values()) / total:.3f} | |")
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
fis = {"plain (active_area=None)": FrameInterpolator(model, **common),
       f"active_area={RECT}": FrameInterpolator(model, **common, active_area=RECT),
       'active_area="auto"': FrameInterpolator(model, **common, active_area="auto")}
rate, count = {k: [] for k in fis}, {}
parent_rate = []
for name, fi in fis.items():
    sum(1 for _ in fi.run(clip[:17]))                 # warm-up
for _ in range(args.rounds):
    for name, fi in fis.items():                      # alternating
        r, count[name] = stream_rate(fi, clip)
        rate[name].append(r)
    if child is not None:
        child.stdin.write("go\n"); child.stdin.flush()
        parent_rate.append(json.loads(child.stdout.readline())["rate"])
if child is not None:
    child.stdin.close()
    child.wait(timeout=60)
say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} yuv420p8, picture {RECT[3]} x {RECT[2]}, factor 1, batch 8, bf16, "
    f"copy_out=False; each figure the median of three runs of the stream, {args.rounds} alternating rounds)")
say()
say("| harness | output frames per run | rectangle in force | share | output frames/s: median of the rounds | min | max |")
say("|---|---|---|---|---|---|---|")
for name, fi in fis.items():
    r = rate[name]
    say(f"| {name} | {count[name]} | {fi.active_rect} | {fi.active_share:.3f} | {statistics.median(r):.1f} | {min(r):.1f} | {max(r):.1f} |")
if parent_rate:
    say(f"| plain, the parent commit's tree (its own process, same alternation) | | | | {statistics.median(parent_rate):.1f} | {min(parent_rate):.1f} | {max(parent_rate):.1f} |")
say()
base = statistics.median(rate["plain (active_area=None)"])
for name in list(fis)[1:]:
    say(f"- {name}: {statistics.median(rate[name]) / base:.3f} x the plain rate (1 / share = {1 / SHARE:.3f}).")
say()

# ---------------------------------------------------------------- (c) the kernels, resident frames
rng = np.random.default_rng(0)
kernels = {}
for fmt in ("bgr24", "nv12", "p010"):
    layout, C, sb, depth, shift = lib.static_frame_format(fmt)
    shape = (H, W, 3) if fmt == "bgr24" else (H * 3 // 2, W * sb)
    fb = int(np.prod(shape))
    frames = torch.from_numpy(rng.integers(0, 256, (9, *shape), dtype=np.uint8)).to(dev)
    d = torch.empty(8, *shape, dtype=torch.uint8, device=dev)
    bounds = torch.empty(9, 4, dtype=torch.int32, device=dev)
    img = frames if fmt == "bgr24" else (frames[:, :H].view(torch.int16) if sb == 2 else frames[:, :H].unsqueeze(-1))
    level = lib.active_level_units(0.0, depth, fmt != "bgr24", False)
    scanned = 9 * H * W * (3 if fmt == "bgr24" else sb)
    outside = fb - fb * RECT[2] // H                   # the bars' bytes of one frame: full rows in every plane
    kernels[f"{fmt}: active_bounds, 9 frames"] = (lambda i=img, l=level, dp=depth, s=shift, o=bounds: lib.active_bounds(i, l, depth=dp, shift=s, out=o),
                                                  float(scanned))
    kernels[f"{fmt}: fill_outside_frames, 8 frames"] = (
        lambda d=d, s=frames, f=(layout, C, sb): lib.fill_outside_frames(d, s, list(range(8)), (H, W), RECT, layout=f[0], C=f[1], sample_bytes=f[2]),
        float(2 * 8 * outside))
for name, (fn, _) in kernels.items():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times, full = {k: [] for k in kernels}, {k: [] for k in kernels}
for _ in range(max(20, args.samples)):
    for name, (fn, _) in kernels.items():     # interleaved
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)
REP = 10
plug = torch.randn(4096, 4096, device=dev)
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
for title, data in ((f"one call on an idle queue (HIP events around the call, 3 warm-up calls, {len(next(iter(times.values())))} interleaved samples; the "
                     "Python wrapper, the initialising launch and the launch latency are inside)", times),
                    (f"the queue kept full ({REP} calls enqueued behind a few ms of matrix products, so the events bracket device time alone; "
                     f"{len(next(iter(full.values())))} interleaved samples)", full)):
    say(f"## (c) Kernels on resident frames of {W} x {H}: {title}")
    say()
    say("| launch | us per call: median | min | max | MB moved (the definition's bytes) | TB/s | of 8.0 TB/s HBM peak |")
    say("|---|---|---|---|---|---|---|")
    for name, (_, nbytes) in kernels.items():
        t = data[name]
        m = statistics.median(t)
        say(f"| {name} | {m:.1f} | {min(t):.1f} | {max(t):.1f} | {nbytes / 1e6:.2f} | {nbytes / (m * 1e-6) / 1e12:.3f} | {100 * nbytes / (m * 1e-6) / HBM_PEAK:.1f} % |")
    say()

# ---------------------------------------------------------------- (d) the pre-pass alone
fi = fis['active_area="auto"']
frames = {i: f for i, f in enumerate(clip)}
fi._prepass(frames, 0, len(clip) - 1, False, True)
ts = []
for _ in range(max(5, args.rounds)):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    got = fi._prepass(frames, 0, len(clip) - 1, False, True)[2]
    ts.append((time.perf_counter() - t0) * 1e3)
say(f"## (d) The pre-pass of active_area=\"auto\" alone: {len(clip)} frames of {W} x {H} yuv420p8 staged, uploaded a second time, scanned, ONE host wait")
say()
say(f"- host clock around the pre-pass, which ends in its wait: median {statistics.median(ts):.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}) = "
    f"{statistics.median(ts) / len(clip):.3f} ms per frame, {len(clip) * H * W * 3 // 2 / 1e6:.1f} MB uploaded; rectangle found: "
    f"{lib.active_rect(got, H, W)}.")
say()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
