#!/usr/bin/env python3
"""What does mixing in linear light cost (round 26)?  One process, one box:
  (a) emavfi_accumulate_frames_linear beside emavfi_accumulate_frames on resident 1280 x 720 frames, bgr24 (the whole frame in light) and
      nv12 (the Y plane in light, chroma coded), 8 output frames per call - one launch - at n = 5 taps per output (180 degrees at depth 3)
      and at n = 33.  With `--other-lib PATH` the coded entry of a second build of the library (the parent commit's, say) is timed in the
      same interleaved rounds through ctypes: the coded kernel before and after a change, same box, same session; the two trade places
      every other round, so that neither is always the first to run after another format's calls.  Every call reads frames
      of its own from a pool of 96 (above the Infinity Cache), as tools/bench_shutter.py does; HIP events around 10 calls enqueued behind a
      few ms of matrix products; `--samples` interleaved samples; median, min .. max and the median of either half of the samples.
  (b) the harness's PCIe-inclusive rate, host frames in and out (`--pairs` pairs of 720p bgr24, batch 8, bf16, copy_out=False; the median
      of three runs of the stream): shutter=180 at ratio 1 and depth 3 (4 forwards per pair) with light=None and with light="bt709",
      alternating, `--rounds` times each.
Nothing here is a gate.  Writes a markdown note (default profiles/r26_linear_light.md)."""
import argparse, ctypes, os, platform, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))
import numpy as np, torch
from emavfi import EMA_VFI, FrameInterpolator, lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_linear_light.md"))
ap.add_argument("--other-lib", default=None, help="a second build of libemavfi.so whose emavfi_accumulate_frames is timed in the same rounds")
ap.add_argument("--other-name", default="the parent commit's build")
ap.add_argument("--samples", type=int, default=30)
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--skip-harness", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12   # B/s, HBM3E specification of the MI355X
dev = torch.device("cuda:0")
H, W, N, POOL, REP = 720, 1280, 8, 96, 10
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say("# Linear light: the accumulation kernel in light beside the coded one, and the harness (tools/bench_linear_light.py)")
say()
say(f"Box: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, torch {torch.__version__}, "
    f"HIP {torch.version.hip}, {platform.machine()} host with {len(os.sched_getaffinity(0))} CPUs granted.")
say()

other = None
if args.other_lib:
    other = ctypes.CDLL(os.path.abspath(args.other_lib))
    other.emavfi_accumulate_frames.restype, other.emavfi_accumulate_frames.argtypes = lib._PROTOTYPES["emavfi_accumulate_frames"]


def other_accumulate(dst, srcs, nodes, table, sf):
    """emavfi_accumulate_frames of the second build: dense pools, no flags"""
    arr = (lib.AccumulateEntry * len(table))()
    for k, (taps, weights, f, h) in enumerate(table):
        arr[k].n, arr[k].f, arr[k].h = len(taps), f, h
        for i, (t, w) in enumerate(zip(taps, weights)):
            arr[k].tap[i], arr[k].w[i] = t, w
    fb = dst[0].numel()
    rc = other.emavfi_accumulate_frames(dst.data_ptr(), fb, len(table), srcs.data_ptr(), fb, srcs.shape[0], nodes.data_ptr(), fb, nodes.shape[0],
                                        ctypes.cast(arr, ctypes.c_void_p), None, 0, fb, *sf, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


# ---------------------------------------------------------------- (a) the kernels, resident frames
rng = np.random.default_rng(0)
cursor = 0


def walk(n):
    """the next N * n frames of the pool, as N tap lists"""
    global cursor
    taps = [[lib.RESAMPLE_NODES | ((cursor + k * n + i) % POOL) for i in range(n)] for k in range(N)]
    cursor = (cursor + N * n) % POOL
    return taps


def weights(n):
    return [1, 2] + [2] * (n - 3) + [1]


kernels, checks = {}, []
for fmt, shape, name, full in (("bgr24", (H, W, 3), "srgb", True), ("nv12", (H * 3 // 2, W), "bt709", False)):
    fb = int(np.prod(shape))
    lb = fb if fmt == "bgr24" else fb * 2 // 3
    one = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).to(dev)
    nodes = torch.stack([one.roll(k, 0) for k in range(POOL)])
    srcs, dst = nodes[:1], torch.empty(N, *shape, dtype=torch.uint8, device=dev)
    sf = lib.resample_sample_format(fmt)
    table = lib.transfer_table(name, 8, full)
    lib.transfer_table_check(table, 8)
    lin = torch.from_numpy(table.view(np.int32)).to(dev)
    for n in (5, 33):
        def coded(d=dst, s=srcs, p=nodes, sf=sf, n=n):
            lib.accumulate_frames(d, s, p, [(t, weights(n), 0, 0) for t in walk(n)], None, *sf)

        def linear(d=dst, s=srcs, p=nodes, sf=sf, n=n, lin=lin, lb=lb):
            lib.accumulate_frames_linear(d, s, p, [(t, weights(n), 0, 0) for t in walk(n)], lin, lb, None, *sf)

        kernels[f"{fmt} accumulate_frames, n = {n}"] = (coded, (n + 1.0) * N * fb)
        if other is not None:
            def coded_other(d=dst, s=srcs, p=nodes, sf=sf, n=n):
                other_accumulate(d, s, p, [(t, weights(n), 0, 0) for t in walk(n)], sf)
            kernels[f"{fmt} accumulate_frames of {args.other_name}, n = {n}"] = (coded_other, (n + 1.0) * N * fb)
        kernels[f"{fmt} accumulate_frames_linear ({name}, {lb * 100 // fb} % of the frame in light), n = {n}"] = (linear, (n + 1.0) * N * fb)
    if other is not None:      # the two builds compute the same bytes
        a, b = torch.empty_like(dst), torch.empty_like(dst)
        tab = [(t, weights(5), 0, 0) for t in walk(5)]
        lib.accumulate_frames(a, srcs, nodes, tab, None, *sf)
        other_accumulate(b, srcs, nodes, tab, sf)
        checks.append((fmt, bool(torch.equal(a, b))))
for fn, _ in kernels.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
plug = torch.randn(4096, 4096, device=dev)
times = {k: [] for k in kernels}
order = list(kernels)
swapped = list(order)
for i, name in enumerate(order):              # the two builds' coded entries trade places every other round: the first form timed after another
    if " of " in name and "_linear" not in name:   # format's calls finds colder caches, and neither build is to carry that alone
        swapped[i - 1], swapped[i] = order[i], order[i - 1]
for rnd in range(max(10, args.samples)):
    for name in (swapped if rnd & 1 else order):     # interleaved: every round times each form once
        fn = kernels[name][0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(6):
            plug @ plug
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / REP)
n_s = len(next(iter(times.values())))
say(f"## (a) The kernels on resident {W} x {H} frames, {N} output frames per call ({REP} calls behind a few ms of matrix products between two HIP "
    f"events: device time; 5 warm-up calls, {n_s} interleaved samples; every call reads the next frames of a pool of {POOL})")
say()
say("| launch | us per call: median | min | max | median, first half / second half | MB read + written (algorithmic) | GB/s | of 8.0 TB/s HBM peak |")
say("|---|---|---|---|---|---|---|---|")
med = {}
for name, (_, nbytes) in kernels.items():
    t = times[name]
    m = med[name] = statistics.median(t)
    h1, h2 = statistics.median(t[:len(t) // 2]), statistics.median(t[len(t) // 2:])
    say(f"| {name} | {m:.1f} | {min(t):.1f} | {max(t):.1f} | {h1:.1f} / {h2:.1f} | {nbytes / 1e6:.1f} | {nbytes / (m * 1e-6) / 1e9:.0f} | "
        f"{100 * nbytes / (m * 1e-6) / HBM_PEAK:.1f} % |")
say()
names = list(kernels)
for name in names:
    if "_linear" in name:
        base = name.split(" accumulate")[0] + " accumulate_frames, " + name.rsplit(", ", 1)[1]
        say(f"- {name}: {med[name] / med[base]:.2f} x the coded entry's time ({med[name]:.1f} against {med[base]:.1f} us).")
    elif " of " in name:
        base = name.split(" of ")[0] + ", " + name.rsplit(", ", 1)[1]
        t, u = times[base], times[name]
        say(f"- {base}: {med[base]:.1f} us in this build against {med[name]:.1f} us in {args.other_name} ({med[base] / med[name]:.3f} x); the samples "
            f"span {min(t):.1f} .. {max(t):.1f} and {min(u):.1f} .. {max(u):.1f} us.")
for fmt, ok in checks:
    say(f"- {fmt}: the coded entries of the two builds wrote {'the same bytes' if ok else 'DIFFERENT bytes'}.")
say()

# ---------------------------------------------------------------- (b) the harness, host frames in and out
if not args.skip_harness:
    u8, _ = synth.synthetic_frames_u8(3, 1, H, W, "natural")
    frames = [np.roll(u8[0], 3 * i, axis=1) for i in range(args.pairs + 1)]
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    common = dict(batch_pairs=8, copy_out=False, reference_quirks=False, mode="resample", rate_in=24, rate_out=24, shutter=180)
    fis = {"shutter 180, coded mean": FrameInterpolator(model, **common),
           "shutter 180, light=\"bt709\"": FrameInterpolator(model, light="bt709", **common)}
    secs = {k: [] for k in fis}

    def stream(fi):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sum(1 for _ in fi.run(frames))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    for fi in fis.values():
        sum(1 for _ in fi.run(frames[:17]))                   # warm-up
    for _ in range(args.rounds):
        for name, fi in fis.items():                          # alternating
            secs[name].append(stream(fi))
    say(f"## (b) Harness, host frames in and out ({args.pairs} pairs of {W} x {H} bgr24, batch 8, bf16, copy_out=False, 4 forwards per pair; each "
        f"figure the median of three runs of the stream, {args.rounds} alternating rounds)")
    say()
    say("| harness | source pairs/s: median of the rounds | min | max | ms per batch of 8 pairs at the median |")
    say("|---|---|---|---|---|")
    ms = {}
    for name in fis:
        r = [args.pairs / s for s in secs[name]]
        m = statistics.median(r)
        ms[name] = 8e3 / m
        say(f"| {name} | {m:.1f} | {min(r):.1f} | {max(r):.1f} | {ms[name]:.2f} |")
    say()
    a, b = ms["shutter 180, coded mean"], ms["shutter 180, light=\"bt709\""]
    say(f"The linear mix adds {b - a:+.3f} ms to a step of {a:.2f} ms ({100 * (b - a) / a:+.2f} %); the mix runs on the post lane beside the next "
        "batch's forwards, so what shows here is what it does not hide.")
    say()
say("## Not measured")
say()
say("Counters (LDS bank conflicts, achieved HBM traffic) were not collected: the fractions above are algorithmic bytes over event time.  The "
    "10- and 12-bit formats (a 4 / 16 KiB table per workgroup), other frame sizes, the blend's two taps, more than one GPU, and the "
    "idle-queue latency of a single call were not measured.  bench.py, the flagship measurement, does not run this path and is unchanged.")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
