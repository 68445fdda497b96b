"""A/B of FrameInterpolator(numa="auto") against numa="off" on the PCIe-inclusive streaming leg (bench.py's also_stream_pcie: 64 pairs of
720p uint8 host frames, interpolation_factor 1, batch 8, uint8 host frames out).  Every measurement is a fresh process under its own
time limit; the modes alternate, `--rounds` times each.  Where the host has a second NUMA node, a third variant "far" runs numa="off"
in a process confined to that node's CPUs (as many as the plan has): the misplacement numa="auto" exists to prevent.  Prints frames/s
per process, the median and spread per variant, the plan, and on which NUMA nodes the pages of the mappings holding the harness's
pinned buffers sit (/proc/self/numa_maps, read only).  Stops at the first process that fails.

    python tools/numa_stream_ab.py [--rounds 3] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-frame-interpolation_amd"))


def pages_by_node(ptr):
    """(start, {node: pages}) of the mapping that holds address `ptr`, from /proc/self/maps + numa_maps (None: not found)."""
    start = None
    with open("/proc/self/maps") as f:
        for line in f:
            lo, hi = (int(x, 16) for x in line.split()[0].split("-"))
            if lo <= ptr < hi:
                start = lo
                break
    if start is None:
        return None
    with open("/proc/self/numa_maps") as f:
        for line in f:
            fields = line.split()
            if int(fields[0], 16) == start:
                return start, {k[1:]: int(v) for k, v in (x.split("=", 1) for x in fields[1:] if x[:1] == "N" and "=" in x)}
    return None


def child(mode, reps, cpus):
    if cpus:
        os.sched_setaffinity(0, cpus)      # "far": before torch starts a thread
    import numpy as np
    import torch
    if cpus:
        torch.set_num_threads(len(cpus))
    from emavfi import EMA_VFI, FrameInterpolator, synth
    dev = "cuda:0"
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    u8, _ = synth.synthetic_frames_u8(3, 1, 720, 1280, "natural")
    frames = [np.roll(u8[0], 3 * i, axis=1) for i in range(65)]
    fi = FrameInterpolator(model, interpolation_factor=1, batch_pairs=8, copy_out=False, numa=mode)
    sum(1 for _ in fi.run(frames[:25]))                      # warm-up: buffers, the half-size first batch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in fi.run(frames))
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    maps = dict(filter(None, (pages_by_node(slot[k].data_ptr()) for slot in fi._slots for k in ("h_in", "h_pred", "h_src"))))
    pages = {}
    for per_node in maps.values():
        for node, cnt in per_node.items():
            pages[node] = pages.get(node, 0) + cnt
    print(json.dumps({"numa": "far" if cpus else mode, "plan": fi.numa, "frames_out": n, "fps": [round(64 / t, 2) for t in ts],
                      "median_fps": round(64 / statistics.median(ts), 2), "pinned_pages_by_node": pages, "pinned_mappings": len(maps),
                      "process_cpus": len(os.sched_getaffinity(0))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("auto", "off"), default=None)
    ap.add_argument("--cpus", default="", help="child: confine the process to these CPUs first (comma list)")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, [int(c) for c in a.cpus.split(",") if c])
    from emavfi.dist import parse_cpulist
    rows, far = [], None
    for r in range(a.rounds):
        variants = ["auto", "off"] + (["far"] if far else [])
        for mode in (variants if r % 2 == 0 else variants[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "off" if mode == "far" else mode, "--reps", str(a.reps)]
            if mode == "far":
                cmd += ["--cpus", ",".join(map(str, far))]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"round {r} numa={mode}: timed out after {a.timeout} s; stopping", flush=True)
                return 1
            if p.returncode != 0:
                print(f"round {r} numa={mode}: exit {p.returncode}; stopping\n{p.stderr[-3000:]}", flush=True)
                return 1
            row = json.loads(p.stdout.strip().splitlines()[-1])
            row["round"] = r
            rows.append(row)
            plan = row["plan"]
            if far is None and mode == "auto" and plan["bind"]:   # another node's CPUs, as many as the plan binds to
                mask = os.sched_getaffinity(0)
                for node_dir in sorted(os.listdir("/sys/devices/system/node")):
                    if node_dir.startswith("node") and node_dir[4:].isdigit() and int(node_dir[4:]) != plan["numa_node"]:
                        with open(os.path.join("/sys/devices/system/node", node_dir, "cpulist")) as f:
                            other = [c for c in parse_cpulist(f.read()) if c in mask]
                        if len(other) >= len(plan["cpus"]):
                            far = other[:len(plan["cpus"])]
                            break
            print(f"round {r} numa={mode:4s}: {row['median_fps']:8.2f} interpolated frames/s (runs {row['fps']}), "
                  f"pinned pages by node {row['pinned_pages_by_node']}", flush=True)
    summary = {}
    for mode in ("auto", "off", "far"):
        med = [x["median_fps"] for x in rows if x["numa"] == mode]
        if not med:
            continue
        summary[mode] = {"median_fps_per_process": med, "median": round(statistics.median(med), 2),
                         "spread_pct": round(100 * (max(med) - min(med)) / statistics.median(med), 2)}
    summary["auto_over_off"] = round(summary["auto"]["median"] / summary["off"]["median"], 4)
    plan = next(x["plan"] for x in rows if x["numa"] == "auto")
    print(f"plan: {json.dumps(plan)}")
    print(f"numa=auto {summary['auto']['median']} (spread {summary['auto']['spread_pct']} %), numa=off {summary['off']['median']} "
          f"(spread {summary['off']['spread_pct']} %), auto/off = {summary['auto_over_off']}")
    if "far" in summary:
        summary["auto_over_far"] = round(summary["auto"]["median"] / summary["far"]["median"], 4)
        print(f"far (numa=off on CPUs {far[0]}..{far[-1]} of another node) {summary['far']['median']} (spread {summary['far']['spread_pct']} %), "
              f"auto/far = {summary['auto_over_far']}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"leg": "64 pairs 1280x720 uint8 host in/out, factor 1, batch 8, copy_out=False, bf16", "plan": plan,
                       "far_cpus": far, "summary": summary, "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
