#!/usr/bin/env python3
"""The adaptive pack route (EMA_VFI.pack_adapt, include/emavfi.h emavfi_forward_adaptive) against the two fixed policies, bf16 at
B = 8 x 720p by default, with every block's offset_conv rescaled to offsets of about +-s px (tools/route_spread.py's recipe).

  python tools/adaptive_route.py --out profiles/r08_adaptive_route.json
      whole forward per spread under pack_policy "window", "gather" and pack_adapt (0.75, 0.65) starting from the window: every model
      warmed up by three forwards (the adaptive one then runs in its steady state), the policies interleaved, median of --steps
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adaptive_route.py --kernel-run S --out DIR/kernel_run.json
      the launches a per-kernel timing needs at spread S: --steps forwards of each fixed policy and of the adaptive forward (started
      from the route it settles on, so that the routed kernel runs one body throughout); one rocprofv3 run per spread
  python tools/adaptive_route.py --merge S=DIR [S=DIR ...] --out profiles/r08_adaptive_route.json
      adds the median duration of the plain window pack, the plain gather kernel and the routed pack at each spread to the JSON
      (from the kernel trace of each run)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-frame-interpolation_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

ADAPT = (0.75, 0.65)
# kernel names as rocprofv3 reports them (it demangles the plain pack, garbling its __bf16 template argument)
KERNELS = {"window": r"deform_pack3_kernelIDF16bLb1E|^void deform_pack3_kernel<bool _Accum, bool, E>", "gather": r"deform_gather3_kernelIDF16bE",
           "routed": r"Route3IDF16bE"}


def scaled_state_dicts(dev, B, H, W, spreads):
    """{spread: state dict} with every block's offsets at about +-spread px (route_spread.forward_leg's sigma estimate)"""
    import torch
    from emavfi import EMA_VFI, lib, synth
    from route_spread import OFFCH, rescale
    sd = synth.synthetic_state_dict(seed=0)
    f1, f2 = synth.fast_frames(100, 1, H, W, device=dev)
    base = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    base.load_state_dict(sd, strict=True)
    with torch.no_grad():
        _, taps = base(f1, f2, return_taps=True)
    sig = []
    for i in range(3):
        xin = taps[f"fused_{i - 1}"] if i > 0 else torch.cat([taps["feat"], taps["warped"]], dim=1)
        w = sd[f"attention_blocks.{i}.offset_conv.weight"].to(dev)
        sig.append(lib.conv3x3(xin, w, torch.zeros(27, device=dev), dtype="fp32")[:, OFFCH].std().item())
    del taps, base
    out = {}
    for s in spreads:
        sdx = dict(sd)
        for i in range(3):
            sdx[f"attention_blocks.{i}.offset_conv.weight"], sdx[f"attention_blocks.{i}.offset_conv.bias"] = rescale(sd, i, s, sig[i])
        out[s] = sdx
    return out


def models(sd, dev, start="window"):
    from emavfi import EMA_VFI
    ms = {}
    for pol in ("window", "gather", "adaptive"):
        m = EMA_VFI(compute_dtype="bf16").to(dev).eval()
        m.load_state_dict(sd, strict=True)
        m.pack_policy = start if pol == "adaptive" else pol
        if pol == "adaptive":
            m.pack_adapt = ADAPT
        ms[pol] = m
    return ms


def forward_leg(dev, B, H, W, spreads, steps):
    import torch
    from emavfi import synth
    f1, f2 = synth.fast_frames(100, B, H, W, device=dev)
    rows = []
    for s, sd in scaled_state_dicts(dev, B, H, W, spreads).items():
        ms = models(sd, dev)
        t = {pol: [] for pol in ms}
        with torch.no_grad():
            for m in ms.values():
                for _ in range(3):
                    m(f1, f2)
            torch.cuda.synchronize()
            for _ in range(steps):
                for pol, m in ms.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    m(f1, f2)
                    b.record()
                    torch.cuda.synchronize()
                    t[pol].append(a.elapsed_time(b))
        row = {"spread_px": s}
        for pol in ms:
            row[f"{pol}_ms"] = round(statistics.median(t[pol]), 3)
            row[f"{pol}_ms_all"] = [round(x, 3) for x in t[pol]]
        row["adaptive_vs_window"] = round(row["adaptive_ms"] / row["window_ms"], 4)
        row["adaptive_vs_gather"] = round(row["adaptive_ms"] / row["gather_ms"], 4)
        row["routes"] = [r["ran"] for r in ms["adaptive"].pack_routes()]
        row["fixup_share"] = [round(r["fixup_share"], 4) for r in ms["adaptive"].pack_routes()]
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), file=sys.stderr, flush=True)
        rows.append(row)
        del ms
        torch.cuda.empty_cache()
    return {"dtype": "bf16", "pairs": B, "height": H, "width": W, "pack_adapt": list(ADAPT), "steps": steps, "rows": rows}


def kernel_run(dev, B, H, W, s, steps, out):
    import torch
    from emavfi import synth
    f1, f2 = synth.fast_frames(100, B, H, W, device=dev)
    sd = scaled_state_dicts(dev, B, H, W, [s])[s]
    probe = models(sd, dev)["adaptive"]
    with torch.no_grad():
        probe(f1, f2)
        probe(f1, f2)
    settled = probe.pack_routes()[1]["next"]
    del probe
    ms = models(sd, dev, start=settled)
    with torch.no_grad():
        for pol, m in ms.items():
            for _ in range(steps):
                m(f1, f2)
        torch.cuda.synchronize()
    res = {"spread_px": s, "routed_body": settled, "routes": [r["ran"] for r in ms["adaptive"].pack_routes()]}
    with open(out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


def merge(pairs, out, steps):
    """per-launch medians from the kernel trace: of each kernel, the last 3 * steps dispatches of the full batch (the timed forwards;
    the routed kernel's first ones belong to the probe that found the settled route, the small ones to the offset calibration)"""
    res = json.load(open(out)) if os.path.exists(out) else {}
    rows = []
    for pair in pairs:
        s, d = pair.split("=", 1)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"{d}: expected one kernel_trace.csv, found {files}")
        disp = {k: [] for k in KERNELS}
        for r in csv.DictReader(open(files[0])):
            for k, pat in KERNELS.items():
                if re.search(pat, r["Kernel_Name"]):
                    grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
                    disp[k].append((int(r["Start_Timestamp"]), grid, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
        row = {"spread_px": float(s)}
        for k, v in disp.items():
            if not v:
                continue
            v.sort()
            big = max(g for _, g, _ in v)
            t = [ms for _, g, ms in v if g == big][-3 * steps:]
            row[f"{k}_ms"] = round(statistics.median(t), 4)
            row[f"{k}_launches"] = len(t)
        body = json.load(open(os.path.join(d, "kernel_run.json")))["routed_body"]
        row["routed_body"] = body
        if "routed_ms" in row and f"{body}_ms" in row:
            row["routed_vs_plain"] = round(row["routed_ms"] / row[f"{body}_ms"], 4)
        rows.append(row)
    res["kernels"] = {"source": "rocprofv3 --kernel-trace, median per launch (one attention block) of the timed forwards", "rows": rows}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="adaptive_route.json")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--spreads", default="0,4,8,12,16,24")
    ap.add_argument("--kernel-run", type=float, default=None)
    ap.add_argument("--merge", nargs="*", default=None)
    a = ap.parse_args()
    if a.merge is not None:
        return merge(a.merge, a.out, a.steps)
    import torch
    dev = torch.device("cuda:0")
    if a.kernel_run is not None:
        return kernel_run(dev, a.B, a.H, a.W, a.kernel_run, a.steps, a.out)
    t0 = time.time()
    res = {"device": torch.cuda.get_device_name(0),
           "forward": forward_leg(dev, a.B, a.H, a.W, [float(s) for s in a.spreads.split(",")], a.steps)}
    res["seconds"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"seconds": res["seconds"]}))


if __name__ == "__main__":
    main()
