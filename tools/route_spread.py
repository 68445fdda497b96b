#!/usr/bin/env python3
"""Both routes of the one-launch ModulatedDeformConvPack over the offset spread (include/emavfi.h, EMAVFI_ROUTE_*).

  python tools/route_spread.py [--out profiles/r07_route_spread.json] [--B 8 --H 720 --W 1280] [--reps 5] [--steps 5]

Part 1 - one block: attention_blocks.1 on its real input (the second pack of a bf16 forward), f16 in / out as inside the forward,
run through lib.mdcn(..., route=...) with its offset_conv rescaled so that the offsets span about +-s px (bench.pack_vs_offset_spread's
recipe: weights to a standard deviation of s / 2, bias to U(+-s / 2)).  Both routes alternate in one process, `reps` event-timed
launches each, the median is reported with the kernel's own census (identical for both routes by construction).
Part 2 - the whole bf16 forward under pack_policy window / gather at the headline offsets and at +-8 / +-16 px (every block's
offset_conv rescaled with the same recipe), with the census' fix-up share per block.
Prints one JSON object and writes it to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "video-frame-interpolation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench import Hip  # noqa: E402
from emavfi import EMA_VFI, lib, synth  # noqa: E402

OFFCH = list(range(0, 9)) + list(range(18, 27))


def rescale(sd, i, s_px, sigma0):
    """offset_conv of block i rescaled to offsets of about +-s_px (bench.pack_vs_offset_spread's recipe)."""
    w = sd[f"attention_blocks.{i}.offset_conv.weight"].clone()
    b = sd[f"attention_blocks.{i}.offset_conv.bias"].clone()
    w[OFFCH] *= 0.5 * s_px / sigma0
    b[OFFCH] *= 0.5 * s_px
    return w, b


def block_leg(hip, sd, dev, B, H, W, spreads, reps):
    model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    model.load_state_dict(sd, strict=True)
    f1, f2 = synth.fast_frames(100, B, H, W, device=dev)
    with torch.no_grad():
        _, taps = model(f1, f2, return_taps=True)
    x = taps["fused_0"].clone()
    del taps, f1, f2, model
    torch.cuda.empty_cache()
    dw = sd["attention_blocks.1.dcn_v2.weight"].to(dev)
    db = sd["attention_blocks.1.dcn_v2.bias"].to(dev)
    ow0 = sd["attention_blocks.1.offset_conv.weight"].to(dev)
    raw0 = lib.conv3x3(x[:1], ow0, torch.zeros(27, device=dev), dtype="fp32")
    sigma0 = raw0[:, OFFCH].std().item()
    flags = lib.MDCN_IN_F16 | lib.MDCN_OUT_F16
    ev = hip.events(2)
    rows = []
    for s_px in spreads:
        ow, ob = (t.to(dev) for t in rescale(sd, 1, s_px, sigma0))
        times = {"window": [], "gather": []}
        census = {}
        for r in ("window", "gather"):
            lib.mdcn(x, ow, ob, dw, db, dtype="bf16", flags=flags, route=r)   # warm-up
        for _ in range(reps):
            for r in ("window", "gather"):
                lib.mdcn(x, ow, ob, dw, db, dtype="bf16", flags=flags, route=r, _events=(ctypes.cast(ev, ctypes.c_void_p), 2))
                torch.cuda.synchronize()
                times[r].append(hip.elapsed_ms(ev[0], ev[1]) * 1e3)
                census[r] = lib.mdcn_census(B, 67, H, W, dtype="bf16", flags=flags, device=dev)[0]
        row = {"spread_px": s_px}
        for r in ("window", "gather"):
            row[f"{r}_us"] = round(statistics.median(times[r]), 1)
            row[f"{r}_us_all"] = [round(t, 1) for t in times[r]]
        kc = census["window"]
        row["kernel_census"] = {"fixup_share": round(kc["fixup_share"], 5), "samples_outside_share": round(kc["samples_outside_share"], 6),
                                "abs_offset_px_max": round(kc["abs_offset_px_max"], 2)}
        row["census_identical"] = census["window"] == census["gather"]
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    hip.destroy(ev)
    return {"kernel": "attention_blocks.1 via emavfi_mdcn_routed, bf16, f16 in / out", "pairs": B, "height": H, "width": W, "rows": rows}


def forward_leg(sd, dev, B, H, W, spreads, steps):
    f1, f2 = synth.fast_frames(100, B, H, W, device=dev)
    base = EMA_VFI(compute_dtype="bf16").to(dev).eval()
    base.load_state_dict(sd, strict=True)
    with torch.no_grad():
        _, taps = base(f1[:1], f2[:1], return_taps=True)
    sig = []
    for i in range(3):
        xin = taps["fused_{}".format(i - 1)] if i > 0 else None
        if xin is None:   # block 0's input: feat + warped frame, rebuilt from the taps
            xin = torch.cat([taps["feat"], taps["warped"]], dim=1)
        w = sd[f"attention_blocks.{i}.offset_conv.weight"].to(dev)
        sig.append(lib.conv3x3(xin, w, torch.zeros(27, device=dev), dtype="fp32")[:, OFFCH].std().item())
    del taps, base
    rows = []
    for s_px in spreads:
        sdx = dict(sd)
        if s_px is not None:
            for i in range(3):
                sdx[f"attention_blocks.{i}.offset_conv.weight"], sdx[f"attention_blocks.{i}.offset_conv.bias"] = rescale(sd, i, s_px, sig[i])
        row = {"spread_px": "headline" if s_px is None else s_px}
        for pol in ("window", "gather"):
            m = EMA_VFI(compute_dtype="bf16").to(dev).eval()
            m.load_state_dict(sdx, strict=True)
            m.pack_policy = pol
            with torch.no_grad():
                for _ in range(3):          # warm-up
                    m(f1, f2)
                    torch.cuda.synchronize()
                t = []
                for _ in range(steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    m(f1, f2)
                    b.record()
                    torch.cuda.synchronize()
                    t.append(a.elapsed_time(b))
            row[f"{pol}_ms"] = round(statistics.median(t), 3)
            row["fixup_share"] = [round(r["fixup_share"], 4) if r else None for r in m.pack_census()]
            del m
            torch.cuda.empty_cache()
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    return {"dtype": "bf16", "pairs": B, "height": H, "width": W, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="route_spread.json")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--spreads", default="0,1,2,3,4,6,8,12,16")
    ap.add_argument("--skip-forward", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth.synthetic_state_dict(seed=0)
    hip = Hip()
    t0 = time.time()
    res = {"device": torch.cuda.get_device_name(0),
           "block": block_leg(hip, sd, dev, a.B, a.H, a.W, [float(s) for s in a.spreads.split(",")], a.reps)}
    if not a.skip_forward:
        res["forward"] = forward_leg(sd, dev, a.B, a.H, a.W, [None, 8.0, 16.0], a.steps)
    res["seconds"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
