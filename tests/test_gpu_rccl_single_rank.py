"""RCCL on the MI355X at world size 1: a real one-rank "nccl" process group (dist.init(single_rank_group=True)) in a fresh child
process, the weight broadcast and the rank census through it, and a forward from the broadcast blob.  The N > 1 collectives of
the multi-GPU run take the same code path; what this cannot show is anything that needs a second device."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from emavfi import EMA_VFI, synth

pytestmark = pytest.mark.gpu

PKG = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "video-frame-interpolation_amd"))

_CHILD = r"""
import json, os, sys
sys.path[:0] = [%(pkg)r]
import numpy as np, torch
import torch.distributed as tdist
from emavfi import EMA_VFI, lib, synth, dist as vdist
bind = %(bind)r
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
plan = vdist.numa_plan(dev) if bind else None          # what binding will apply, computed before it does
vdist.init("nccl", dev, bind=bind, single_rank_group=True)
res = {"backend": tdist.get_backend(), "world": tdist.get_world_size(), "rank": tdist.get_rank(),
       "mask": sorted(os.sched_getaffinity(0)), "threads": torch.get_num_threads(), "plan": plan,
       "rccl": str(torch.cuda.nccl.version())}
model = EMA_VFI(compute_dtype="bf16").to(dev).eval()
model.load_state_dict(synth.synthetic_state_dict(seed=0))
blob = vdist.share_model_weights(model, "bf16", dev)     # rank 0 packs, RCCL broadcasts the blob
lib.packed_check(model.in_channels, model.mid_channels, model.num_blocks, lib.dtype_code("bf16"), blob)
res["packed_check"] = "ok"
res["blob_bytes"] = blob.numel()
res["gather"] = vdist.all_gather_floats([3.0, 1.25], dev)   # device tensors over RCCL
res["max"] = vdist.max_over_ranks(2.75, dev)
fresh = EMA_VFI(compute_dtype="bf16").to(dev).eval()    # its own random init; only the broadcast blob is installed
fresh.load_packed_weights("bf16", blob.clone())
f1, f2 = synth.synthetic_frames(91, 2, 256, 256, "natural")
with torch.no_grad():
    out = fresh(f1.to(dev), f2.to(dev))
np.save(%(out)r, out.cpu().numpy())
torch.cuda.synchronize()
tdist.destroy_process_group()
res["destroyed"] = not tdist.is_initialized()
print("RESULT " + json.dumps(res), flush=True)
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_child(tmp_path, bind):
    out = str(tmp_path / "frames.npy")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_WORLD_SIZE", "EMAVFI_NUMA_BIND")}
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    # one attempt, under its own limit: a failing or hanging child fails the test
    p = subprocess.run([sys.executable, "-c", _CHILD % {"pkg": PKG, "bind": bind, "out": out}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, p.stdout[-2000:]
    res = json.loads(line[-1][len("RESULT "):])
    print(json.dumps(res))
    return res, np.load(out)


def _plain_forward():
    """The same forward without any process group, in this process."""
    model = EMA_VFI(compute_dtype="bf16").to("cuda:0").eval()
    model.load_state_dict(synth.synthetic_state_dict(seed=0))
    f1, f2 = synth.synthetic_frames(91, 2, 256, 256, "natural")
    with torch.no_grad():
        return model(f1.to("cuda:0"), f2.to("cuda:0")).cpu().numpy()


def _check_collectives(res, got):
    assert res["backend"] == "nccl" and res["world"] == 1 and res["rank"] == 0   # RCCL really loaded
    assert res["packed_check"] == "ok" and res["blob_bytes"] > 0
    assert res["gather"] == [[3.0, 1.25]] and res["max"] == 2.75
    assert res["destroyed"]
    ref = _plain_forward()
    assert got.shape == ref.shape == (2, 3, 256, 256) and got.dtype == ref.dtype
    assert np.array_equal(got, ref)


def test_rccl_single_rank_group_broadcast_census_forward(tmp_path):
    res, got = _run_child(tmp_path, bind=False)
    assert res["plan"] is None and res["mask"] == sorted(os.sched_getaffinity(0))   # no binding asked for: mask inherited
    _check_collectives(res, got)


def test_rccl_single_rank_group_with_numa_binding(tmp_path):
    res, got = _run_child(tmp_path, bind=True)
    plan = res["plan"]
    assert plan["device"] == 0 and plan["pci"]
    if plan["bind"]:
        assert res["mask"] == plan["cpus"] and res["threads"] == len(plan["cpus"])
    else:       # no NUMA information on this host: binding changed nothing
        assert res["mask"] == plan["cpus"] == sorted(os.sched_getaffinity(0))
    _check_collectives(res, got)
