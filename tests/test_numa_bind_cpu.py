"""NUMA placement of a rank's host work (emavfi.dist.numa_plan / bind_rank) on a fake sysfs tree, and the opt-in switches of
dist.init.  No GPU: the device properties are stand-ins."""
import json
import os
import socket
import subprocess
import sys
import types

import pytest
import torch

from emavfi import dist as vdist

PKG = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "video-frame-interpolation_amd"))

# device ordinal -> (PCI address, functions {function: (class, numa_node or None for no file)})
DEVICES = {
    0: ("0000:03:00", {0: ("0x120000", "0")}),
    1: ("0000:83:00", {0: ("0x038000", "1")}),
    2: ("0000:c1:00", {0: ("0x120000", "-1")}),
    3: ("0000:44:00", {0: ("0x040300", "0"), 1: ("0x120000", "1")}),   # an audio function first, the accelerator second
    4: ("0000:a0:00", {}),                                               # no function under sysfs at all
    5: ("0000:a1:00", {0: ("0x120000", None)}),                          # no numa_node file
    6: ("0000:a2:00", {0: ("0x120000", "2")}),                           # a node without a cpulist
}


def make_sysfs(root, nodes=None, quota=None, siblings=True):
    """nodes: {node: cpulist text}; siblings: cpu c and c + 8 share a core (c < 8)."""
    nodes = nodes if nodes is not None else {0: "0-3,8-11", 1: "4-7,12-15"}
    for dev, (pci, funcs) in DEVICES.items():
        for fn, (cls, node) in funcs.items():
            d = root / "bus" / "pci" / "devices" / f"{pci}.{fn}"
            d.mkdir(parents=True)
            (d / "class").write_text(cls + "\n")
            if node is not None:
                (d / "numa_node").write_text(node + "\n")
    for node, text in nodes.items():
        d = root / "devices" / "system" / "node" / f"node{node}"
        d.mkdir(parents=True)
        (d / "cpulist").write_text(text + "\n")
    if siblings:
        for c in range(16):
            d = root / "devices" / "system" / "cpu" / f"cpu{c}" / "topology"
            d.mkdir(parents=True)
            (d / "thread_siblings_list").write_text(f"{c % 8},{c % 8 + 8}\n")
    if quota is not None:
        d = root / "fs" / "cgroup"
        d.mkdir(parents=True)
        (d / "cpu.max").write_text(quota + "\n")
    return str(root)


def fake_props(index):
    if index not in DEVICES:
        raise RuntimeError(f"no device {index}")
    dom, bus, dev = (int(x, 16) for x in DEVICES[index][0].split(":"))
    return types.SimpleNamespace(pci_domain_id=dom, pci_bus_id=bus, pci_device_id=dev)


@pytest.fixture
def fake_gpus(monkeypatch):
    monkeypatch.setattr(torch.cuda, "get_device_properties", fake_props)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: len(DEVICES))
    for k in ("LOCAL_RANK", "LOCAL_WORLD_SIZE", "EMAVFI_CPU_THREADS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


ALL = set(range(16))


def test_parse_cpulist():
    assert vdist.parse_cpulist("0-23,96-119\n") == list(range(24)) + list(range(96, 120))
    assert vdist.parse_cpulist("5") == [5]
    assert vdist.parse_cpulist("") == [] and vdist.parse_cpulist("\n") == []
    assert vdist.parse_cpulist("7, 0-2,2") == [0, 1, 2, 7]


def test_node_selection_follows_the_pci_function(tmp_path, fake_gpus):
    sysfs = make_sysfs(tmp_path)
    p0 = vdist.numa_plan(0, sysfs, affinity=ALL)
    assert p0["pci"] == "0000:03:00" and p0["numa_node"] == 0 and p0["bind"]
    assert p0["cpus"] == [0, 1, 2, 3, 8, 9, 10, 11] and p0["device"] == 0
    p1 = vdist.numa_plan(torch.device("cuda", 1), sysfs, affinity=ALL)
    assert p1["numa_node"] == 1 and p1["cpus"] == [4, 5, 6, 7, 12, 13, 14, 15]
    # two functions at the address: the accelerator class wins over the audio function listed first
    p3 = vdist.numa_plan("cuda:3", sysfs, affinity=ALL)
    assert p3["numa_node"] == 1 and p3["bind"]
    assert set(p0) == {"device", "pci", "numa_node", "cpus", "reason", "bind"}


def test_intersection_with_the_affinity_mask(tmp_path, fake_gpus):
    sysfs = make_sysfs(tmp_path)
    p = vdist.numa_plan(0, sysfs, affinity={0, 2, 9, 5, 20})
    assert p["cpus"] == [0, 2, 9] and p["bind"]
    # empty intersection: the current mask, unchanged, and nothing to bind
    p = vdist.numa_plan(0, sysfs, affinity={4, 5, 20})
    assert p["numa_node"] == 0 and p["cpus"] == [4, 5, 20] and not p["bind"] and "mask kept" in p["reason"]


def test_quota_cap_prefers_one_thread_per_core(tmp_path, fake_gpus):
    sysfs = make_sysfs(tmp_path, quota="300000 100000")
    assert vdist.granted_cpu_threads(sysfs, ALL) == 3
    assert vdist.numa_plan(0, sysfs, affinity=ALL)["cpus"] == [0, 1, 2]
    fake_gpus.setenv("EMAVFI_CPU_THREADS", "2")
    assert vdist.granted_cpu_threads(sysfs, ALL) == 2
    assert vdist.numa_plan(1, sysfs, affinity=ALL)["cpus"] == [4, 5]
    fake_gpus.setenv("EMAVFI_CPU_THREADS", "6")
    assert vdist.numa_plan(1, make_sysfs(tmp_path / "q"), affinity=ALL)["cpus"] == [4, 5, 6, 7, 12, 13]   # four cores' first threads, then siblings


def test_granted_share_defaults(tmp_path, fake_gpus):
    assert vdist.granted_cpu_threads(make_sysfs(tmp_path / "a"), set(range(256))) == 16        # no cpu.max: the stated share
    assert vdist.granted_cpu_threads(make_sysfs(tmp_path / "b", quota="max 100000"), set(range(4))) == 4
    assert vdist.granted_cpu_threads(make_sysfs(tmp_path / "c", quota="garbage"), set(range(64))) == 16


def test_local_ranks_split_their_node(tmp_path, fake_gpus):
    sysfs = make_sysfs(tmp_path)
    # four local ranks on devices 0..3 (nodes 0, 1, none, 1): ranks 1 and 3 share node 1, rank 0 has node 0 alone
    fake_gpus.setenv("LOCAL_WORLD_SIZE", "4")
    plans = {}
    for r in (0, 1, 3):
        fake_gpus.setenv("LOCAL_RANK", str(r))
        plans[r] = vdist.numa_plan(r, sysfs, affinity=ALL)
    assert plans[0]["cpus"] == [0, 1, 2, 3, 8, 9, 10, 11]
    assert plans[1]["cpus"] == [4, 5, 12, 13] and plans[3]["cpus"] == [6, 7, 14, 15]
    assert not set(plans[1]["cpus"]) & set(plans[3]["cpus"])
    # every process sees one device (peers not visible): all local ranks count as peers of the node
    fake_gpus.setattr(torch.cuda, "device_count", lambda: 1)
    fake_gpus.setenv("LOCAL_WORLD_SIZE", "2")
    got = []
    for r in (0, 1):
        fake_gpus.setenv("LOCAL_RANK", str(r))
        got.append(vdist.numa_plan(0, sysfs, affinity=ALL)["cpus"])
    assert got == [[0, 1, 8, 9], [2, 3, 10, 11]]
    # without topology every CPU is its own core; the split stays disjoint and covers the node
    sysfs2 = make_sysfs(tmp_path / "flat", siblings=False)
    fake_gpus.setenv("LOCAL_WORLD_SIZE", "3")
    parts = []
    for r in range(3):
        fake_gpus.setenv("LOCAL_RANK", str(r))
        parts.append(vdist.numa_plan(0, sysfs2, affinity=ALL)["cpus"])
    assert sorted(sum(parts, [])) == [0, 1, 2, 3, 8, 9, 10, 11] and all(parts)


def test_no_numa_information_changes_nothing(tmp_path, fake_gpus):
    sysfs = make_sysfs(tmp_path)
    mask = {1, 4, 9}
    for dev, why in ((2, "-1 or missing"), (4, "-1 or missing"), (5, "-1 or missing"), (9, "not readable")):
        p = vdist.numa_plan(dev, sysfs, affinity=mask)
        assert p["numa_node"] is None and p["cpus"] == [1, 4, 9] and not p["bind"], p
        assert p["reason"].startswith("no NUMA information") and why in p["reason"], p
    p = vdist.numa_plan(6, sysfs, affinity=mask)
    assert p["numa_node"] == 2 and p["cpus"] == [1, 4, 9] and not p["bind"] and "no cpulist" in p["reason"]


def test_apply_false_never_changes_the_mask(tmp_path, fake_gpus):
    real = sorted(os.sched_getaffinity(0))
    half = max(1, len(real) // 2)
    sysfs = make_sysfs(tmp_path, nodes={0: ",".join(map(str, real[:half])), 1: ",".join(map(str, real[half:] or real))},
                       siblings=False)
    threads = torch.get_num_threads()
    for dev in (0, 1, 2, 4):
        plan = vdist.bind_rank(dev, sysfs, apply=False)
        assert sorted(os.sched_getaffinity(0)) == real and torch.get_num_threads() == threads
    assert plan == vdist.numa_plan(4, sysfs)


_CHILD = r"""
import json, os, sys, types
sys.path.insert(0, %(pkg)r)
import torch
from emavfi import dist as vdist
addr = {0: (0, 0x03, 0), 1: (0, 0x83, 0)}
torch.cuda.get_device_properties = lambda i: types.SimpleNamespace(pci_domain_id=addr[i][0], pci_bus_id=addr[i][1], pci_device_id=addr[i][2])
torch.cuda.device_count = lambda: 2
plan = vdist.bind_rank(1, %(sysfs)r)
print(json.dumps({"plan": plan, "mask": sorted(os.sched_getaffinity(0)), "threads": torch.get_num_threads()}))
"""


def test_bind_rank_applies_the_plan_in_a_fresh_process(tmp_path):
    real = sorted(os.sched_getaffinity(0))
    half = max(1, len(real) // 2)
    node1 = real[half:] or real
    sysfs = make_sysfs(tmp_path, nodes={0: ",".join(map(str, real[:half])), 1: ",".join(map(str, node1))}, siblings=False)
    env = {k: v for k, v in os.environ.items() if k not in ("LOCAL_RANK", "LOCAL_WORLD_SIZE", "EMAVFI_CPU_THREADS")}
    out = subprocess.run([sys.executable, "-c", _CHILD % {"pkg": PKG, "sysfs": sysfs}], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    plan = res["plan"]
    assert plan["numa_node"] == 1 and plan["bind"] and plan["cpus"] == node1[:16]
    assert res["mask"] == plan["cpus"] and res["threads"] == len(plan["cpus"])
    assert sorted(os.sched_getaffinity(0)) == real          # the parent's mask is untouched


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_init_switches(monkeypatch):
    """Default init at world size 1 creates no group and binds nothing; EMAVFI_NUMA_BIND=1 / bind=True call bind_rank first;
    single_rank_group=True creates a real one-rank group, through which the collectives then run (as the identity)."""
    import torch.distributed as tdist
    for k in ("RANK", "LOCAL_RANK", "EMAVFI_NUMA_BIND"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    calls = []
    monkeypatch.setattr(vdist, "bind_rank", lambda device, *a, **k: calls.append(device))
    assert not tdist.is_initialized()
    assert vdist.init("gloo") == (0, 1) and not tdist.is_initialized() and calls == []
    monkeypatch.setenv("EMAVFI_NUMA_BIND", "1")
    vdist.init("gloo")
    monkeypatch.delenv("EMAVFI_NUMA_BIND")
    vdist.init("gloo", "cuda:0", bind=True)
    assert calls == [0, "cuda:0"] and not tdist.is_initialized()
    seen = []
    real_broadcast = tdist.broadcast
    monkeypatch.setattr(tdist, "broadcast", lambda *a, **k: (seen.append("broadcast"), real_broadcast(*a, **k))[1])
    try:
        assert vdist.init("gloo", single_rank_group=True) == (0, 1)
        assert tdist.is_initialized() and tdist.get_world_size() == 1 and tdist.get_backend() == "gloo"
        blob = torch.arange(10, dtype=torch.uint8)
        assert vdist.broadcast_packed(blob) is blob and torch.equal(blob, torch.arange(10, dtype=torch.uint8))
        assert seen == ["broadcast"]
        assert vdist.max_over_ranks(2.5) == 2.5
        assert vdist.all_gather_floats([1, 2.5]) == [[1.0, 2.5]]
    finally:
        tdist.destroy_process_group()
