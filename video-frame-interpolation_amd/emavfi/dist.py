"""Multi-GPU host logic for the EMA-VFI path: one process per GPU, frame pairs sharded
contiguously, no collective inside the forward.

The reference has no distributed code at all (single process, single device; its ``warp`` even
hard-codes ``.cuda()``, ema_vfi.py:159-160).  What this module adds is exactly what
BASELINE.json asks for: ONE broadcast of the packed weight blob from rank 0 (RCCL over xGMI when
the backend is "nccl"; gloo in the CPU tests) and a max-over-ranks reduction of wall time for
the benchmark.  Every function works with any initialised torch.distributed backend and
degrades to a no-op in a process without a process group.

``numa_plan`` / ``bind_rank`` (opt-in) place a rank's host work on the CPUs of its GPU's NUMA node:
sysfs is only read, and the one thing ever changed is this process's own CPU mask.
"""
from __future__ import annotations

import glob
import os

import torch
import torch.distributed as dist


def env_rank_world():
    """(rank, world_size, local_rank) from the torchrun environment (defaults: single process)."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")),
            int(os.environ.get("LOCAL_RANK", "0")))


def init(backend: str, device=None, bind: bool = False, single_rank_group: bool = False):
    """Initialise torch.distributed from the torchrun environment; rendezvous on 127.0.0.1 unless
    MASTER_ADDR says otherwise (container hostnames may not resolve).

    Both switches are opt-in; with both off (and EMAVFI_NUMA_BIND unset) nothing changes: a single process
    returns before any process group exists.  ``bind=True`` or EMAVFI_NUMA_BIND=1: ``bind_rank(device)``
    first, i.e. before this rank's first pinned allocation.  ``single_rank_group=True``: create a real
    process group at WORLD_SIZE 1 too (a one-rank RCCL communicator; every collective here is then the
    identity, but goes through the backend)."""
    rank, world, local_rank = env_rank_world()
    if bind or os.environ.get("EMAVFI_NUMA_BIND", "0") == "1":
        bind_rank(device if device is not None else local_rank)
    if (world == 1 and not single_rank_group) or dist.is_initialized():
        return rank, world
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL on this driver
    kwargs = {"device_id": device} if (backend == "nccl" and device is not None) else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kwargs)
    return rank, world


def shard_range(n_items: int, rank: int, world: int):
    """Contiguous slice [lo, hi) of ``n_items`` frame pairs owned by ``rank``: sizes differ by at
    most one, earlier ranks take the remainder, every item belongs to exactly one rank."""
    if world < 1 or not (0 <= rank < world) or n_items < 0:
        raise ValueError(f"bad shard request: n_items={n_items} rank={rank} world={world}")
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def broadcast_packed(blob: torch.Tensor, src: int = 0) -> torch.Tensor:
    """The path's one collective: broadcast the packed weight blob (uint8) from ``src`` in place."""
    if dist.is_initialized():
        dist.broadcast(blob, src=src)
    return blob


def share_model_weights(model, dtype, device):
    """Rank 0 packs its parameters; every rank ends up with the identical packed blob installed.
    Returns the blob (for checks)."""
    from . import lib
    dt = lib.dtype_code(dtype)
    rank = dist.get_rank() if dist.is_initialized() else 0
    nbytes = lib.load().emavfi_packed_bytes(model.in_channels, model.mid_channels, model.num_blocks, dt)
    blob = model.packed_weights(dt, device) if rank == 0 else torch.empty(nbytes, dtype=torch.uint8, device=device)
    broadcast_packed(blob, 0)
    if rank != 0:
        model.load_packed_weights(dt, blob)
    return blob


def max_over_ranks(value: float, device=None) -> float:
    """MAX-reduce a host scalar (the benchmark's elapsed time) over all ranks."""
    if not dist.is_initialized():
        return float(value)
    on_cpu = device is None or dist.get_backend() == "gloo"
    t = torch.tensor([value], dtype=torch.float64, device="cpu" if on_cpu else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def all_gather_floats(values, device=None):
    """All-gather a short list of host floats over the initialised backend (device tensors over RCCL when it is "nccl"): one row
    per rank, in rank order.  bench.py's rank census - which ranks the collective backend actually saw, and each one's step time."""
    row = [float(v) for v in values]
    if not dist.is_initialized():
        return [row]
    on_cpu = device is None or dist.get_backend() == "gloo"
    t = torch.tensor(row, dtype=torch.float64, device="cpu" if on_cpu else device)
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [[float(x) for x in o.cpu()] for o in out]


def barrier():
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


# ---- NUMA placement of a rank's host work (opt-in: dist.init(bind=True), EMAVFI_NUMA_BIND=1, FrameInterpolator(numa="auto"))

def parse_cpulist(text: str):
    """Kernel cpulist syntax ("0-23,96-119", "5", "" for none) -> sorted list of CPU numbers."""
    cpus = set()
    for part in text.strip().split(","):
        part = part.strip()
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return sorted(cpus)


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def granted_cpu_threads(sysfs: str = "/sys", affinity=None) -> int:
    """The cores this process is granted: its affinity mask, capped by a cgroup v2 CPU quota ({sysfs}/fs/cgroup/cpu.max) and by
    the stated share of a one-GPU job (EMAVFI_CPU_THREADS, default 16).  The same rule as bench.py's helper of that name, which
    the library does not import."""
    granted = len(affinity if affinity is not None else os.sched_getaffinity(0))
    quota = (_read(os.path.join(sysfs, "fs", "cgroup", "cpu.max")) or "max").split()
    try:
        if quota[0] != "max":
            granted = min(granted, max(1, int(quota[0]) // int(quota[1])))
    except (IndexError, ValueError):
        pass
    return max(1, min(granted, int(os.environ.get("EMAVFI_CPU_THREADS", "16"))))


def _device_index(device) -> int:
    if isinstance(device, int):
        return device
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def _pci_function(index: int, sysfs: str):
    """(PCI address "DDDD:BB:DD", sysfs directory of the device's function or None).  The address comes from the runtime's device
    properties, so HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES renumbering is already applied."""
    p = torch.cuda.get_device_properties(index)
    pci = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}"
    funcs = sorted(glob.glob(os.path.join(sysfs, "bus", "pci", "devices", pci + ".*")))
    if len(funcs) > 1:   # several functions (e.g. an audio function beside the GPU): the display (0x03) / accelerator (0x12) class
        gpu = [f for f in funcs if (_read(os.path.join(f, "class")) or "")[:4].lower() in ("0x03", "0x12")]
        funcs = gpu or funcs
    return pci, (funcs[0] if funcs else None)


def _device_node(index: int, sysfs: str):
    """NUMA node of device ``index`` (None: unknown) and the PCI address it was found under."""
    try:
        pci, func = _pci_function(index, sysfs)
    except (RuntimeError, AssertionError, AttributeError, ValueError):
        return None, None
    node = _read(os.path.join(func, "numa_node")) if func else None
    try:
        node = int(node)
    except (TypeError, ValueError):
        node = -1
    return (node if node >= 0 else None), pci


def _cores(cpus, sysfs: str):
    """``cpus`` grouped into physical cores (hardware threads that share one: thread_siblings_list); one group per CPU where the
    topology is not readable.  Groups in order of their first CPU."""
    cores, seen, allowed = [], set(), set(cpus)
    for c in cpus:
        if c in seen:
            continue
        sib = _read(os.path.join(sysfs, "devices", "system", "cpu", f"cpu{c}", "topology", "thread_siblings_list"))
        group = [x for x in parse_cpulist(sib or "") if x in allowed and x not in seen]
        if c not in group:
            group = [c]
        seen.update(group)
        cores.append(group)
    return cores


def numa_plan(device, sysfs: str = "/sys", affinity=None) -> dict:
    """Where this rank's host work belongs: ``{device, pci, numa_node, cpus, reason, bind}``.  Reads sysfs, changes nothing.

    device -> PCI address (torch device properties) -> ``{sysfs}/bus/pci/devices/<address>.*/numa_node`` -> the node's cpulist,
    intersected with ``affinity`` (default: this process's mask).  Of that node's local ranks (LOCAL_RANK / LOCAL_WORLD_SIZE,
    local rank r on device r; when a peer's device is not visible here, every local rank counts as a peer) each takes a disjoint
    share of the node's physical cores, and this rank keeps at most ``granted_cpu_threads()`` of its share, primary threads first.
    No NUMA information (no device, no PCI function, numa_node -1 or missing, no cpulist) or an empty intersection: ``cpus`` is
    the current mask, unchanged, and ``bind`` is False - binding then changes nothing; ``reason`` says which case it was."""
    mask = sorted(affinity if affinity is not None else os.sched_getaffinity(0))
    try:
        index = _device_index(device)
    except (RuntimeError, AssertionError):
        index = None
    node, pci = _device_node(index, sysfs) if index is not None else (None, None)
    plan = {"device": index, "pci": pci, "numa_node": node, "cpus": mask, "reason": "", "bind": False}
    if pci is None:
        plan["reason"] = "no NUMA information: device properties not readable"
        return plan
    if node is None:
        plan["reason"] = f"no NUMA information: numa_node of PCI {pci} is -1 or missing"
        return plan
    listed = _read(os.path.join(sysfs, "devices", "system", "node", f"node{node}", "cpulist"))
    allowed = set(mask)
    local = [c for c in parse_cpulist(listed or "") if c in allowed]
    if not local:
        plan["reason"] = (f"node {node}: no cpulist" if listed is None else f"node {node}: no CPU of the node in the affinity mask") \
            + "; current mask kept"
        return plan
    _, _, local_rank = env_rank_world()
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    try:
        visible = torch.cuda.device_count()
    except RuntimeError:
        visible = 0
    if local_world > visible:
        peers = list(range(local_world))
    else:
        peers = [r for r in range(local_world) if r == local_rank or _device_node(r, sysfs)[0] == node]
    if local_rank not in peers:
        peers = sorted(peers + [local_rank])
    cores = _cores(local, sysfs)
    slot, n = peers.index(local_rank), len(peers)
    if len(cores) < n:
        plan["reason"] = f"node {node}: {len(cores)} cores for {n} local ranks; current mask kept"
        return plan
    mine = cores[slot * len(cores) // n:(slot + 1) * len(cores) // n]
    ordered = [g[d] for d in range(max(map(len, mine))) for g in mine if d < len(g)]   # first threads of every core, then second
    cap = granted_cpu_threads(sysfs, mask)
    plan["cpus"] = sorted(ordered[:cap])
    plan["bind"] = True
    plan["reason"] = (f"node {node}: local rank {local_rank} takes core share {slot + 1}/{n} of {len(cores)} cores, "
                      f"{len(plan['cpus'])} CPUs (cap {cap})")
    return plan


def bind_rank(device, sysfs: str = "/sys", apply: bool = True) -> dict:
    """Pin this process to its GPU's NUMA node: ``numa_plan(device, sysfs)``, then (``apply`` and a node-local plan)
    ``os.sched_setaffinity(0, cpus)`` and ``torch.set_num_threads(len(cpus))``.  Returns the plan.

    Call it BEFORE the first pinned host allocation and before any thread pool starts: threads created later inherit the
    mask and pages are placed by the CPU that first touches them; what already exists stays where it is.  ``apply=False``
    computes the plan only.  Nothing is written under /sys or /proc; the only change is this process's own CPU mask."""
    plan = numa_plan(device, sysfs)
    if apply and plan["bind"]:
        os.sched_setaffinity(0, plan["cpus"])
        torch.set_num_threads(len(plan["cpus"]))
    return plan
