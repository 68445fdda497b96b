"""Guard-banded, poisoned memory for the compute entries (tests/test_gpu_workspace.py).  A plain module: no fixture, no pytest setting.

What it builds:
  * guarded(nbytes, fill, guard_fill): one flat uint8 allocation [guard | rup256(nbytes) | guard] and the exact-size view of its body.
    The body holds `fill`; the guards AND the round-up slack behind the body hold `guard_fill`.  guard = 4096 keeps the 16-byte
    alignment the entries demand (torch allocates at 256-byte boundaries or better).
  * guarded_like(t, guard_fill): the same around a copy of an input tensor, or around an output pre-filled with a sentinel byte.
  * exact_workspace(monkeypatch, fill, guard_fill): replaces emavfi.lib.workspace, so every wrapper (they all call it as a module
    attribute) hands the C-ABI a workspace of EXACTLY the bytes the entry asked for, with chosen prior contents.
  * guarded_outputs(monkeypatch, guard_fill): while it is in force every device tensor the wrappers allocate with torch.empty /
    torch.empty_like (their outputs and taps, the route state of an adaptive forward) lies between guards and is pre-filled with
    the sentinel byte, so an element the entry never wrote is seen.
  * run_case(...): the one statement of tests/test_gpu_workspace.py, made about a callable.

Fill patterns: 0x00; 0xFF (NaN as f16, bf16 and fp32, 0xFFFFFFFF as a counter); 0x7B (finite and huge in all three types: about 6.1e4
as f16, 1.3e36 as bf16 / fp32 - seen wherever a weight is small rather than zero).  The guards of a run never hold the body's
pattern, so a read that strays into a guard changes the result even where a stray into the body would not."""
import contextlib

import pytest
import torch

from emavfi import lib

GUARD = 4096
FILLS = (0x00, 0xFF, 0x7B)
GUARD_OF = {0x00: 0x7B, 0xFF: 0x00, 0x7B: 0xFF}   # the guards' pattern under each body fill: never the same
SENTINEL = 0xCB                                   # outputs before the call: 0xCBCBCBCB is -2.67e7 as fp32, finite and improbable
DEV = "cuda:0"


def rup256(n):
    return (int(n) + 255) // 256 * 256


def guarded(nbytes, fill, guard_fill, guard=GUARD, device=DEV):
    """(flat, view): flat uint8 [guard + rup256(nbytes) + guard], view = flat[guard : guard + nbytes]"""
    nbytes = int(nbytes)
    flat = torch.full((guard + rup256(nbytes) + guard,), guard_fill, dtype=torch.uint8, device=device)
    view = flat[guard:guard + nbytes]
    view.fill_(fill)
    return flat, view


def assert_guards(flat, nbytes, guard_fill, guard=GUARD, what="buffer"):
    """both guards (and the round-up slack behind the body) still hold guard_fill, byte for byte"""
    for name, part, base in (("in front of", flat[:guard], 0), ("behind", flat[guard + int(nbytes):], guard + int(nbytes))):
        bad = (part != guard_fill).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} bytes {name} the {int(nbytes)} bytes handed out were written; the first at byte "
                                  f"{int(bad[0]) + base - guard} relative to the body")


def guarded_like(t, guard_fill, fill=None, guard=GUARD, device=None):
    """(flat, view): a tensor of t's shape and dtype between guards - a copy of t (fill None), or every byte `fill` (an output)"""
    nbytes = t.numel() * t.element_size()
    flat, body = guarded(nbytes, 0 if fill is None else fill, guard_fill, guard, device if device is not None else (t.device if t.is_cuda else DEV))
    view = body.view(t.dtype).view(t.shape)
    if fill is None:
        view.copy_(t)
    return flat, view


def bits(t):
    """a tensor's elements as integers of the same width, flat"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).flatten()


def first_difference(a, b):
    """None where a and b agree bit for bit, else a description of the first element that does not"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes / types differ: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    ne = (bits(a) != bits(b)).nonzero()
    if ne.numel() == 0:
        return None
    i = int(ne[0])
    return f"{ne.shape[0]} of {a.numel()} elements differ, the first at flat index {i}: {a.flatten()[i].item()!r} against {b.flatten()[i].item()!r}"


class ExactWorkspace:
    """What exact_workspace() puts in lib.workspace's place.  One buffer per (device, stream), as lib.workspace keeps them: the same key
    gets the same buffer when asked for no more than before (EMA_VFI.pack_census compares data_ptr() with the last forward's).
    `short`: hand out that many bytes fewer than asked for (the entries must then refuse)."""

    def __init__(self, fill, guard_fill, short=0):
        self.fill, self.guard_fill, self.short = fill, guard_fill, short
        self.by_key = {}
        self.handed = []   # (flat, bytes handed out, bytes asked for)

    def __call__(self, nbytes, device):
        device = torch.device(device)
        index = device.index if device.index is not None else torch.cuda.current_device()
        key = (index, torch.cuda.current_stream(device).cuda_stream)
        hit = self.by_key.get(key)
        if hit is not None and nbytes <= hit[1]:
            return hit[0][:nbytes - self.short]   # the same data_ptr(), and never more bytes than this request's
        flat, view = guarded(nbytes - self.short, self.fill, self.guard_fill, device=torch.device("cuda", index))
        self.by_key[key] = (view, nbytes)
        self.handed.append((flat, nbytes - self.short, nbytes))
        return view

    def check_guards(self, what):
        for flat, n, _ in self.handed:
            assert_guards(flat, n, self.guard_fill, what=f"{what}: workspace")


def exact_workspace(monkeypatch, fill, guard_fill, short=0):
    ws = ExactWorkspace(fill, guard_fill, short)
    monkeypatch.setattr(lib, "workspace", ws)
    return ws


class GuardedOutputs:
    """torch.empty / torch.empty_like for device tensors while guarded_outputs() is in force"""

    def __init__(self, guard_fill, sentinel=SENTINEL):
        self.guard_fill, self.sentinel = guard_fill, sentinel
        self.made = []   # (flat, view)
        self._empty, self._empty_like = torch.empty, torch.empty_like

    def _make(self, shape, dtype, device):
        like = self._empty(tuple(shape), dtype=dtype, device="meta")
        flat, view = guarded_like(like, self.guard_fill, fill=self.sentinel, device=device)
        self.made.append((flat, view))
        return view

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if device is None or torch.device(device).type != "cuda" or kw:
            return self._empty(*size, dtype=dtype, device=device, **kw)
        return self._make(size, dtype if dtype is not None else torch.get_default_dtype(), torch.device(device))

    def empty_like(self, t, **kw):
        if not t.is_cuda or kw or not t.is_contiguous():
            return self._empty_like(t, **kw)
        return self._make(t.shape, t.dtype, t.device)

    def check(self, what, finite=True):
        """guards intact; no element still holds the sentinel; floating-point outputs finite"""
        for k, (flat, view) in enumerate(self.made):
            name = f"{what}: output {k} {tuple(view.shape)} {view.dtype}"
            assert_guards(flat, view.numel() * view.element_size(), self.guard_fill, what=name)
            left = (view.contiguous().view(torch.uint8).view(-1, view.element_size()) == self.sentinel).all(dim=1).nonzero()
            assert left.numel() == 0, f"{name}: {left.shape[0]} elements were never written, the first at flat index {int(left[0])}"
            if finite and view.is_floating_point():
                bad = (~torch.isfinite(view)).flatten().nonzero()
                assert bad.numel() == 0, f"{name}: {bad.shape[0]} elements are not finite, the first at flat index {int(bad[0])}"


def guarded_outputs(monkeypatch, guard_fill, sentinel=SENTINEL):
    g = GuardedOutputs(guard_fill, sentinel)
    monkeypatch.setattr(torch, "empty", g.empty)
    monkeypatch.setattr(torch, "empty_like", g.empty_like)
    return g


def _snapshot(result):
    """the call's result as {name: tensor clone | plain value}"""
    if torch.is_tensor(result):
        result = {"out": result}
    return {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in result.items()}


def _compare(label, a_name, a, b_name, b, verdict):
    assert a.keys() == b.keys(), (label, sorted(a), sorted(b))
    for k in a:
        if torch.is_tensor(a[k]):
            d = first_difference(a[k], b[k])
        else:
            d = None if repr(a[k]) == repr(b[k]) else f"{a[k]!r} against {b[k]!r}"
        assert d is None, f"{label}: {verdict}: `{k}` under {a_name} against {b_name}: {d}"


def run_case(monkeypatch, label, call, inputs, has_workspace=True):
    """The statement of tests/test_gpu_workspace.py about call(list of device tensors) -> tensor | {name: tensor or plain value}:
    the entry run in a workspace of exactly the bytes it asked for, under each fill, on guarded inputs and into guarded,
    sentinel-filled outputs, gives bit for bit what it gives through the ordinary cached workspace; every guard is unchanged; every
    output element is written and finite; a workspace one byte short is refused with EMAVFI_E_WORKSPACE (-3).  The 0x00 run is made
    twice first: a case that differs from itself fails as "not deterministic", not as a workspace dependence."""
    inputs = [t.to(DEV) for t in inputs]
    plain = _snapshot(call(inputs))
    torch.cuda.synchronize()
    runs = {}
    for name, fill in (("0x00", 0x00), ("0x00 again", 0x00), ("0xFF", 0xFF), ("0x7B", 0x7B)):
        gfill = GUARD_OF[fill]
        what = f"{label} [workspace {name}, guards 0x{gfill:02X}]"
        with monkeypatch.context() as m:
            ws = exact_workspace(m, fill, gfill)
            gin = [guarded_like(t, gfill) for t in inputs]
            outs = guarded_outputs(m, gfill)
            got = call([v for _, v in gin])
            torch.cuda.synchronize()
        runs[name] = _snapshot(got)
        assert bool(ws.handed) == has_workspace, f"{what}: the entry asked for {len(ws.handed)} workspaces"
        assert all(n == asked for _, n, asked in ws.handed)
        ws.check_guards(what)
        for k, ((flat, v), t) in enumerate(zip(gin, inputs)):
            assert_guards(flat, t.numel() * t.element_size(), gfill, what=f"{what}: input {k}")
            assert first_difference(v, t) is None, f"{what}: input {k} was written"
        assert outs.made, f"{what}: no output was allocated through torch.empty"
        outs.check(what)
    _compare(label, "0x00", runs["0x00"], "the same run again", runs["0x00 again"], "NOT DETERMINISTIC (no statement about the workspace)")
    for name in ("0xFF", "0x7B"):
        _compare(label, name, runs[name], "0x00", runs["0x00"], "the result DEPENDS ON WHAT THE WORKSPACE HELD")
    _compare(label, "0x00", runs["0x00"], "the cached workspace", plain, "the exact-size workspace gives another result than the cached one")
    if has_workspace:
        with monkeypatch.context() as m:
            exact_workspace(m, 0x00, GUARD_OF[0x00], short=1)
            with pytest.raises(RuntimeError, match=r"\(-3\)"):
                call(inputs)
        torch.cuda.synchronize()


@contextlib.contextmanager
def debug_switch(bit, on=True):
    """one bit of emavfi_debug_switches for the duration (the `switch` fixture of tests/test_gpu_conv_rounding_model.py as a context)"""
    old = lib.debug_switches()
    lib.debug_switches(~bit, bit if on else 0)
    try:
        yield
    finally:
        lib.debug_switches(0, old)
