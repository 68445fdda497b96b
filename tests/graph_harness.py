"""A captured graph's replay against the eager call (tests/test_gpu_graph_replay.py).  A plain module: no fixture, no pytest setting.

What it builds:
  * replay_case(...): the one statement of tests/test_gpu_graph_replay.py, made about a callable that only enqueues work.
  * GraphHooks: how capture and replay happen - torch.cuda.graph on one side stream and g.replay().  The protocol itself knows neither:
    tests/test_graph_harness_cpu.py runs it over a stand-in whose "capture" records Python steps.
  * EagerReference: what a replay is held to.  By default the eager results R_a and R_b of the two contents, computed once; a test
    whose entry keeps state ACROSS calls (the adaptive route) passes its own `reference(step, inputs)`.

The protocol (no tolerance anywhere): eager R_a and R_b, which must differ in every tensor; one warm-up call on static inputs holding
A, then the capture, during which no workspace may be handed out; then four replays -
  1  A still in the static inputs, the stream's whole workspace filled with 0xFF, every returned tensor with the sentinel    = R_a
  2  B copied in, the workspace filled with 0x7B, the outputs with the sentinel                                               = R_b
  3  nothing touched: the workspace holds exactly what replay 2 left, the outputs replay 2's result                           = R_b
  4  A copied back, nothing else touched                                                                                      = R_a
Fill patterns and the sentinel are workspace_harness.py's.  A failed comparison names what it shows (VERDICTS): before it is raised
the same replay is made once more with nothing touched, and then over a workspace of 0x00, so that a counter that moves on is named
as state carried between replays and a page that follows the fill as a dependence on the workspace, at whichever replay they first
show; what neither moves is a plain difference on the captured or on new content, with the elements the sentinel still holds."""
import contextlib

import torch

from emavfi import lib
from workspace_harness import DEV, SENTINEL, _compare, _snapshot, bits

VERDICTS = {
    "captured": "replay differs from eager on the captured content",
    "new": "replay differs from eager on new content",
    "carried": "a second replay of the same content differs from the first (state carried between replays)",
    "workspace": "the replay depends on what the workspace held before the replay",
}
# (what the static inputs hold, workspace fill or None, sentinel in the outputs, the verdict of a plain mismatch)
STEPS = (("A", 0xFF, True, "captured"), ("B", 0x7B, True, "new"), ("B", None, False, "carried"), ("A", None, False, "new"))
OTHER_FILL = 0x00   # the second opinion after a mismatch under a fill: the same replay over another pattern


class GraphHooks:
    """torch.cuda.graph / g.replay() on one side stream of cuda:0, shared by every case of a process: lib.workspace keeps one buffer per
    (device, stream), and a buffer a capture saw is held until release_workspaces()"""
    device = DEV
    _side = None

    def __init__(self):
        if GraphHooks._side is None:
            GraphHooks._side = torch.cuda.Stream(device=DEV)
        self.side = GraphHooks._side

    @contextlib.contextmanager
    def on_stream(self):
        """eager work of the case (references, warm-up, read_after) runs here: the capture stream"""
        self.side.wait_stream(torch.cuda.current_stream(self.side.device))
        with torch.cuda.stream(self.side), torch.no_grad():
            yield
        torch.cuda.current_stream(self.side.device).wait_stream(self.side)

    def synchronize(self):
        torch.cuda.synchronize()

    def workspace(self):
        """the buffer lib.workspace holds for the capture stream (None: the entry takes no workspace)"""
        return lib._ws_cache.get((self.side.device.index, self.side.cuda_stream))

    def capture(self, fn):
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g, stream=self.side):
            result = fn()
        return g, result

    def replay(self, handle):
        handle.replay()


class EagerReference:
    """R_a and R_b: the call on fresh copies of each content through the ordinary workspace, with read_after where given"""

    def __init__(self, label, eager, inputs_a, inputs_b):
        self.r = {"A": eager(inputs_a), "B": eager(inputs_b)}
        same = [k for k, v in self.r["A"].items() if torch.is_tensor(v) and torch.equal(bits(v), bits(self.r["B"][k]))]
        assert not same, f"{label}: the two contents give the same `{same}`: the case says nothing about new content"

    def __call__(self, step, inputs):
        return self.r[STEPS[step][0]]


def _fill_bytes(t, byte):
    assert t.is_contiguous(), "a returned tensor that is not contiguous cannot be pre-filled"
    t.view(torch.uint8).fill_(byte)


def _sentinel_left(got, want):
    """elements of `got` that still hold the sentinel in every byte where the expected result does not"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return 0, None
    is_sentinel = lambda t: (t.contiguous().view(torch.uint8).view(-1, t.element_size()) == SENTINEL).all(dim=1)
    left = (is_sentinel(got) & ~is_sentinel(want)).nonzero()
    return left.shape[0], (int(left[0]) if left.numel() else None)


def replay_case(label, call, inputs_a, inputs_b, read_after=None, hooks=None, reference=None):
    """The statement of tests/test_gpu_graph_replay.py about call(list of device tensors) -> tensor | {name: tensor}, which only
    enqueues work, and read_after() -> {name: plain value}, which reads back outside the graph (a census, the routes): captured once
    after one warm-up, every one of four replays gives bit for bit - census rows included - what the eager call gives on the content
    the static inputs hold then, whatever the workspace and the outputs held before, and the capture asked for no new workspace.
    `reference(step, inputs)`: the expected result of replay `step` (0..3) instead of R_a / R_b, for an entry whose state outlives
    a call; it is called once per step, in order.  hooks: GraphHooks by default."""
    h = hooks if hooks is not None else GraphHooks()
    content = {"A": [t.to(h.device) for t in inputs_a], "B": [t.to(h.device) for t in inputs_b]}
    assert len(content["A"]) == len(content["B"]) and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(content["A"], content["B"])), label

    def read(result):
        res = _snapshot(result)
        if read_after is not None:
            with h.on_stream():
                extra = read_after()
            assert not set(extra) & set(res), (label, sorted(extra), sorted(res))
            res.update(_snapshot(extra))
        return res

    def eager(inputs):
        with h.on_stream():
            got = call([t.clone() for t in inputs])
        h.synchronize()
        return read(got)

    if reference is None:
        reference = EagerReference(label, eager, content["A"], content["B"])

    static = [t.clone() for t in content["A"]]
    with h.on_stream():
        call(static)                      # the warm-up: every allocation, the workspace included, exists before the capture
    h.synchronize()
    before = h.workspace()
    handle, captured = h.capture(lambda: call(static))
    after = h.workspace()
    assert (before is None) == (after is None) and (before is None or (before.data_ptr() == after.data_ptr() and before.numel() == after.numel())), \
        f"{label}: the capture was handed a workspace the warm-up had not made"
    outs = {"out": captured} if torch.is_tensor(captured) else dict(captured)
    assert outs and all(torch.is_tensor(v) for v in outs.values()), f"{label}: the captured call must return tensors, got {outs!r}"

    def replay(fill, sentinel):
        if fill is not None and after is not None:
            after.fill_(fill)
        if sentinel:
            for t in outs.values():
                _fill_bytes(t, SENTINEL)
        h.synchronize()
        h.replay(handle)
        h.synchronize()
        ws = h.workspace()
        assert (ws is None) == (after is None) and (ws is None or ws.data_ptr() == after.data_ptr()), f"{label}: the workspace was replaced under the graph"
        return read(outs)

    for k, (name, fill, sentinel, verdict) in enumerate(STEPS):
        what = f"{label} [replay {k + 1}: content {name}, workspace " + ("as the last replay left it" if fill is None else f"0x{fill:02X}") + "]"
        if k in (1, 3):
            for s, t in zip(static, content[name]):
                s.copy_(t)
        want = reference(k, content[name])
        got = replay(fill, sentinel)
        try:
            _compare(what, "the replay", got, "the eager call", want, VERDICTS[verdict])
        except AssertionError as first:
            note = ""
            if sentinel:
                left = {n: _sentinel_left(got[n], want[n]) for n in outs if n in want and torch.is_tensor(want[n])}
                note = "".join(f"; `{n}`: {c} elements were never written, the first at flat index {i}" for n, (c, i) in left.items() if c)
            # second opinions, so that the failure names its cause: the same replay once more with nothing touched (a counter that was
            # not cleared moves on), then over another workspace pattern (a page that was not cleared moves with it)
            for opinion, again in (("carried", lambda: replay(None, False)), ("workspace", lambda: replay(OTHER_FILL, sentinel))):
                if opinion == verdict or (opinion == "workspace" and (fill is None or after is None)):
                    continue
                try:
                    _compare(what, "the failed replay", got, "the same replay " + ("again, nothing touched" if opinion == "carried" else
                                                                                   f"over a workspace of 0x{OTHER_FILL:02X}"), again(), VERDICTS[opinion])
                except AssertionError as moved:
                    raise AssertionError(f"{moved}; and: {first}{note}") from None
            raise AssertionError(f"{first}{note}") from None
