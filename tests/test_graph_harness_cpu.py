"""tests/graph_harness.py must SEE a replay that is not the eager call.  No deliberately broken graph may run on a GPU, so the
sensitivity is shown here: replay_case over stand-in hooks whose "capture" records a list of Python steps over CPU tensors - it
executes nothing, as a stream capture does - and whose "replay" runs the list again.  The stand-in entry has what the real ones
have: a workspace with a zero page that reads beyond the row land on, a scratch row and a counter, all cleared by steps of the entry
itself.  The correct stand-in passes; four injected defects of the kind a graph produces are each caught under the verdict named for
them (graph_harness.VERDICTS)."""
import contextlib

import pytest
import torch

import graph_harness as gh

N = 37                      # elements of a row
ZPAGE, SCRATCH, SCRATCH_END, COUNTER, WS_BYTES = 0, 16, 16 + 4 * N, 16 + 4 * (N + 1), 16 + 4 * (N + 1) + 8   # fp32[4] | fp32[N] | pad | int64


class StandIn:
    """out[i] = 2 x[i] + right(i), right(i) = 2 x[i + 1], or the zero page's first word beyond the row; the counter counts x > 0.
    `defect` changes the RECORDED steps only - the eager call is right, as the eager runs of a real entry are."""

    def __init__(self, defect=None):
        self.defect, self.tape, self.ws = defect, None, None

    def _do(self, step):
        if self.tape is not None:
            self.tape.append(step)
        else:
            step()

    def workspace(self):
        if self.ws is None:
            assert self.tape is None, "a workspace made under capture"
            self.ws = torch.full((WS_BYTES,), 0x55, dtype=torch.uint8)   # what an earlier call left
        return self.ws

    def call(self, inp):
        x, ws, recorded = inp[0], self.workspace(), self.tape is not None
        zpage, scratch, counter = ws[ZPAGE:SCRATCH].view(torch.float32), ws[SCRATCH:SCRATCH_END].view(torch.float32), ws[COUNTER:].view(torch.int64)
        out = torch.zeros(N)
        defect = self.defect if recorded else None
        src = x.clone() if defect == "input" else x            # the input read when the call is recorded, not when it runs
        if defect != "zero_page":
            self._do(lambda: zpage.zero_())
        if defect != "counter":
            self._do(lambda: counter.zero_())
        self._do(lambda: scratch.copy_(2 * src))
        self._do(lambda: counter.add_(int((src > 0).sum())))
        last = N - 1 if defect == "unwritten" else N

        def finish():
            right = torch.cat([scratch[1:], zpage[:1]])
            out[:last] = (scratch + right)[:last]
        self._do(finish)
        return out

    def census(self):
        return {"census": [int(self.workspace()[COUNTER:].view(torch.int64)[0])]}


class TapeHooks:
    """capture = record the entry's steps, replay = run them again"""
    device = "cpu"

    def __init__(self, entry):
        self.entry = entry

    @contextlib.contextmanager
    def on_stream(self):
        yield

    def synchronize(self):
        pass

    def workspace(self):
        return self.entry.ws

    def capture(self, fn):
        self.entry.tape = []
        try:
            return self.entry.tape, fn()
        finally:
            self.entry.tape = None

    def replay(self, tape):
        for step in tape:
            step()


def contents():
    g = torch.Generator().manual_seed(4)
    return [torch.randn(N, generator=g)], [torch.randn(N, generator=g) + 0.5]


def run(defect):
    entry = StandIn(defect)
    a, b = contents()
    gh.replay_case(f"stand-in {defect}", entry.call, a, b, read_after=entry.census, hooks=TapeHooks(entry))


def test_the_correct_stand_in_passes():
    run(None)


def test_the_two_contents_count_differently():
    """or the counter defect below could pass: both counts lie inside the row and differ"""
    a, b = contents()
    na, nb = int((a[0] > 0).sum()), int((b[0] > 0).sum())
    assert 0 < na < N and 0 < nb < N and na != nb


@pytest.mark.parametrize("defect,verdict,detail", [
    ("counter", "carried", "`census`"),          # the clearing step dropped from the recorded list: the counter accumulates
    ("zero_page", "workspace", "`out`"),         # the zero-page clear dropped: seen only through the fill
    ("input", "new", "`out`"),                   # an input read at capture time instead of replay time
    ("unwritten", "captured", "never written"),  # an output element the recorded steps never write
])
def test_an_injected_defect_fails_under_its_verdict(defect, verdict, detail):
    with pytest.raises(AssertionError) as e:
        run(defect)
    text = str(e.value)
    assert gh.VERDICTS[verdict] in text.split("; and: ")[0], text
    assert detail in text, text
    if defect == "unwritten":
        assert f"1 elements were never written, the first at flat index {N - 1}" in text, text
    if defect == "input":
        assert "replay 2" in text, text
    else:
        assert "replay 1" in text, text


def test_identical_contents_are_refused():
    entry = StandIn()
    a, _ = contents()
    with pytest.raises(AssertionError, match="says nothing about new content"):
        gh.replay_case("stand-in same", entry.call, a, [a[0].clone()], read_after=entry.census, hooks=TapeHooks(entry))


def test_a_workspace_made_under_capture_is_refused():
    """the harness's own check that the capture handed out no buffer: a stand-in whose workspace appears only while recording"""
    class Late(StandIn):
        def workspace(self):
            if self.ws is None and self.tape is not None:
                self.ws = torch.zeros(WS_BYTES, dtype=torch.uint8)
            return self.ws if self.ws is not None else torch.zeros(WS_BYTES, dtype=torch.uint8)
    entry = Late()
    a, b = contents()
    with pytest.raises(AssertionError, match="handed a workspace the warm-up had not made"):
        gh.replay_case("stand-in late", entry.call, a, b, hooks=TapeHooks(entry))
