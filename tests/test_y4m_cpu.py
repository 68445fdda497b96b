"""YUV4MPEG2 in and out (emavfi/y4m.py), the reference's factor choice restated, and run_chunked's chunk plan: pure host logic, no GPU."""
import io
import itertools

import numpy as np
import pytest

from emavfi import FrameInterpolator, cli, y4m

HEAD8 = b"YUV4MPEG2 W4 H2 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n"


class Pipe(io.RawIOBase):
    """a non-seekable stream over a bytes buffer that hands out short reads / collects writes, as a pipe does"""

    def __init__(self, data=b"", piece=5):
        self._r, self._piece, self.written = io.BytesIO(data), piece, bytearray()

    def readable(self):
        return True

    def writable(self):
        return True

    def seekable(self):
        return False

    def read(self, n=-1):
        return self._r.read(min(n, self._piece) if n and n > 0 else self._piece)

    def write(self, b):
        self.written += bytes(b)
        return len(b)

    def seek(self, *a):
        raise io.UnsupportedOperation("seek")

    def tell(self):
        raise io.UnsupportedOperation("tell")


def test_literal_8_bit_stream_parses_to_its_planes():
    data = HEAD8 + b"FRAME\n" + bytes(range(12))
    r = y4m.Y4MReader(io.BytesIO(data))
    h = r.header
    assert (h.width, h.height, h.fps_num, h.fps_den, h.interlacing, h.aspect, h.colorspace, h.extensions) == \
        (4, 2, 30000, 1001, "p", "1:1", "420jpeg", ("YSCSS=420JPEG",))
    assert h.depth == 8 and h.pixel_format == "yuv420p8" and h.frame_shape == (3, 4) and h.frame_bytes == 12
    frames = list(r)
    assert len(frames) == 1 and frames[0].dtype == np.uint8 and frames[0].shape == (3, 4) and r.frames_read == 1
    f = frames[0]
    assert f[:2].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]                        # Y
    assert f[2:].reshape(2, 1, 2)[0].tolist() == [[8, 9]] and f[2:].reshape(2, 1, 2)[1].tolist() == [[10, 11]]   # U, then V
    assert f.flags.writeable and f.flags.c_contiguous


def test_literal_10_bit_stream_and_frame_parameters():
    words = np.array([0, 1, 512, 1023, 64, 940, 700, 300, 512, 513, 1000, 4], "<u2")
    data = b"YUV4MPEG2 W4 H2 F25:1 C420p10\nFRAME Ip\n" + words.tobytes() + b"FRAME\n" + words[::-1].tobytes()
    r = y4m.Y4MReader(Pipe(data))
    assert r.header.depth == 10 and r.header.pixel_format == "yuv420p10" and r.header.interlacing is None and r.header.aspect is None
    a, b = list(r)
    assert a.dtype == np.uint16 and a.shape == (3, 4) and a.reshape(-1).tolist() == words.tolist() and b.reshape(-1).tolist() == words[::-1].tolist()
    # a missing C is 420jpeg; the other accepted tags
    assert y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2 F25:1\n")).header.colorspace == "420jpeg"
    for tag, depth in (("420jpeg", 8), ("420mpeg2", 8), ("420paldv", 8), ("420", 8), ("420p10", 10), ("420p12", 12), ("420p16", 16)):
        h = y4m.Y4MReader(io.BytesIO(f"YUV4MPEG2 W4 H2 F25:1 I? C{tag}\n".encode())).header
        assert h.depth == depth and h.colorspace == tag and h.line() == f"YUV4MPEG2 W4 H2 F25:1 I? C{tag}\n".encode()


def test_round_trip_over_a_non_seekable_stream():
    rng = np.random.default_rng(5)
    for tag, dt, top in (("420mpeg2", np.uint8, 256), ("420p12", np.uint16, 4096)):
        head = y4m.Y4MHeader(6, 4, 24000, 1001, "p", "128:117", tag, ("YSCSS=X", "COLORRANGE=LIMITED"))
        frames = [rng.integers(0, top, (6, 6)).astype(dt) for _ in range(3)]
        pipe = Pipe()
        with y4m.Y4MWriter(pipe, head) as w:
            for f in frames:
                w.write(f)
            assert w.frames_written == 3
        assert bytes(pipe.written).startswith(head.line()) and bytes(pipe.written).count(b"FRAME\n") >= 3
        r = y4m.Y4MReader(Pipe(bytes(pipe.written), piece=7))
        assert r.header == head
        got = list(r)
        assert len(got) == 3 and all(g.dtype == dt and np.array_equal(g, f) for g, f in zip(got, frames))
        with pytest.raises(ValueError, match="expected"):
            y4m.Y4MWriter(Pipe(), head).write(np.zeros((6, 8), dt))
        with pytest.raises(ValueError, match="expected"):
            y4m.Y4MWriter(Pipe(), head).write(np.zeros((6, 6), np.float32))


@pytest.mark.parametrize("line,word", [
    (b"YUV4MPEG2 W4 H2 F25:1 Cmono", "Cmono"), (b"YUV4MPEG2 W4 H2 F25:1 C422", "C422"), (b"YUV4MPEG2 W4 H2 F25:1 C422p10", "C422p10"),
    (b"YUV4MPEG2 W4 H2 F25:1 C444", "C444"), (b"YUV4MPEG2 W4 H2 F25:1 C444alpha", "C444alpha"), (b"YUV4MPEG2 W4 H2 F25:1 C411", "C411"),
    (b"YUV4MPEG2 W4 H2 F25:1 C420p14", "C420p14"), (b"YUV4MPEG2 W4 H2 F25:1 It", "It"), (b"YUV4MPEG2 W4 H2 F25:1 Ib", "Ib"),
    (b"YUV4MPEG2 W4 H2 F25:1 Im", "Im"), (b"YUV4MPEG2 W5 H2 F25:1", "W5"), (b"YUV4MPEG2 W4 H3 F25:1", "H3"), (b"YUV4MPEG W4 H2 F25:1", "YUV4MPEG2"),
    (b"YUV4MPEG2 H2 F25:1", "W / H"), (b"YUV4MPEG2 W4 H2", "F<num>"), (b"YUV4MPEG2 W4 H2 F0:1", "F0:1"),
])
def test_refused_headers_name_the_tag_or_reason(line, word):
    with pytest.raises(ValueError, match=word):
        y4m.Y4MReader(io.BytesIO(line + b"\nFRAME\n" + bytes(64)))


def test_truncated_and_broken_frames_name_the_frame():
    good = HEAD8 + b"FRAME\n" + bytes(12)
    r = y4m.Y4MReader(io.BytesIO(good + b"FRAME\n" + bytes(7)))
    it = iter(r)
    next(it)
    with pytest.raises(ValueError, match="frame 1 is truncated: 7 of 12"):
        next(it)
    it = iter(y4m.Y4MReader(Pipe(good + b"FRAM")))
    next(it)
    with pytest.raises(ValueError, match="frame 1"):
        next(it)
    it = iter(y4m.Y4MReader(io.BytesIO(good + b"BLOCK\n" + bytes(12))))
    next(it)
    with pytest.raises(ValueError, match="frame 1 does not start with FRAME"):
        next(it)
    with pytest.raises(ValueError, match="truncated"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2"))
    assert list(y4m.Y4MReader(io.BytesIO(HEAD8))) == []                          # a stream of no frames is valid
    for p in (True, False):                                                      # "Ip" and "I?" pass
        assert list(y4m.Y4MReader(io.BytesIO(good.replace(b"Ip", b"Ip" if p else b"I?")))) != []


def test_output_header_rewriting():
    def fps(num, den, factor):
        h = y4m.Y4MHeader(4, 2, num, den, "p", "1:1", "420jpeg", ("YSCSS=420JPEG",)).for_output(factor)
        assert (h.width, h.height, h.interlacing, h.aspect, h.colorspace, h.extensions) == (4, 2, "p", "1:1", "420jpeg", ("YSCSS=420JPEG",))
        return h.fps_num, h.fps_den
    assert fps(30000, 1001, 1) == (60000, 1001)      # x 2
    assert fps(25, 1, 3) == (100, 1)                 # x 4
    assert fps(24, 2, 0) == (12, 1) and fps(24, 2, 1) == (24, 1)   # x 1 and x 2, reduced
    h = y4m.Y4MReader(io.BytesIO(HEAD8)).header.for_output(1, size=(8, 6))
    assert h.line() == b"YUV4MPEG2 W6 H8 F60000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n"
    with pytest.raises(ValueError, match="even"):
        y4m.Y4MReader(io.BytesIO(HEAD8)).header.for_output(1, size=(8, 5))


def test_choose_factor():
    assert [y4m.choose_factor(f)[0] for f in (30, 15, 10, 25, 24)] == [1, 3, 4, 1, 1]      # 24: 48 and 72 tie, the first wins
    assert y4m.choose_factor(30) == (1, 60) and y4m.choose_factor(10) == (4, 50) and y4m.choose_factor(15, None, 2) == (2, 45)
    assert y4m.choose_factor(30, 60) == (1, 60) and y4m.choose_factor(30, 120) == (3, 120)
    assert y4m.choose_factor(30, 100) == (2, 90)                                           # round(2.33) = 2; the target is capped to 90
    assert y4m.choose_factor(24, 60) == (2, 60)                                            # round(1.5) = 2 (half to even): no cap needed
    assert y4m.choose_factor(24, 84) == (2, 72)                                            # round(2.5) = 2 (half to even): capped
    assert y4m.choose_factor(30000 / 1001)[0] == 1
    # (fps, target_fps, max_interpolation_factor) -> (factor, target_fps), each worked out by hand from the two rules in choose_factor's docstring
    table = [
        # no target: the first factor in 1..max whose fps * (factor + 1) is closest to 60
        ((7.5, None, 8), (7, 60.0)), ((10, None, 8), (5, 60)), ((10, None, 4), (4, 50)), ((10, None, 2), (2, 30)), ((10, None, 1), (1, 20)),
        ((12.5, None, 4), (4, 62.5)), ((12.5, None, 8), (4, 62.5)), ((15, None, 4), (3, 60)), ((15, None, 2), (2, 45)), ((20, None, 4), (2, 60)),
        ((24, None, 4), (1, 48)), ((25, None, 4), (1, 50)), ((30, None, 4), (1, 60)), ((50, None, 4), (1, 100)), ((60, None, 4), (1, 120)),
        ((120, None, 8), (1, 240)), ((30, None, 0), (0, 30)),
        # a target: round(target / fps - 1), half to even; the target is capped to fps * (factor + 1)
        ((30, 60, 4), (1, 60)), ((30, 120, 4), (3, 120)), ((30, 100, 4), (2, 90)), ((25, 60, 4), (1, 50)), ((25, 100, 4), (3, 100)),
        ((24, 60, 4), (2, 60)), ((24, 84, 4), (2, 72)), ((10, 144, 1), (13, 140)), ((50, 60, 4), (0, 50)), ((60, 30, 4), (0, 30)),
        ((60, 20, 4), (-1, 0)), ((29.97, 59.94, 4), (1, 59.94)),
    ]
    for args, want in table:
        assert y4m.choose_factor(*args) == want, (args, want)
    with pytest.raises(ValueError, match="fps"):
        y4m.choose_factor(0)


def test_chunk_plan_composed_with_emission_plan_is_the_unchunked_plan():
    for n, interval, pairs, factor, quirks in itertools.product(range(41), (1, 2, 3), (1, 2, 3, 4, 5), range(4), (False, True)):
        want = FrameInterpolator.emission_plan(n, factor, interval, reference_quirks=quirks)
        plan = FrameInterpolator.chunk_plan(n, interval, pairs)
        got = []
        for lo, hi, final in plan:
            assert hi - lo <= pairs * interval + 1 and lo % interval == 0              # the memory bound, the phase
            for item in FrameInterpolator.emission_plan(hi - lo, factor, interval, reference_quirks=quirks):
                if item[0] == "pred":
                    got.append(("pred", item[1] + lo, item[2] + lo, item[3]))
                elif item[0] == "src":
                    got.append(("src", item[1] + lo))
                elif final:
                    got.append(("tail", item[1] + lo, item[2]))
        assert got == want, (n, interval, pairs, factor, quirks)
        assert [c[2] for c in plan] == [False] * (len(plan) - 1) + [True] * bool(plan)
        assert all(a[1] - 1 == b[0] for a, b in zip(plan, plan[1:])) and (not plan or (plan[0][0] == 0 and plan[-1][1] == n))
    with pytest.raises(ValueError):
        FrameInterpolator.chunk_plan(5, 1, 0)


def test_run_chunked_reads_lazily_and_holds_a_bounded_number_of_frames():
    """the chunking itself, with run() replaced by a recorder: no device"""
    for n, interval, pairs in itertools.product((0, 1, 2, 7, 12, 13), (1, 2, 3), (1, 2, 4)):
        fi = FrameInterpolator.__new__(FrameInterpolator)
        fi.interval, seen, pulled = interval, [], []

        def run(held, _emit_tail=True, fi=fi, seen=seen, pulled=pulled):
            seen.append((list(held), _emit_tail, len(pulled)))
            fi.scene_cuts = [(0, 1, 7)] if len(held) > 1 else []
            fi.scene_scores = list(fi.scene_cuts)
            yield from held

        def source():
            for i in range(n):
                pulled.append(i)
                yield i

        fi.run = run
        out = list(fi.run_chunked(source(), chunk_pairs=pairs))
        plan = FrameInterpolator.chunk_plan(n, interval, pairs)
        assert [(h[0], h[-1] + 1, t) for h, t, _ in seen] == plan
        assert all(len(h) <= pairs * interval + 1 and h == list(range(h[0], h[-1] + 1)) for h, _, _ in seen)
        assert all(got == h[-1] + 1 for h, _, got in seen), "a chunk runs as soon as its frames have been read: nothing is read ahead"
        assert out == [f for h, _, _ in seen for f in h]
        assert fi.scene_cuts == [(lo, lo + 1, 7) for lo, hi, _ in plan if hi - lo > 1] == fi.scene_scores
    with pytest.raises(ValueError, match="chunk_pairs"):
        list(FrameInterpolator.__new__(FrameInterpolator).run_chunked([], chunk_pairs=0))


def test_cli_refuses_bad_input_without_a_device(tmp_path, capsys):
    bad = tmp_path / "bad.y4m"
    bad.write_bytes(b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C422\nFRAME\n" + bytes(16))
    assert cli.main([str(bad), str(tmp_path / "out.y4m"), "--synthetic-weights", "0"]) != 0
    assert "C422" in capsys.readouterr().err
    assert cli.main([str(tmp_path / "missing.y4m"), str(tmp_path / "out.y4m"), "--synthetic-weights", "0"]) != 0
    assert "missing.y4m" in capsys.readouterr().err
    assert cli.main([str(bad)]) != 0                                     # neither --weights nor --synthetic-weights
    capsys.readouterr()
    ok = tmp_path / "ok.y4m"
    ok.write_bytes(HEAD8 + b"FRAME\n" + bytes(12))
    assert cli.main([str(ok), "--synthetic-weights", "0"]) != 0          # no output and no --evaluate
    assert "output" in capsys.readouterr().err
    assert cli.main([str(ok), str(tmp_path / "o.y4m"), "--synthetic-weights", "0", "--target-fps", "10"]) != 0
    assert "negative" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["--help"])
    text = capsys.readouterr().out
    assert "NOT resized" in text and "--reference-quirks" in text and "--chunk-pairs" in text
