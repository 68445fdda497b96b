"""YUV4MPEG2 (``.y4m``) in and out, in pure Python and numpy: a text header plus raw planar frames - the container that needs no library.

It is what ``ffmpeg -f yuv4mpegpipe`` reads and writes on a pipe, so a video file of any codec reaches the harness, and leaves it, through
two ffmpeg processes and no Python dependency.  A stream is

    YUV4MPEG2 W<width> H<height> F<num>:<den> I<interlacing> A<num>:<den> C<colour space> X<extension> ...\\n
    FRAME[ parameters]\\n  <Y plane> <U plane> <V plane>          (once per frame)

and a frame, as this module hands it over and takes it back, is ONE contiguous buffer exactly as the stream stores it: a numpy
``[H*3/2, W]`` array, ``uint8`` at 8 bits, little-endian ``uint16`` (the sample in the low bits) above - H rows of Y, then the dense U plane,
then the dense V plane.  That is the frame layout of ``FrameInterpolator(pixel_format="yuv420p8" | "yuv420p10" | ...)``: nothing is
re-packed on the host in either direction.  Only progressive 4:2:0 with even W and H is accepted; everything else is refused with a
``ValueError`` that names the tag or the reason.
"""
from __future__ import annotations

import sys
from fractions import Fraction
from math import gcd
from typing import Iterator, NamedTuple, Optional, Tuple

import numpy as np

from . import formats

MAGIC = b"YUV4MPEG2"
# colour-space tag -> bits per sample.  The 8-bit tags differ in chroma siting only, which is carried through to the output header: the
# project's colour definition has one siting (include/emavfi.h)
DEPTH_OF_TAG = {"420jpeg": 8, "420mpeg2": 8, "420paldv": 8, "420": 8, "420p10": 10, "420p12": 12, "420p16": 16}
MAX_HEADER = 4096     # bytes of a header or FRAME line before the stream counts as broken


class Y4MHeader(NamedTuple):
    """The stream header.  ``colorspace``: the C tag without its letter (``"420jpeg"`` when the stream has none); ``interlacing`` /
    ``aspect``: the I / A parameters without their letters, or None; ``extensions``: the X parameters without theirs, in order."""
    width: int
    height: int
    fps_num: int
    fps_den: int
    interlacing: Optional[str] = None
    aspect: Optional[str] = None
    colorspace: str = "420jpeg"
    extensions: Tuple[str, ...] = ()

    @property
    def format(self) -> formats.PixelFormat:
        """the record of the planar format this stream's frames have"""
        return formats.lookup(f"yuv420p{DEPTH_OF_TAG[self.colorspace]}")

    @property
    def depth(self) -> int:
        return self.format.depth

    @property
    def pixel_format(self) -> str:
        """the ``FrameInterpolator`` pixel format of this stream's frames"""
        return self.format.name

    @property
    def fps(self) -> float:
        return self.fps_num / self.fps_den

    @property
    def frame_shape(self) -> Tuple[int, int]:
        return self.height * 3 // 2, self.width

    @property
    def dtype(self):
        return np.dtype("<u2") if self.format.words else np.dtype(np.uint8)

    @property
    def frame_bytes(self) -> int:
        return self.frame_shape[0] * self.frame_shape[1] * self.dtype.itemsize

    def line(self) -> bytes:
        """the header line as it is written, C always present"""
        parts = [MAGIC.decode(), f"W{self.width}", f"H{self.height}", f"F{self.fps_num}:{self.fps_den}"]
        if self.interlacing is not None:
            parts.append("I" + self.interlacing)
        if self.aspect is not None:
            parts.append("A" + self.aspect)
        parts.append("C" + self.colorspace)
        parts += ["X" + x for x in self.extensions]
        return " ".join(parts).encode("ascii") + b"\n"

    def for_output(self, factor: int = 0, size=None) -> "Y4MHeader":
        """The header of the interpolated stream: F becomes ``num * (factor + 1) : den`` reduced by their gcd - the reference's
        ``target_fps = fps * (factor + 1)`` (inference.py:112 / :121), whatever ``frame_interval`` is -, W and H become ``size = (H, W)``
        when the frames are resized; everything else, the X parameters included, is copied."""
        if factor < 0:
            raise ValueError("factor must be >= 0")
        num, den = self.fps_num * (factor + 1), self.fps_den
        g = gcd(num, den) or 1
        h = self._replace(fps_num=num // g, fps_den=den // g)
        if size is not None:
            h = h._replace(height=int(size[0]), width=int(size[1]))
            check_header(h)
        return h

    @property
    def rate(self) -> Fraction:
        """F as an exact rational"""
        return Fraction(self.fps_num, self.fps_den)

    def for_output_rate(self, rate, size=None) -> "Y4MHeader":
        """The header of a stream converted to the frame rate ``rate`` (anything ``fractions.Fraction`` accepts): F becomes exactly that
        rational, reduced; W, H and everything else as ``for_output`` treats them."""
        try:
            rate = Fraction(rate)
        except (TypeError, ValueError, ZeroDivisionError):
            raise ValueError(f"frame rate {rate!r} is refused: a positive rational expected") from None
        if rate <= 0:
            raise ValueError(f"frame rate {rate} is refused: it must be positive")
        h = self._replace(fps_num=rate.numerator, fps_den=rate.denominator)
        if size is not None:
            h = h._replace(height=int(size[0]), width=int(size[1]))
            check_header(h)
        return h


def parse_rate(text) -> Fraction:
    """A frame rate as the command line and a Y4M header spell it - ``60``, ``59.94``, ``60000/1001`` or ``60000:1001`` - as an exact
    positive ``Fraction`` (a decimal is taken digit for digit: ``59.94`` is 2997/50, not 60000/1001).  ValueError otherwise."""
    try:
        rate = Fraction(str(text).strip().replace(":", "/"))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"frame rate {text!r} is refused: 60, 59.94, 60000/1001 or 60000:1001 expected") from None
    if rate <= 0:
        raise ValueError(f"frame rate {text!r} is refused: it must be positive")
    return rate


def check_header(h: Y4MHeader) -> None:
    if h.colorspace not in DEPTH_OF_TAG:
        why = ("4:2:0 with 14 bits has no device format" if h.colorspace == "420p14" else
               "only planar 4:2:0 is supported (C420jpeg, C420mpeg2, C420paldv, C420, C420p10, C420p12, C420p16)")
        raise ValueError(f"y4m: colour space C{h.colorspace} is refused: {why}")
    if h.interlacing not in (None, "p", "?"):
        raise ValueError(f"y4m: interlacing I{h.interlacing} is refused: only progressive streams (Ip, I?) are interpolated")
    if h.width < 2 or h.height < 2 or h.width % 2 or h.height % 2:
        raise ValueError(f"y4m: W{h.width} H{h.height} is refused: the packed 4:2:0 frame needs an even width and height")
    if h.fps_num < 1 or h.fps_den < 1:
        raise ValueError(f"y4m: frame rate F{h.fps_num}:{h.fps_den} is refused: both terms must be positive")


def parse_header(line: bytes) -> Y4MHeader:
    """``line``: the first line of a stream, without its newline"""
    try:
        tokens = line.decode("ascii").split()
    except UnicodeDecodeError:
        raise ValueError("y4m: the stream header is not ASCII") from None
    if not tokens or tokens[0] != MAGIC.decode():
        raise ValueError(f"y4m: the stream does not start with {MAGIC.decode()}")
    f = {"X": []}
    for tok in tokens[1:]:
        if tok[0] == "X":
            f["X"].append(tok[1:])
        else:
            f[tok[0]] = tok[1:]
    try:
        w, hgt = int(f["W"]), int(f["H"])
    except (KeyError, ValueError):
        raise ValueError("y4m: the stream header has no valid W / H") from None
    try:
        num, den = (int(v) for v in f["F"].split(":"))
    except (KeyError, ValueError):
        raise ValueError("y4m: the stream header has no valid F<num>:<den>") from None
    h = Y4MHeader(w, hgt, num, den, f.get("I"), f.get("A"), f.get("C", "420jpeg"), tuple(f["X"]))
    check_header(h)
    return h


def _open(path_or_file, mode):
    """(binary file object, whether this module opened it)"""
    if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__"):
        if path_or_file in ("-", b"-"):
            return (sys.stdin.buffer if mode == "rb" else sys.stdout.buffer), False
        return open(path_or_file, mode), True
    return path_or_file, False


class Y4MReader:
    """Iterates the frames of a YUV4MPEG2 stream as numpy ``[H*3/2, W]`` arrays (module docstring).  ``path_or_file``: a path, ``"-"``
    for stdin, or a binary file object; only ``read()`` is used, so a pipe or a socket works.  ``header`` is available at once;
    ``frames_read`` counts.  Every frame is a fresh array the caller owns."""

    def __init__(self, path_or_file):
        self._f, self._own = _open(path_or_file, "rb")
        try:
            self.header = parse_header(self._line("the stream header"))
        except Exception:
            self.close()
            raise
        self.frames_read = 0

    def _read(self, n):
        """exactly n bytes, fewer only at the end of the stream (a pipe hands out short reads)"""
        parts, got = [], 0
        while got < n:
            b = self._f.read(n - got)
            if not b:
                break
            parts.append(b)
            got += len(b)
        return parts[0] if len(parts) == 1 else b"".join(parts)

    def _line(self, what):
        """one line without its newline; b"" at a clean end of stream"""
        out = bytearray()
        while True:
            c = self._f.read(1)
            if not c:
                if out:
                    raise ValueError(f"y4m: {what} is truncated")
                return b""
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > MAX_HEADER:
                raise ValueError(f"y4m: {what} is longer than {MAX_HEADER} bytes")

    def __iter__(self) -> Iterator[np.ndarray]:
        h = self.header
        while True:
            line = self._line(f"the FRAME line of frame {self.frames_read}")
            if not line:
                return
            if line.split(b" ")[0] != b"FRAME":        # parameters after FRAME are tolerated and ignored
                raise ValueError(f"y4m: frame {self.frames_read} does not start with FRAME")
            data = self._read(h.frame_bytes)
            if len(data) != h.frame_bytes:
                raise ValueError(f"y4m: frame {self.frames_read} is truncated: {len(data)} of {h.frame_bytes} bytes")
            self.frames_read += 1
            # bytearray: the array is writable and owns its memory
            yield np.frombuffer(bytearray(data), dtype=h.dtype).reshape(h.frame_shape)

    def close(self):
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes ``header`` once, then ``FRAME\\n`` and the buffer of every frame handed to ``write``.  ``path_or_file``: a path, ``"-"`` for
    stdout, or a binary file object."""

    def __init__(self, path_or_file, header: Y4MHeader):
        check_header(header)
        self.header = header
        self._f, self._own = _open(path_or_file, "wb")
        self._f.write(header.line())
        self.frames_written = 0

    def write(self, frame: np.ndarray) -> None:
        h = self.header
        if frame.shape != h.frame_shape or frame.dtype.itemsize != h.dtype.itemsize or frame.dtype.kind != "u":
            raise ValueError(f"y4m: frame {self.frames_written}: {h.dtype} {h.frame_shape} expected, got {frame.dtype} {frame.shape}")
        self._f.write(b"FRAME\n")
        self._f.write(np.ascontiguousarray(frame, dtype=h.dtype).data)
        self.frames_written += 1

    def close(self):
        self._f.flush()
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def choose_factor(fps: float, target_fps: Optional[float] = None, max_interpolation_factor: int = 4):
    """The reference's choice of the interpolation factor (inference.py:102-124), restated: ``(factor, target_fps)``.
    Without ``target_fps``: the first factor in ``1..max_interpolation_factor`` whose ``fps * (factor + 1)`` lies closest to 60 (a tie
    goes to the smaller factor; 0 when the range is empty).  With one: ``round(target_fps / fps - 1)`` - Python's round, half to even, as
    there -, and a ``target_fps`` above ``fps * (factor + 1)`` is capped to it."""
    if not fps > 0:
        raise ValueError("fps must be positive")
    if target_fps is None:
        factor, best = 0, float("inf")
        for f in range(1, max_interpolation_factor + 1):
            diff = abs(fps * (f + 1) - 60)
            if diff < best:
                best, factor = diff, f
        target_fps = fps * (factor + 1)
    else:
        factor = round(target_fps / fps - 1)
    return factor, min(target_fps, fps * (factor + 1))
