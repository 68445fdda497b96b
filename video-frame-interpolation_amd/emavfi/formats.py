"""The pixel formats of the harness, each described once: a row of `FORMATS` says what the samples of a frame are and how they lie in
memory, and everything a caller needs to know of a format - what it may be combined with, the shapes of its frames, the plane views the
kernels take - is derived here from that row.  Pure host logic: nothing of the library is imported, and torch only where a tensor is
viewed.  The next pixel format is one more row.
"""
from __future__ import annotations

from dataclasses import dataclass

LAYOUT_INTERLEAVED, LAYOUT_NV12, LAYOUT_I420 = 0, 1, 2   # EMAVFI_LAYOUT_* (include/emavfi.h)


@dataclass(frozen=True)
class PixelFormat:
    """`layout`: interleaved colour [H, W, C]; NV12, H rows of Y and then H/2 rows of U,V pairs; or I420, H rows of Y, then the dense U
    plane, then the dense V plane.  `C`: samples per pixel of the first plane.  A sample is one byte or one 16-bit word (`sample_bytes`)
    that holds `depth` bits, `shift` bits above the word's low end."""
    name: str
    layout: int
    C: int
    sample_bytes: int
    depth: int
    shift: int

    # ---- what a format may be combined with
    @property
    def yuv(self) -> bool:
        """4:2:0 Y'CbCr frames [H*3/2, W] whose first H rows are the Y plane"""
        return self.layout != LAYOUT_INTERLEAVED

    @property
    def words(self) -> bool:
        return self.sample_bytes == 2

    @property
    def takes_bt2020(self) -> bool:
        """the high-bit-depth colour definition is the only one that knows BT.2020"""
        return self.words

    @property
    def byte_kernels(self) -> bool:
        """the resize, signature and metric kernels read bytes: only a byte format is resized, scanned for cuts or scored by evaluate()"""
        return not self.words

    @property
    def light_table_fits(self) -> bool:
        """a table of 2^depth values of light fits LDS up to 12 bits"""
        return self.depth <= 12

    @property
    def even_resize(self) -> bool:
        """a resized [H*3/2, W] frame needs an even destination H and W"""
        return self.yuv and self.byte_kernels

    @property
    def fused_resize(self) -> bool:
        """the preprocess entry resizes in its own launch (interleaved frames, and NV12's two planes); I420's three planes are resized
        ahead of it, each as a one-channel image"""
        return self.layout != LAYOUT_I420

    @property
    def family(self) -> str:
        """which of lib's preprocess_ / postprocess_ pairs serves the format: "u8", "nv12", "p010" or "yuv420p" (all but "u8" and
        "nv12" take the depth)"""
        return "u8" if not self.yuv else "yuv420p" if self.layout == LAYOUT_I420 else "p010" if self.words else "nv12"

    @property
    def display(self) -> str:
        """the name as messages spell it"""
        return self.name.upper()

    # ---- frames on the host: numpy arrays of samples as they arrive and leave, arrays of bytes in between
    @property
    def dtype(self):
        import numpy as np
        return np.dtype(np.uint16 if self.words else np.uint8)

    @property
    def rank(self) -> int:
        return 2 if self.yuv else 3

    def check_frames(self, frames, first, what):
        """every frame of `frames` a numpy array of this format with the shape of `first`"""
        for f in frames:
            if f.dtype != self.dtype or f.ndim != self.rank or f.shape != first.shape:
                raise ValueError(f"{what}: same-shape {self.dtype.name} {f'[H*3/2, W] {self.display}' if self.yuv else 'HWC'} frames expected")
        if self.yuv and (first.shape[0] % 3 or first.shape[1] % 2):   # H = 2 * rows / 3 is then even
            raise ValueError(f"{what}: the packed {self.display} layout [H*3/2, W] needs even H and W")

    def as_bytes(self, frame):
        """an arriving frame as its bytes: a frame of words [H*3/2, W] becomes [H*3/2, 2 W] (a view: no copy)"""
        import numpy as np
        return frame.view(np.uint8) if self.words else frame

    def as_samples(self, frame):
        """the bytes of a frame as it is yielded: as_bytes the other way round (a view: no copy)"""
        return frame.view(self.dtype) if self.words else frame

    # ---- shapes
    def geometry(self, byte_shape):
        """(Hs, Ws, C) of a frame whose bytes have the shape `byte_shape`: the picture's height and width and the channels of the
        normalised tensor"""
        if not self.yuv:
            return tuple(byte_shape)
        return byte_shape[0] * 2 // 3, byte_shape[1] // self.sample_bytes, 3

    def byte_shape(self, H, W):
        """the shape of the bytes of an H x W frame"""
        return (H * 3 // 2, W * self.sample_bytes) if self.yuv else (H, W, self.C)

    def luma_bytes(self, frame_bytes):
        """how many of a frame's bytes, from its start, are luma (linear light mixes those): an interleaved frame whole, the first two
        thirds of a 4:2:0 frame"""
        return frame_bytes * 2 // 3 if self.yuv else frame_bytes

    # ---- views of n contiguous frames, uint8 [n, *byte_shape(H, W)], device or pinned
    def planes(self, buf):
        """the planes as the pre / post kernels take them, words as int16: (buf,) of interleaved frames; Y [n,H,W] and UV [n,H/2,W/2,2] of
        the NV12 layout; Y [n,H,W], U and V [n,H/2,W/2] of the I420 layout, whose chroma planes are dense and need not start on a row of
        `buf`"""
        if not self.yuv:
            return (buf,)
        import torch
        n, H = buf.shape[0], buf.shape[1] * 2 // 3
        y, c = buf[:, :H], buf[:, H:]
        if self.words:
            y, c = y.view(torch.int16), c.view(torch.int16)
        if self.layout == LAYOUT_NV12:
            return y, c.unflatten(2, (c.shape[2] // 2, 2))
        c = c.view(n, 2, H // 2, c.shape[2] // 2)
        return y, c[:, 0], c[:, 1]

    def luma(self, buf):
        """the image the signature, difference, bounds and metric kernels read: interleaved colour as it is, else the Y plane - of bytes
        as a one-channel image [n,H,W,1], of words as [n,H,W]"""
        y = self.planes(buf)[0]
        return y.unsqueeze(-1) if self.yuv and not self.words else y

    # ---- what the frame-level entries are told of the samples
    @property
    def sample_format(self):
        """(sample_bytes, depth, shift), as emavfi_resample_frames takes them"""
        return self.sample_bytes, self.depth, self.shift

    @property
    def frame_format(self):
        """(layout, C, sample_bytes, depth, shift), as emavfi_static_guard_frames takes them"""
        return self.layout, self.C, self.sample_bytes, self.depth, self.shift


FORMATS = {f.name: f for f in (
    PixelFormat("bgr24", LAYOUT_INTERLEAVED, 3, 1, 8, 0),
    PixelFormat("nv12", LAYOUT_NV12, 1, 1, 8, 0),
    PixelFormat("p010", LAYOUT_NV12, 1, 2, 10, 6),       # P01x: the sample in the word's top bits
    PixelFormat("p012", LAYOUT_NV12, 1, 2, 12, 4),
    PixelFormat("p016", LAYOUT_NV12, 1, 2, 16, 0),
    PixelFormat("yuv420p8", LAYOUT_I420, 1, 1, 8, 0),
    PixelFormat("yuv420p10", LAYOUT_I420, 1, 2, 10, 0),  # planar words: the sample in the low bits
    PixelFormat("yuv420p12", LAYOUT_I420, 1, 2, 12, 0),
    PixelFormat("yuv420p16", LAYOUT_I420, 1, 2, 16, 0),
)}


def lookup(name) -> PixelFormat:
    """the record of a pixel format's name; the one place that refuses a name the harness does not know"""
    try:
        return FORMATS[name]
    except (KeyError, TypeError):
        raise ValueError("pixel_format must be 'bgr24' (uint8 HWC frames), 'nv12' (uint8 [H*3/2, W] frames), 'p010' / 'p012' / 'p016' "
                         "(uint16 [H*3/2, W] frames) or planar 'yuv420p8' (uint8) / 'yuv420p10' / 'yuv420p12' / 'yuv420p16' (uint16)") from None
