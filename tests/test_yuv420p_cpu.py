"""Planar 4:2:0 frames without a GPU: every argument guard of emavfi_preprocess_yuv420p / emavfi_postprocess_yuv420p through the C-ABI (all are
refused on the host, before any device work), the Python layer's validation, what the harness accepts and refuses, and the host check."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from emavfi import formats, lib


# valid defaults: W = 64, H = 8 at depth 10: 128 bytes per Y row, 64 per chroma row
def _call_pre(L, y=256, yp=128, ybs=1024, u=2048, up=64, ubs=256, v=4096, vp=64, vbs=256, f32=8192, B=1, H=8, W=64, d=10, st=0, od=0,
              mean=(0.5,) * 3, std=(0.5,) * 3):
    m = (ctypes.c_float * 3)(*mean) if mean is not None else None
    s = (ctypes.c_float * 3)(*std) if std is not None else None
    return L.emavfi_preprocess_yuv420p(y, yp, ybs, u, up, ubs, v, vp, vbs, f32, B, H, W, d, st, od, m, s, None), lib.last_error()


def _call_post(L, y=256, yp=128, ybs=1024, u=2048, up=64, ubs=256, v=4096, vp=64, vbs=256, f32=8192, B=1, H=8, W=64, d=10, st=0, od=0,
               mean=(0.5,) * 3, std=(0.5,) * 3):
    m = (ctypes.c_double * 3)(*mean) if mean is not None else None
    s = (ctypes.c_double * 3)(*std) if std is not None else None
    return L.emavfi_postprocess_yuv420p(f32, y, yp, ybs, u, up, ubs, v, vp, vbs, B, H, W, d, st, od, m, s, 1, None), lib.last_error()


D8 = dict(d=8, yp=64, ybs=512, up=32, ubs=128, vp=32, vbs=128)      # the same frame in bytes


@pytest.mark.parametrize("call", [_call_pre, _call_post])
def test_bad_arguments_are_refused_with_a_message(call):
    """fake (never dereferenced) and null pointers are enough: nothing reaches a device"""
    L = lib.load()
    assert "emavfi_preprocess_yuv420p" in lib.SYMBOLS and "emavfi_postprocess_yuv420p" in lib.SYMBOLS and L.emavfi_version() == 403
    bad = [
        (dict(y=None), "null"), (dict(u=None), "null"), (dict(v=None), "null"), (dict(f32=None), "null"), (dict(mean=None), "null"), (dict(std=None), "null"),
        (dict(d=9), "depth"), (dict(d=11), "depth"), (dict(d=14), "depth"), (dict(d=0), "depth"), (dict(d=-10), "depth"), (dict(d=32), "depth"),
        (dict(st=6), "standard"), (dict(st=-1), "standard"), ({**D8, "st": 4}, "standard"), ({**D8, "st": 5}, "standard"),
        (dict(od=2), "order"), (dict(od=-1), "order"),
        (dict(yp=126), "y_pitch"), (dict(yp=129, ybs=129 * 8), "y_pitch"), ({**D8, "yp": 63}, "y_pitch"),
        (dict(up=62), "u_pitch"), (dict(up=65, ubs=65 * 4), "u_pitch"), ({**D8, "up": 31}, "u_pitch"),
        (dict(vp=62), "v_pitch"), (dict(vp=67, vbs=67 * 4), "v_pitch"), ({**D8, "vp": 31}, "v_pitch"),
        (dict(W=65, yp=130, ybs=130 * 8, up=66, ubs=66 * 4), "v_pitch"),                       # odd W: ceil(65 / 2) = 33 words
        (dict(y=257), "y pointer"), (dict(u=2049), "u pointer"), (dict(v=4099), "v pointer"),
        (dict(B=2, ybs=128 * 7 + 126), "y batch stride"), (dict(B=2, ubs=64 * 3 + 62), "u batch stride"), (dict(B=2, vbs=64 * 3 + 62), "v batch stride"),
        (dict(B=2, ybs=1025), "y batch stride"), (dict(B=2, vbs=257), "v batch stride"),       # large enough, misaligning frame 1
        ({**D8, "B": 2, "ubs": 32 * 3 + 31}, "u batch stride"),
        (dict(std=(0.5, 0.0, 0.5)), "std[1]"),
        (dict(B=0), ">= 1"), (dict(H=0), ">= 1"), (dict(W=0, yp=0, up=0, vp=0), ">= 1"), (dict(B=-1), ">= 1"),
        # with null frame pointers every non-pointer check is still reached and named
        (dict(y=None, u=None, v=None, yp=126), "y_pitch"), (dict(y=None, u=None, v=None, st=7), "standard"), (dict(y=None, u=None, v=None, d=9), "depth"),
        (dict(y=None, u=None, v=None, od=5), "order"), (dict(y=None, u=None, v=None, std=(0.0, 1.0, 1.0)), "std[0]"),
        # huge shapes: the size arithmetic does not wrap
        (dict(B=2, H=2 ** 31 - 1, W=2 ** 31 - 1, yp=2 ** 32, ybs=64, up=2 ** 32, ubs=64, vp=2 ** 32, vbs=64), "batch stride"),
        (dict(B=2, H=2 ** 31 - 1, W=2 ** 31 - 1, yp=2 ** 64 - 2, ybs=2 ** 64 - 2, up=2 ** 64 - 2, ubs=2 ** 64 - 2, vp=2 ** 64 - 2, vbs=2 ** 64 - 2), "batch stride"),
    ]
    for kw, word in bad:
        rc, msg = call(L, **kw)
        assert rc == -1 and word in msg and "yuv420p" in msg, (kw, rc, msg)
    # every depth with every standard of its range passes these checks: the next refusal is the last one
    for d, last in ((8, 4), (10, 6), (12, 6), (16, 6)):
        for st in range(last):
            rc, msg = call(L, **{**(D8 if d == 8 else dict(d=d)), "st": st, "od": st & 1, "f32": 8194})
            assert rc == -1 and "fp32 pointer" in msg, (d, st, msg)
    # depth 8 takes odd pitches, odd batch strides and odd pointers; B = 1 ignores the batch strides
    rc, msg = call(L, d=8, y=257, yp=65, ybs=65 * 8 + 1, u=2049, up=33, ubs=33 * 4 + 1, v=4099, vp=35, vbs=35 * 4 + 1, B=2, f32=8194)
    assert rc == -1 and "fp32 pointer" in msg, msg
    rc, msg = call(L, ybs=0, ubs=1, vbs=3, f32=8194)
    assert rc == -1 and "fp32 pointer" in msg, msg


class _FakePinned:
    """what _yuv420p_planes looks at, of a tensor that claims to be pinned: no device needed"""

    def __init__(self, t):
        self._t = t
        self.dtype, self.shape, self.device, self.is_cuda = t.dtype, t.shape, t.device, False

    def is_pinned(self):
        return True

    def element_size(self):
        return self._t.element_size()

    def dim(self):
        return self._t.dim()

    def stride(self, k):
        return self._t.stride(k)

    def data_ptr(self):
        return self._t.data_ptr()


def test_python_wrappers_validate_before_the_library():
    import torch
    word = lib.word_dtype()
    fake = lambda shape, dt=torch.uint8: _FakePinned(torch.zeros(shape, dtype=dt))
    with pytest.raises(RuntimeError, match="PINNED"):
        lib.preprocess_yuv420p(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.uint8))
    for depth in (True, 9, 14, "8", None):
        with pytest.raises(ValueError, match="depth"):
            lib.preprocess_yuv420p(fake((1, 4, 4)), fake((1, 2, 2)), fake((1, 2, 2)), depth=depth)
    planes = lib._yuv420p_planes
    with pytest.raises(ValueError, match="y must be uint8"):
        planes(fake((1, 4, 4), word), fake((1, 2, 2)), fake((1, 2, 2)), 8, "x")
    with pytest.raises(ValueError, match="v must hold 16-bit"):
        planes(fake((1, 4, 4), word), fake((1, 2, 2), word), fake((1, 2, 2)), 10, "x")
    with pytest.raises(ValueError, match="u must hold 16-bit"):
        planes(fake((1, 4, 4), word), fake((1, 2, 2), torch.float16), fake((1, 2, 2), word), 10, "x")
    with pytest.raises(ValueError, match="u must be a 3-d"):
        planes(fake((1, 4, 4)), fake((1, 2, 2, 1)), fake((1, 2, 2)), 8, "x")
    with pytest.raises(ValueError, match=r"u must be \(1, 3, 4\)"):
        planes(fake((1, 5, 7)), fake((1, 2, 4)), fake((1, 3, 4)), 8, "x")
    with pytest.raises(ValueError, match=r"v must be \(1, 3, 4\)"):
        planes(fake((1, 5, 7)), fake((1, 3, 4)), fake((1, 3, 3)), 8, "x")
    with pytest.raises(ValueError, match="y is empty"):
        planes(fake((1, 0, 4)), fake((1, 0, 2)), fake((1, 0, 2)), 8, "x")
    with pytest.raises(ValueError, match="rows of v must be dense"):
        planes(fake((1, 4, 8)), fake((1, 2, 4)), _FakePinned(torch.zeros(1, 2, 8, dtype=torch.uint8)[:, :, ::2]), 8, "x")
    # pitches and batch strides come from .stride(), in BYTES, per plane
    y, u, v = torch.zeros(2, 5, 7, dtype=torch.uint8), torch.zeros(2, 3, 6, dtype=torch.uint8)[:, :, :4], torch.zeros(3, 3, 4, dtype=torch.uint8)[::2]
    B, H, W, p = planes(_FakePinned(y), _FakePinned(u), _FakePinned(v), 8, "x")
    assert (B, H, W) == (2, 5, 7) and p == [y.data_ptr(), 7, 35, u.data_ptr(), 6, 18, v.data_ptr(), 4, 24]
    yw, uw, vw = torch.zeros(2, 5, 7, dtype=word), torch.zeros(2, 3, 6, dtype=word)[:, :, :4], torch.zeros(2, 3, 4, dtype=torch.int16)
    assert planes(_FakePinned(yw), _FakePinned(uw), _FakePinned(vw), 12, "x")[3] == [yw.data_ptr(), 14, 70, uw.data_ptr(), 12, 36, vw.data_ptr(), 8, 24]
    one = torch.zeros(1, 1, 1, dtype=word)                                # size-1 dimensions: the dense values stand in
    assert planes(_FakePinned(one), _FakePinned(one), _FakePinned(one), 16, "x")[3][1:3] == [2, 2]
    with pytest.raises(ValueError, match="bt601"):                        # BT.2020 belongs to the deeper formats
        lib.preprocess_yuv420p(fake((1, 4, 4)), fake((1, 2, 2)), fake((1, 2, 2)), 8, "bt2020")
    with pytest.raises(ValueError, match="bt2020"):
        lib.preprocess_yuv420p(fake((1, 4, 4), word), fake((1, 2, 2), word), fake((1, 2, 2), word), 10, "bt2100")
    with pytest.raises(ValueError, match="order"):
        lib.preprocess_yuv420p(fake((1, 4, 4)), fake((1, 2, 2)), fake((1, 2, 2)), 8, order="gbr")
    with pytest.raises(ValueError, match="uint16"):
        lib.preprocess_yuv420p(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 2, 2), np.uint16), np.zeros((1, 2, 2), np.uint16), 10)
    assert lib.PLANAR_DEPTHS == {"yuv420p8": 8, "yuv420p10": 10, "yuv420p12": 12, "yuv420p16": 16}


def test_frame_interpolator_accepts_and_refuses():
    from emavfi import EMA_VFI, FrameInterpolator
    model = EMA_VFI(mid_channels=8)
    for fmt in ("yuv420p8", "yuv420p10", "yuv420p12", "yuv420p16"):
        with pytest.raises(RuntimeError, match="no CPU path"):      # a known format gets as far as the device check
            FrameInterpolator(model, pixel_format=fmt)
    for kw in (dict(scale=0.5), dict(size=(24, 40)), dict(scene_threshold=0.2), dict(size=(24, 40), scene_threshold=0.2, mode="recursive", interpolation_factor=3)):
        with pytest.raises(RuntimeError, match="no CPU path"):      # the byte format takes them all, as NV12 does
            FrameInterpolator(model, pixel_format="yuv420p8", **kw)
    for fmt in ("yuv420p10", "yuv420p12", "yuv420p16"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            FrameInterpolator(model, pixel_format=fmt, yuv_standard="bt2020", yuv_full_range=True)
        with pytest.raises(ValueError, match=f"{fmt}.*scale / size"):
            FrameInterpolator(model, pixel_format=fmt, scale=0.5)
        with pytest.raises(ValueError, match=f"{fmt}.*scale / size"):
            FrameInterpolator(model, pixel_format=fmt, size=(24, 40))
        with pytest.raises(ValueError, match=f"{fmt}.*scene_threshold"):
            FrameInterpolator(model, pixel_format=fmt, scene_threshold=0.2)
        with pytest.raises(ValueError, match="bt2020"):
            FrameInterpolator(model, pixel_format=fmt, yuv_standard="bt2100")
        fi = FrameInterpolator.__new__(FrameInterpolator)         # evaluate() refuses before it touches a frame or the device
        fi.fmt = formats.FORMATS[fmt]
        with pytest.raises(ValueError, match=f"evaluate.*{fmt}"):
            fi.evaluate([np.zeros((36, 40), np.uint16)] * 3)
    with pytest.raises(ValueError, match="bt601"):
        FrameInterpolator(model, pixel_format="yuv420p8", yuv_standard="bt2020")
    with pytest.raises(ValueError, match="even destination"):
        FrameInterpolator(model, pixel_format="yuv420p8", size=(25, 40))
    with pytest.raises(ValueError, match="yuv420p8.*even destination"):
        FrameInterpolator.output_size(100, 90, scale=0.5, pixel_format="yuv420p8")
    assert FrameInterpolator.output_size(100, 88, scale=0.5, pixel_format="yuv420p8") == (50, 44)
    for name in ("i420", "yuv420p", "p014", "yuv420p14", "yv12", "YUV420P8"):      # the names that stay refused
        with pytest.raises(ValueError, match="pixel_format"):
            FrameInterpolator(model, pixel_format=name)


def test_planar_views_of_a_frame_buffer():
    """the harness's plane views: the chroma planes are dense and need not start on a row of the [H*3/2, W] array"""
    import torch
    H, W, n = 6, 4, 2                                     # U starts at row 6, V in the MIDDLE of row 7
    for fmt, wb in (("yuv420p8", W), ("yuv420p10", 2 * W)):
        depth = 0 if fmt == "yuv420p8" else 10
        buf = torch.arange(n * (H * 3 // 2) * wb, dtype=torch.int32).to(torch.uint8).view(n, H * 3 // 2, wb)
        y, u, v = formats.FORMATS[fmt].planes(buf)
        es = 2 if depth else 1
        assert tuple(y.shape) == (n, H, W) and tuple(u.shape) == tuple(v.shape) == (n, H // 2, W // 2) and y.element_size() == es
        frame = H * 3 // 2 * wb
        for k in range(n):
            assert y[k].data_ptr() == buf.data_ptr() + k * frame
            assert u[k].data_ptr() == buf.data_ptr() + k * frame + H * W * es
            assert v[k].data_ptr() == u[k].data_ptr() + H * W * es // 4
        assert (u.stride(1), u.stride(2), u.stride(0) * es) == (W // 2, 1, frame)
        flat = buf[1].reshape(-1).view(torch.int16 if depth else torch.uint8)
        assert torch.equal(u[1].reshape(-1), flat[H * W:H * W + H * W // 4]) and torch.equal(v[1].reshape(-1), flat[H * W * 5 // 4:])
    # the NV12 layout, bytes and words: the UV rows follow the Y rows, one U,V pair per chroma position
    for fmt, wb in (("nv12", W), ("p010", 2 * W)):
        es = wb // W
        buf = torch.arange(n * (H * 3 // 2) * wb, dtype=torch.int32).to(torch.uint8).view(n, H * 3 // 2, wb)
        y, uv = formats.FORMATS[fmt].planes(buf)
        assert tuple(y.shape) == (n, H, W) and tuple(uv.shape) == (n, H // 2, W // 2, 2) and y.element_size() == uv.element_size() == es
        frame = H * 3 // 2 * wb
        for k in range(n):
            assert y[k].data_ptr() == buf.data_ptr() + k * frame
            assert uv[k].data_ptr() == buf.data_ptr() + k * frame + H * W * es
            assert uv[k, 1, 1, 1].data_ptr() == uv[k].data_ptr() + (W + 3) * es      # row 1, pair 1, V: one row of W samples and three more
        assert (y.stride(0) * es, y.stride(1), y.stride(2)) == (frame, W, 1) and (uv.stride(0) * es, uv.stride(1), uv.stride(2), uv.stride(3)) == (frame, W, 2, 1)
        flat = buf[1].reshape(-1).view(torch.int16 if es == 2 else torch.uint8)
        assert torch.equal(y[1].reshape(-1), flat[:H * W]) and torch.equal(uv[1].reshape(-1), flat[H * W:])
    # interleaved frames are their own single plane
    buf = torch.zeros(n, H, W, 3, dtype=torch.uint8)
    assert formats.FORMATS["bgr24"].planes(buf)[0] is buf and len(formats.FORMATS["bgr24"].planes(buf)) == 1


def test_yuv420p_host_check_runs_clean_under_asan_ubsan():
    """the sanitizer build of the host side (csrc/Makefile, `make asan`) also builds tests/host/host_check_yuv420p, a stand-alone program: every
    guard of the two entries (huge shapes included) and the per-element path against the interleaved element functions, under ASan + UBSan"""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(llvm) or shutil.which("make") is None:
        pytest.skip("ROCm clang not available")
    rt = subprocess.run([llvm, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("no shared ASan runtime in this toolchain")
    csrc = os.path.join(ROOT, "video-frame-interpolation_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "asan", "-j", str(min(8, os.cpu_count() or 1))], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "build", "csrc_asan", "host_check_yuv420p")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               LD_LIBRARY_PATH=os.path.dirname(rt) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "host_check_yuv420p: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
