"""emavfi.formats: the one table of pixel formats behind lib and the harness.  The rows, and what is derived from them, against the
constructor and lib's tuples (tests/test_gpu_formats.py runs every format through the harness's pre / post kernels)."""
import numpy as np
import pytest

from emavfi import EMA_VFI, FrameInterpolator, formats, lib

# name: (layout, C, sample_bytes, depth, shift)
ROWS = {
    "bgr24": ("interleaved", 3, 1, 8, 0),
    "nv12": ("NV12", 1, 1, 8, 0),
    "p010": ("NV12", 1, 2, 10, 6),
    "p012": ("NV12", 1, 2, 12, 4),
    "p016": ("NV12", 1, 2, 16, 0),
    "yuv420p8": ("I420", 1, 1, 8, 0),
    "yuv420p10": ("I420", 1, 2, 10, 0),
    "yuv420p12": ("I420", 1, 2, 12, 0),
    "yuv420p16": ("I420", 1, 2, 16, 0),
}
LAYOUTS = {"interleaved": 0, "NV12": 1, "I420": 2}     # EMAVFI_LAYOUT_*
REFUSED = ("i420", "yuv420p", "p014", "yuv420p14", "yv12", "YUV420P8")


def test_the_nine_rows():
    assert list(formats.FORMATS) == list(ROWS)
    for name, (layout, C, sb, depth, shift) in ROWS.items():
        f = formats.lookup(name)
        assert (f.name, f.layout, f.C, f.sample_bytes, f.depth, f.shift) == (name, LAYOUTS[layout], C, sb, depth, shift)
        with pytest.raises(AttributeError):      # frozen
            f.depth = 9
    assert (lib.LAYOUT_INTERLEAVED, lib.LAYOUT_NV12, lib.LAYOUT_I420) == (0, 1, 2) == (formats.LAYOUT_INTERLEAVED, formats.LAYOUT_NV12, formats.LAYOUT_I420)
    assert lib.DEPTHS == {"p010": 10, "p012": 12, "p016": 16}
    assert lib.PLANAR_DEPTHS == {"yuv420p8": 8, "yuv420p10": 10, "yuv420p12": 12, "yuv420p16": 16}


def test_the_tuples_are_what_lib_hands_out():
    for name, (layout, C, sb, depth, shift) in ROWS.items():
        f = formats.FORMATS[name]
        assert f.sample_format == lib.resample_sample_format(name) == (sb, depth, shift)
        assert f.frame_format == lib.static_frame_format(name) == (LAYOUTS[layout], C, sb, depth, shift)


def test_names_that_stay_refused():
    model = EMA_VFI(mid_channels=8)
    for name in REFUSED:
        with pytest.raises(ValueError, match="pixel_format must be 'bgr24'"):
            formats.lookup(name)
        with pytest.raises(ValueError, match="pixel_format must be 'bgr24'"):
            FrameInterpolator(model, pixel_format=name)
        with pytest.raises(ValueError, match="pixel_format"):
            lib.static_frame_format(name)


def accepted(model, **kw):
    """the constructor takes the arguments (it then gets as far as the device check: the model lives on the CPU) or refuses them"""
    try:
        FrameInterpolator(model, **kw)
    except RuntimeError as e:
        assert "no CPU path" in str(e)
        return True
    except ValueError:
        return False
    raise AssertionError("a FrameInterpolator on a CPU model")


def test_the_capability_flags_are_the_constructors():
    model = EMA_VFI(mid_channels=8)
    mixes = dict(mode="resample", reference_quirks=False, rate_in=24, rate_out=60, resample_method="blend")
    for name, (layout, C, sb, depth, shift) in ROWS.items():
        f = formats.FORMATS[name]
        assert accepted(model, pixel_format=name)
        assert f.byte_kernels == (sb == 1) == accepted(model, pixel_format=name, scale=0.5) == accepted(model, pixel_format=name, size=(24, 40))
        assert f.byte_kernels == accepted(model, pixel_format=name, scene_threshold=0.2)
        assert f.light_table_fits == (depth <= 12) == accepted(model, pixel_format=name, light="bt709", **mixes)
        assert f.takes_bt2020 == (sb == 2) == accepted(model, pixel_format=name, yuv_standard="bt2020")
        assert f.even_resize == (name in ("nv12", "yuv420p8"))
        if f.byte_kernels:
            assert accepted(model, pixel_format=name, size=(25, 41)) == (not f.even_resize)
            assert FrameInterpolator.output_size(100, 88, scale=0.5, pixel_format=name) == (50, 44)
        assert f.yuv == (name != "bgr24") and f.words == (sb == 2)
        # evaluate() on a bare interpolator: a word format is refused before a frame or the device is touched
        fi = FrameInterpolator.__new__(FrameInterpolator)
        fi.fmt = f
        if f.byte_kernels:
            assert fi.evaluate([]).channels == (1 if f.yuv else 3)
        else:
            with pytest.raises(ValueError, match=f"evaluate.*{name}"):
                fi.evaluate([])


def test_shapes_round_trip_at_6_by_4():
    import torch
    H, W, n = 6, 4, 2
    for name, (layout, C, sb, depth, shift) in ROWS.items():
        f = formats.FORMATS[name]
        shape = f.byte_shape(H, W)
        assert shape == ((H, W, 3) if layout == "interleaved" else (H * 3 // 2, W * sb))
        assert f.geometry(shape) == (H, W, 3)
        nbytes = int(np.prod(shape))
        assert f.luma_bytes(nbytes) == (nbytes if layout == "interleaved" else H * W * sb)
        assert f.dtype == np.dtype(np.uint8 if sb == 1 else np.uint16) and f.rank == len(shape) and f.display == name.upper()
        # a frame as it arrives, its bytes, and back
        frame = np.arange(nbytes // sb, dtype=f.dtype).reshape(shape[:-1] + (shape[-1] // sb,))
        raw = f.as_bytes(frame)
        assert raw.dtype == np.uint8 and raw.shape == shape and np.shares_memory(raw, frame)
        back = f.as_samples(raw)
        assert back.dtype == frame.dtype and np.array_equal(back, frame) and np.shares_memory(back, frame)
        f.check_frames([frame, frame.copy()], frame, "x")
        with pytest.raises(ValueError, match=f"x: same-shape {'uint8' if sb == 1 else 'uint16'}"):
            f.check_frames([frame.astype(np.uint32)], frame, "x")
        with pytest.raises(ValueError, match="same-shape"):
            f.check_frames([frame[:-1]], frame, "x")
        if f.yuv:
            with pytest.raises(ValueError, match=f"{name.upper()} layout .* needs even H and W"):
                f.check_frames([frame[:-1]], frame[:-1], "x")
        # the plane views and the luma image of n frames
        buf = torch.zeros(n, *shape, dtype=torch.uint8)
        planes = f.planes(buf)
        want = {"interleaved": [(n, H, W, 3)], "NV12": [(n, H, W), (n, H // 2, W // 2, 2)], "I420": [(n, H, W)] + [(n, H // 2, W // 2)] * 2}[layout]
        assert [tuple(p.shape) for p in planes] == want and all(p.element_size() == sb for p in planes)
        luma = f.luma(buf)
        assert tuple(luma.shape) == ((n, H, W, 3) if layout == "interleaved" else (n, H, W, 1) if sb == 1 else (n, H, W))
        assert luma.data_ptr() == buf.data_ptr() and luma.element_size() == sb
