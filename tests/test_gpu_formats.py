"""Every pixel format through the harness's pre / post kernels (FrameInterpolator._pre_kernel / _post_kernel, which take their plane views
from emavfi.formats), bit for bit against the same lib calls on planes the test cuts out of the byte buffer itself."""
import numpy as np
import pytest

from emavfi import EMA_VFI, FrameInterpolator, lib, synth
from test_formats_cpu import ROWS


@pytest.fixture(scope="module")
def model():
    m = EMA_VFI(mid_channels=8, compute_dtype="fp32").cuda().eval()
    m.load_state_dict(synth.synthetic_state_dict(seed=0, mid_channels=8), strict=True)
    return m


def own_planes(name, buf, H, W, rect=None):
    """the planes of the frames in `buf` (uint8 [n, ...] on the device), cut to `rect` = (top, left, height, width), by pointer arithmetic
    over the samples: torch.as_strided, not the record's views"""
    import torch
    layout, C, sb, depth, shift = ROWS[name]
    t, l, h, w = rect or (0, 0, H, W)
    n = buf.shape[0]
    if layout == "interleaved":
        return [torch.as_strided(buf, (n, h, w, 3), (H * W * 3, W * 3, 3, 1), (t * W + l) * 3)]
    flat = buf.view(n, -1)
    flat = flat.view(torch.int16) if sb == 2 else flat
    F, S = H * W * 3 // 2, H * W                                 # samples per frame, per Y plane
    y = torch.as_strided(flat, (n, h, w), (F, W, 1), t * W + l)
    if layout == "NV12":
        return [y, torch.as_strided(flat, (n, h // 2, w // 2, 2), (F, W, 2, 1), S + (t // 2) * W + l)]
    at = (t // 2) * (W // 2) + l // 2
    return [y] + [torch.as_strided(flat, (n, h // 2, w // 2), (F, W // 2, 1), S + k * (S // 4) + at) for k in (0, 1)]


def own_calls(name, pitched=False):
    """(preprocess(planes), postprocess(x, planes)) of lib for the format, denormalize off; `pitched`: interleaved frames have an entry of
    their own for views with a pitch"""
    layout, C, sb, depth, shift = ROWS[name]
    if layout == "interleaved" and pitched:
        return (lambda p: lib.preprocess_u8_pitched(p[0]), lambda x, p: lib.postprocess_u8_pitched(x, p[0], denormalize=False))
    if layout == "interleaved":
        return (lambda p: lib.preprocess_u8(p[0]), lambda x, p: lib.postprocess_u8(x, denormalize=False, out=p[0]))
    if layout == "I420":
        return (lambda p: lib.preprocess_yuv420p(*p, depth), lambda x, p: lib.postprocess_yuv420p(x, depth, denormalize=False, out=tuple(p)))
    if sb == 2:
        return (lambda p: lib.preprocess_p010(*p, depth), lambda x, p: lib.postprocess_p010(x, depth, denormalize=False, out=tuple(p)))
    return (lambda p: lib.preprocess_nv12(*p), lambda x, p: lib.postprocess_nv12(x, denormalize=False, out=tuple(p)))


def staged(name, n, H, W, seed):
    """n frames of valid random samples as the harness stages them: uint8 [n, *byte shape] on the device"""
    import torch
    layout, C, sb, depth, shift = ROWS[name]
    rng = np.random.default_rng(seed)
    count = n * H * W * 3 // (1 if layout == "interleaved" else 2)       # samples: 4:2:0 has half a chroma pair per pixel
    samples = (rng.integers(0, 1 << depth, count) << shift).astype(np.uint8 if sb == 1 else np.uint16)
    shape = (n, H, W, 3) if layout == "interleaved" else (n, H * 3 // 2, W * sb)
    return torch.from_numpy(samples.view(np.uint8).reshape(shape)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_pre_and_post_kernel_of_every_format(model, name):
    """H = 6, W = 4: the smallest frame whose U plane starts on a row boundary and whose V plane starts in the middle of a row"""
    import torch
    n, H, W = 2, 6, 4
    fi = FrameInterpolator(model, reference_quirks=False, pixel_format=name)
    pre, post = own_calls(name)
    buf = staged(name, n, H, W, 7)
    x = fi._pre_kernel(buf)
    want = pre(own_planes(name, buf, H, W))
    assert tuple(x.shape) == (n, 3, H, W) and torch.equal(x, want)
    got = fi._post_kernel(x, False)
    ref = torch.full_like(buf, 0xA5)
    post(want, own_planes(name, ref, H, W))
    assert got.dtype == torch.uint8 and got.shape == buf.shape and torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bgr24", "nv12", "p010", "yuv420p10"])
def test_pre_and_post_kernel_inside_an_active_rectangle(model, name):
    """H = 8, W = 48 with the rectangle (2, 16, 4, 16), edges on multiples of ACTIVE_ALIGN = (2, 16): the kernels read and write inside
    it, and no byte of `out` outside it changes"""
    import torch
    n, H, W, rect = 2, 8, 48, (2, 16, 4, 16)
    assert lib.ACTIVE_ALIGN == (2, 16)
    fi = FrameInterpolator(model, reference_quirks=False, pixel_format=name, active_area=rect)
    fi._dst = (H, W)
    fi._set_active(rect)
    pre, post = own_calls(name, pitched=True)
    buf = staged(name, n, H, W, 11)
    x = fi._pre_kernel(buf)
    want = pre(own_planes(name, buf, H, W, rect))
    assert tuple(x.shape) == (n, 3, rect[2], rect[3]) and torch.equal(x, want)
    out, ref, inside = torch.full_like(buf, 0xA5), torch.full_like(buf, 0xA5), torch.zeros_like(buf)
    assert fi._post_kernel(x, False, out=out) is out
    post(want, own_planes(name, ref, H, W, rect))
    assert torch.equal(out, ref)
    for p in own_planes(name, inside, H, W, rect):
        p.fill_(-1 if p.dtype == torch.int16 else 255)
    assert int((inside != 0).sum()) == n * rect[2] * rect[3] * ROWS[name][2] * 3 // (1 if name == "bgr24" else 2)     # the rectangle's bytes
    assert bool((out[inside == 0] == 0xA5).all())
