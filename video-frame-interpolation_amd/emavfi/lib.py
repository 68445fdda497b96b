"""ctypes binding of libemavfi.so (C-ABI: include/emavfi.h).

There is deliberately no fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes
import numbers
import os
import collections
import threading
from ctypes import c_int, c_size_t, c_void_p, c_char_p, POINTER

from .formats import FORMATS, LAYOUT_INTERLEAVED, LAYOUT_NV12, LAYOUT_I420   # EMAVFI_LAYOUT_*

F32, BF16, F16, AMP16, F32X3 = 0, 1, 2, 3, 4
ACT_NONE, ACT_RELU, ACT_TANH01 = 0, 1, 2
MDCN_IN_F16, MDCN_OUT_F16, MDCN_SPLIT_TAIL = 1, 2, 4
# emavfi_debug_switches bits (include/emavfi.h)
SW_NO_CONV_FIRST, SW_NO_FIRSTRING, SW_NO_HEAD, SW_NO_TAILFUSE, SW_NO_CONV_LIGHT, SW_NO_PERSISTENT_CONV, SW_NO_RING2, SW_NO_POOLFUSE, SW_RING_ONE_WG, SW_NO_RING_CHUNK = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
DTYPES = {"fp32": F32, "f32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16,
          "fp16": F16, "f16": F16, "float16": F16, "half": F16,
          # the reference's forward under torch.cuda.amp.autocast(), op policy restated (include/emavfi.h, EMAVFI_AMP16)
          "amp16": AMP16, "autocast": AMP16, "autocast16": AMP16,
          # fp32-accurate three-term f16 split on the 16-bit matrix pipe; fp32 DCN sampling, its contraction on the split at the reference width (include/emavfi.h, EMAVFI_F32X3)
          "fp32x3": F32X3, "f32x3": F32X3}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EMAVFI_LIB", os.path.join(_HERE, "lib", "libemavfi.so"))

# every symbol include/emavfi.h declares: (restype, argtypes)
_PROTOTYPES = {
    "emavfi_version": (c_int, []),
    "emavfi_last_error": (c_char_p, []),
    "emavfi_supported": (c_int, [c_int] * 4),
    "emavfi_param_count": (c_int, [c_int]),
    "emavfi_packed_bytes": (c_size_t, [c_int] * 4),
    "emavfi_pack_weights": (c_int, [c_int] * 3 + [POINTER(c_void_p), c_int, c_void_p, c_size_t, c_int, c_void_p]),
    "emavfi_workspace_bytes": (c_size_t, [c_int] * 7),
    "emavfi_layout_tag": (c_int, []),
    "emavfi_packed_check": (c_int, [c_int] * 4 + [c_void_p, c_size_t]),
    "emavfi_forward": (c_int, [c_int] * 3 + [c_void_p, c_size_t] + [c_void_p] * 4 + [c_size_t] + [c_int] * 4 + [POINTER(c_void_p), c_void_p]),
    "emavfi_forward_launches": (c_int, [c_int] * 7 + [c_char_p, c_size_t, POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int]),
    "emavfi_warp": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p]),
    "emavfi_preprocess_u8": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_postprocess_u8": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int, c_void_p]),
    "emavfi_yuv_coefficients": (c_int, [c_int, POINTER(c_int), POINTER(c_int)]),
    "emavfi_preprocess_nv12": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_void_p] + [c_int] * 5
                               + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_postprocess_nv12": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 5
                                + [POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int, c_void_p]),
    "emavfi_yuv_coefficients_depth": (c_int, [c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "emavfi_preprocess_p010": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_void_p] + [c_int] * 6
                               + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_postprocess_p010": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 6
                                + [POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int, c_void_p]),
    "emavfi_preprocess_yuv420p": (c_int, [c_void_p, c_size_t, c_size_t] * 3 + [c_void_p] + [c_int] * 6
                                  + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_postprocess_yuv420p": (c_int, [c_void_p] + [c_void_p, c_size_t, c_size_t] * 3 + [c_int] * 6
                                   + [POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int, c_void_p]),
    "emavfi_resize_u8": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 6 + [c_void_p]),
    "emavfi_preprocess_u8_resized": (c_int, [c_void_p] * 3 + [c_int] * 6 + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_preprocess_nv12_resized": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_void_p,
                                               c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 7
                                       + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_luma_signature_u8": (c_int, [c_void_p, c_size_t, c_size_t] + [c_int] * 5 + [c_void_p, c_void_p]),
    "emavfi_scene_flags": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t] + [c_int] * 3 + [ctypes.c_uint, c_void_p, c_void_p, c_void_p]),
    "emavfi_hold_frames_u8": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_void_p, c_int, c_size_t, c_void_p]),
    "emavfi_resample_frames": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_int,
                                       c_size_t, c_int, c_int, c_int, c_void_p]),
    "emavfi_accumulate_frames": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_void_p, c_int,
                                         c_size_t, c_int, c_int, c_int, c_void_p]),
    "emavfi_transfer_table": (c_int, [c_int, c_int, c_int, c_void_p]),
    "emavfi_transfer_table_check": (c_int, [c_void_p, c_int]),
    "emavfi_accumulate_frames_linear": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p, c_void_p,
                                                c_int, c_size_t, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "emavfi_frame_diff_cells": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 8 + [c_void_p, c_void_p]),
    "emavfi_duplicate_flags": (c_int, [c_void_p, c_size_t, c_int, ctypes.c_uint, c_void_p, c_void_p, c_void_p]),
    "emavfi_static_guard_frames": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p] + [c_int] * 8
                                   + [ctypes.c_uint, c_void_p, c_void_p]),
    "emavfi_active_bounds": (c_int, [c_void_p, c_size_t, c_size_t] + [c_int] * 7 + [ctypes.c_uint, c_void_p, c_void_p]),
    "emavfi_fill_outside_frames": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_size_t, c_int, c_void_p] + [c_int] * 9 + [c_void_p]),
    "emavfi_preprocess_u8_pitched": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p] + [c_int] * 4
                                     + [POINTER(ctypes.c_float), POINTER(ctypes.c_float), c_void_p]),
    "emavfi_postprocess_u8_pitched": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t] + [c_int] * 4
                                      + [POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int, c_void_p]),
    "emavfi_flip_f32": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "emavfi_ensemble_mean_f32": (c_int, [POINTER(c_void_p), POINTER(c_int), c_int, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "emavfi_border_pad_f32": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_void_p]),
    "emavfi_border_crop_f32": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "emavfi_downscale_f32": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "emavfi_upsample_flow_f32": (c_int, [c_void_p, c_void_p, c_size_t] + [c_int] * 5 + [c_void_p]),
    "emavfi_forward_flow": (c_int, [c_int] * 3 + [c_void_p, c_size_t] + [c_void_p] * 4 + [c_size_t] + [c_int] * 4 + [c_void_p]),
    "emavfi_forward_given_flow": (c_int, [c_int] * 3 + [c_void_p, c_size_t] + [c_void_p] * 5 + [c_size_t] + [c_int] * 4
                                  + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, ctypes.c_uint, c_void_p]),
    "emavfi_forward_flow_launches": (c_int, [c_int] * 7 + [c_char_p, c_size_t, POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int]),
    "emavfi_forward_given_flow_launches": (c_int, [c_int] * 7 + [ctypes.c_uint, c_char_p, c_size_t, POINTER(ctypes.c_double),
                                                                 POINTER(ctypes.c_double), c_int]),
    "emavfi_agreement_guard_f32": (c_int, [c_void_p] * 5 + [c_int] * 5 + [ctypes.c_float, POINTER(ctypes.c_float), POINTER(ctypes.c_float),
                                           c_void_p, c_void_p]),
    "emavfi_align_signature_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "emavfi_align_workspace_bytes": (c_size_t, [c_int] * 2),
    "emavfi_align_search": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "emavfi_shift_f32": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_int, c_void_p]),
    "emavfi_frame_metrics_workspace_bytes": (c_size_t, [c_int] * 4),
    "emavfi_frame_metrics_u8": (c_int, [c_void_p, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t] + [c_int] * 4
                                + [c_void_p, c_void_p, c_size_t, c_void_p]),
    "emavfi_conv3x3_workspace_bytes": (c_size_t, [c_int] * 7),
    "emavfi_conv3x3": (c_int, [c_void_p] * 4 + [c_int] * 8 + [c_void_p, c_size_t, c_void_p]),
    "emavfi_deform_conv2d_workspace_bytes": (c_size_t, [c_int] * 6),
    "emavfi_deform_conv2d": (c_int, [c_void_p] * 6 + [c_int] * 6 + [c_void_p, c_size_t, c_void_p]),
    "emavfi_mdcn_workspace_bytes": (c_size_t, [c_int] * 6),
    "emavfi_mdcn": (c_int, [c_void_p] * 6 + [c_int] * 6 + [c_void_p, c_size_t, c_void_p]),
    "emavfi_forward_census": (c_int, [c_int] * 7 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "emavfi_mdcn_census": (c_int, [c_int] * 6 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "emavfi_forward_routed": (c_int, [c_int] * 3 + [c_void_p, c_size_t] + [c_void_p] * 4 + [c_size_t] + [c_int] * 4
                              + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, ctypes.c_uint, c_void_p]),
    "emavfi_forward_launches_routed": (c_int, [c_int] * 7 + [ctypes.c_uint, c_char_p, c_size_t, POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int]),
    "emavfi_mdcn_routed": (c_int, [c_void_p] * 6 + [c_int] * 7 + [c_void_p, c_size_t, POINTER(c_void_p), c_int, c_void_p]),
    "emavfi_route_state_bytes": (c_size_t, []),
    "emavfi_route_state_init": (c_int, [c_void_p, c_int, ctypes.c_uint, c_void_p]),
    "emavfi_forward_adaptive": (c_int, [c_int] * 3 + [c_void_p, c_size_t] + [c_void_p] * 4 + [c_size_t] + [c_int] * 4
                                + [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, c_void_p, ctypes.c_float, ctypes.c_float, c_void_p]),
    "emavfi_forward_launches_adaptive": (c_int, [c_int] * 7 + [c_char_p, c_size_t, POINTER(ctypes.c_double), POINTER(ctypes.c_double), c_int]),
    "emavfi_context_workspace_bytes": (c_size_t, [c_int] * 5),
    "emavfi_context": (c_int, [c_void_p, POINTER(c_void_p), c_void_p] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p]),
    "emavfi_reconstruct_workspace_bytes": (c_size_t, [c_int] * 5),
    "emavfi_reconstruct": (c_int, [c_void_p, POINTER(c_void_p), c_void_p] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p]),
    "emavfi_debug_switches": (c_int, [c_int, c_int]),
}
SYMBOLS = tuple(_PROTOTYPES)

_lib = None
_lock = threading.Lock()


def load() -> ctypes.CDLL:
    """Load libemavfi.so once; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"libemavfi.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` or `make -C video-frame-interpolation_amd/csrc` (hipcc, gfx950). "
                        "There is no CPU or PyTorch fallback for this path.")
                lib = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in _PROTOTYPES.items():
                    fn = getattr(lib, name)
                    fn.restype, fn.argtypes = res, args
                _lib = lib
    return _lib


_fingerprint = None


def fingerprint() -> str:
    """sha256 of the loaded libemavfi.so: part of the key of the on-disk packed-weight cache (the packed layout is a
    property of the build, not of emavfi_version())."""
    global _fingerprint
    if _fingerprint is None:
        import hashlib
        load()
        with open(LIB_PATH, "rb") as f:
            _fingerprint = hashlib.sha256(f.read()).hexdigest()
    return _fingerprint


def layout_switches() -> str:
    """The process-wide switches the PACKED LAYOUT depends on, as the LIBRARY latched them at first use (emavfi_layout_tag(),
    include/emavfi.h) - not os.environ, which may have changed since (two sources of truth).  Part of the in-memory and
    on-disk cache keys of the packed weights; the blob header carries the same tag and emavfi_packed_check compares it."""
    return f"layout_tag={load().emavfi_layout_tag()}"


def packed_check(in_channels, mid_channels, num_blocks, dt, blob) -> None:
    """emavfi_packed_check on a uint8 tensor (device or host): header fields and payload checksum; RuntimeError names the mismatch.
    Synchronises - call when a blob ARRIVES (cache file, broadcast, load_packed_weights), never per frame."""
    if not blob.is_contiguous():
        raise ValueError("packed_check: contiguous uint8 tensor expected")
    check(load().emavfi_packed_check(in_channels, mid_channels, num_blocks, dt, blob.data_ptr(), blob.numel()), "emavfi_packed_check")


def debug_switches(and_mask=-1, or_mask=0) -> int:
    """Test hook (include/emavfi.h, emavfi_debug_switches): returns the previous switch word."""
    return load().emavfi_debug_switches(and_mask, or_mask)


def last_error() -> str:
    return (load().emavfi_last_error() or b"").decode("utf-8", "replace")


def check(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError(f"{what} failed ({code}): {last_error()}")


def dtype_code(name) -> int:
    if isinstance(name, int):
        return name
    try:
        return DTYPES[str(name).lower()]
    except KeyError:
        raise ValueError(f"compute dtype must be one of {sorted(DTYPES)}, got {name!r}") from None


def _stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _events_arg(_events):
    """The `_events` measurement argument (bench.py): (c_void_p to an array of hipEvent_t, count) or None -> the C-ABI's
    (events, n_events)."""
    return (ctypes.cast(_events[0], POINTER(c_void_p)), _events[1]) if _events is not None else (None, 0)


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("emavfi: tensors must live on a ROCm device (MI355X); "
                               "this build has no CPU path - use the reference or the oracle for CPU runs")


def _f32c(t):
    import torch
    return t.detach().to(torch.float32).contiguous()


# Scratch memory (caller-owned, as the C-ABI requires): one grow-only buffer per (device, stream).
#   * two streams (or two threads on different streams) never share scratch - forwards on different streams may
#     run concurrently;
#   * a buffer is allocated while its stream is current, so the caching allocator's stream-ordered reuse makes
#     dropping the old buffer on growth safe: it was only ever used on that stream;
#   * a buffer that was handed out while its stream was being captured into a hipGraph has its address baked into the
#     graph: it is never freed on growth but parked in _ws_graph_held (until release_workspaces()), so replaying the
#     graph after a later, larger forward still writes to memory nobody else owns;
#   * the cache holds at most EMAVFI_WS_CACHE_MAX (default 8) buffers: a caller that runs forwards on transient streams would
#     otherwise pin one workspace (GBs at B = 8 x 720p) per stream handle it ever used.  The least recently used buffer that no
#     captured graph may point at is dropped first (the caching allocator keeps a freed block on its allocation stream's pool,
#     so work still queued on that stream is not disturbed).  Captured buffers are only released by release_workspaces().
_ws_cache = collections.OrderedDict()   # (device index, stream handle) -> uint8 tensor, least recently used first
_ws_captured = set()  # keys whose current buffer a captured graph may point at
_ws_graph_held = []
_ws_lock = threading.Lock()


def workspace(nbytes: int, device):
    import torch
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, torch.cuda.current_stream(device).cuda_stream)
    capturing = torch.cuda.is_current_stream_capturing()
    with _ws_lock:
        buf = _ws_cache.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None and key in _ws_captured:
                _ws_graph_held.append(buf)
                _ws_captured.discard(key)
            with torch.cuda.device(index):
                buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=torch.device("cuda", index))
            _ws_cache[key] = buf
            cap = max(1, int(os.environ.get("EMAVFI_WS_CACHE_MAX", "8")))
            for old in [k for k in _ws_cache if k != key and k not in _ws_captured][:max(0, len(_ws_cache) - cap)]:
                del _ws_cache[old]
        _ws_cache.move_to_end(key)
        if capturing:
            _ws_captured.add(key)
    return buf


def release_workspaces():
    """Drop every cached workspace, including those kept alive for captured graphs (destroy the graphs first)."""
    with _ws_lock:
        _ws_cache.clear()
        _ws_captured.clear()
        del _ws_graph_held[:]


# ---------------------------------------------------------------- HIP events / side streams for the pipelined forward (model.py)
class _Hip:
    """hipEvent* / hipStreamWaitEvent of the HIP runtime torch has already loaded into this process (plain handles: what the C-ABI's
    stage events are).  Events are created once per (device, purpose) and re-recorded: a hipStreamWaitEvent captures the record
    that precedes it in host call order."""

    def __init__(self):
        path = None
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
        self.rt = ctypes.CDLL(path or "libamdhip64.so")
        self.rt.hipEventCreateWithFlags.argtypes = [POINTER(c_void_p), ctypes.c_uint]
        self.rt.hipEventRecord.argtypes = [c_void_p, c_void_p]
        self.rt.hipStreamWaitEvent.argtypes = [c_void_p, c_void_p, ctypes.c_uint]
        self._events = {}

    def event(self, key):
        """One event per key, created on first use and kept for the life of the process (keys are (device, caller stream, purpose): a
        handful per stream that ever ran a pipelined forward)."""
        e = self._events.get(key)
        if e is None:
            with _lock:
                e = self._events.get(key)
                if e is None:
                    h = c_void_p()
                    rc = self.rt.hipEventCreateWithFlags(ctypes.byref(h), 2)   # hipEventDisableTiming
                    if rc != 0:
                        raise RuntimeError(f"hipEventCreateWithFlags failed ({rc})")
                    e = self._events[key] = h
        return e

    def record(self, event, stream):
        rc = self.rt.hipEventRecord(event, c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"hipEventRecord failed ({rc})")

    def wait(self, stream, event):
        rc = self.rt.hipStreamWaitEvent(c_void_p(stream.cuda_stream), event, 0)
        if rc != 0:
            raise RuntimeError(f"hipStreamWaitEvent failed ({rc})")


_hip = None
_side_streams = {}


def hip() -> _Hip:
    global _hip
    if _hip is None:
        with _lock:
            if _hip is None:
                _hip = _Hip()
    return _hip


def side_stream(device, which=0, priority=0):
    """One cached side stream per (device, which): the pipelined forward's second lane, the harness's pre / post lanes."""
    import torch
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, which, priority)
    s = _side_streams.get(key)
    if s is None:
        with _lock:
            s = _side_streams.get(key)
            if s is None:
                s = _side_streams[key] = torch.cuda.Stream(device=torch.device("cuda", index), priority=priority)
    return s


# ---------------------------------------------------------------- operator-level wrappers
def warp(frame2, flow):
    """EMA_VFI.warp (reference ema_vfi.py:149-171) on the GPU."""
    import torch
    _require_cuda(frame2, flow)
    f2, fl = _f32c(frame2), _f32c(flow)
    B, C, H, W = f2.shape
    if fl.shape != (B, 2, H, W):
        raise ValueError(f"flow must be [B,2,H,W] = {(B, 2, H, W)}, got {tuple(fl.shape)}")
    out = torch.empty_like(f2)
    with torch.cuda.device(f2.device):
        check(load().emavfi_warp(f2.data_ptr(), fl.data_ptr(), out.data_ptr(), B, C, H, W, _stream()), "emavfi_warp")
    return out


def conv3x3(x, weight, bias, stride=1, act=ACT_NONE, dtype="fp32"):
    """One conv / conv_block of the reference (ema_vfi.py:7-14)."""
    import torch
    _require_cuda(x, weight, bias)
    dt = dtype_code(dtype)
    x, w = _f32c(x), _f32c(weight)
    b = _f32c(bias) if bias is not None else torch.zeros(w.shape[0], device=x.device)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    if tuple(w.shape) != (Cout, Cin, 3, 3):
        raise ValueError(f"weight must be [Cout,{Cin},3,3], got {tuple(w.shape)}")
    L = load()
    n = L.emavfi_conv3x3_workspace_bytes(B, Cin, Cout, H, W, stride, dt)
    if n == 0:
        raise RuntimeError(f"emavfi_conv3x3: {last_error()}")
    ws = workspace(n, x.device)
    y = torch.empty(B, Cout, (H + stride - 1) // stride, (W + stride - 1) // stride, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(L.emavfi_conv3x3(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, Cin, Cout, H, W, stride, act, dt,
                               ws.data_ptr(), ws.numel(), _stream()), "emavfi_conv3x3")
    return y


def deform_conv2d(x, offset, mask, weight, bias, dtype="fp32"):
    """torchvision.ops.deform_conv2d as configured at reference ema_vfi.py:45-51."""
    import torch
    _require_cuda(x, offset, mask, weight, bias)
    dt = dtype_code(dtype)
    x, off, msk, w = _f32c(x), _f32c(offset), _f32c(mask), _f32c(weight)
    B, C, H, W = x.shape
    O = w.shape[0]
    b = _f32c(bias) if bias is not None else torch.zeros(O, device=x.device)
    if tuple(off.shape) != (B, 18, H, W) or tuple(msk.shape) != (B, 9, H, W) or tuple(w.shape) != (O, C, 3, 3):
        raise ValueError("deform_conv2d: offset [B,18,H,W], mask [B,9,H,W], weight [O,C,3,3] expected")
    L = load()
    n = L.emavfi_deform_conv2d_workspace_bytes(B, C, O, H, W, dt)
    if n == 0:
        raise RuntimeError(f"emavfi_deform_conv2d: {last_error()}")
    ws = workspace(n, x.device)
    y = torch.empty(B, O, H, W, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(L.emavfi_deform_conv2d(x.data_ptr(), off.data_ptr(), msk.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                     B, C, O, H, W, dt, ws.data_ptr(), ws.numel(), _stream()), "emavfi_deform_conv2d")
    return y


ROUTES = {"window": 0, "gather": 1}   # include/emavfi.h: EMAVFI_ROUTE_WINDOW / EMAVFI_ROUTE_GATHER


def mdcn(x, offset_weight, offset_bias, dcn_weight, dcn_bias, dtype="fp32", flags=0, _events=None, route="window"):
    """ModulatedDeformConvPack.forward (reference ema_vfi.py:53-60) as ONE stage, routed as a block of the forward is
    (include/emavfi.h, emavfi_mdcn_routed): the one-launch kernel in the 16-bit modes at the reference width.
    `_events` (bench.py): (ctypes array of hipEvent_t, count) bracketing the stage's own launches.
    `route`: "window" (deform_pack3_kernel, the default) or "gather" (the window-free kernel; 16-bit modes at C = 65..67 only -
    elsewhere the C error is raised)."""
    if route not in ROUTES:
        raise ValueError(f"mdcn: route must be one of {sorted(ROUTES)}, got {route!r}")
    import torch
    _require_cuda(x, offset_weight, offset_bias, dcn_weight, dcn_bias)
    dt = dtype_code(dtype)
    x, ow, ob, dw = _f32c(x), _f32c(offset_weight), _f32c(offset_bias), _f32c(dcn_weight)
    db = _f32c(dcn_bias) if dcn_bias is not None else None
    B, C, H, W = x.shape
    if tuple(ow.shape) != (27, C, 3, 3) or tuple(ob.shape) != (27,) or tuple(dw.shape) != (C, C, 3, 3) or (db is not None and tuple(db.shape) != (C,)):
        raise ValueError(f"mdcn: offset_conv [27,{C},3,3] + [27] and dcn_v2 [{C},{C},3,3] + [{C}] expected")
    L = load()
    n = L.emavfi_mdcn_workspace_bytes(B, C, H, W, dt, flags)
    if n == 0:
        raise RuntimeError(f"emavfi_mdcn: {last_error()}")
    ws = workspace(n, x.device)
    y = torch.empty_like(x)
    ev, nev = _events_arg(_events)
    with torch.cuda.device(x.device):
        check(L.emavfi_mdcn_routed(x.data_ptr(), ow.data_ptr(), ob.data_ptr(), dw.data_ptr(), db.data_ptr() if db is not None else None,
                                   y.data_ptr(), B, C, H, W, dt, flags, ROUTES[route], ws.data_ptr(), ws.numel(), ev, nev, _stream()),
              "emavfi_mdcn_routed")
    return y


def _census_rows(raw, samples):
    """[blocks][4] u64 (device) -> list of dicts (one blocking copy)"""
    import struct
    rows = []
    for fix, total, parked, mx in raw.cpu().tolist():
        if total == 0:
            rows.append(None)   # this block did not run the one-launch kernel
            continue
        rows.append({"fixup_wave_taps": fix, "wave_taps": total, "fixup_share": fix / total, "samples_outside_window": parked,
                     "samples_outside_share": parked / samples, "abs_offset_px_max": struct.unpack("<f", struct.pack("<I", mx & 0xffffffff))[0]})
    return rows


def mdcn_census(B, C, H, W, dtype="bf16", flags=0, device=None):
    """What the one-launch pack kernel counted during the LAST lib.mdcn(...) call of this shape on the current stream
    (include/emavfi.h, emavfi_mdcn_census): [{fixup_wave_taps, wave_taps, fixup_share, samples_outside_window, ...}] or [None]."""
    import torch
    L = load()
    dt = dtype_code(dtype)
    dev = torch.device(device if device is not None else "cuda")
    n = L.emavfi_mdcn_workspace_bytes(B, C, H, W, dt, flags)
    if n == 0:
        raise RuntimeError(f"emavfi_mdcn_census: {last_error()}")
    ws = workspace(n, dev)
    out = torch.zeros(1, 4, dtype=torch.int64, device=ws.device)
    with torch.cuda.device(ws.device):
        check(L.emavfi_mdcn_census(B, C, H, W, dt, flags, ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()), "emavfi_mdcn_census")
    return _census_rows(out, B * H * W * 9)


def _stage(entry, ws_entry, x, params, out_shape, mid, dtype, what):
    import torch
    _require_cuda(x, *params)
    dt = dtype_code(dtype)
    x = _f32c(x)
    ps = [_f32c(p) for p in params]
    B, _, H, W = x.shape
    L = load()
    n = getattr(L, ws_entry)(B, mid, H, W, dt)
    if n == 0:
        raise RuntimeError(f"{what}: {last_error()}")
    ws = workspace(n, x.device)
    out = torch.empty(out_shape, device=x.device, dtype=torch.float32)
    arr = (c_void_p * len(ps))(*[p.data_ptr() for p in ps])
    with torch.cuda.device(x.device):
        check(getattr(L, entry)(x.data_ptr(), ctypes.cast(arr, POINTER(c_void_p)), out.data_ptr(), B, mid, H, W, dt, ws.data_ptr(), ws.numel(), _stream()), what)
    return out


def context(feat, params, dtype="fp32"):
    """context_encoding(feat) -> ctx [B, mid] (reference ema_vfi.py:79-86, :120); params: the 8 tensors of the Sequential in
    registration order.  The launches the forward runs for the stage (include/emavfi.h, emavfi_context)."""
    mid = feat.shape[1]
    shapes = [(2 * mid, mid, 3, 3), (2 * mid,), (4 * mid, 2 * mid, 3, 3), (4 * mid,), (4 * mid, 4 * mid, 3, 3), (4 * mid,), (mid, 4 * mid), (mid,)]
    if len(params) != 8 or [tuple(p.shape) for p in params] != shapes:
        raise ValueError(f"context: 8 tensors of shapes {shapes} expected")
    return _stage("emavfi_context", "emavfi_context_workspace_bytes", feat, params, (feat.shape[0], mid), mid, dtype, "emavfi_context")


def reconstruct(fused, params, dtype="fp32"):
    """reconstruction(fused) -> frame [B, 3, H, W] in [0, 1] (reference ema_vfi.py:102-107, :144-146); params: the 6 tensors of the
    Sequential in registration order.  The launches the forward runs for the stage (include/emavfi.h, emavfi_reconstruct)."""
    mid = fused.shape[1] - 3
    shapes = [(mid, mid + 3, 3, 3), (mid,), (mid // 2, mid, 3, 3), (mid // 2,), (3, mid // 2, 3, 3), (3,)]
    if len(params) != 6 or [tuple(p.shape) for p in params] != shapes:
        raise ValueError(f"reconstruct: 6 tensors of shapes {shapes} expected")
    return _stage("emavfi_reconstruct", "emavfi_reconstruct_workspace_bytes", fused, params, (fused.shape[0], 3, fused.shape[2], fused.shape[3]), mid, dtype,
                  "emavfi_reconstruct")


def forward_launches(in_channels, mid_channels, num_blocks, B, H, W, dtype, gather_blocks=0, adaptive=False, flow=None):
    """[(name, algorithmic_flops, algorithmic_bytes)] for every kernel launch of one forward.  gather_blocks: bit i routes attention
    block i to the window-free kernel (emavfi_forward_launches_routed); 0 lists exactly what emavfi_forward launches.  adaptive: the
    launches of emavfi_forward_adaptive (a routed pack per block plus one route_select; in modes without a one-launch pack exactly
    emavfi_forward's).  flow: None (the whole forward), "stop" (emavfi_forward_flow: the prefix through the launch that writes the
    flow) or "given" (emavfi_forward_given_flow: without context encoding and motion estimation)."""
    L = load()
    dt = dtype_code(dtype)
    if adaptive and gather_blocks:
        raise ValueError("forward_launches: adaptive and gather_blocks exclude each other")
    if flow not in (None, "stop", "given"):
        raise ValueError(f"forward_launches: flow must be None, 'stop' or 'given', got {flow!r}")
    if flow is not None and (adaptive or (flow == "stop" and gather_blocks)):
        raise ValueError("forward_launches: the adaptive route has no given-flow form, and the flow's prefix has no attention block to route")
    model = (in_channels, mid_channels, num_blocks, B, H, W, dt)
    if flow == "stop":
        entry, what, args = L.emavfi_forward_flow_launches, "emavfi_forward_flow_launches", model
    elif flow == "given":
        entry, what, args = L.emavfi_forward_given_flow_launches, "emavfi_forward_given_flow_launches", model + (gather_blocks,)
    elif adaptive:
        entry, what, args = L.emavfi_forward_launches_adaptive, "emavfi_forward_launches_adaptive", model
    else:
        entry, what, args = L.emavfi_forward_launches_routed, "emavfi_forward_launches_routed", model + (gather_blocks,)
    n = entry(*args, None, 0, None, None, 0)
    if n < 0:
        raise RuntimeError(f"{what}: {last_error()}")
    names = ctypes.create_string_buffer(128 * n)
    fl, by = (ctypes.c_double * n)(), (ctypes.c_double * n)()
    check(min(0, entry(*args, names, len(names), fl, by, n)), what)
    labels = names.value.decode().strip().split("\n")
    return [(labels[i], fl[i], by[i]) for i in range(n)]


IMAGENET_MEAN = (0.485, 0.456, 0.406)  # reference inference.py:40
IMAGENET_STD = (0.229, 0.224, 0.225)


def _stats(mean, std, C, ctype=ctypes.c_float):
    if len(mean) != C or len(std) != C:
        raise ValueError(f"mean/std must have {C} entries")
    return (ctype * C)(*mean), (ctype * C)(*std)


def _pinned_or_cuda(t, what):
    if not (t.is_cuda or (t.device.type == "cpu" and t.is_pinned())):
        raise RuntimeError(f"{what}: a ROCm tensor or a PINNED host tensor (read / written by the kernel over PCIe) is expected")


def _resize_target(size, what):
    """(Hd, Wd) of a `size=` argument, each 1 .. RESIZE_MAX_DIM"""
    try:
        Hd, Wd = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: size must be (Hd, Wd)") from None
    if not (1 <= Hd <= RESIZE_MAX_DIM and 1 <= Wd <= RESIZE_MAX_DIM):
        raise ValueError(f"{what}: size {(Hd, Wd)} must lie in 1..{RESIZE_MAX_DIM}")
    return Hd, Wd


def preprocess_u8(frames_hwc, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None, size=None, resized_out=None):
    """ToTensor + Normalize of reference inference.py:38-41 on the GPU: uint8 [B,H,W,C] -> fp32 [B,C,H,W].
    `frames_hwc` may be a pinned host tensor: the kernel then reads it in place over PCIe (no separate H2D copy;
    `device` names the GPU) - the caller keeps it unchanged until the kernel has run.  `out`: a contiguous fp32 [B,C,H,W] device
    tensor to fill (the streaming harness keeps one per buffer slot, so nothing is allocated on its side streams).
    `size=(Hd, Wd)`: the frames are resized first (cv2.resize of inference.py:46; the resize definition of include/emavfi.h) in the same
    launch - the result, fp32 [B,C,Hd,Wd], is preprocess_u8(resize_u8(frames_hwc, size)) bit for bit; `resized_out`: a contiguous uint8
    [B,Hd,Wd,C] device tensor that then also receives the resized bytes."""
    import torch
    _pinned_or_cuda(frames_hwc, "preprocess_u8")
    if frames_hwc.dtype != torch.uint8 or frames_hwc.dim() != 4:
        raise ValueError("preprocess_u8: uint8 [B,H,W,C] tensor expected")
    x = frames_hwc if frames_hwc.is_contiguous() else frames_hwc.contiguous()
    dev = x.device if x.is_cuda else torch.device(device if device is not None else "cuda")
    B, H, W, C = x.shape
    m, s = _stats(mean, std, C)
    if size is not None:
        Hd, Wd = _resize_target(size, "preprocess_u8")
        if out is None:
            out = torch.empty(B, C, Hd, Wd, dtype=torch.float32, device=dev)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, C, Hd, Wd) and out.is_contiguous()):
            raise ValueError("preprocess_u8: out must be a contiguous fp32 [B,C,Hd,Wd] device tensor")
        if resized_out is not None and not (resized_out.is_cuda and resized_out.dtype == torch.uint8 and resized_out.is_contiguous()
                                            and tuple(resized_out.shape) == (B, Hd, Wd, C)):
            raise ValueError("preprocess_u8: resized_out must be a contiguous uint8 [B,Hd,Wd,C] device tensor")
        with torch.cuda.device(dev):
            check(load().emavfi_preprocess_u8_resized(x.data_ptr(), out.data_ptr(), resized_out.data_ptr() if resized_out is not None else None,
                                                      B, H, W, Hd, Wd, C, m, s, _stream()), "emavfi_preprocess_u8_resized")
        return out
    if resized_out is not None:
        raise ValueError("preprocess_u8: resized_out needs size=")
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, C, H, W) and out.is_contiguous()):
        raise ValueError("preprocess_u8: out must be a contiguous fp32 [B,C,H,W] device tensor")
    with torch.cuda.device(dev):
        check(load().emavfi_preprocess_u8(x.data_ptr(), out.data_ptr(), B, H, W, C, m, s, _stream()), "emavfi_preprocess_u8")
    return out


def postprocess_u8(frames_nchw, denormalize=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """denormalize_frame of reference inference.py:51-58 on the GPU: fp32 [B,C,H,W] -> uint8 [B,H,W,C].
    `out` may be a pinned host tensor [B,H,W,C]: the kernel then writes the frames straight into host memory."""
    import torch
    _require_cuda(frames_nchw)
    x = _f32c(frames_nchw)
    if x.dim() != 4:
        raise ValueError("postprocess_u8: [B,C,H,W] tensor expected")
    B, C, H, W = x.shape
    m, s = _stats(mean, std, C, ctypes.c_double)  # numpy's float64 constants (inference.py:55)
    if out is None:
        out = torch.empty(B, H, W, C, dtype=torch.uint8, device=x.device)
    else:
        _pinned_or_cuda(out, "postprocess_u8(out=)")
        if out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, C) or not out.is_contiguous():
            raise ValueError("postprocess_u8: out must be a contiguous uint8 [B,H,W,C] tensor")
    with torch.cuda.device(x.device):
        check(load().emavfi_postprocess_u8(x.data_ptr(), out.data_ptr(), B, H, W, C, m, s, 1 if denormalize else 0, _stream()),
              "emavfi_postprocess_u8")
    return out


# ---------------------------------------------------------------- frames resized on the device (include/emavfi.h, "RESIZE DEFINITION")
RESIZE_MAX_DIM = 16384   # EMAVFI_RESIZE_MAX_DIM


def _byte_image(t, what, shape=None):
    """(pointer, pitch, batch stride) in bytes of a uint8 [B,H,W,C] image; rows and batches may be strided, a row must be dense"""
    import torch
    _pinned_or_cuda(t, what)
    if t.dtype != torch.uint8 or t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"{what}: a non-empty uint8 [B,H,W,C] tensor expected")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(shape)} expected, got {tuple(t.shape)}")
    B, H, W, C = t.shape
    if (C > 1 and t.stride(3) != 1) or (W > 1 and t.stride(2) != C):
        raise ValueError(f"{what}: the rows must be dense (only rows and batches may be strided)")
    pitch = t.stride(1) if H > 1 else W * C     # a dimension of size 1 has no meaningful stride: the dense value stands in
    return t.data_ptr(), pitch, (t.stride(0) if B > 1 else pitch * H)


def resize_u8(src, size, out=None, device=None):
    """cv2.resize(frame, (Wd, Hd)) of reference inference.py:46 on the GPU, by THE PROJECT'S OWN DEFINITION (include/emavfi.h: bilinear,
    half-pixel centres, 11-bit weights, integer arithmetic; no byte parity with cv2 is claimed): uint8 [B,Hs,Ws,C] -> uint8 [B,Hd,Wd,C],
    C in 1..4, each channel on its own.  `src` / `out`: device tensors (src may be pinned host memory; `device` names the GPU) whose rows and
    batches may be strided - pitches come from .stride(); bytes between the rows of a pitched `out` are left as they were."""
    import torch
    Hd, Wd = _resize_target(size, "resize_u8")
    sp, spitch, sbs = _byte_image(src, "resize_u8")
    B, Hs, Ws, C = src.shape
    dev = src.device if src.is_cuda else torch.device(device if device is not None else "cuda")
    if out is None:
        out = torch.empty(B, Hd, Wd, C, dtype=torch.uint8, device=dev)
    dp, dpitch, dbs = _byte_image(out, "resize_u8(out=)", (B, Hd, Wd, C))
    with torch.cuda.device(dev):
        check(load().emavfi_resize_u8(sp, spitch, sbs, dp, dpitch, dbs, B, Hs, Ws, Hd, Wd, C, _stream()), "emavfi_resize_u8")
    return out


# ---------------------------------------------------------------- NV12 frames (include/emavfi.h, "NV12")
YUV_STANDARDS = {("bt601", False): 0, ("bt601", True): 1, ("bt709", False): 2, ("bt709", True): 3}   # EMAVFI_YUV_*
ORDERS = {"bgr": 0, "rgb": 1}                                                                        # EMAVFI_ORDER_*


def yuv_standard_code(standard="bt601", full_range=False) -> int:
    try:
        return YUV_STANDARDS[(str(standard).lower(), bool(full_range))]
    except KeyError:
        raise ValueError(f"yuv standard must be 'bt601' or 'bt709', got {standard!r}") from None


def _order_code(order) -> int:
    try:
        return ORDERS[str(order).lower()]
    except KeyError:
        raise ValueError(f"order must be 'bgr' or 'rgb', got {order!r}") from None


def yuv_coefficients(standard="bt601", full_range=False, depth=8):
    """The fixed-point tables of the colour definition (include/emavfi.h): (decode [CY, CVR, CUG, CVG, CUB],
    encode [YR, YG, YB, UR, UG, UB, VR, VG, VB]), each floor(k * 2^20 + 0.5).  Host only.  `depth` 10, 12 or 16: the tables of the
    high-bit-depth definition, which also knows "bt2020"."""
    dec, enc = (c_int * 5)(), (c_int * 9)()
    if depth == 8:
        check(load().emavfi_yuv_coefficients(yuv_standard_code(standard, full_range), dec, enc), "emavfi_yuv_coefficients")
    else:
        check(load().emavfi_yuv_coefficients_depth(yuv_standard_code_deep(standard, full_range), _depth(depth), dec, enc),
              "emavfi_yuv_coefficients_depth")
    return list(dec), list(enc)


def _yuv420_planes(planes, es, what):
    """The plane geometry of 4:2:0 frames, stated once: B, H, W and per plane (pitch, batch stride) in BYTES of `planes` = (y, uv) -
    chroma interleaved, uv [B,ceil(H/2),ceil(W/2),2] - or (y, u, v) - chroma separate, u and v [B,ceil(H/2),ceil(W/2)] - around y
    [B,H,W].  `es`, the element size: uint8 tensors at 1, 16-bit integer tensors at 2.  Device or pinned host tensors; the rows and
    batches of each plane may be strided on their own, a row must be dense."""
    import torch
    names = ("y", "uv") if len(planes) == 2 else ("y", "u", "v")
    for name, t in zip(names, planes):
        _pinned_or_cuda(t, what)
        if t.dim() != (4 if name == "uv" else 3):
            raise ValueError(f"{what}: {name} must be a {4 if name == 'uv' else 3}-d tensor (y [B,H,W]; uv [B,ceil(H/2),ceil(W/2),2]; "
                             f"u, v [B,ceil(H/2),ceil(W/2)]), got {t.dim()} dimensions")
        if es == 1 and t.dtype != torch.uint8:
            raise ValueError(f"{what}: {name} must be uint8, got {t.dtype}")
        if es == 2 and (t.element_size() != 2 or t.dtype.is_floating_point):
            raise ValueError(f"{what}: {name} must hold 16-bit integers (torch.uint16 or torch.int16), got {t.dtype}")
    y = planes[0]
    B, H, W = y.shape
    if min(B, H, W) < 1:
        raise ValueError(f"{what}: y is empty")
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    geometry = []
    for name, t in zip(names, planes):
        h, w, k = (H, W, 1) if name == "y" else (H2, W2, 2) if name == "uv" else (H2, W2, 1)     # k: samples per position of a row
        want = (B, h, w, 2) if name == "uv" else (B, h, w)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: {name} must be {want} for y {(B, H, W)}, got {tuple(t.shape)}")
        if t.is_cuda != y.is_cuda or (t.is_cuda and t.device != y.device):
            raise ValueError(f"{what}: {name} and y must live in the same memory")
        if (w > 1 and t.stride(2) != k) or (k == 2 and t.stride(3) != 1):
            raise ValueError(f"{what}: the rows of {name} must be dense (only rows and batches may be strided)")
        # a dimension of size 1 has no meaningful stride: the dense value stands in
        pitch = es * (t.stride(1) if h > 1 else k * w)
        geometry.append((pitch, es * t.stride(0) if B > 1 else pitch * h))
    return B, H, W, geometry


def _nv12_planes(y, uv, what):
    """Shapes, pitches and batch strides (bytes) of a Y [B,H,W] / UV [B,ceil(H/2),ceil(W/2),2] pair of uint8 tensors; rows and
    batches may be strided, the innermost dimensions must be dense."""
    B, H, W, (yg, uvg) = _yuv420_planes((y, uv), 1, what)
    return (B, H, W, *yg, *uvg)


def _preprocess_yuv420(family, planes, es, depth, standard, full_range, order, mean, std, device, out, size=None, resized_out=None):
    """The one body of preprocess_nv12 / _p010 / _yuv420p: emavfi_preprocess_<family> on the checked planes; `depth`: () for NV12, whose
    entry takes none, else (depth,).  `size` / `resized_out`: NV12's fused resize, emavfi_preprocess_nv12_resized."""
    import torch
    what = "preprocess_" + family
    if es == 2:
        planes = [_words(t, device) for t in planes]
    B, H, W, geometry = _yuv420_planes(planes, es, what)
    st = (yuv_standard_code_deep if es == 2 else yuv_standard_code)(standard, full_range)
    od = _order_code(order)
    dev = planes[0].device if planes[0].is_cuda else torch.device(device if device is not None else "cuda")
    m, s = _stats(mean, std, 3)
    Hd, Wd = (H, W) if size is None else _resize_target(size, what)
    if resized_out is not None and size is None:
        raise ValueError(f"{what}: resized_out needs size=")
    if out is None:
        out = torch.empty(B, 3, Hd, Wd, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, Hd, Wd) and out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous fp32 [B,3,{'H,W' if size is None else 'Hd,Wd'}] device tensor")
    args = [a for t, g in zip(planes, geometry) for a in (t.data_ptr(), *g)] + [out.data_ptr()]
    if size is None:
        entry, args = "emavfi_" + what, args + [B, H, W, *depth]
    else:
        yo, uvo = resized_out if resized_out is not None else (None, None)
        ya = _byte_image(yo.unsqueeze(-1), f"{what}(resized_out=)", (B, Hd, Wd, 1)) if yo is not None else (None, 0, 0)
        ua = _byte_image(uvo, f"{what}(resized_out=)", (B, (Hd + 1) // 2, (Wd + 1) // 2, 2)) if uvo is not None else (None, 0, 0)
        entry, args = "emavfi_preprocess_nv12_resized", args + [*ya, *ua, B, H, W, Hd, Wd]
    with torch.cuda.device(dev):
        check(getattr(load(), entry)(*args, st, od, m, s, _stream()), entry)
    return out


def _postprocess_yuv420(family, frames_nchw, nplanes, es, depth, standard, full_range, order, denormalize, mean, std, out):
    """The one body of postprocess_nv12 / _p010 / _yuv420p: emavfi_postprocess_<family> into the `nplanes` checked planes of `out`, or
    into fresh dense ones; `depth` as for _preprocess_yuv420."""
    import torch
    what = "postprocess_" + family
    _require_cuda(frames_nchw)
    x = _f32c(frames_nchw)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{what}: [B,3,H,W] tensor expected")
    B, _, H, W = x.shape
    st = (yuv_standard_code_deep if es == 2 else yuv_standard_code)(standard, full_range)
    od = _order_code(order)
    m, s = _stats(mean, std, 3, ctypes.c_double)
    chroma = (B, (H + 1) // 2, (W + 1) // 2)
    if out is None:
        dt = torch.uint8 if es == 1 else word_dtype()
        shapes = [(B, H, W)] + ([(*chroma, 2)] if nplanes == 2 else [chroma, chroma])
        planes = tuple(torch.empty(shape, dtype=dt, device=x.device) for shape in shapes)
    else:
        try:
            planes = tuple(out)
        except TypeError:
            planes = ()
        if len(planes) != nplanes:
            raise ValueError(f"{what}: out must be the {nplanes} planes {'(y, uv)' if nplanes == 2 else '(y, u, v)'}")
    *shape, geometry = _yuv420_planes(planes, es, f"{what}(out=)")
    if tuple(shape) != (B, H, W):
        raise ValueError(f"{what}: out must be the planes of frames {(B, H, W)}, y [B,H,W] and chroma of ceil(H/2) x ceil(W/2)")
    args = [a for t, g in zip(planes, geometry) for a in (t.data_ptr(), *g)]
    with torch.cuda.device(x.device):
        check(getattr(load(), "emavfi_" + what)(x.data_ptr(), *args, B, H, W, *depth, st, od, m, s, 1 if denormalize else 0, _stream()),
              "emavfi_" + what)
    return planes


def preprocess_nv12(y, uv, standard="bt601", full_range=False, order="bgr", mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None,
                    size=None, resized_out=None):
    """NV12 frames -> fp32 [B,3,H,W], defined as preprocess_u8 of the decoded bytes (include/emavfi.h, "NV12").
    `y` uint8 [B,H,W], `uv` uint8 [B,ceil(H/2),ceil(W/2),2]: device tensors or pinned host tensors (read in place over PCIe; `device`
    names the GPU), each may be strided in its row and batch dimensions - the pitches are taken from .stride().  `order`: which colour is
    channel 0 ("bgr": what cv2 hands the reference).  `out`: a contiguous fp32 [B,3,H,W] device tensor to fill.
    `size=(Hd, Wd)`: the planes are resized first in the same launch (Y as a 1-channel image to Hd x Wd, UV as a 2-channel image to
    ceil(Hd/2) x ceil(Wd/2); the resize definition of include/emavfi.h) - the result, fp32 [B,3,Hd,Wd], is preprocess_nv12 of the
    resize_u8-resized planes bit for bit; `resized_out=(y_out, uv_out)`: device tensors, strided like y / uv, either may be None, that then
    also receive the resized planes."""
    return _preprocess_yuv420("nv12", (y, uv), 1, (), standard, full_range, order, mean, std, device, out, size, resized_out)


def postprocess_nv12(frames_nchw, standard="bt601", full_range=False, order="bgr", denormalize=True, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                     out=None):
    """fp32 [B,3,H,W] -> NV12 (y [B,H,W], uv [B,ceil(H/2),ceil(W/2),2]), defined as the encode of the bytes postprocess_u8 would write
    (include/emavfi.h, "NV12").  `out=(y, uv)`: device or pinned host tensors to fill, strided as for preprocess_nv12; bytes between
    the rows of a pitched destination are left as they were."""
    return _postprocess_yuv420("nv12", frames_nchw, 2, 1, (), standard, full_range, order, denormalize, mean, std, out)


# ---------------------------------------------------------------- 16-bit-word frames, P010 / P012 / P016 (include/emavfi.h, "HIGH BIT DEPTH")
YUV_STANDARDS_DEEP = {**YUV_STANDARDS, ("bt2020", False): 4, ("bt2020", True): 5}         # EMAVFI_YUV_*, BT.2020 included
# pixel format -> bits per sample, of the table's word formats in the NV12 layout and of its planar formats
DEPTHS = {f.name: f.depth for f in FORMATS.values() if f.layout == LAYOUT_NV12 and f.words}
PLANAR_DEPTHS = {f.name: f.depth for f in FORMATS.values() if f.layout == LAYOUT_I420}
_word = None


def yuv_standard_code_deep(standard="bt601", full_range=False) -> int:
    """the standard's code for the high-bit-depth entries, the only ones that accept BT.2020"""
    try:
        return YUV_STANDARDS_DEEP[(str(standard).lower(), bool(full_range))]
    except KeyError:
        raise ValueError(f"yuv standard must be 'bt601', 'bt709' or 'bt2020', got {standard!r}") from None


def _depth(depth, family=DEPTHS) -> int:
    """`depth` where a format of `family` has it"""
    if isinstance(depth, bool) or depth not in family.values():
        ds = sorted(family.values())
        raise ValueError(f"depth must be {', '.join(str(d) for d in ds[:-1])} or {ds[-1]} ({', '.join(n.upper() for n in family)}), got {depth!r}")
    return int(depth)


def word_dtype():
    """the torch dtype of a 16-bit sample word: torch.uint16 where this torch can allocate, view and copy it, else torch.int16 (the same
    bits; the kernels only ever see the pointer)"""
    global _word
    if _word is None:
        import torch
        try:
            t = torch.zeros(4, dtype=torch.uint16)
            torch.empty(4, dtype=torch.uint16).copy_(t)
            assert t.view(torch.uint8).numel() == 8 and t.numpy().dtype.itemsize == 2
            _word = torch.uint16
        except Exception:
            _word = torch.int16
    return _word


def _words(t, device):
    """a numpy uint16 array becomes a device tensor of words (one upload); tensors pass through"""
    import numpy as np
    import torch
    if isinstance(t, np.ndarray):
        if t.dtype != np.uint16:
            raise ValueError("numpy planes must be uint16")
        dev = torch.device(device if device is not None else "cuda")
        return torch.from_numpy(np.ascontiguousarray(t).view(np.int16)).to(dev).view(word_dtype())
    return t


def _p010_planes(y, uv, what):
    """Shapes, pitches and batch strides (BYTES) of a Y [B,H,W] / UV [B,ceil(H/2),ceil(W/2),2] pair of 16-bit tensors; rows and batches
    may be strided, the innermost dimensions must be dense."""
    B, H, W, (yg, uvg) = _yuv420_planes((y, uv), 2, what)
    return (B, H, W, *yg, *uvg)


def preprocess_p010(y, uv, depth=10, standard="bt601", full_range=False, order="bgr", mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None,
                    out=None):
    """P010 / P012 / P016 frames (`depth` 10 / 12 / 16) -> fp32 [B,3,H,W]: ((v / P) - mean) / std of the decoded `depth`-bit integers
    (include/emavfi.h, "HIGH BIT DEPTH").  `y` [B,H,W] and `uv` [B,ceil(H/2),ceil(W/2),2] hold one 16-bit word per sample, the sample in
    the word's top bits: device tensors or pinned host tensors (read in place over PCIe; `device` names the GPU) of `word_dtype()` or
    torch.int16, strided in their row and batch dimensions as for preprocess_nv12; numpy uint16 arrays are uploaded first.  `standard`
    also takes "bt2020"."""
    return _preprocess_yuv420("p010", (y, uv), 2, (_depth(depth),), standard, full_range, order, mean, std, device, out)


def postprocess_p010(frames_nchw, depth=10, standard="bt601", full_range=False, order="bgr", denormalize=True, mean=IMAGENET_MEAN,
                     std=IMAGENET_STD, out=None):
    """fp32 [B,3,H,W] -> P010 / P012 / P016 planes (y [B,H,W], uv [B,ceil(H/2),ceil(W/2),2]) of 16-bit words: the encode of the integers
    trunc(clip(x std + mean, 0, 1) P) (include/emavfi.h, "HIGH BIT DEPTH"); the low 16 - depth bits of every word are zero.
    `out=(y, uv)`: device or pinned host tensors to fill, strided as for preprocess_p010; bytes between the rows of a pitched destination
    are left as they were.  Without `out` the planes are dense device tensors of `word_dtype()`."""
    return _postprocess_yuv420("p010", frames_nchw, 2, 2, (_depth(depth),), standard, full_range, order, denormalize, mean, std, out)


# ---------------------------------------------------------------- planar 4:2:0 frames (include/emavfi.h, "PLANAR 4:2:0")
def _yuv420p_planes(y, u, v, depth, what):
    """Shapes and, per plane, (pointer, pitch, batch stride) in BYTES of a Y [B,H,W] / U, V [B,ceil(H/2),ceil(W/2)] triple: uint8 tensors
    at depth 8, 16-bit integer tensors above; rows and batches may be strided, a row must be dense."""
    B, H, W, geometry = _yuv420_planes((y, u, v), 1 if depth == 8 else 2, what)
    return B, H, W, [a for t, g in zip((y, u, v), geometry) for a in (t.data_ptr(), *g)]


def preprocess_yuv420p(y, u, v, depth=8, standard="bt601", full_range=False, order="bgr", mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None,
                       out=None):
    """Planar 4:2:0 frames -> fp32 [B,3,H,W] (include/emavfi.h, "PLANAR 4:2:0"): `y` [B,H,W], `u` and `v` [B,ceil(H/2),ceil(W/2)].
    `depth` 8: uint8 tensors, the result is preprocess_nv12 of the interleaved chroma planes bit for bit.  `depth` 10 / 12 / 16: 16-bit
    tensors (`word_dtype()` or torch.int16; numpy uint16 arrays are uploaded first) with the sample in the word's LOW bits - yuv420p10le,
    Y4M's C420p10 -, the result is preprocess_p010 of the words shifted to the top; `standard` then also takes "bt2020".  Device tensors or
    pinned host tensors (read in place over PCIe; `device` names the GPU), each plane strided in its row and batch dimensions on its own.
    YV12 is the caller swapping `u` and `v`.  `out`: a contiguous fp32 [B,3,H,W] device tensor to fill."""
    d = _depth(depth, PLANAR_DEPTHS)
    return _preprocess_yuv420("yuv420p", (y, u, v), 1 if d == 8 else 2, (d,), standard, full_range, order, mean, std, device, out)


def postprocess_yuv420p(frames_nchw, depth=8, standard="bt601", full_range=False, order="bgr", denormalize=True, mean=IMAGENET_MEAN,
                        std=IMAGENET_STD, out=None):
    """fp32 [B,3,H,W] -> planar 4:2:0 (y [B,H,W], u and v [B,ceil(H/2),ceil(W/2)]): at `depth` 8 the bytes postprocess_nv12 writes,
    de-interleaved; at 10 / 12 / 16 the words postprocess_p010 writes, shifted down into the LOW bits (the high bits are zero).
    `out=(y, u, v)`: device or pinned host tensors to fill, strided as for preprocess_yuv420p; bytes between the rows of a pitched
    destination are left as they were.  Without `out` the planes are dense device tensors (uint8 / `word_dtype()`)."""
    d = _depth(depth, PLANAR_DEPTHS)
    return _postprocess_yuv420("yuv420p", frames_nchw, 3, 1 if d == 8 else 2, (d,), standard, full_range, order, denormalize, mean, std, out)


# ---------------------------------------------------------------- scene cuts on the device (include/emavfi.h, "SCENE CUT DEFINITION")
SCENE_GRID = 32          # EMAVFI_SCENE_GRID
SCENE_SIG_WORDS = 1024   # EMAVFI_SCENE_SIG_WORDS


def scene_threshold_units(fraction, H, W) -> int:
    """The u32 threshold of scene_flags for "the mean absolute difference of the two 32 x 32 luma thumbnails reaches `fraction` of full
    scale": ceil(fraction * 4080 * cells), cells = min(H, 32) * min(W, 32) (a cell's mean is kept in sixteenths of a count: 0..4080)."""
    import math
    if not (1 <= int(H) <= RESIZE_MAX_DIM and 1 <= int(W) <= RESIZE_MAX_DIM):
        raise ValueError(f"scene_threshold_units: H, W must lie in 1..{RESIZE_MAX_DIM}")
    fraction = float(fraction)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError("scene_threshold_units: fraction must lie in 0..1")
    return int(math.ceil(fraction * (4080 * min(int(H), SCENE_GRID) * min(int(W), SCENE_GRID))))


def _u32_rows(t, what, n=None):
    """(pointer, row stride in words, rows) of an int32 device tensor [rows, 1024] (or [1024]: one row) whose rows are dense"""
    import torch
    _require_cuda(t)
    if t.dtype != torch.int32 or t.dim() not in (1, 2) or t.shape[-1] != SCENE_SIG_WORDS or t.stride(-1) != 1:
        raise ValueError(f"{what}: an int32 device tensor [n, {SCENE_SIG_WORDS}] with dense rows expected")
    rows = t.shape[0] if t.dim() == 2 else 1
    if n is not None and rows not in (1, n):
        raise ValueError(f"{what}: {n} rows (or one, compared with every pair) expected, got {rows}")
    return t.data_ptr(), (t.stride(0) if t.dim() == 2 and rows > 1 else 0), rows


def luma_signature_u8(frames, order="bgr", out=None, device=None):
    """uint8 [B,H,W,C] frames, C = 1 (a Y plane) or 3 (interleaved colour, `order` says which byte is red) -> int32 [B,1024]: the luma sum of
    each cell of a 32 x 32 grid over the frame (the scene-cut definition of include/emavfi.h; the sums fit 31 bits).  `frames`: a device
    tensor or pinned host memory (`device` names the GPU), rows and batches may be strided.  `out`: a contiguous int32 [B,1024] device tensor
    to fill - every word is written."""
    import torch
    sp, pitch, bs = _byte_image(frames, "luma_signature_u8")
    B, H, W, C = frames.shape
    dev = frames.device if frames.is_cuda else torch.device(device if device is not None else "cuda")
    if out is None:
        out = torch.empty(B, SCENE_SIG_WORDS, dtype=torch.int32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (B, SCENE_SIG_WORDS) and out.is_contiguous()):
        raise ValueError(f"luma_signature_u8: out must be a contiguous int32 [B,{SCENE_SIG_WORDS}] device tensor")
    with torch.cuda.device(dev):
        check(load().emavfi_luma_signature_u8(sp, pitch, bs, B, H, W, C, _order_code(order), out.data_ptr(), _stream()), "emavfi_luma_signature_u8")
    return out


def scene_flags(sig_a, sig_b, size, threshold, flags=None, scores=None, with_scores=True):
    """Per pair k: score = sum over the cells of |mean_a - mean_b| of two signatures of `size` = (H, W) frames, flag = score >= threshold
    (an int in score units: scene_threshold_units).  `sig_a` / `sig_b`: int32 device tensors [n,1024], rows may be strided (a slice with a
    step); a [1024] or [1,1024] tensor is compared with every pair.  Returns (flags, scores): int32 [n] device tensors (`flags=` / `scores=`
    fill given ones; with_scores=False passes NULL and returns None for the scores)."""
    import torch
    H, W = (int(v) for v in size)
    pa, sa, na = _u32_rows(sig_a, "scene_flags(sig_a)")
    pb, sb, nb = _u32_rows(sig_b, "scene_flags(sig_b)")
    n = max(na, nb)
    if na not in (1, n) or nb not in (1, n):
        raise ValueError(f"scene_flags: {na} and {nb} signatures do not pair up")
    threshold = int(threshold)
    if not 0 <= threshold < 2 ** 32:
        raise ValueError("scene_flags: threshold must be a u32 in score units")
    dev = sig_a.device

    def vec(t, name):
        if t is None:
            return torch.empty(n, dtype=torch.int32, device=dev)
        if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (n,) and t.is_contiguous()):
            raise ValueError(f"scene_flags: {name} must be a contiguous int32 [{n}] device tensor")
        return t
    flags = vec(flags, "flags")
    scores = vec(scores, "scores") if (with_scores or scores is not None) else None
    with torch.cuda.device(dev):
        check(load().emavfi_scene_flags(pa, sa, pb, sb, n, H, W, threshold, flags.data_ptr(), scores.data_ptr() if scores is not None else None,
                                        _stream()), "emavfi_scene_flags")
    return flags, scores


def hold_frames_u8(dst, alt, flags, rep=1):
    """For every pair k with flags[k] != 0: frame alt[k] is copied over the frames dst[k * rep : (k + 1) * rep]; everything else is left as it
    was.  `dst` uint8 [n * rep, ...], `alt` uint8 [n, ...]: device tensors or pinned host memory with the same
    dense frame shape; their first dimension may be strided (a slice with a step).  `flags`: int32 [n] device tensor (scene_flags)."""
    import torch
    for t, what in ((dst, "hold_frames_u8(dst)"), (alt, "hold_frames_u8(alt)")):
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous():
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames expected")
    n, rep = alt.shape[0], int(rep)
    if rep < 1 or dst.shape[0] != n * rep or tuple(dst.shape[1:]) != tuple(alt.shape[1:]):
        raise ValueError(f"hold_frames_u8: dst {tuple(dst.shape)} is not rep = {rep} frames of alt's shape {tuple(alt.shape[1:])} per pair ({n} pairs)")
    if not (flags.is_cuda and flags.dtype == torch.int32 and tuple(flags.shape) == (n,) and flags.is_contiguous()):
        raise ValueError(f"hold_frames_u8: flags must be a contiguous int32 [{n}] device tensor")
    fb = dst[0].numel()
    ds = dst.stride(0) if dst.shape[0] > 1 else fb
    as_ = alt.stride(0) if n > 1 else fb
    with torch.cuda.device(flags.device):
        check(load().emavfi_hold_frames_u8(dst.data_ptr(), ds, rep, alt.data_ptr(), as_, flags.data_ptr(), n, fb, _stream()), "emavfi_hold_frames_u8")
    return dst


# ---------------------------------------------------------------- temporal resampling (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION")
RESAMPLE_NODES = 0x80000000     # EMAVFI_RESAMPLE_NODES: the pool bit of a table entry's a / b
RESAMPLE_LAUNCH_CAP = 64        # EMAVFI_RESAMPLE_LAUNCH_CAP: table entries per launch
RESAMPLE_MAX_DEPTH = 5          # the deepest dyadic tree of the definition: G = 32


class ResampleEntry(ctypes.Structure):
    """emavfi_resample_entry"""
    _fields_ = [("a", ctypes.c_uint), ("b", ctypes.c_uint), ("w", ctypes.c_uint), ("f", ctypes.c_uint), ("h", ctypes.c_uint)]


def resample_sample_format(pixel_format):
    """(sample_bytes, depth, shift) of the samples of a harness pixel format as emavfi_resample_frames takes them: bytes; P01x words with the
    sample in the top bits; planar words with it in the low bits"""
    return FORMATS[pixel_format].sample_format if pixel_format in FORMATS else (1, 8, 0)


def resample_frames(dst, srcs, nodes, table, flags=None, sample_bytes=1, depth=8, shift=0):
    """Assembles the frames of `dst` from two pools of frames, one table entry per output (the temporal resample definition of
    include/emavfi.h).  `dst` uint8 [n_out, ...], `srcs` uint8 [n_srcs, ...], `nodes` uint8 [n_nodes, ...] or None: device tensors or pinned
    host memory with the same dense frame shape, their first dimension may be strided.  `table`: n_out tuples (a, b, w, f, h) - a, b: a frame
    index in `srcs`, or RESAMPLE_NODES + an index in `nodes`; w 0..256; f: 0, or 1 + an index into `flags`; h: the `srcs` frame a flagged
    entry holds.  `flags`: an int32 device tensor or None.  16-bit frames travel as their bytes with sample_bytes = 2 and the sample's
    `depth` and `shift`.  The table is consumed before the call returns."""
    import torch
    pools = [(dst, "resample_frames(dst)"), (srcs, "resample_frames(srcs)")] + ([(nodes, "resample_frames(nodes)")] if nodes is not None else [])
    for t, what in pools:
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous() or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames of dst's frame shape expected")
    table = list(table)
    if len(table) != dst.shape[0]:
        raise ValueError(f"resample_frames: {len(table)} table entries for {dst.shape[0]} output frames")
    if flags is not None and not (flags.is_cuda and flags.dtype == torch.int32 and flags.dim() == 1 and flags.is_contiguous()):
        raise ValueError("resample_frames: flags must be a contiguous int32 [n] device tensor")
    fb = dst[0].numel()
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else fb     # a dimension of size 1 has no meaningful stride
    arr = (ResampleEntry * len(table))(*(ResampleEntry(*(int(v) for v in e)) for e in table))
    dev = next((t.device for t, _ in pools if t.is_cuda), None) or (flags.device if flags is not None else torch.device("cuda"))
    with torch.cuda.device(dev):
        check(load().emavfi_resample_frames(dst.data_ptr(), stride(dst), len(table), srcs.data_ptr(), stride(srcs), srcs.shape[0],
                                            nodes.data_ptr() if nodes is not None else None, stride(nodes) if nodes is not None else 0,
                                            nodes.shape[0] if nodes is not None else 0, ctypes.cast(arr, c_void_p),
                                            flags.data_ptr() if flags is not None else None, flags.numel() if flags is not None else 0,
                                            fb, int(sample_bytes), int(depth), int(shift), _stream()), "emavfi_resample_frames")
    return dst


# ---------------------------------------------------------------- shutter accumulation (include/emavfi.h, "SHUTTER DEFINITION")
ACCUMULATE_MAX_TAPS = 33        # EMAVFI_ACCUMULATE_MAX_TAPS: the nodes 0 .. G of the deepest tree
ACCUMULATE_LAUNCH_CAP = 8       # EMAVFI_ACCUMULATE_LAUNCH_CAP: table entries per launch
ACCUMULATE_MAX_SUM = 65535      # the largest sum of an entry's weights


class AccumulateEntry(ctypes.Structure):
    """emavfi_accumulate_entry"""
    _fields_ = [("n", ctypes.c_uint), ("f", ctypes.c_uint), ("h", ctypes.c_uint), ("tap", ctypes.c_uint * ACCUMULATE_MAX_TAPS),
                ("w", ctypes.c_uint * ACCUMULATE_MAX_TAPS)]


def accumulate_frames(dst, srcs, nodes, table, flags=None, sample_bytes=1, depth=8, shift=0):
    """Every frame of `dst` the weighted integer mean of frames of two pools, one table entry per output (the shutter definition of
    include/emavfi.h).  `dst`, `srcs`, `nodes`, `flags` and the sample format as for resample_frames.  `table`: n_out tuples
    (taps, weights, f, h) - taps: 1..33 frame indices in `srcs`, or RESAMPLE_NODES + an index in `nodes`; weights: as many positive
    integers that sum to 65535 at the most; f: 0, or 1 + an index into `flags`; h: the `srcs` frame a flagged entry holds.  The table is
    consumed before the call returns."""
    import torch
    pools = [(dst, "accumulate_frames(dst)"), (srcs, "accumulate_frames(srcs)")] + ([(nodes, "accumulate_frames(nodes)")] if nodes is not None else [])
    for t, what in pools:
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous() or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames of dst's frame shape expected")
    table = list(table)
    if len(table) != dst.shape[0]:
        raise ValueError(f"accumulate_frames: {len(table)} table entries for {dst.shape[0]} output frames")
    if flags is not None and not (flags.is_cuda and flags.dtype == torch.int32 and flags.dim() == 1 and flags.is_contiguous()):
        raise ValueError("accumulate_frames: flags must be a contiguous int32 [n] device tensor")
    arr = (AccumulateEntry * len(table))()
    for k, (taps, weights, f, h) in enumerate(table):
        if len(taps) != len(weights) or len(taps) > ACCUMULATE_MAX_TAPS:
            raise ValueError(f"accumulate_frames: table[{k}] has {len(taps)} taps and {len(weights)} weights (as many of each, "
                             f"{ACCUMULATE_MAX_TAPS} at the most)")
        arr[k].n, arr[k].f, arr[k].h = len(taps), int(f), int(h)
        for i, (t, w) in enumerate(zip(taps, weights)):
            arr[k].tap[i], arr[k].w[i] = int(t), int(w)
    fb = dst[0].numel()
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else fb     # a dimension of size 1 has no meaningful stride
    dev = next((t.device for t, _ in pools if t.is_cuda), None) or (flags.device if flags is not None else torch.device("cuda"))
    with torch.cuda.device(dev):
        check(load().emavfi_accumulate_frames(dst.data_ptr(), stride(dst), len(table), srcs.data_ptr(), stride(srcs), srcs.shape[0],
                                              nodes.data_ptr() if nodes is not None else None, stride(nodes) if nodes is not None else 0,
                                              nodes.shape[0] if nodes is not None else 0, ctypes.cast(arr, c_void_p),
                                              flags.data_ptr() if flags is not None else None, flags.numel() if flags is not None else 0,
                                              fb, int(sample_bytes), int(depth), int(shift), _stream()), "emavfi_accumulate_frames")
    return dst


# ---------------------------------------------------------------- linear light (include/emavfi.h, "LINEAR LIGHT DEFINITION")
TRANSFERS = ("srgb", "bt709", "hlg")     # EMAVFI_TRANSFER_SRGB, _BT709, _HLG: the index is the code
LIGHT_DEPTHS = (8, 10, 12)
LIGHT_ONE, LIGHT_BIAS, LIGHT_LIMIT = 1 << 28, 1 << 26, 1 << 30


def transfer_table(name, depth=8, full_range=True):
    """The built-in table of the transfer function `name` ("srgb", "bt709", "hlg") for `depth`-bit codes (8, 10 or 12) at full or limited
    range: a numpy uint32 array of 2^depth values of light, LIGHT_BIAS at nominal black and LIGHT_BIAS + LIGHT_ONE at nominal white.  Pure
    host code."""
    import numpy as np
    if not isinstance(name, str) or name not in TRANSFERS:
        raise ValueError(f"transfer_table: the transfer function must be one of {TRANSFERS}, got {name!r}")
    if isinstance(depth, bool) or not isinstance(depth, int) or depth not in LIGHT_DEPTHS:
        raise ValueError(f"transfer_table: depth must be one of {LIGHT_DEPTHS}, got {depth!r}")
    lin = np.empty(1 << depth, np.uint32)
    check(load().emavfi_transfer_table(TRANSFERS.index(name), depth, 1 if full_range else 0, lin.ctypes.data), "emavfi_transfer_table")
    return lin


def transfer_table_check(table, depth=8):
    """Raises (RuntimeError, the message naming the first offending index) unless `table` - 2^depth values - is strictly increasing with
    every value below 2^30: what emavfi_accumulate_frames_linear expects of the table it is given.  Pure host code."""
    import numpy as np
    lin = np.ascontiguousarray(table, dtype=np.uint32)
    if isinstance(depth, bool) or not isinstance(depth, int) or depth not in LIGHT_DEPTHS:
        raise ValueError(f"transfer_table_check: depth must be one of {LIGHT_DEPTHS}, got {depth!r}")
    if lin.shape != (1 << depth,):
        raise ValueError(f"transfer_table_check: {lin.shape} values for depth {depth} ({1 << depth} expected)")
    check(load().emavfi_transfer_table_check(lin.ctypes.data, depth), "emavfi_transfer_table_check")
    return table


def accumulate_frames_linear(dst, srcs, nodes, table, lin, linear_bytes, flags=None, sample_bytes=1, depth=8, shift=0):
    """accumulate_frames with the first `linear_bytes` bytes of every frame averaged in light (the linear light definition of
    include/emavfi.h) and the rest as accumulate_frames does.  `lin`: a contiguous int32 DEVICE tensor of 2^depth words, the bits of a table
    that passed transfer_table_check (it is not checked again: the kernel is memory-safe for any content, and a table that is not valid
    gives wrong samples).  Everything else as for accumulate_frames."""
    import torch
    pools = [(dst, "accumulate_frames_linear(dst)"), (srcs, "accumulate_frames_linear(srcs)")] + \
        ([(nodes, "accumulate_frames_linear(nodes)")] if nodes is not None else [])
    for t, what in pools:
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous() or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames of dst's frame shape expected")
    table = list(table)
    if len(table) != dst.shape[0]:
        raise ValueError(f"accumulate_frames_linear: {len(table)} table entries for {dst.shape[0]} output frames")
    if flags is not None and not (flags.is_cuda and flags.dtype == torch.int32 and flags.dim() == 1 and flags.is_contiguous()):
        raise ValueError("accumulate_frames_linear: flags must be a contiguous int32 [n] device tensor")
    if depth not in LIGHT_DEPTHS:
        raise ValueError(f"accumulate_frames_linear: depth must be one of {LIGHT_DEPTHS}, got {depth!r}")
    if not (isinstance(lin, torch.Tensor) and lin.is_cuda and lin.dtype == torch.int32 and lin.dim() == 1 and lin.is_contiguous()
            and lin.numel() == 1 << depth):
        raise ValueError(f"accumulate_frames_linear: lin must be a contiguous int32 [{1 << depth}] device tensor (the bits of the uint32 table)")
    arr = (AccumulateEntry * len(table))()
    for k, (taps, weights, f, h) in enumerate(table):
        if len(taps) != len(weights) or len(taps) > ACCUMULATE_MAX_TAPS:
            raise ValueError(f"accumulate_frames_linear: table[{k}] has {len(taps)} taps and {len(weights)} weights (as many of each, "
                             f"{ACCUMULATE_MAX_TAPS} at the most)")
        arr[k].n, arr[k].f, arr[k].h = len(taps), int(f), int(h)
        for i, (t, w) in enumerate(zip(taps, weights)):
            arr[k].tap[i], arr[k].w[i] = int(t), int(w)
    fb = dst[0].numel()
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else fb     # a dimension of size 1 has no meaningful stride
    with torch.cuda.device(lin.device):
        check(load().emavfi_accumulate_frames_linear(dst.data_ptr(), stride(dst), len(table), srcs.data_ptr(), stride(srcs), srcs.shape[0],
                                                     nodes.data_ptr() if nodes is not None else None, stride(nodes) if nodes is not None else 0,
                                                     nodes.shape[0] if nodes is not None else 0, ctypes.cast(arr, c_void_p),
                                                     flags.data_ptr() if flags is not None else None, flags.numel() if flags is not None else 0,
                                                     fb, int(sample_bytes), int(depth), int(shift), lin.data_ptr(), int(linear_bytes), _stream()),
              "emavfi_accumulate_frames_linear")
    return dst


# ---------------------------------------------------------------- duplicate frames (include/emavfi.h, "DUPLICATE FRAME DEFINITION")
def dedup_threshold_units(fraction, depth=8) -> int:
    """The u32 threshold of duplicate_flags for "no cell's mean absolute luma difference exceeds `fraction` of full scale":
    floor(fraction * 16 * (2^depth - 1)) (a cell's measure is kept in sixteenths of a count); depth 8 for byte frames.  0 flags exactly the
    pairs whose luma is bit-identical."""
    import math
    if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0.0 <= fraction <= 1.0:
        raise ValueError("dedup_threshold_units: fraction must be a number in 0..1")
    if isinstance(depth, bool) or depth not in (8, 10, 12, 16):
        raise ValueError("dedup_threshold_units: depth must be 8, 10, 12 or 16")
    return int(math.floor(float(fraction) * (16 * ((1 << depth) - 1))))


def _sample_image(t, what, shape=None):
    """(pointer, pitch, batch stride in BYTES, sample_bytes) of an image batch [n,H,W,C] of bytes (uint8, C = 1 or 3) or of 16-bit words
    ([n,H,W] or [n,H,W,1], torch.uint16 / torch.int16); rows and batches may be strided, a row must be dense"""
    import torch
    _pinned_or_cuda(t, what)
    if t.dtype == torch.uint8:
        sb = 1
    elif t.element_size() == 2 and not t.dtype.is_floating_point:
        sb = 2
        if t.dim() == 3:
            t = t.unsqueeze(-1)
    else:
        raise ValueError(f"{what}: uint8 [n,H,W,C] or 16-bit integer [n,H,W] images expected, got {t.dtype}")
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f"{what}: a non-empty [n,H,W,C] image batch expected")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(shape)} expected, got {tuple(t.shape)}")
    n, H, W, C = t.shape
    if (C > 1 and t.stride(3) != 1) or (W > 1 and t.stride(2) != C):
        raise ValueError(f"{what}: the rows must be dense (only rows and batches may be strided)")
    pitch = t.stride(1) if H > 1 else W * C     # in samples; a dimension of size 1 has no meaningful stride: the dense value stands in
    return t.data_ptr(), pitch * sb, (t.stride(0) if n > 1 else pitch * H) * sb, sb, tuple(t.shape)


def frame_diff_cells(a, b, order="bgr", depth=None, shift=0, out=None, device=None):
    """Per pair k and cell of the 32 x 32 scene grid: the ceiling of the mean absolute luma difference of image k of `a` and image k of `b`
    in sixteenths of a count (the duplicate-frame definition of include/emavfi.h) -> int32 [n,1024].  `a` / `b`: uint8 [n,H,W,C], C = 1 (a
    Y plane) or 3 (interleaved colour, `order` says which byte is red), or 16-bit integer [n,H,W] planes whose samples are
    (word >> shift) & (2^depth - 1), depth 10, 12 or 16; device tensors or pinned host memory (`device` names the GPU), rows and batches
    may be strided, and the two may overlap (frames[:-1] against frames[1:]).  `out`: a contiguous int32 [n,1024] device tensor to fill -
    every word is written."""
    import torch
    pa, apitch, abs_, sb, shape = _sample_image(a, "frame_diff_cells(a)")
    pb, bpitch, bbs, sb2, _ = _sample_image(b, "frame_diff_cells(b)", shape)
    if sb != sb2:
        raise ValueError("frame_diff_cells: a and b must hold the same kind of sample")
    n, H, W, C = shape
    depth = (8 if sb == 1 else 16) if depth is None else int(depth)
    dev = next((t.device for t in (a, b) if t.is_cuda), None) or torch.device(device if device is not None else "cuda")
    if out is None:
        out = torch.empty(n, SCENE_SIG_WORDS, dtype=torch.int32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (n, SCENE_SIG_WORDS) and out.is_contiguous()):
        raise ValueError(f"frame_diff_cells: out must be a contiguous int32 [n,{SCENE_SIG_WORDS}] device tensor")
    with torch.cuda.device(dev):
        check(load().emavfi_frame_diff_cells(pa, apitch, abs_, pb, bpitch, bbs, n, H, W, C, _order_code(order), sb, depth, int(shift),
                                             out.data_ptr(), _stream()), "emavfi_frame_diff_cells")
    return out


def duplicate_flags(cells, threshold, flags=None, scores=None, with_scores=True):
    """Per pair k: score = the maximum of its 1024 cell measures (frame_diff_cells), flag = score <= threshold (an int in score units:
    dedup_threshold_units).  `cells`: an int32 device tensor [n,1024] with dense rows (the rows may be strided).  Returns (flags, scores):
    int32 [n] device tensors (`flags=` / `scores=` fill given ones; with_scores=False passes NULL and returns None for the scores)."""
    import torch
    _require_cuda(cells)
    if cells.dtype != torch.int32 or cells.dim() != 2 or cells.shape[0] < 1 or cells.shape[1] != SCENE_SIG_WORDS or cells.stride(1) != 1:
        raise ValueError(f"duplicate_flags: an int32 device tensor [n, {SCENE_SIG_WORDS}] with dense rows expected")
    n = cells.shape[0]
    threshold = int(threshold)
    if not 0 <= threshold < 2 ** 32:
        raise ValueError("duplicate_flags: threshold must be a u32 in score units")

    def vec(t, name):
        if t is None:
            return torch.empty(n, dtype=torch.int32, device=cells.device)
        if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (n,) and t.is_contiguous()):
            raise ValueError(f"duplicate_flags: {name} must be a contiguous int32 [{n}] device tensor")
        return t
    flags = vec(flags, "flags")
    scores = vec(scores, "scores") if (with_scores or scores is not None) else None
    with torch.cuda.device(cells.device):
        check(load().emavfi_duplicate_flags(cells.data_ptr(), cells.stride(0) if n > 1 else SCENE_SIG_WORDS, n, threshold, flags.data_ptr(),
                                            scores.data_ptr() if scores is not None else None, _stream()), "emavfi_duplicate_flags")
    return flags, scores


# ---------------------------------------------------------------- static regions (include/emavfi.h, "STATIC REGION DEFINITION")
LAYOUTS = {"interleaved": LAYOUT_INTERLEAVED, "nv12": LAYOUT_NV12, "i420": LAYOUT_I420}
STATIC_MAX_RADIUS = 16                                   # EMAVFI_STATIC_MAX_RADIUS


class StaticEntry(ctypes.Structure):
    """emavfi_static_entry"""
    _fields_ = [("a", ctypes.c_uint), ("b", ctypes.c_uint)]


def static_tolerance_units(fraction, depth=8) -> int:
    """The `tol` of static_guard_frames for "two samples that differ by at most `fraction` of full scale count as the same":
    floor(fraction * (2^depth - 1)); depth 8 for byte frames.  0 accepts bit-equal samples only."""
    import math
    if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not 0.0 <= fraction <= 1.0:
        raise ValueError("static_tolerance_units: fraction must be a number in 0..1")
    if isinstance(depth, bool) or depth not in (8, 10, 12, 16):
        raise ValueError("static_tolerance_units: depth must be 8, 10, 12 or 16")
    return int(math.floor(float(fraction) * ((1 << depth) - 1)))


def static_frame_format(pixel_format):
    """(layout, C, sample_bytes, depth, shift) of a harness pixel format as emavfi_static_guard_frames takes it: "bgr24" is interleaved
    bytes of 3 channels; "nv12" / "p01x" the NV12 layout (P01x: words with the sample in the top bits); "yuv420pN" the I420 layout (words
    with the sample in the low bits above 8 bits)"""
    if pixel_format not in FORMATS:
        raise ValueError(f"static_frame_format: unknown pixel_format {pixel_format!r}")
    return FORMATS[pixel_format].frame_format


def static_guard_frames(dst, srcs, table, size, layout=LAYOUT_INTERLEAVED, C=1, sample_bytes=1, depth=8, shift=0, radius=0, tol=0, counts=None):
    """Holds the static regions of `dst`'s frames (the static region definition of include/emavfi.h): frame k of `dst` - a post-processed
    prediction for the pair table[k] = (a, b) of frames of `srcs` - receives a's samples wherever a and b agree within `tol` (sample units:
    static_tolerance_units) over the whole window of `radius` around the pixel; every other byte is left as it was.  `dst` uint8
    [n_dst, ...], `srcs` uint8 [n_srcs, ...]: device tensors or pinned host memory with the same dense frame shape, the bytes of `size` =
    (H, W) frames of `layout` (a name of LAYOUTS or its code; C channels when interleaved); their first dimension may be strided.  16-bit
    frames travel as their bytes with sample_bytes = 2 and the sample's `depth` and `shift`.  `counts`: None, or a contiguous int32
    [n_dst] device tensor that receives every entry's number of core pixels.  The table is consumed before the call returns."""
    import torch
    H, W = (int(v) for v in size)
    layout = LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    for t, what in ((dst, "static_guard_frames(dst)"), (srcs, "static_guard_frames(srcs)")):
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous() or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames of dst's frame shape expected")
    table = list(table)
    if len(table) != dst.shape[0]:
        raise ValueError(f"static_guard_frames: {len(table)} table entries for {dst.shape[0]} destination frames")
    fb = dst[0].numel()
    want = H * W * int(sample_bytes) * (int(C) if layout == LAYOUT_INTERLEAVED else 3) // (1 if layout == LAYOUT_INTERLEAVED else 2)
    if fb != want:
        raise ValueError(f"static_guard_frames: a frame of {fb} bytes is not a {H} x {W} frame of this layout ({want} bytes)")
    if counts is not None and not (counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (len(table),) and counts.is_contiguous()):
        raise ValueError(f"static_guard_frames: counts must be a contiguous int32 [{len(table)}] device tensor")
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else fb     # a dimension of size 1 has no meaningful stride
    arr = (StaticEntry * len(table))(*(StaticEntry(int(a), int(b)) for a, b in table))
    dev = next((t.device for t in (dst, srcs) if t.is_cuda), None) or (counts.device if counts is not None else torch.device("cuda"))
    with torch.cuda.device(dev):
        check(load().emavfi_static_guard_frames(dst.data_ptr(), stride(dst), len(table), srcs.data_ptr(), stride(srcs), srcs.shape[0],
                                                ctypes.cast(arr, c_void_p), H, W, layout, int(C), int(sample_bytes), int(depth), int(shift),
                                                int(radius), int(tol), counts.data_ptr() if counts is not None else None, _stream()),
              "emavfi_static_guard_frames")
    return dst


# ---------------------------------------------------------------- the active picture (include/emavfi.h, "ACTIVE AREA DEFINITION")
ACTIVE_ALIGN = (2, 16)     # a rectangle's rows / columns: multiples of these (ACTIVE_ALIGN_Y, ACTIVE_ALIGN_X of csrc/active_elem.h)


def active_level_units(tolerance, depth=8, yuv=False, full_range=False) -> int:
    """The `level` of active_bounds: black plus floor(tolerance * (2^depth - 1)); a sample above it is content.  Black is 16 << (depth - 8)
    for a limited-range Y'CbCr format (`yuv` and not `full_range`) and 0 otherwise; `tolerance` a fraction of full scale in [0, 1].  Clipped to
    2^depth - 1 (nothing is content there)."""
    import math
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not 0.0 <= tolerance <= 1.0:
        raise ValueError("active_level_units: tolerance must be a number in 0..1")
    if isinstance(depth, bool) or depth not in (8, 10, 12, 16):
        raise ValueError("active_level_units: depth must be 8, 10, 12 or 16")
    full = (1 << depth) - 1
    black = (16 << (depth - 8)) if (yuv and not full_range) else 0
    return min(full, black + int(math.floor(float(tolerance) * full)))


def active_rect(bounds, H, W):
    """The rectangle (top, left, height, width) of a set of frame bounds [(top, bottom, left, right), ...] as active_bounds writes them:
    their union, grown outward to even rows and to columns that are multiples of 16, clipped to the H x W frame.  An empty union - no
    bounds, or no frame with content - and a rectangle that covers the frame give the whole frame, (0, 0, H, W).  Pure host integers."""
    H, W = int(H), int(W)
    top, bottom, left, right = H, 0, W, 0
    for b in bounds:
        t, bo, l, r = (int(v) for v in b)
        top, bottom, left, right = min(top, t), max(bottom, bo), min(left, l), max(right, r)
    if bottom <= top or right <= left:
        return 0, 0, H, W
    ay, ax = ACTIVE_ALIGN
    top, left = top // ay * ay, left // ax * ax
    bottom, right = min(H, -(-bottom // ay) * ay), min(W, -(-right // ax) * ax)
    return top, left, bottom - top, right - left


def active_rect_check(rect, H, W, what="active_area"):
    """(top, left, height, width) as ints, validated as the harness takes an explicit rectangle: four integers, with area, inside the H x W
    frame, top and bottom multiples of 2 and left and right multiples of 16 - a bottom or right edge may instead be the frame's own.  With
    H and W None the frame is not known yet: only what can be said of the rectangle alone is checked.  ValueError names the rule."""
    if (not isinstance(rect, (tuple, list)) or len(rect) != 4
            or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in rect)):
        raise ValueError(f"{what}: None (the whole frame), 'auto' or a rectangle (top, left, height, width) of integers expected, got {rect!r}")
    top, left, height, width = (int(v) for v in rect)
    if height < 1 or width < 1:
        raise ValueError(f"{what}: the rectangle {(top, left, height, width)} has no area")
    if top < 0 or left < 0 or (H is not None and (top + height > H or left + width > W)):
        raise ValueError(f"{what}: the rectangle {(top, left, height, width)} leaves the frame" + (f" of {H} x {W}" if H is not None else ""))
    ay, ax = ACTIVE_ALIGN
    if top % ay or (H is not None and (top + height) % ay and top + height != H):
        raise ValueError(f"{what}: top and bottom of {(top, left, height, width)} must be multiples of {ay} (the bottom may be the frame's): "
                         "4:2:0 chroma crops at whole samples")
    if left % ax or (W is not None and (left + width) % ax and left + width != W):
        raise ValueError(f"{what}: left and right of {(top, left, height, width)} must be multiples of {ax} (the right may be the frame's): "
                         "the pitched kernels keep their 16-byte accesses")
    return top, left, height, width



def active_bounds(img, level=0, depth=None, shift=0, out=None, device=None):
    """Per image k the bounds {top, bottom, left, right} of its content (the active area definition of include/emavfi.h) -> int32 [n,4]; an
    image without content gives {H, 0, W, 0}.  `img`: uint8 [n,H,W,C], C = 1 (a Y plane) or 3 (interleaved colour: any channel above `level`
    counts), or 16-bit integer [n,H,W] planes whose samples are (word >> shift) & (2^depth - 1), depth 10, 12 or 16; a device tensor or pinned
    host memory (`device` names the GPU), rows and batches may be strided.  `level`: a sample above it is content (active_level_units).
    `out`: a contiguous int32 [n,4] device tensor to fill - every word is written whatever it held."""
    import torch
    p, pitch, bs, sb, (n, H, W, C) = _sample_image(img, "active_bounds(img)")
    depth = (8 if sb == 1 else 16) if depth is None else int(depth)
    dev = img.device if img.is_cuda else torch.device(device if device is not None else "cuda")
    if out is None:
        out = torch.empty(n, 4, dtype=torch.int32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (n, 4) and out.is_contiguous()):
        raise ValueError("active_bounds: out must be a contiguous int32 [n,4] device tensor")
    level = int(level)
    if not 0 <= level < 2 ** 32:
        raise ValueError("active_bounds: level must be a u32 in sample units")
    with torch.cuda.device(dev):
        check(load().emavfi_active_bounds(p, pitch, bs, n, H, W, C, sb, depth, int(shift), level, out.data_ptr(), _stream()),
              "emavfi_active_bounds")
    return out


def fill_outside_frames(dst, srcs, table, size, rect, layout=LAYOUT_INTERLEAVED, C=1, sample_bytes=1):
    """Puts the bars back: frame k of `dst` receives the samples of frame table[k] of `srcs` OUTSIDE `rect` = (top, left, height, width);
    bytes inside it are neither read nor written (the active area definition of include/emavfi.h).  `dst` uint8 [n_dst, ...], `srcs` uint8
    [n_srcs, ...]: device tensors or pinned host memory with the same dense frame shape, the bytes of `size` = (H, W) frames of `layout` (a
    name of LAYOUTS or its code; C channels when interleaved); their first dimension may be strided.  16-bit frames travel as their bytes
    with sample_bytes = 2.  The table is consumed before the call returns."""
    import torch
    H, W = (int(v) for v in size)
    top, left, height, width = (int(v) for v in rect)
    layout = LAYOUTS[layout] if isinstance(layout, str) else int(layout)
    for t, what in ((dst, "fill_outside_frames(dst)"), (srcs, "fill_outside_frames(srcs)")):
        _pinned_or_cuda(t, what)
        if t.dtype != torch.uint8 or t.dim() < 2 or t.numel() == 0 or not t[0].is_contiguous() or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise ValueError(f"{what}: a non-empty uint8 [frames, ...] tensor with dense frames of dst's frame shape expected")
    table = [int(v) for v in table]
    if len(table) != dst.shape[0]:
        raise ValueError(f"fill_outside_frames: {len(table)} table entries for {dst.shape[0]} destination frames")
    if any(not 0 <= v < 2 ** 32 for v in table):
        raise ValueError("fill_outside_frames: the table holds u32 indices into srcs")
    fb = dst[0].numel()
    want = H * W * int(sample_bytes) * (int(C) if layout == LAYOUT_INTERLEAVED else 3) // (1 if layout == LAYOUT_INTERLEAVED else 2)
    if fb != want:
        raise ValueError(f"fill_outside_frames: a frame of {fb} bytes is not a {H} x {W} frame of this layout ({want} bytes)")
    stride = lambda t: t.stride(0) if t.shape[0] > 1 else fb     # a dimension of size 1 has no meaningful stride
    arr = (ctypes.c_uint * len(table))(*table)
    dev = next((t.device for t in (dst, srcs) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_fill_outside_frames(dst.data_ptr(), stride(dst), len(table), srcs.data_ptr(), stride(srcs), srcs.shape[0],
                                                ctypes.cast(arr, c_void_p), H, W, layout, int(C), int(sample_bytes), top, left, height, width,
                                                _stream()), "emavfi_fill_outside_frames")
    return dst


def preprocess_u8_pitched(frames_hwc, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None, out=None):
    """preprocess_u8 of the dense copy of `frames_hwc`, bit for bit, WITHOUT making that copy: uint8 [B,H,W,C] whose rows and batches may be
    strided (a sub-rectangle of larger frames; pitches come from .stride()) -> fp32 [B,C,H,W].  A device tensor or pinned host memory
    (`device` names the GPU); bytes between the rows are never read.  `out`: a contiguous fp32 [B,C,H,W] device tensor to fill."""
    import torch
    p, pitch, bs = _byte_image(frames_hwc, "preprocess_u8_pitched")
    B, H, W, C = frames_hwc.shape
    dev = frames_hwc.device if frames_hwc.is_cuda else torch.device(device if device is not None else "cuda")
    m, s = _stats(mean, std, C)
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, C, H, W) and out.is_contiguous()):
        raise ValueError("preprocess_u8_pitched: out must be a contiguous fp32 [B,C,H,W] device tensor")
    with torch.cuda.device(dev):
        check(load().emavfi_preprocess_u8_pitched(p, pitch, bs, out.data_ptr(), B, H, W, C, m, s, _stream()), "emavfi_preprocess_u8_pitched")
    return out


def postprocess_u8_pitched(frames_nchw, out, denormalize=True, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """postprocess_u8 into `out`, uint8 [B,H,W,C] whose rows and batches may be strided (a sub-rectangle of larger frames; a device tensor or
    pinned host memory): the bytes postprocess_u8 would write into a dense tensor, bit for bit; bytes between the rows are left as they were."""
    import torch
    _require_cuda(frames_nchw)
    x = _f32c(frames_nchw)
    if x.dim() != 4:
        raise ValueError("postprocess_u8_pitched: [B,C,H,W] tensor expected")
    B, C, H, W = x.shape
    p, pitch, bs = _byte_image(out, "postprocess_u8_pitched(out=)", (B, H, W, C))
    m, s = _stats(mean, std, C, ctypes.c_double)
    with torch.cuda.device(x.device):
        check(load().emavfi_postprocess_u8_pitched(x.data_ptr(), p, pitch, bs, B, H, W, C, m, s, 1 if denormalize else 0, _stream()),
              "emavfi_postprocess_u8_pitched")
    return out


# ---------------------------------------------------------------- test-time ensembling (include/emavfi.h, "ENSEMBLE DEFINITION")
FLIP_H, FLIP_V = 1, 2                            # EMAVFI_FLIP_H, EMAVFI_FLIP_V; 3 = both, 0 = the identity
ENSEMBLES = (None, "reverse", "flip", "full")    # EMA_VFI.ensemble
ENSEMBLE_FLIPS = (0, 3, 1, 2)                    # the member order of "flip" and of each half of "full": the pairs {identity, HV}, {H, V}


def _ensemble_planes(t, what):
    """(planes, H, W) of a dense fp32 [..., H, W] tensor on the device or in pinned host memory"""
    import torch
    _pinned_or_cuda(t, what)
    if t.dtype != torch.float32 or t.dim() < 2 or t.numel() == 0 or not t.is_contiguous():
        raise ValueError(f"{what}: a non-empty contiguous float32 [..., H, W] tensor expected")
    H, W = int(t.shape[-2]), int(t.shape[-1])
    return t.numel() // (H * W), H, W


def flip_f32(x, flip, out=None):
    """out = x mirrored over its last two dimensions (the ensemble definition of include/emavfi.h): flip & FLIP_H maps column x to W - 1 - x,
    flip & FLIP_V row y to H - 1 - y; 0 is a copy.  `x`, `out`: contiguous float32 [..., H, W] of one shape, device tensors or pinned host
    memory, not overlapping.  Runs on the current stream; returns `out`."""
    import torch
    planes, H, W = _ensemble_planes(x, "flip_f32(x)")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device if x.is_cuda else "cuda")
    elif _ensemble_planes(out, "flip_f32(out)") != (planes, H, W) or out.shape != x.shape:
        raise ValueError(f"flip_f32: out {tuple(out.shape)} is not of x's shape {tuple(x.shape)}")
    dev = next((t.device for t in (x, out) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_flip_f32(x.data_ptr(), out.data_ptr(), planes, H, W, int(flip), _stream()), "emavfi_flip_f32")
    return out


def ensemble_mean_f32(members, flips, out=None):
    """out = the tree mean of n in {1, 2, 4, 8} members, member k read through flips[k] (the ensemble definition of include/emavfi.h): a
    balanced pairwise tree of fp32 additions in the order given, then one multiplication by 1 / n.  `members`: contiguous float32
    [..., H, W] tensors of one shape, device tensors or pinned host memory; `out` the same, overlapping none of them.  The lists are
    consumed before the call returns.  Runs on the current stream; returns `out`."""
    import torch
    members, flips = list(members), [int(f) for f in flips]
    if not members or len(members) != len(flips):
        raise ValueError(f"ensemble_mean_f32: {len(members)} members for {len(flips)} flips")
    planes, H, W = _ensemble_planes(members[0], "ensemble_mean_f32(members[0])")
    for k, m in enumerate(members[1:], 1):
        if _ensemble_planes(m, f"ensemble_mean_f32(members[{k}])") != (planes, H, W) or m.shape != members[0].shape:
            raise ValueError(f"ensemble_mean_f32: members[{k}] {tuple(m.shape)} is not of members[0]'s shape {tuple(members[0].shape)}")
    if out is None:
        out = torch.empty(members[0].shape, dtype=torch.float32, device=next((m.device for m in members if m.is_cuda), "cuda"))
    elif _ensemble_planes(out, "ensemble_mean_f32(out)") != (planes, H, W) or out.shape != members[0].shape:
        raise ValueError(f"ensemble_mean_f32: out {tuple(out.shape)} is not of the members' shape {tuple(members[0].shape)}")
    n = len(members)
    ptrs = (c_void_p * n)(*(m.data_ptr() for m in members))
    codes = (c_int * n)(*flips)
    dev = next((t.device for t in (out, *members) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_ensemble_mean_f32(ctypes.cast(ptrs, POINTER(c_void_p)), ctypes.cast(codes, POINTER(c_int)), n, out.data_ptr(),
                                              planes, H, W, _stream()), "emavfi_ensemble_mean_f32")
    return out


# ---------------------------------------------------------------- frame borders (include/emavfi.h, "BORDER DEFINITION")
BORDER_REPLICATE, BORDER_REFLECT = 0, 1          # EMAVFI_BORDER_REPLICATE, EMAVFI_BORDER_REFLECT
BORDER_MODES = ("replicate", "reflect")          # by code
BORDER_MAX = 64                                  # EMAVFI_BORDER_MAX


def _border_n(N, what, least=0):
    if isinstance(N, bool) or not isinstance(N, int) or not least <= N <= BORDER_MAX:
        raise ValueError(f"{what}: the border N must be an int in {least}..{BORDER_MAX}, got {N!r}")
    return N


def _border_mode(mode, what):
    """the code of a mode given by name or by code"""
    if isinstance(mode, str) and mode in BORDER_MODES:
        return BORDER_MODES.index(mode)
    if not isinstance(mode, bool) and isinstance(mode, int) and 0 <= mode < len(BORDER_MODES):
        return mode
    raise ValueError(f"{what}: the border mode must be one of {BORDER_MODES}, got {mode!r}")


def border_padded_size(H, W, N):
    """(H + 2 N, W + 2 N): the size of an H x W picture extended by N pixels on each side.  Pure; refuses an N outside 0..BORDER_MAX and
    any dimension of either size outside 1..16384, as the entries do."""
    H, W, N = int(H), int(W), _border_n(N, "border_padded_size")
    Hp, Wp = H + 2 * N, W + 2 * N
    if not (1 <= H and 1 <= W and Hp <= RESIZE_MAX_DIM and Wp <= RESIZE_MAX_DIM):
        raise ValueError(f"border_padded_size: {H} x {W} with a border of {N} ({Hp} x {Wp} padded): every dimension must lie in 1..{RESIZE_MAX_DIM}")
    return Hp, Wp


def _border_out(x, out, shape, what):
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=x.device if x.is_cuda else "cuda")
    _ensemble_planes(out, f"{what}(out)")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: out {tuple(out.shape)} is not of the shape {tuple(shape)} that x {tuple(x.shape)} gives")
    return out


def border_pad_f32(x, N, mode="replicate", out=None):
    """out = x extended by N pixels on each side of its last two dimensions (the border definition of include/emavfi.h): mode "replicate"
    repeats the edge sample, "reflect" mirrors about it without repeating it (several reflections where N > size - 1).  `x`: contiguous
    float32 [..., H, W]; `out`: the same with [H + 2 N, W + 2 N]; device tensors or pinned host memory, not overlapping.  N = 0 is a copy.
    Runs on the current stream; returns `out`."""
    import torch
    what = "border_pad_f32"
    planes, H, W = _ensemble_planes(x, f"{what}(x)")
    N, code = _border_n(N, what), _border_mode(mode, what)
    out = _border_out(x, out, tuple(x.shape[:-2]) + border_padded_size(H, W, N), what)
    dev = next((t.device for t in (x, out) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_border_pad_f32(x.data_ptr(), out.data_ptr(), planes, H, W, N, code, _stream()), "emavfi_border_pad_f32")
    return out


def border_crop_f32(x, N, out=None):
    """out = x without the N pixels on each side of its last two dimensions: the inverse of border_pad_f32 in either mode.  `x`: contiguous
    float32 [..., H + 2 N, W + 2 N]; `out`: the same with [H, W]; device tensors or pinned host memory, not overlapping.  Runs on the
    current stream; returns `out`."""
    import torch
    what = "border_crop_f32"
    planes, Hp, Wp = _ensemble_planes(x, f"{what}(x)")
    N = _border_n(N, what)
    H, W = Hp - 2 * N, Wp - 2 * N
    if H < 1 or W < 1:
        raise ValueError(f"{what}: x {tuple(x.shape)} has nothing inside a border of {N}")
    border_padded_size(H, W, N)
    out = _border_out(x, out, tuple(x.shape[:-2]) + (H, W), what)
    dev = next((t.device for t in (x, out) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_border_crop_f32(x.data_ptr(), out.data_ptr(), planes, H, W, N, _stream()), "emavfi_border_crop_f32")
    return out


# ---------------------------------------------------------------- coarse flow (include/emavfi.h, "COARSE FLOW DEFINITION")
FLOW_SCALES = (2, 4, 8)                          # EMA_VFI.flow_scale, beside None


def flow_scale_arg(s, what):
    """s of the coarse flow definition: an int, one of FLOW_SCALES"""
    if isinstance(s, bool) or not isinstance(s, int) or s not in FLOW_SCALES:
        raise ValueError(f"{what}: the flow scale must be one of {FLOW_SCALES}, got {s!r}")
    return s


def coarse_size(H, W, s):
    """(ceil(H / s), ceil(W / s)): the size at which an H x W pair's flow is estimated.  Pure."""
    H, W, s = int(H), int(W), flow_scale_arg(s, "coarse_size")
    if not (1 <= H <= RESIZE_MAX_DIM and 1 <= W <= RESIZE_MAX_DIM):
        raise ValueError(f"coarse_size: {H} x {W}: every dimension must lie in 1..{RESIZE_MAX_DIM}")
    return (H + s - 1) // s, (W + s - 1) // s


def downscale_f32(x, s, out=None):
    """out = down_s(x) over the last two dimensions (step 1 of the coarse flow definition): the balanced quadtree mean of s x s blocks,
    edge blocks filled by clamping.  `x`: contiguous float32 [..., H, W]; `out`: the same with [ceil(H / s), ceil(W / s)]; device
    tensors or pinned host memory, not overlapping.  Runs on the current stream; returns `out`."""
    import torch
    what = "downscale_f32"
    planes, H, W = _ensemble_planes(x, f"{what}(x)")
    s = flow_scale_arg(s, what)
    out = _border_out(x, out, tuple(x.shape[:-2]) + coarse_size(H, W, s), what)
    dev = next((t.device for t in (x, out) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_downscale_f32(x.data_ptr(), out.data_ptr(), planes, H, W, s, _stream()), "emavfi_downscale_f32")
    return out


def upsample_flow_f32(flow_s, size, s, out=None):
    """out = step 3 of the coarse flow definition: `flow_s` (contiguous float32 [..., Hs, Ws], estimated at 1 / s) sampled bilinearly
    at half-pixel centres to `size` = (H, W) and multiplied by s.  Hs, Ws must be coarse_size(H, W, s).  Device tensors or pinned host
    memory, not overlapping.  Runs on the current stream; returns `out`."""
    import torch
    what = "upsample_flow_f32"
    planes, Hs, Ws = _ensemble_planes(flow_s, f"{what}(flow_s)")
    s = flow_scale_arg(s, what)
    H, W = (int(v) for v in size)
    if coarse_size(H, W, s) != (Hs, Ws):
        raise ValueError(f"{what}: flow_s is {Hs} x {Ws}, but {H} x {W} at s = {s} has a coarse size of {coarse_size(H, W, s)}")
    out = _border_out(flow_s, out, tuple(flow_s.shape[:-2]) + (H, W), what)
    dev = next((t.device for t in (flow_s, out) if t.is_cuda), None) or torch.device("cuda")
    with torch.cuda.device(dev):
        check(load().emavfi_upsample_flow_f32(flow_s.data_ptr(), out.data_ptr(), planes, Hs, Ws, H, W, s, _stream()),
              "emavfi_upsample_flow_f32")
    return out


def _forward_pair(frame1, frame2, what):
    """two checked fp32 contiguous [B, C, H, W] device batches of one shape"""
    _require_cuda(frame1, frame2)
    if frame1.shape != frame2.shape or frame1.dim() != 4 or frame1.device != frame2.device:
        raise ValueError(f"{what}: two [B,C,H,W] tensors of one shape on one device expected, got {tuple(frame1.shape)} and {tuple(frame2.shape)}")
    return _f32c(frame1), _f32c(frame2)


def _forward_workspace(model, B, H, W, dt, dev):
    nws = load().emavfi_workspace_bytes(*model, B, H, W, dt)
    if nws == 0:
        raise RuntimeError(f"emavfi_workspace_bytes: {last_error()}")
    return workspace(nws, dev)


def forward_flow(packed, frame1, frame2, mid_channels, num_blocks, dtype, out=None):
    """The flow [B, 2, H, W] (float32) of the plain forward of (frame1, frame2): emavfi_forward_flow, the forward's launches up to the
    one that writes the flow - bit for bit taps["flow"] of EMA_VFI.forward(..., return_taps=True).  `packed`: the model's blob for
    `dtype` (EMA_VFI.packed_weights).  Runs on the current stream."""
    import torch
    f1, f2 = _forward_pair(frame1, frame2, "forward_flow")
    B, C, H, W = f1.shape
    dt, dev = dtype_code(dtype), f1.device
    if out is None:
        out = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 2, H, W) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"forward_flow: out must be a contiguous float32 {(B, 2, H, W)} tensor on {dev}")
    with torch.cuda.device(dev):
        ws = _forward_workspace((C, mid_channels, num_blocks), B, H, W, dt, dev)
        check(load().emavfi_forward_flow(C, mid_channels, num_blocks, packed.data_ptr(), packed.numel(), f1.data_ptr(), f2.data_ptr(),
                                         out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, dt, _stream()), "emavfi_forward_flow")
    return out


def forward_given_flow(packed, frame1, frame2, flow, mid_channels, num_blocks, dtype, out=None, return_taps=False, gather_blocks=0,
                       stage=None, _events=None):
    """The plain forward of (frame1, frame2) with `flow` (contiguous float32 [B, 2, H, W], read in place) where motion estimation's
    output would be: emavfi_forward_given_flow (step 4 of the coarse flow definition; context encoding and motion estimation are not
    launched).  Returns the float32 frame, or (frame, taps) with the taps such a forward has: feat, warped, fused_i.  gather_blocks:
    emavfi_forward_routed's mask; stage / _events: the C-ABI's stage-event array and bench.py's (events, count).  Runs on the current
    stream."""
    import torch
    from collections import OrderedDict
    f1, f2 = _forward_pair(frame1, frame2, "forward_given_flow")
    B, C, H, W = f1.shape
    dt, dev = dtype_code(dtype), f1.device
    if not flow.is_cuda or flow.device != dev or flow.dtype != torch.float32 or tuple(flow.shape) != (B, 2, H, W) or not flow.is_contiguous():
        raise ValueError(f"forward_given_flow: flow must be a contiguous float32 {(B, 2, H, W)} tensor on {dev}")
    if out is None:
        out = torch.empty_like(f1)
    elif out.dtype != torch.float32 or out.shape != f1.shape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"forward_given_flow: out must be a contiguous float32 {tuple(f1.shape)} tensor on {dev}")
    taps, taps_arg = None, None
    if return_taps:
        m = mid_channels
        taps = OrderedDict(feat=torch.empty(B, m, H, W, device=dev), warped=torch.empty(B, C, H, W, device=dev))
        ptrs = [taps["feat"].data_ptr(), None, None, taps["warped"].data_ptr(), None]
        for i in range(num_blocks):
            taps[f"fused_{i}"] = torch.empty(B, m + 3, H, W, device=dev)
            ptrs.append(taps[f"fused_{i}"].data_ptr())
        taps_arg = ctypes.cast((c_void_p * len(ptrs))(*ptrs), POINTER(c_void_p))
    evp, nev = _events_arg(_events)
    with torch.cuda.device(dev):
        ws = _forward_workspace((C, mid_channels, num_blocks), B, H, W, dt, dev)
        check(load().emavfi_forward_given_flow(C, mid_channels, num_blocks, packed.data_ptr(), packed.numel(), f1.data_ptr(), f2.data_ptr(),
                                               flow.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, dt, taps_arg, stage, evp,
                                               nev, int(gather_blocks), _stream()), "emavfi_forward_given_flow")
    return (out, taps) if return_taps else out


# ---------------------------------------------------------------- agreement guard (include/emavfi.h, "AGREEMENT GUARD DEFINITION")
AGREEMENT_MAX_BATCH = 65535                      # EMAVFI_AGREEMENT_MAX_BATCH
AGREEMENT_ENSEMBLES = ("reverse", "full")        # the ensembles that run both time directions


def agreement_args(tol, radius, what):
    """(tol, radius) of an agreement guard as a float in [0, 1] and an int in 0..STATIC_MAX_RADIUS, or a ValueError naming `what`"""
    import math
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or math.isnan(tol) or not 0.0 <= tol <= 1.0:
        raise ValueError(f"{what}: the agreement tolerance must be a number in [0, 1] (the output's full scale), got {tol!r}")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= STATIC_MAX_RADIUS:
        raise ValueError(f"{what}: the agreement radius must be an int in 0..{STATIC_MAX_RADIUS}, got {radius!r}")
    return float(tol), radius


def agreement_guard_f32(u, v, a, b, tol, radius=0, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None, counts=None):
    """out = the agreement guard of include/emavfi.h ("AGREEMENT GUARD DEFINITION"): (u + v) / 2 where the two time directions `u` and `v`
    agree within `tol` (full-scale units) over the whole window of `radius` around the pixel, and the de-normalised, clamped blend of the
    normalised sources `a`, `b` where they do not.  All five: contiguous float32 [B, C, H, W] of one shape, C = 1..4, device tensors or
    pinned host memory; `out` overlaps none of the inputs.  `counts`: None, or a contiguous int32 [B] device tensor that receives every
    sample's number of held pixels.  Runs on the current stream; returns `out`."""
    import torch
    what = "agreement_guard_f32"
    tol, radius = agreement_args(tol, radius, what)
    for t, name in ((u, "u"), (v, "v"), (a, "a"), (b, "b")):
        _ensemble_planes(t, f"{what}({name})")
        if t.dim() != 4 or t.shape != u.shape:
            raise ValueError(f"{what}: {name} {tuple(t.shape)}: four [B, C, H, W] tensors of one shape expected (u is {tuple(u.shape)})")
    B, C, H, W = (int(d) for d in u.shape)
    if not (1 <= C <= 4 and B <= AGREEMENT_MAX_BATCH):
        raise ValueError(f"{what}: [B, C, H, W] = {tuple(u.shape)}: C must be 1..4 and B at most {AGREEMENT_MAX_BATCH}")
    m, s = _stats(mean, std, C)
    dev = next((t.device for t in (u, v, a, b, out, counts) if t is not None and t.is_cuda), None) or torch.device("cuda")
    if out is None:
        out = torch.empty(u.shape, dtype=torch.float32, device=dev)
    elif _ensemble_planes(out, f"{what}(out)") is None or out.shape != u.shape:
        raise ValueError(f"{what}: out {tuple(out.shape)} is not of the inputs' shape {tuple(u.shape)}")
    if counts is not None and not (counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (B,) and counts.is_contiguous()):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{B}] device tensor")
    with torch.cuda.device(dev):
        check(load().emavfi_agreement_guard_f32(u.data_ptr(), v.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), B, C, H, W, radius, tol,
                                                m, s, counts.data_ptr() if counts is not None else None, _stream()),
              "emavfi_agreement_guard_f32")
    return out


# ---------------------------------------------------------------- global motion (include/emavfi.h, "ALIGN DEFINITION")
ALIGN_CELL = 4            # EMAVFI_ALIGN_CELL
ALIGN_MAX_RADIUS = 32     # EMAVFI_ALIGN_MAX_RADIUS, in cells
ALIGN_MAX_RATIO = 1024    # EMAVFI_ALIGN_MAX_RATIO


def align_args(R_px, ratio, what):
    """(R, ratio units) of an alignment given as a radius in pixels - a multiple of 4 in 4..128 - and an acceptance ratio in [0, 1]: the
    radius in cells and round(ratio * 1024), or a ValueError naming `what`"""
    import math
    if isinstance(R_px, bool) or not isinstance(R_px, int) or R_px % ALIGN_CELL or not ALIGN_CELL <= R_px <= ALIGN_CELL * ALIGN_MAX_RADIUS:
        raise ValueError(f"{what}: the align radius must be an int multiple of {ALIGN_CELL} in {ALIGN_CELL}..{ALIGN_CELL * ALIGN_MAX_RADIUS} "
                         f"pixels, got {R_px!r}")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or math.isnan(ratio) or not 0.0 <= ratio <= 1.0:
        raise ValueError(f"{what}: the align ratio must be a number in [0, 1], got {ratio!r}")
    return R_px // ALIGN_CELL, int(round(ratio * ALIGN_MAX_RATIO))


def align_fits(R, H, W):
    """whether a radius of R cells keeps at least half of each axis of an H x W frame's grid: 2 R <= min(H // 4, W // 4)"""
    return 2 * R <= min(int(H) // ALIGN_CELL, int(W) // ALIGN_CELL)


def _align_words(t, what, shape=None):
    """a contiguous device tensor of 16-bit words (int16 or uint16: the words are unsigned either way) [B, Hc, Wc]"""
    import torch
    kinds = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)
    if not t.is_cuda:
        _require_cuda(t)
    if t.dtype not in kinds or t.dim() != 3 or t.numel() == 0 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what}: a non-empty contiguous 16-bit integer [B, Hc, Wc] device tensor expected"
                         + (f" of shape {tuple(shape)}" if shape is not None else "") + f", got {t.dtype} {tuple(t.shape)}")
    return tuple(int(d) for d in t.shape)


def _align_frames(x, what):
    import torch
    if not x.is_cuda:
        _require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError(f"{what}: a non-empty contiguous float32 [B, C, H, W] device tensor expected, got {x.dtype} {tuple(x.shape)}")
    return tuple(int(d) for d in x.shape)


def align_signature_f32(x, out=None):
    """out = the signature grid of the align definition: per 4 x 4 cell the sum of the 16 quantised lumas, 0..16368.  `x`: contiguous
    float32 [B, 3, H, W] on the device, H and W in 8..16384; `out`: int16 [B, H // 4, W // 4] (the words are unsigned; no value reaches
    the sign bit).  Runs on the current stream; returns `out`."""
    import torch
    what = "align_signature_f32"
    B, C, H, W = _align_frames(x, f"{what}(x)")
    if C != 3:
        raise ValueError(f"{what}: x {tuple(x.shape)}: three channels expected")
    if not (8 <= H <= RESIZE_MAX_DIM and 8 <= W <= RESIZE_MAX_DIM):
        raise ValueError(f"{what}: x {tuple(x.shape)}: H and W must lie in 8..{RESIZE_MAX_DIM}")
    shape = (B, H // ALIGN_CELL, W // ALIGN_CELL)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=x.device)
    else:
        _align_words(out, f"{what}(out)", shape)
    with torch.cuda.device(x.device):
        check(load().emavfi_align_signature_f32(x.data_ptr(), out.data_ptr(), B, H, W, _stream()), "emavfi_align_signature_f32")
    return out


def align_search(sig_a, sig_b, R, ratio, out=None, workspace_=None):
    """out = the records {4 dy*, 4 dx*, m(d*), m(0)} of the align definition for the B samples of two signature batches: int32 [B, 4] on
    the device.  `sig_a`, `sig_b`: 16-bit integer [B, Hc, Wc] device tensors of one shape; `R`: the radius in cells, 1..32, with
    2 R <= min(Hc, Wc); `ratio`: the acceptance ratio in 1024ths, 0..1024.  `workspace_`: None (the stream's scratch buffer) or a uint8
    device tensor of at least emavfi_align_workspace_bytes(B, R) bytes; it is cleared by the entry.  Runs on the current stream."""
    import torch
    what = "align_search"
    B, Hc, Wc = _align_words(sig_a, f"{what}(sig_a)")
    _align_words(sig_b, f"{what}(sig_b)", (B, Hc, Wc))
    for v, name in ((R, "R"), (ratio, "ratio")):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an int, got {v!r}")
    if out is None:
        out = torch.empty(B, 4, dtype=torch.int32, device=sig_a.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (B, 4) and out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous int32 [{B}, 4] device tensor")
    with torch.cuda.device(sig_a.device):
        L = load()
        ws = workspace_ if workspace_ is not None else workspace(max(L.emavfi_align_workspace_bytes(B, R), 8), sig_a.device)
        check(L.emavfi_align_search(sig_a.data_ptr(), sig_b.data_ptr(), B, Hc, Wc, R, ratio, ws.data_ptr(), ws.numel() * ws.element_size(),
                                    out.data_ptr(), _stream()), "emavfi_align_search")
    return out


def shift_f32(x, shifts, sign, out=None):
    """out[b] = x[b] moved by sign * (shifts[b, 0] >> 1, shifts[b, 1] >> 1) pixels with its edges replicated (step 4 of the align
    definition): sign = +1 makes a' of a, sign = -1 makes b' of b.  `x`, `out`: contiguous float32 [B, C, H, W] device tensors, not
    overlapping; `shifts`: contiguous int32 [B, 4] on the device, read there by the kernel - nothing waits on the host, and any content is
    safe.  Runs on the current stream; returns `out`."""
    import torch
    what = "shift_f32"
    B, C, H, W = _align_frames(x, f"{what}(x)")
    if not (shifts.is_cuda and shifts.dtype == torch.int32 and tuple(shifts.shape) == (B, 4) and shifts.is_contiguous()):
        raise ValueError(f"{what}: shifts must be a contiguous int32 [{B}, 4] device tensor")
    if isinstance(sign, bool) or not isinstance(sign, int) or sign not in (1, -1):
        raise ValueError(f"{what}: sign must be +1 or -1, got {sign!r}")
    if out is None:
        out = torch.empty_like(x)
    elif _align_frames(out, f"{what}(out)") != (B, C, H, W):
        raise ValueError(f"{what}: out {tuple(out.shape)} is not of x's shape {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        check(load().emavfi_shift_f32(x.data_ptr(), out.data_ptr(), B, C, H, W, shifts.data_ptr(), int(sign), _stream()), "emavfi_shift_f32")
    return out


def align_pair_f32(a, b, R_px, ratio):
    """(a', b', shifts) of the align definition for two normalised float32 [B, 3, H, W] device batches: the signatures of both, the
    search, and both frames moved into the midpoint's coordinates - five launches and a clear on the current stream, no host wait.
    `R_px`: the search radius in pixels, a multiple of 4 in 4..128 with 2 R_px / 4 <= min(H // 4, W // 4); `ratio`: the acceptance
    ratio in [0, 1].  `shifts`: int32 [B, 4] = {dy, dx in pixels, m(d*), m(0)} per sample, on the device."""
    what = "align_pair_f32"
    R, units = align_args(R_px, ratio, what)
    shape = _align_frames(a, f"{what}(a)")
    if _align_frames(b, f"{what}(b)") != shape or shape[1] != 3:
        raise ValueError(f"{what}: two [B, 3, H, W] tensors of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    if min(shape[2:]) < 8 or not align_fits(R, *shape[2:]):
        raise ValueError(f"{what}: a radius of {R_px} pixels ({R} cells) needs frames of at least {8 * R} x {8 * R} pixels "
                         f"(2 R <= min(H // 4, W // 4)), got {shape[2]} x {shape[3]}")
    shifts = align_search(align_signature_f32(a), align_signature_f32(b), R, units)
    return shift_f32(a, shifts, 1), shift_f32(b, shifts, -1), shifts


# ---------------------------------------------------------------- frame metrics on the device (include/emavfi.h, "FRAME METRIC DEFINITION")
METRICS_WINDOW = 11      # EMAVFI_METRICS_WINDOW


def frame_metrics_u8(a, b, out=None, device=None):
    """Scores image a against image b per channel: uint8 [B,H,W,C] each, C = 1..4 -> int64 [B,C,2] = {sse, ssimq} (the frame-metric definition
    of include/emavfi.h: the sum of squared differences, and the sum over the 11 x 11 windows of floor(ssim * 2^32)); `psnr` and `ssim` turn
    the two into the usual figures.  `a` / `b`: device tensors or pinned host memory (`device` names the GPU), rows and batches may be
    strided, each side on its own.  `out`: a contiguous int64 [B,C,2] device or pinned tensor to fill - every word is written."""
    import torch
    ap, apitch, abs_ = _byte_image(a, "frame_metrics_u8(a)")
    bp, bpitch, bbs = _byte_image(b, "frame_metrics_u8(b)", a.shape)
    B, H, W, C = a.shape
    dev = next((t.device for t in (a, b) if t.is_cuda), None) or torch.device(device if device is not None else "cuda")
    if out is None:
        out = torch.empty(B, C, 2, dtype=torch.int64, device=dev)
    else:
        _pinned_or_cuda(out, "frame_metrics_u8(out=)")
        if out.dtype != torch.int64 or tuple(out.shape) != (B, C, 2) or not out.is_contiguous():
            raise ValueError("frame_metrics_u8: out must be a contiguous int64 [B,C,2] tensor")
    with torch.cuda.device(dev):
        need = load().emavfi_frame_metrics_workspace_bytes(B, H, W, C)
        ws = workspace(need, dev)
        check(load().emavfi_frame_metrics_u8(ap, apitch, abs_, bp, bpitch, bbs, B, H, W, C, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "emavfi_frame_metrics_u8")
    return out


def psnr(sse, n) -> float:
    """10 log10(255^2 n / sse) over n samples; inf for sse == 0.  Pure host arithmetic."""
    import math
    sse, n = int(sse), int(n)
    if sse < 0 or n < 1:
        raise ValueError("psnr: sse >= 0 and n >= 1 expected")
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 * 255.0 * n / sse)


def ssim(ssimq, H, W) -> float:
    """ssimq / (2^32 windows) with windows = (H - 10)(W - 10); nan where H or W is below 11 (no window).  Pure host arithmetic."""
    import math
    n = max(int(H) - METRICS_WINDOW + 1, 0) * max(int(W) - METRICS_WINDOW + 1, 0)
    return math.nan if n == 0 else int(ssimq) / (4294967296.0 * n)
