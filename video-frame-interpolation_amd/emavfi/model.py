"""Drop-in mirror of the reference model API (reference ``src/models/ema_vfi.py``).

Same names, constructor arguments, parameter names / shapes (so reference
checkpoints load with ``strict=True``) and call signatures as the reference:

* ``conv`` / ``conv_block``                      (ema_vfi.py:7-14)
* ``ModulatedDeformConvPack``                     (ema_vfi.py:23-60)
* ``EMA_VFI(in_channels=3, mid_channels=64, num_blocks=3)`` with
  ``forward(frame1, frame2)`` and ``warp(frame2, feature, flow)``  (ema_vfi.py:63-171)

The modules below only HOLD parameters (``nn.Conv2d`` gives the reference's
initialisation and state_dict keys for free); every operator of the model's
arithmetic executes in ``libemavfi.so``.  What torch still does around a call:
contiguity / dtype normalisation of the inputs (no-ops for the fp32 contiguous
frames the reference passes) and, under ``amp16`` only, the final cast of the
fp32-stored, fp16-valued frame to an fp16 tensor.  Inference only.  There is no CPU or
PyTorch fallback: CPU tensors or a missing library raise ``RuntimeError``.
"""
from __future__ import annotations

import hashlib
import math
import os
import tempfile
from collections import OrderedDict
import ctypes
from ctypes import POINTER, c_void_p, cast
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import lib as _lib

# EMA_VFI.pack_policy ("Pack policy").  No census-driven "auto" policy value: the window-free kernel does not beat the
# window at +-8 px (profiles/r07_gather_route_kill.md); the census-driven choice is EMA_VFI.pack_adapt, which starts from pack_policy
PACK_POLICIES = ("window", "gather")
# EMA_VFI.pack_adapt's (enter, leave) fix-up shares for EMAVFI_PACK_ADAPT=1: the crossover measured for one block at B = 8 x 720p
# (profiles/r07_gather_route_kill.md) plus hysteresis
PACK_ADAPT_DEFAULT = (0.75, 0.65)
# EMA_VFI.ensemble ("Ensembling"; include/emavfi.h, "ENSEMBLE DEFINITION")
ENSEMBLES = _lib.ENSEMBLES
_MODEL_ENSEMBLE = object()   # forward(ensemble=): "what the model's attribute says"
# EMA_VFI.border ("Frame borders"; include/emavfi.h, "BORDER DEFINITION")
BORDER_MODES, BORDER_MAX = _lib.BORDER_MODES, _lib.BORDER_MAX
_MODEL_BORDER = object()     # forward(border=): "what the model's attribute says"
# EMA_VFI.agreement ("Agreement guard"; include/emavfi.h, "AGREEMENT GUARD DEFINITION")
_MODEL_AGREEMENT = object()  # forward(agreement=): "what the model's attribute says"
# EMA_VFI.flow_scale ("Flow scale"; include/emavfi.h, "COARSE FLOW DEFINITION")
FLOW_SCALES = _lib.FLOW_SCALES
_MODEL_FLOW_SCALE = object() # forward(flow_scale=): "what the model's attribute says"
# EMA_VFI.align ("Global motion"; include/emavfi.h, "ALIGN DEFINITION")
_MODEL_ALIGN = object()      # forward(align=): "what the model's attribute says"


class _LastCall(NamedTuple):
    """The last one-sequence forward of an EMA_VFI: what pack_census() / pack_routes() read back."""
    device: torch.device
    stream: int                  # the HIP stream handle it ran on
    B: int
    H: int
    W: int
    dtype: int
    ws_bytes: int
    ws_ptr: int                  # its workspace (the census lives there)
    gather_mask: Optional[int]   # emavfi_forward_routed's mask, or None: an adaptive forward (the routes are in the route state)


def parse_pack_adapt(value):
    """EMA_VFI.pack_adapt from a value or the EMAVFI_PACK_ADAPT string: None / "" / "0" = off, "1" = PACK_ADAPT_DEFAULT,
    "enter,leave" or an (enter, leave) pair = those thresholds; 0 <= leave < enter <= 1, else ValueError."""
    if value is None:
        return None
    if isinstance(value, str):
        v = value.strip()
        if v in ("", "0"):
            return None
        if v == "1":
            return PACK_ADAPT_DEFAULT
        parts = v.split(",")
        if len(parts) != 2:
            raise ValueError(f"EMAVFI_PACK_ADAPT must be 1 or 'enter,leave', got {value!r}")
        try:
            value = (float(parts[0]), float(parts[1]))
        except ValueError:
            raise ValueError(f"EMAVFI_PACK_ADAPT must be 1 or 'enter,leave', got {value!r}") from None
    try:
        enter, leave = (float(x) for x in value)
    except (TypeError, ValueError):
        raise ValueError(f"EMA_VFI.pack_adapt must be None or an (enter, leave) pair, got {value!r}") from None
    if not (0.0 <= leave < enter <= 1.0):
        raise ValueError(f"EMA_VFI.pack_adapt needs 0 <= leave < enter <= 1, got enter {enter}, leave {leave}")
    return (enter, leave)


def conv(in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True,
         padding_mode='zeros'):
    """Same signature as the reference helper (ema_vfi.py:7-8)."""
    return nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode)


def conv_block(in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True,
               padding_mode='zeros', act=None):
    """Same signature as the reference helper (ema_vfi.py:10-14): Sequential(conv, act)."""
    return nn.Sequential(
        conv(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation,
             groups=groups, bias=bias, padding_mode=padding_mode),
        act if act is not None else nn.ReLU())


class DeformConv2d(nn.Module):
    """Parameter holder with ``torchvision.ops.DeformConv2d``'s constructor and
    initialisation (the class the reference imports at ema_vfi.py:18);
    ``forward(x, offset, mask)`` runs the HIP kernel."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True):
        super().__init__()
        if (kernel_size, stride, padding, dilation, groups) != (3, 1, 1, 1, 1):
            raise NotImplementedError("emavfi DeformConv2d: only the reference's configuration "
                                      "(3x3, stride 1, padding 1, dilation 1, groups 1) is built")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(in_channels * 9)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, offset, mask=None, dtype="fp32"):
        if mask is None:
            mask = torch.ones(x.shape[0], 9, x.shape[2], x.shape[3], device=x.device, dtype=x.dtype)
        return _lib.deform_conv2d(x, offset, mask, self.weight, self.bias, dtype=dtype).to(x.dtype)


class ModulatedDeformConvPack(nn.Module):
    """Mirror of ema_vfi.py:23-60 (note the reference ignores ``out_channels``, :27)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = in_channels
        self.kernel_size, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.groups, self.bias = groups, bias
        self.offset_conv = nn.Conv2d(self.in_channels, self.groups * 3 * kernel_size * kernel_size,
                                     kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, bias=True)
        nn.init.constant_(self.offset_conv.weight, 0.)
        nn.init.constant_(self.offset_conv.bias, 0.)
        self.dcn_v2 = DeformConv2d(self.in_channels, self.out_channels, kernel_size=kernel_size, stride=stride,
                                   padding=padding, dilation=dilation, bias=bias)

    def forward(self, x, dtype="fp32", flags=0):
        """ema_vfi.py:53-60 through the stage-level entry emavfi_mdcn: offset_conv, the chunk / cat / sigmoid routing and dcn_v2 run
        exactly as one attention block of EMA_VFI.forward does (16-bit modes at 67 channels: ONE kernel launch)."""
        return _lib.mdcn(x, self.offset_conv.weight, self.offset_conv.bias, self.dcn_v2.weight, self.dcn_v2.bias, dtype=dtype,
                         flags=flags).to(x.dtype)


class EMA_VFI(nn.Module):
    """MI355X-native EMA-VFI.  ``compute_dtype``:

    * ``"fp32"``  parity mode: exact-fp32 MFMA, <= 1e-3 max-abs vs the reference CPU forward;
    * ``"bf16"``  bf16 convolutions and tensors, fp32 warp / offsets / accumulation (BASELINE.json configs[2]);
    * ``"fp16"``  the same data flow in IEEE half, deformable convolution included - the FAST half mode;
    * ``"amp16"`` the reference's forward under ``torch.cuda.amp.autocast()`` (inference.py:159) with the autocast op
      policy restated: fp16 Conv2d / Linear (weight and bias cast too), but ``grid_sample`` and torchvision's
      ``deform_conv2d`` in fp32 on an fp32 fusion tensor with the fp32 master weights, fp16 roundings after
      sigmoid / tanh / ``(t + 1) / 2``; returns an fp16 tensor as the reference does there;
    * ``None``    fp32, unless autocast is active: ``torch.autocast("cuda", torch.float16)`` (the reference's own
      ``torch.cuda.amp.autocast()``) selects ``"amp16"``, ``torch.autocast("cuda", torch.bfloat16)`` selects ``"bf16"``."""

    def __init__(self, in_channels=3, mid_channels=64, num_blocks=3, compute_dtype=None):
        super().__init__()
        self.in_channels = in_channels
        self.mid_channels = mid_channels
        self.num_blocks = num_blocks
        self.deformable_groups = 8  # present but unused in the reference too (ema_vfi.py:70)
        self.compute_dtype = compute_dtype if compute_dtype is not None else os.environ.get("EMAVFI_DTYPE")
        # pieces of a batch pipelined over two streams (forward(): _forward_pipelined); 1 = the whole batch as one sequence of launches
        self.pipeline = int(os.environ.get("EMAVFI_PIPELINE", "1"))
        # which stage event of piece k releases piece k + 1: 0 = its front (default), 1 = its attention blocks, -1 = none (pieces start together)
        self.pipeline_stagger = int(os.environ.get("EMAVFI_PIPELINE_STAGGER", "0"))
        # route of the 16-bit attention blocks (include/emavfi.h, emavfi_forward_routed): "window" (default) or "gather"; with
        # pack_adapt set, the starting route of the census-driven choice (emavfi_forward_adaptive)
        self._route_states = {}   # (device index, stream handle) -> route state (include/emavfi.h), created by the first adaptive forward
        self.pack_policy = os.environ.get("EMAVFI_PACK_POLICY", "window")
        self.pack_adapt = os.environ.get("EMAVFI_PACK_ADAPT")
        self.ensemble = None
        self.border = None
        self.agreement = None
        self.flow_scale = None
        self.align = None
        self.align_shifts = None       # the last aligned forward's records {dy, dx, m(d*), m(0)} per sample: int32 [B, 4] on the device
        self.agreement_counts = None   # the last guarded forward's held pixels per sample: int32 [B] on the device
        m = mid_channels
        self.feat_ext_conv1 = conv_block(in_channels * 2, m)
        self.feat_ext_blocks = nn.Sequential(OrderedDict(
            [(f'conv_block_{i}', conv_block(m, m)) for i in range(num_blocks)]))
        self.context_encoding = nn.Sequential(
            conv_block(m, m * 2, stride=2), conv_block(m * 2, m * 4, stride=2), conv_block(m * 4, m * 4),
            nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(m * 4, m))
        self.motion_estimation = nn.Sequential(conv_block(m * 2, m), conv_block(m, m), conv(m, 2))
        self.attention_blocks = nn.ModuleList(
            [ModulatedDeformConvPack(m + 3, m + 3, kernel_size=3, padding=1, groups=1) for _ in range(num_blocks)])
        self.reconstruction = nn.Sequential(conv_block(m + 3, m), conv_block(m, m // 2), conv(m // 2, in_channels), nn.Tanh())
        self._packed = {}      # dtype code -> (key, packed uint8 tensor)
        self._installed = {}   # dtype code -> parameter versions when load_packed_weights() installed the blob
        self._params_loaded = True   # False once a foreign blob is installed and no state_dict has been loaded since

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """``nn.Module.load_state_dict`` plus the checkpoint shapes met in practice for this model
        (SURVEY.md section 8f row 4): a ``{"state_dict": ...}`` / ``{"model": ...}`` wrapper, keys saved
        from ``nn.DataParallel`` (``module.`` prefix), half-precision tensors (cast to fp32, the dtype
        ``train.py:182,190`` saves).  Shapes are verified against the reference's parameter table and a
        mismatch raises with the offending key."""
        sd = state_dict
        for wrapper in ("state_dict", "model", "model_state_dict"):
            if isinstance(sd, dict) and wrapper in sd and isinstance(sd[wrapper], dict) and \
                    all(isinstance(k, str) for k in sd[wrapper]):
                sd = sd[wrapper]
                break
        clean = OrderedDict()
        for k, v in sd.items():
            k2 = k[len("module."):] if k.startswith("module.") else k
            clean[k2] = v.float() if torch.is_tensor(v) and v.is_floating_point() and v.dtype != torch.float32 else v
        own = dict(self.named_parameters())
        for k, v in clean.items():
            if k in own and torch.is_tensor(v) and tuple(v.shape) != tuple(own[k].shape):
                raise RuntimeError(f"EMA_VFI.load_state_dict: {k} has shape {tuple(v.shape)}, "
                                   f"expected {tuple(own[k].shape)} for EMA_VFI({self.in_channels}, "
                                   f"{self.mid_channels}, {self.num_blocks})")
        res = super().load_state_dict(clean, strict=strict, assign=assign)
        self._installed.clear()          # the parameters are authoritative again: blobs re-pack from them
        self._packed.clear()
        self._params_loaded = True
        self._reset_route_states()       # the census they hold described other offsets
        return res

    def _ordered_params(self):
        """Tensors in the order emavfi_pack_weights expects = the reference's registration order."""
        return [p for _, p in self.named_parameters()]

    def _weights_key(self, device):
        return (str(device), _lib.layout_switches()) + tuple((p.data_ptr(), p._version) for p in self._ordered_params())

    def _versions(self):
        return tuple(p._version for p in self._ordered_params())

    def packed_weights(self, dt: int, device):
        """Packed blob for this dtype, re-packed lazily after load_state_dict / .to() / in-place edits."""
        inst = self._installed.get(dt)
        if inst is not None:
            # a blob installed by load_packed_weights() (another rank's weights): it stays in force across .to() /
            # device moves; this rank's nn.Parameters are NOT its source, so an in-place edit cannot be honoured
            if inst != self._versions():
                raise RuntimeError("EMA_VFI: parameters were modified in place, but this model runs on packed weights "
                                   "installed by load_packed_weights() and never loaded a state_dict - call "
                                   "load_state_dict() (then the blob is re-packed from the parameters)")
            blob = self._packed[dt][1]
            if blob.device != torch.device(device):
                blob = blob.to(device)
                self._packed[dt] = (None, blob)
            return blob
        if not self._params_loaded:
            raise RuntimeError(f"EMA_VFI: no packed weights for dtype code {dt}: this model received its weights through "
                               "load_packed_weights() for another dtype and its nn.Parameters were never loaded")
        key = self._weights_key(device)
        hit = self._packed.get(dt)
        if hit is not None and hit[0] == key:
            return hit[1]
        L = _lib.load()
        nbytes = L.emavfi_packed_bytes(self.in_channels, self.mid_channels, self.num_blocks, dt)
        if nbytes == 0:
            raise RuntimeError(f"EMA_VFI: {_lib.last_error()}")
        params = [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in self._ordered_params()]
        n = L.emavfi_param_count(self.num_blocks)
        if len(params) != n:
            raise RuntimeError(f"EMA_VFI: expected {n} parameter tensors, module has {len(params)}")
        # on-disk cache keyed by CONTENT (the reference reloads and re-prepares its checkpoint at every
        # process start, inference.py:69): state_dict bytes + dtype + model shape + the library build
        path = self._cache_path(params, dt, nbytes)
        blob = self._cache_read(path, nbytes, device)
        if blob is not None:
            try:   # the header says what the file IS (version, model, dtype, layout tag, checksum): a foreign file is re-packed, never run
                _lib.packed_check(self.in_channels, self.mid_channels, self.num_blocks, dt, blob)
            except RuntimeError:
                blob = None
        if blob is None:
            blob = torch.empty(nbytes, dtype=torch.uint8, device=device)
            arr = (c_void_p * n)(*[p.data_ptr() for p in params])
            with torch.cuda.device(device):
                _lib.check(L.emavfi_pack_weights(self.in_channels, self.mid_channels, self.num_blocks,
                                                 cast(arr, POINTER(c_void_p)), n, blob.data_ptr(), nbytes, dt, _lib._stream()),
                           "emavfi_pack_weights")
            self._cache_write(path, blob)
        self._packed[dt] = (key, blob)
        return blob

    # ------------------------------------------------------------------ packed-weight cache on disk
    @staticmethod
    def cache_dir():
        """Directory of the packed-weight cache, or None when disabled (EMAVFI_CACHE=0)."""
        if os.environ.get("EMAVFI_CACHE", "1") == "0":
            return None
        return os.environ.get("EMAVFI_CACHE_DIR") or os.path.join(
            os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "emavfi")

    def _cache_path(self, params, dt, nbytes):
        d = self.cache_dir()
        if d is None:
            return None
        h = hashlib.sha256()
        h.update(f"{_lib.fingerprint()}|{_lib.layout_switches()}|{dt}|{self.in_channels}|{self.mid_channels}|{self.num_blocks}|{nbytes}".encode())
        for name, p in zip((k for k, _ in self.named_parameters()), params):
            h.update(name.encode())
            h.update(p.cpu().numpy().tobytes())
        return os.path.join(d, f"packed_{h.hexdigest()[:32]}.bin")

    @staticmethod
    def _cache_read(path, nbytes, device):
        """The file is the blob followed by the sha256 of the blob: a truncated, foreign or bit-rotten file is ignored (and
        overwritten by the re-pack), never run."""
        if path is None or not os.path.isfile(path) or os.path.getsize(path) != nbytes + 32:
            return None
        try:
            import numpy as np
            raw = np.fromfile(path, dtype=np.uint8)
        except OSError:
            return None
        if raw.size != nbytes + 32 or hashlib.sha256(raw[:nbytes].tobytes()).digest() != raw[nbytes:].tobytes():
            return None
        return torch.from_numpy(raw[:nbytes].copy()).to(device)

    @staticmethod
    def _cache_write(path, blob):
        if path is None:
            return
        try:  # best effort: a read-only or full cache directory must never fail a forward
            os.makedirs(os.path.dirname(path), exist_ok=True)
            fd, tmp = tempfile.mkstemp(dir=os.path.dirname(path), suffix=".tmp")
            data = blob.cpu().numpy().tobytes()
            with os.fdopen(fd, "wb") as f:
                f.write(data)
                f.write(hashlib.sha256(data).digest())
            os.replace(tmp, path)  # atomic: concurrent ranks write identical bytes
        except OSError:
            pass

    def load_packed_weights(self, dt, blob, params_are_source=False):
        """Install an already-packed blob (e.g. received by an RCCL broadcast from rank 0).  The blob is pinned: it is
        used as is until load_state_dict() is called.  ``params_are_source=True`` (the broadcasting rank, whose own
        parameters produced the blob) keeps the normal re-pack-on-change behaviour."""
        dt = _lib.dtype_code(dt)
        nbytes = _lib.load().emavfi_packed_bytes(self.in_channels, self.mid_channels, self.num_blocks, dt)
        if blob.dtype != torch.uint8 or blob.numel() != nbytes:
            raise ValueError(f"load_packed_weights: a uint8 blob of {nbytes} bytes is expected for this model / dtype")
        # the blob's header must say this model, this dtype, this library version and this process's layout switches
        _lib.packed_check(self.in_channels, self.mid_channels, self.num_blocks, dt, blob)
        self._reset_route_states()
        if params_are_source:
            self._packed[dt] = (self._weights_key(blob.device), blob)
            return
        self._packed[dt] = (None, blob)
        self._installed[dt] = self._versions()
        self._params_loaded = False

    def _resolve_dtype(self) -> int:
        if self.compute_dtype is not None:
            return _lib.dtype_code(self.compute_dtype)
        if not torch.is_autocast_enabled():
            return _lib.F32
        get = getattr(torch, "get_autocast_dtype", None)
        auto = get("cuda") if get is not None else torch.get_autocast_gpu_dtype()
        return _lib.BF16 if auto == torch.bfloat16 else _lib.AMP16

    # ------------------------------------------------------------------ pack route
    @property
    def pack_policy(self):
        """Which kernel runs the one-launch ModulatedDeformConvPack of each 16-bit attention block ("Pack policy"):
        "window" (default) deform_pack3_kernel everywhere - the launches and frames of every earlier version; "gather" the window-free
        kernel on every block (flat in the offsets, faster beyond about +-10 px; raises, with the library's error text, in modes
        without a one-launch pack: fp32, amp16, fp32x3).  Initial value: EMAVFI_PACK_POLICY."""
        return self._pack_policy

    @pack_policy.setter
    def pack_policy(self, value):
        if value not in PACK_POLICIES:
            raise ValueError(f"EMA_VFI.pack_policy must be one of {PACK_POLICIES}, got {value!r}")
        changed = getattr(self, "_pack_policy", value) != value
        self._pack_policy = value
        if changed:
            self._reset_route_states()   # the starting route of the adaptive choice

    @property
    def pack_adapt(self):
        """Census-driven route per 16-bit attention block ("Pack policy"; include/emavfi.h, emavfi_forward_adaptive):
        None (default: pack_policy decides alone) or the (enter, leave) fix-up shares of the hysteresis - a block on the window route
        moves to the gather route in the next forward when its share reaches `enter`, and back when it falls to `leave`.  The choice is
        made on the device from every forward's census (no host sync; a captured graph adapts on replay); pack_policy is the starting
        route.  Modes without a one-launch pack (fp32, amp16, fp32x3) run their plain forward.  A batch runs as one sequence
        (pipeline is ignored).  Initial value: EMAVFI_PACK_ADAPT (1 = PACK_ADAPT_DEFAULT, or "enter,leave").  Changing the thresholds
        keeps the route state; load_state_dict, load_packed_weights and a new pack_policy reset it to the starting route.  Every forward
        advances the state, so the members of an ensemble may run different routes: the exact symmetries of `ensemble` and of the
        `agreement` guard (guard(a, b) == guard(b, a), flip equivariance) hold for a fixed route only, that is with pack_adapt unset."""
        return self._pack_adapt

    @pack_adapt.setter
    def pack_adapt(self, value):
        self._pack_adapt = parse_pack_adapt(value)

    @property
    def ensemble(self):
        """Test-time ensembling of forward() ("Ensembling"; include/emavfi.h, "ENSEMBLE DEFINITION"): None (default: the
        plain forward, every launch and byte as without the attribute), "reverse" (the pair and the reversed pair: 2 forwards, exactly
        symmetric in time), "flip" (the pair under the four mirrorings: 4 forwards, exactly equivariant under flips) or "full" (both: 8
        forwards).  The members are plain forwards of the same batch; the mirrored inputs and the tree mean run on the device
        (emavfi_flip_f32, emavfi_ensemble_mean_f32); no host synchronisation is added."""
        return self._ensemble

    @ensemble.setter
    def ensemble(self, value):
        self._ensemble = self._check_ensemble(value)

    @staticmethod
    def _check_ensemble(value):
        if value is not None and (not isinstance(value, str) or value not in ENSEMBLES):
            raise ValueError(f"EMA_VFI.ensemble must be one of {ENSEMBLES}, got {value!r}")
        return value

    @property
    def border(self):
        """Frames extended past their edges for forward() ("Frame borders"; include/emavfi.h, "BORDER DEFINITION"): None
        (default: the plain forward, every launch and byte as without the attribute), an int N in 1..64 (N pixels of replicated edge on
        each side) or (N, "replicate" | "reflect"); read back as None or the pair (N, mode).  Both inputs are padded on the device
        (emavfi_border_pad_f32), the plain or ensembled forward runs on the (H + 2N) x (W + 2N) batch, and the fp32 result is cropped
        (emavfi_border_crop_f32) before it is converted; no host synchronisation is added."""
        return self._border

    @border.setter
    def border(self, value):
        self._border = self._check_border(value)

    @staticmethod
    def _check_border(value):
        """None or (N, mode name) of a border given as None, N or (N, mode)"""
        if value is None:
            return None
        N, mode = value if isinstance(value, tuple) and len(value) == 2 else (value, BORDER_MODES[0])
        if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= BORDER_MAX or not isinstance(mode, str) or mode not in BORDER_MODES:
            raise ValueError(f"EMA_VFI.border must be None, an int N in 1..{BORDER_MAX} or (N, mode) with mode one of {BORDER_MODES}, got {value!r}")
        return N, mode

    @property
    def agreement(self):
        """The agreement guard of forward() ("Agreement guard"; include/emavfi.h, "AGREEMENT GUARD DEFINITION"): None
        (default: off), a tolerance `tol` in [0, 1] of the output's full scale, or (tol, radius) with the radius of the dilation in 0..16;
        read back as None or the pair (tol, radius).  Needs both time directions: the call's ensemble must be "reverse" or "full", anything
        else is refused, never upgraded.  Where the time-forward and the time-reversed half of the ensemble differ by more than `tol` in any
        channel, within `radius` pixels, the blend of the two source frames is emitted instead of the ensemble's mean; one launch
        (emavfi_agreement_guard_f32) in place of the ensemble's last mean.  The held pixels per sample of the last guarded forward stay on
        the device as `agreement_counts` (int32 [B]); no host synchronisation is added."""
        return self._agreement

    @agreement.setter
    def agreement(self, value):
        self._agreement = self._check_agreement(value)

    @staticmethod
    def _check_agreement(value):
        """None or (tol, radius) of a guard given as None, tol or (tol, radius)"""
        if value is None:
            return None
        tol, radius = value if isinstance(value, tuple) and len(value) == 2 else (value, 0)
        try:
            return _lib.agreement_args(tol, radius, "EMA_VFI.agreement")
        except ValueError:
            raise ValueError(f"EMA_VFI.agreement must be None, a tolerance in [0, 1] or (tolerance, radius) with an int radius in "
                             f"0..{_lib.STATIC_MAX_RADIUS}, got {value!r}") from None

    @property
    def flow_scale(self):
        """The scale at which forward() estimates the flow ("Flow scale"; include/emavfi.h, "COARSE FLOW DEFINITION"):
        None (default: the plain forward, every launch and byte as without the attribute) or s in (2, 4, 8).  Both inputs are reduced
        by s on the device (emavfi_downscale_f32), the front of the forward runs on the reduced pair up to its flow
        (emavfi_forward_flow), the flow is brought back to full size and multiplied by s (emavfi_upsample_flow_f32), and the full-size
        forward runs with it (emavfi_forward_given_flow), without context encoding and motion estimation.  The output keeps its size;
        what changes is how far the motion may reach: about 7 s pixels instead of 7.  Every F of an ensemble, of a bordered forward and
        of the agreement guard becomes this F_s.  A batch runs as one sequence (pipeline is ignored); pack_policy applies to the
        full-size forward; pack_adapt and return_taps are refused.  No host synchronisation is added."""
        return self._flow_scale

    @flow_scale.setter
    def flow_scale(self, value):
        self._flow_scale = self._check_flow_scale(value)

    @staticmethod
    def _check_flow_scale(value):
        if value is not None and (isinstance(value, bool) or not isinstance(value, int) or value not in FLOW_SCALES):
            raise ValueError(f"EMA_VFI.flow_scale must be None or one of {FLOW_SCALES}, got {value!r}")
        return value

    @property
    def align(self):
        """Global motion compensated before forward() ("Global motion"; include/emavfi.h, "ALIGN DEFINITION"): None
        (default: the plain forward, every launch and byte as without the attribute) or (R_px, ratio): the search radius in pixels, a
        multiple of 4 in 4..128, and the acceptance ratio in [0, 1] (taken as round(ratio * 1024)); there is no one-argument form and no
        default.  One translation per pair, a multiple of 4 pixels per axis, is found on the device from 4 x 4 cell sums of both frames
        (emavfi_align_signature_f32, emavfi_align_search); both frames are moved by half of it into the midpoint's coordinates
        (emavfi_shift_f32), and whatever forward would otherwise run - plain, ensembled, bordered, coarse, guarded - runs on the moved
        pair.  The records {dy, dx, m(d*), m(0)} of the last aligned forward stay on the device as `align_shifts` (int32 [B, 4]); no
        host synchronisation is added."""
        return self._align

    @align.setter
    def align(self, value):
        self._align = self._check_align(value)

    @staticmethod
    def _check_align(value):
        """None or (R_px, ratio) of an alignment given as None or (R_px, ratio)"""
        if value is None:
            return None
        try:
            if not isinstance(value, tuple) or len(value) != 2:
                raise ValueError
            _lib.align_args(value[0], value[1], "EMA_VFI.align")
        except ValueError:
            raise ValueError(f"EMA_VFI.align must be None or (R_px, ratio) with R_px an int multiple of {_lib.ALIGN_CELL} in "
                             f"{_lib.ALIGN_CELL}..{_lib.ALIGN_CELL * _lib.ALIGN_MAX_RADIUS} and ratio a number in [0, 1], got {value!r}") from None
        return value[0], float(value[1])

    def _check_border_size(self, B, H, W, border, dt):
        """(H + 2N, W + 2N), or a refusal from the shapes alone where the padded batch is beyond what the forward admits (include/emavfi.h,
        SIZE LIMITS: B*H*W < 2^31, H*W < 2^24, the fusion plane < 4 GiB) - before anything is launched"""
        N, mode = border
        Hp, Wp = H + 2 * N, W + 2 * N
        fpad = (self.mid_channels + 3 + 15) // 16 * 16
        widest = 2 if dt in (_lib.BF16, _lib.F16) else 4
        why = (f"a dimension is above {_lib.RESIZE_MAX_DIM}" if max(Hp, Wp) > _lib.RESIZE_MAX_DIM else
               "H*W must be < 2^24" if Hp * Wp >= 1 << 24 else
               "B*H*W must be < 2^31" if B * Hp * Wp >= 1 << 31 else
               "one sample's activation plane must be < 4 GiB" if Hp * Wp * fpad * widest >= 1 << 32 else None)
        if why is not None:
            raise ValueError(f"EMA_VFI.forward: border ({N}, {mode!r}) extends the {H} x {W} frames to {Hp} x {Wp}, beyond the forward's "
                             f"size limits ({why})")
        return Hp, Wp

    def _start_mask(self):
        return (1 << self.num_blocks) - 1 if self._pack_policy == "gather" else 0

    def _reset_route_states(self):
        """Every route state back to the starting route, in place (a captured graph keeps the state's address), on its own stream."""
        L = None
        for (dev_index, stream), st in self._route_states.items():
            L = L or _lib.load()
            with torch.cuda.device(dev_index):
                _lib.check(L.emavfi_route_state_init(st.data_ptr(), self.num_blocks, self._start_mask(), c_void_p(stream)),
                           "emavfi_route_state_init")

    def _route_state(self, dev):
        """The route state of the current stream of `dev`, created (and initialised on that stream) by its first adaptive forward."""
        stream = torch.cuda.current_stream(dev).cuda_stream
        key = (dev.index, stream)
        st = self._route_states.get(key)
        if st is None:
            if torch.cuda.is_current_stream_capturing():
                # created inside a capture, its initialisation would be part of every replay
                raise RuntimeError("EMA_VFI: no route state for the capturing stream yet; run one adaptive forward on that stream "
                                   "(a warm-up) before capturing")
            L = _lib.load()
            st = torch.empty(L.emavfi_route_state_bytes() // 4, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L.emavfi_route_state_init(st.data_ptr(), self.num_blocks, self._start_mask(), _lib._stream()),
                           "emavfi_route_state_init")
            self._route_states[key] = st
        return st

    def pack_routes(self):
        """The adaptive route of every attention block on the current stream (pack_adapt): per block a dict {ran, next, fixup_share,
        switches} - the route ("window" | "gather") of the last adaptive forward, the route of the next one, the fix-up share that
        forward measured and the route changes since the state was (re)set - or None for a block without a routed pack (fp32 / autocast
        modes, other widths).  One blocking D2H copy."""
        last = getattr(self, "_last_call", None)
        if last is None or last.gather_mask is not None:
            raise RuntimeError("EMA_VFI.pack_routes: no adaptive one-sequence forward has run yet")
        if torch.cuda.current_stream(last.device).cuda_stream != last.stream:
            raise RuntimeError("EMA_VFI.pack_routes: call it on the stream the forward ran on")
        routed = any(n.startswith("deform_routed") for n, _, _ in
                     _lib.forward_launches(self.in_channels, self.mid_channels, self.num_blocks, last.B, last.H, last.W, last.dtype, adaptive=True))
        if not routed:
            return [None] * self.num_blocks
        w = self._route_states[(last.device.index, last.stream)].cpu()
        ran, share, sw = int(w[3]), w[16:24].view(torch.float32), w[24:32]
        name = ("window", "gather")
        return [{"ran": name[(ran >> i) & 1], "next": name[int(w[8 + i]) & 1], "fixup_share": float(share[i]), "switches": int(sw[i])}
                for i in range(self.num_blocks)]

    # ------------------------------------------------------------------ forward
    def forward(self, frame1, frame2, return_taps=False, _events=None, ensemble=_MODEL_ENSEMBLE, border=_MODEL_BORDER,
                agreement=_MODEL_AGREEMENT, flow_scale=_MODEL_FLOW_SCALE, align=_MODEL_ALIGN):
        """ema_vfi.py:110-147.  `ensemble`: one of ENSEMBLES for this call alone (FrameInterpolator passes its own); by default the
        model's attribute decides.  `border`: None, N or (N, mode) for this call alone, likewise.  `agreement`: None, tol or
        (tol, radius) for this call alone, likewise.  `flow_scale`: None, 2, 4 or 8 for this call alone, likewise.  `align`: None or
        (R_px, ratio) for this call alone, likewise."""
        ensemble = self._ensemble if ensemble is _MODEL_ENSEMBLE else self._check_ensemble(ensemble)
        border = self._border if border is _MODEL_BORDER else self._check_border(border)
        agreement = self._agreement if agreement is _MODEL_AGREEMENT else self._check_agreement(agreement)
        fs = self._flow_scale if flow_scale is _MODEL_FLOW_SCALE else self._check_flow_scale(flow_scale)
        align = self._align if align is _MODEL_ALIGN else self._check_align(align)
        if align is not None and return_taps:
            raise ValueError("EMA_VFI.forward: return_taps=True with align: the taps belong to the forward of the moved pair (set align=None)")
        if fs is not None and return_taps:
            raise ValueError("EMA_VFI.forward: return_taps=True with a flow scale: ctx and flow belong to the reduced forward, the rest to "
                             "the full-size one (set flow_scale=None, or call lib.forward_flow / lib.forward_given_flow)")
        if fs is not None and self._pack_adapt is not None:
            raise ValueError("EMA_VFI.forward: flow_scale with pack_adapt: the adaptive route has no given-flow form (unset one of them)")
        if agreement is not None and return_taps:
            raise ValueError("EMA_VFI.forward: return_taps=True with an agreement guard: the taps belong to one forward (set agreement=None)")
        if agreement is not None and ensemble not in _lib.AGREEMENT_ENSEMBLES:
            raise ValueError(f"EMA_VFI.forward: agreement={agreement!r} with ensemble={ensemble!r}: the guard compares the two time directions "
                             f"and needs an ensemble that runs both, one of {_lib.AGREEMENT_ENSEMBLES} (it is not chosen for you)")
        if border is not None and return_taps:
            raise ValueError("EMA_VFI.forward: return_taps=True with a border: the taps belong to the padded forward (set border=None)")
        if ensemble is not None and return_taps:
            raise ValueError("EMA_VFI.forward: return_taps=True with an ensemble: the taps belong to one forward (set ensemble=None)")
        if frame1.shape != frame2.shape or frame1.dim() != 4 or frame1.shape[1] != self.in_channels:
            raise ValueError(f"EMA_VFI.forward: two [B,{self.in_channels},H,W] tensors expected, got "
                             f"{tuple(frame1.shape)} and {tuple(frame2.shape)}")
        if frame1.device != frame2.device:
            raise ValueError("EMA_VFI.forward: frame1 and frame2 are on different devices")
        if align is not None and not (min(frame1.shape[2:]) >= 8 and _lib.align_fits(align[0] // _lib.ALIGN_CELL, *frame1.shape[2:])):
            raise ValueError(f"EMA_VFI.forward: align={align!r}: a radius of {align[0]} pixels needs frames of at least {2 * align[0]} x "
                             f"{2 * align[0]} pixels (2 R_px / 4 <= min(H // 4, W // 4)), got {frame1.shape[2]} x {frame1.shape[3]}")
        if self.in_channels != 3:
            # the reference's fusion width is the literal mid_channels + 3 (ema_vfi.py:97): any other in_channels
            # fails there with a channel mismatch at the first attention block
            raise RuntimeError(f"EMA_VFI: in_channels={self.in_channels} is not runnable (the reference's fusion width "
                               "is mid_channels + 3, ema_vfi.py:97); only in_channels=3 is supported")
        _lib._require_cuda(frame1, frame2)
        if torch.is_grad_enabled() and (frame1.requires_grad or frame2.requires_grad
                                        or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("EMA_VFI (MI355X-native) is inference-only: call it under torch.no_grad() "
                               "as the reference's inference.py:158 does")
        dev, dt = frame1.device, self._resolve_dtype()
        f1, f2 = _lib._f32c(frame1), _lib._f32c(frame2)
        B, C, H, W = f1.shape
        L = _lib.load()
        if border is not None:
            self._check_border_size(B, H, W, border, dt)
        packed = self.packed_weights(dt, dev)
        if align is not None:
            # M(a', b') of the align definition: everything below sees the moved pair, in every role
            f1, f2, self.align_shifts = _lib.align_pair_f32(f1, f2, *align)
        if border is not None:
            # crop_N(G(pad a, pad b)) of the border definition: G sees an ordinary (H + 2N) x (W + 2N) batch
            a, b = f1, f2
            f1, f2 = (_lib.border_pad_f32(f, *border) for f in (f1, f2))
            if agreement is not None:
                # the two halves of the padded ensemble, cropped, then the guard on the picture with the unpadded sources
                u, v = (_lib.border_crop_f32(h, border[0]) for h in self._forward_halves(L, packed, f1, f2, dt, ensemble, _events, fs))
                out = self._agreement_guard(u, v, a, b, agreement)
                return out.half() if dt == _lib.AMP16 else out.to(frame1.dtype)
            if ensemble is not None:
                out = self._forward_ensemble(L, packed, f1, f2, dt, ensemble, _events, fs)
            else:
                out = torch.empty_like(f1)
                self._forward_f32(L, packed, f1, f2, out, dt, None, _events, fs)
            out = _lib.border_crop_f32(out, border[0])
            return out.half() if dt == _lib.AMP16 else out.to(frame1.dtype)
        if agreement is not None:
            u, v = self._forward_halves(L, packed, f1, f2, dt, ensemble, _events, fs)
            out = self._agreement_guard(u, v, f1, f2, agreement)
            return out.half() if dt == _lib.AMP16 else out.to(frame1.dtype)
        if ensemble is not None:
            out = self._forward_ensemble(L, packed, f1, f2, dt, ensemble, _events, fs)
            return out.half() if dt == _lib.AMP16 else out.to(frame1.dtype)
        out = torch.empty_like(f1)
        taps_arg, taps = None, None
        if return_taps:
            m = self.mid_channels
            taps = OrderedDict(feat=torch.empty(B, m, H, W, device=dev), ctx=torch.empty(B, m, device=dev),
                               flow=torch.empty(B, 2, H, W, device=dev), warped=torch.empty(B, C, H, W, device=dev))
            ptrs = [taps["feat"].data_ptr(), taps["ctx"].data_ptr(), taps["flow"].data_ptr(), taps["warped"].data_ptr(), None]
            for i in range(self.num_blocks):
                taps[f"fused_{i}"] = torch.empty(B, m + 3, H, W, device=dev)
                ptrs.append(taps[f"fused_{i}"].data_ptr())
            taps_arg = cast((c_void_p * len(ptrs))(*ptrs), POINTER(c_void_p))
        self._forward_f32(L, packed, f1, f2, out, dt, taps_arg, _events, fs)
        # under autocast the reference's reconstruction tail is fp16, so its frame is an fp16 tensor (the values computed
        # here are fp16-representable: the conversion is exact)
        out = out.half() if dt == _lib.AMP16 else out.to(frame1.dtype)
        if return_taps:
            taps["out"] = out
            return out, taps
        return out

    def _forward_f32(self, L, packed, f1, f2, out, dt, taps_arg=None, _events=None, fs=None):
        """F(f1, f2) of the ensemble definition: the plain forward of two checked fp32 contiguous batches into the fp32 `out`, as one
        sequence of launches or pipelined over two streams.  With a flow scale `fs` it is F_s of the coarse flow definition: its four
        steps on the current stream, one sequence (`_events` bracket the full-size forward's launches)."""
        B, C, H, W = f1.shape
        if fs is not None:
            a_s, b_s = _lib.downscale_f32(f1, fs), _lib.downscale_f32(f2, fs)
            flow_s = _lib.forward_flow(packed, a_s, b_s, self.mid_channels, self.num_blocks, dt)
            flow = _lib.upsample_flow_f32(flow_s, (H, W), fs)
            gmask = (1 << self.num_blocks) - 1 if self._pack_policy == "gather" else 0
            self._last_call = self._launch(L, packed, f1, f2, out, dt, gmask, None, None, _events, flow)
            return
        pieces = min(int(self.pipeline), B)
        if (C * H * W) % 4 != 0:
            pieces = 1   # a slice of the batch must start 16-byte aligned (include/emavfi.h): odd sample sizes run as one sequence
        if self._pack_adapt is not None:
            pieces = 1   # one route state per stream, one census per forward: the adaptive forward runs as one sequence
            gmask = None
        else:
            gmask = (1 << self.num_blocks) - 1 if self._pack_policy == "gather" else 0
        if pieces >= 2 and taps_arg is None and not torch.cuda.is_current_stream_capturing():
            self._forward_pipelined(L, packed, f1, f2, out, dt, pieces, _events, gmask)
        else:
            self._last_call = self._launch(L, packed, f1, f2, out, dt, gmask, taps_arg, None, _events)

    def _forward_ensemble(self, L, packed, f1, f2, dt, ensemble, _events=None, fs=None):
        """The fp32 ensemble of include/emavfi.h, "ENSEMBLE DEFINITION": its members are plain forwards of the same batch, issued in the
        definition's member order (under pack_adapt every one of them advances the route state, as the same calls made by hand would).
        Run one after the other and not as one larger batch: the result is the composition by construction, whatever the kernels do
        across a batch, and eight 720p batches of 8 would not share a workspace anyway.  `_events` bracket the first member's launches."""
        return _lib.ensemble_mean_f32(*self._ensemble_members(L, packed, f1, f2, dt, ensemble, _events, fs))

    def _ensemble_members(self, L, packed, f1, f2, dt, ensemble, _events=None, fs=None):
        """(members, flip codes) of the ensemble, in the definition's order: the plain forwards, each an fp32 tensor of its own"""
        flips = (0,) if ensemble == "reverse" else _lib.ENSEMBLE_FLIPS
        mirrored = {f: (_lib.flip_f32(f1, f), _lib.flip_f32(f2, f)) if f else (f1, f2) for f in flips}
        members, codes = [], []
        for reverse in ((False,) if ensemble == "flip" else (False, True)):
            for f in flips:
                x1, x2 = mirrored[f][::-1] if reverse else mirrored[f]
                m = torch.empty_like(f1)
                self._forward_f32(L, packed, x1, x2, m, dt, None, _events if not members else None, fs)
                members.append(m)
                codes.append(f)
        return members, codes

    def _forward_halves(self, L, packed, f1, f2, dt, ensemble, _events=None, fs=None):
        """(u, v) of the agreement guard definition for ensemble "reverse" or "full": the same members as the ensemble's, in the same
        order, the time-forward half and the time-reversed half each reduced by the definition's tree mean (one member: the member)"""
        members, codes = self._ensemble_members(L, packed, f1, f2, dt, ensemble, _events, fs)
        n = len(members) // 2
        if n == 1:
            return members[0], members[1]
        return _lib.ensemble_mean_f32(members[:n], codes[:n]), _lib.ensemble_mean_f32(members[n:], codes[n:])

    def _agreement_guard(self, u, v, a, b, agreement):
        """the guard's one launch on the fp32 halves and the normalised fp32 sources; the counts stay on the device"""
        self.agreement_counts = torch.empty(u.shape[0], dtype=torch.int32, device=u.device)
        return _lib.agreement_guard_f32(u, v, a, b, agreement[0], agreement[1], counts=self.agreement_counts)

    def pack_census(self):
        """What the one-launch ModulatedDeformConvPack kernels of the LAST one-sequence forward on the current stream counted while
        they ran (include/emavfi.h, emavfi_forward_census): per attention block a dict {fixup_wave_taps, wave_taps, fixup_share,
        samples_outside_window, samples_outside_share, abs_offset_px_max}, or None for a block that ran other kernels (fp32 / autocast
        modes, other widths).  The reference bounds its offsets nowhere (ema_vfi.py:55-60); the kernel's staged window holds offsets up
        to +-2 px beyond the tap and pays for every (4 x 16 pixels, tap) group with a sample outside it.  Every row also says which
        kernel the block ran ("route": "window" | "gather": pack_policy, or under pack_adapt the route the state says ran); both
        count the same thing.  One blocking D2H copy (two under pack_adapt)."""
        last = getattr(self, "_last_call", None)
        if last is None:
            raise RuntimeError("EMA_VFI.pack_census: no one-sequence forward has run yet")
        dev, stream, B, H, W = last.device, last.stream, last.B, last.H, last.W
        if torch.cuda.current_stream(dev).cuda_stream != stream:
            raise RuntimeError("EMA_VFI.pack_census: call it on the stream the forward ran on")
        ws = _lib.workspace(last.ws_bytes, dev)
        if ws.data_ptr() != last.ws_ptr:
            # the stream's workspace was replaced (a larger forward ran since): the counters of that forward are gone
            raise RuntimeError("EMA_VFI.pack_census: the workspace of the last forward has been replaced since; run the forward again")
        out = torch.zeros(self.num_blocks, 4, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().emavfi_forward_census(self.in_channels, self.mid_channels, self.num_blocks, B, H, W, last.dtype, ws.data_ptr(),
                                                         ws.numel(), out.data_ptr(), _lib._stream()), "emavfi_forward_census")
        rows = _lib._census_rows(out, B * H * W * 9)
        gmask = last.gather_mask
        if gmask is None:   # an adaptive forward: the ran mask of this stream's route state
            gmask = int(self._route_states[(dev.index, stream)][3].item())
        for i, row in enumerate(rows):
            if row is not None:
                row["route"] = "gather" if (gmask >> i) & 1 else "window"
        return rows

    def _launch(self, L, packed, f1, f2, out, dt, gather_mask, taps=None, stage=None, _events=None, flow=None):
        """One forward of f1 / f2 into `out` on the current stream of their device: emavfi_forward_routed with `gather_mask`, or
        emavfi_forward_adaptive when it is None (pack_adapt), or - `flow`: a contiguous fp32 [B,2,H,W] tensor -
        emavfi_forward_given_flow with `gather_mask`.  taps / stage: the C-ABI's tap and stage-event pointer arrays or None;
        _events: (hipEvent_t array, count) or None.  Returns the call's _LastCall."""
        B, C, H, W = f1.shape
        dev = f1.device
        state = self._route_state(dev) if gather_mask is None else None
        nws = L.emavfi_workspace_bytes(C, self.mid_channels, self.num_blocks, B, H, W, dt)
        if nws == 0:
            raise RuntimeError(f"EMA_VFI: {_lib.last_error()}")
        ws = _lib.workspace(nws, dev)
        evp, nev = _lib._events_arg(_events)
        args = (C, self.mid_channels, self.num_blocks, packed.data_ptr(), packed.numel(), f1.data_ptr(), f2.data_ptr(), out.data_ptr(),
                ws.data_ptr(), ws.numel(), B, H, W, dt, taps, stage, evp, nev)
        with torch.cuda.device(dev):
            if flow is not None:
                _lib.check(L.emavfi_forward_given_flow(*args[:7], flow.data_ptr(), *args[7:], gather_mask, _lib._stream()),
                           "emavfi_forward_given_flow")
            elif state is not None:
                enter, leave = self._pack_adapt
                _lib.check(L.emavfi_forward_adaptive(*args, state.data_ptr(), enter, leave, _lib._stream()), "emavfi_forward_adaptive")
            else:
                _lib.check(L.emavfi_forward_routed(*args, gather_mask, _lib._stream()), "emavfi_forward_routed")
        return _LastCall(dev, torch.cuda.current_stream(dev).cuda_stream, B, H, W, dt, nws, ws.data_ptr(), gather_mask)

    def _forward_pipelined(self, L, packed, f1, f2, out, dt, pieces, _events=None, gather_blocks=0):
        """The batch as `pieces` contiguous slices alternating between the caller's stream and one side stream, piece k + 1 starting
        when piece k's FRONT (feature extraction, context, motion, warp: ema_vfi.py:112-130) has been enqueued-and-finished, so that one
        piece's attention blocks (the LDS-window pack kernel: gather / blend / MFMA per sample) run beside another piece's plain
        convolutions (LDS-ring kernels: MFMA-dense) on the same CUs - the two kernel families fit beside each other (80.8 KB + <= 80 KiB
        of LDS, <= 256 VGPRs each).  Frame pairs are independent (no cross-sample op in ema_vfi.py:110-147) and every kernel is
        batch-invariant per sample, so the result is bit-identical to the one-sequence forward
        (tests/test_gpu_runtime.py::test_pipelined_forward_is_bit_identical).  Joins back onto the caller's stream before returning.
        `_events`: per-launch event pairs, piece k's launches in [k * count / pieces, (k + 1) * count / pieces)."""
        B, C, H, W = f1.shape
        dev = f1.device
        hip = _lib.hip()
        cur = torch.cuda.current_stream(dev)
        side = _lib.side_stream(dev)
        if side.cuda_stream == cur.cuda_stream:
            side = _lib.side_stream(dev, which=1)
        cuts = [B * k // pieces for k in range(pieces + 1)]
        key = (dev.index, cur.cuda_stream)
        per = (_events[1] // pieces) if _events is not None else 0
        if _events is not None:
            # every piece runs the FULL launch list: an array sized for one sequence would leave most of each piece's launches
            # unbracketed and the caller reading never-recorded events
            nl = L.emavfi_forward_launches(C, self.mid_channels, self.num_blocks, 1, H, W, dt, None, 0, None, None, 0)
            if per < 2 * nl:
                raise ValueError(f"EMA_VFI: a pipelined forward of {pieces} pieces needs {pieces} x 2 x {nl} events, got {_events[1]}")
        front_prev = None
        # hipEventCreateWithFlags binds an event to the CURRENT device: everything that creates, records or waits on one runs under
        # the model's device (a model on cuda:1 while cuda:0 is current got hipErrorInvalidHandle here)
        with torch.cuda.device(dev):
            fork, join = hip.event(key + ("fork",)), hip.event(key + ("join",))
            hip.record(fork, cur)          # the frames (and the packed blob) are ready on the caller's stream
            hip.wait(side, fork)
            try:
                for k in range(pieces):
                    b0, b1 = cuts[k], cuts[k + 1]
                    s = cur if k % 2 == 0 else side
                    if front_prev is not None:
                        hip.wait(s, front_prev)
                    front = hip.event(key + ("stage", k))
                    with torch.cuda.stream(s):
                        stage = (c_void_p * 3)(*[front if i == self.pipeline_stagger else None for i in range(3)])
                        ev = (c_void_p(_events[0].value + k * per * ctypes.sizeof(c_void_p)), per) if _events is not None else None
                        self._launch(L, packed, f1[b0:b1], f2[b0:b1], out[b0:b1], dt, gather_blocks, None, cast(stage, POINTER(c_void_p)), ev)
                    front_prev = front if self.pipeline_stagger >= 0 else None
            finally:
                # also when a piece failed to enqueue: `out` and the frames are known to the caching allocator on the caller's stream
                # only, so whatever the side stream already holds must be ordered in front of their reuse
                hip.record(join, side)
                hip.wait(cur, join)
        # the caching allocator knows `out` (and the frames) only on the caller's stream; the side stream's work on them is ordered
        # before everything the caller enqueues from here on by the join above

    def warp(self, frame2, feature, flow):
        """Same signature as the reference (ema_vfi.py:149); ``feature`` is only a device hint there."""
        return _lib.warp(frame2, flow).to(frame2.dtype)
