"""Batched streaming harness around the native forward.

Reproduces the call pattern and OUTPUT ORDER of the reference's hot loop
(``/root/reference/inference.py:146-205``) for a sequence of uint8 HWC frames (video decode and the video writer stay outside - they are
host codec I/O; the reference's ``cv2.resize`` of every frame to ``--scale`` runs on the device when ``scale`` / ``size`` is given, see below):

    frame1 = first frame
    for every next frame2 (every ``frame_interval``-th loop turn, :161-164):
        for i in 1..interpolation_factor:              # :173-184
            write denormalize(model(frame1, frame2))   # identical arguments for every i (alpha unused, :174)
        write denormalize(normalize(frame1))           # :187-188  (predictions come BEFORE the earlier frame)
        frame1 = frame2
    write the last frame: as read (raw uint8) when the loop ends in the pair branch (:164-167),
                          denormalize(normalize(frame1)) when it ends in the skip branch (:198-201, frame_interval > 1)

What changes is how the work is scheduled, not what is computed:
  * pairs are processed in batches (the reference runs batch 1 with a blocking D2H per frame, :53);
  * ToTensor/Normalize and denormalize/clip/uint8 run on the GPU (emavfi_preprocess_u8 / _postprocess_u8);
  * the ``interpolation_factor`` identical forwards of a pair are computed once and emitted that many
    times (bit-identical to recomputing them);
  * THREE streams (round 5; the reference: one, with a blocking D2H per frame, inference.py:53): the uint8 frames of batch k + 1
    travel host -> HBM by hipMemcpyAsync (the SDMA engines: no compute unit involved) and are normalised by a short device kernel
    on a high-priority side stream while the caller's stream computes batch k; the predictions of batch k - 1 are turned into
    uint8 by a device kernel and copied HBM -> host on another one - chained by events.  Two buffer slots of pinned host
    memory: the host fills slot k+1 and drains slot k-1 while the GPU works on slot k; consecutive pairs share a frame, so a
    batch of n pairs moves n+1 frames (frame_interval 1), not 2n.  Measured beside back-to-back B = 8 x 720p forwards
    (tools/copy_beside_compute.py, profiles/r05_stream_*): a copy + device kernel leg costs the forward 0.6-1.2 % of its rate,
    where the round-1..4 form - the pre / post kernels reading / writing the pinned buffers themselves over PCIe
    (``zero_copy=True`` keeps it) - costs 4.6-5.5 % per leg even on a side stream: a kernel that waits on PCIe holds its
    wave slots, and the persistent convolution kernels need all of them.
``mode="recursive"`` (opt-in, not in the reference, which has no timestep input) replaces the repeated
identical prediction by recursive midpoints: factor 1 -> [1/2]; factor 3 -> [1/4, 1/2, 3/4]; factor 7 -> eighths.
``reference_quirks=False`` drops the de-normalisation of the already-[0,1] model output (appendix A of
SURVEY.md) and passes source frames through untouched; order and counts stay the same.
``numa="auto"`` (opt-in) places the host side of the harness on the CPUs of the device's NUMA node (``dist.numa_plan``): the
staging pool's threads bind themselves to them, and the pinned buffers are allocated and first touched from one of those threads.
Frames are the same either way.
``pixel_format="nv12"`` (opt-in; the default ``"bgr24"`` is the reference's cv2 layout) takes and yields frames in the contiguous NV12
layout video decoders produce - uint8 ``[H*3/2, W]``: H rows of Y, then H/2 rows of interleaved U,V pairs; even H and W - so the pinned
slots and the SDMA copies move 1.5 bytes per pixel instead of 3.  Decode and encode run inside the device kernels
(emavfi_preprocess_nv12 / _postprocess_nv12, colour definition: include/emavfi.h); ``yuv_standard`` / ``yuv_full_range`` pick one of the four
standards.  Order, counts and scheduling are the same; a round-tripped source frame is decode -> normalise -> denormalise -> encode.
``pixel_format="p010"`` / ``"p012"`` / ``"p016"`` (opt-in) is the same layout with one 16-bit word per sample, the sample in the word's top
10 / 12 / 16 bits - what decoders of 10-bit and HDR material produce: frames in and out are numpy uint16 ``[H*3/2, W]``, even H and W.  Nothing
is crushed to 8 bits on the way: emavfi_preprocess_p010 / _postprocess_p010 decode to and encode from ``depth``-bit integers (the high-bit-depth
definition of include/emavfi.h); ``yuv_standard`` additionally takes ``"bt2020"`` for these formats only.  The slots stay bytes, with rows of
2 W bytes, and are reinterpreted as words at the kernel boundary; staging, copies, order and counts are NV12's.  ``scale`` / ``size``,
``scene_threshold`` and ``evaluate()`` are refused with these formats: the resize, signature and metric kernels read bytes.
``scale=s`` (the reference's ``--scale``, inference.py:93-94: frames become ``(int(H * s), int(W * s))``) or ``size=(Hd, Wd)`` (mutually
exclusive; opt-in) resizes every frame on the device, inside the launch that normalises it (emavfi_preprocess_u8_resized /
_preprocess_nv12_resized; the resize definition is the project's own, include/emavfi.h - no byte parity with cv2 is claimed).  Frames are
staged and copied at the source size; everything from the normalised tensor onward, and every yielded frame, has the destination size.  A
frame the reference writes "as read" (:167, which there is the resized frame) and the source frames of ``reference_quirks=False`` are the
device-resized bytes.  ``pixel_format="nv12"`` needs an even destination H and W.  With neither argument the harness takes frames that
already have the size the model runs at, exactly as before.
``scene_threshold=f`` (opt-in, a float in (0, 1]; not in the reference, which interpolates across cuts) holds the earlier frame across a hard
cut: a pair whose 32 x 32 luma thumbnails differ by at least ``f`` of full scale on average (the scene-cut definition of include/emavfi.h;
``lib.scene_threshold_units``) yields its earlier frame in place of each of its in-between frames.  The decision is made on the device from the
staged bytes at their source size (NV12: the Y plane) on the pre lane, and applied on the post lane by overwriting the pair's prediction frames
before they travel to the host; flags and scores ride to a small pinned buffer behind them and are read after the ``done`` wait the drain
already performs - no new synchronisation point.  Order and counts of the output do not change; ``scene_cuts`` lists ``(i1, i2, score)`` of
the flagged pairs of the last ``run`` (global frame indices, in order), ``scene_scores`` every pair's.  Known waste: the forwards of a flagged
pair (in recursive mode all of its midpoints) are still computed and then overwritten - skipping them would need a read-back before the
forward is enqueued.
``pixel_format="yuv420p8"`` / ``"yuv420p10"`` / ``"yuv420p12"`` / ``"yuv420p16"`` (opt-in) takes and yields PLANAR 4:2:0 frames as a YUV4MPEG2
stream and every software decoder hold them (``emavfi.y4m``): one contiguous buffer of H rows of Y, then the dense U plane, then the dense V
plane - numpy ``[H*3/2, W]``, uint8 at depth 8, uint16 with the sample in the word's LOW bits above; even H and W.  The slot has NV12's / P010's
byte size, so staging, copies, order and counts are theirs; only the plane views and the two kernels differ (emavfi_preprocess_yuv420p /
_postprocess_yuv420p, defined by composition on the NV12 / P010 entries: a planar stream is the NV12 / P010 stream de-interleaved).
``"yuv420p8"`` supports ``scene_threshold`` and ``evaluate()`` as NV12 does (the Y plane) and ``scale`` / ``size`` by three emavfi_resize_u8
launches (Y, U, V as one-channel images) into a resized planar buffer ahead of the preprocess kernel - the same bytes as NV12's resized
planes, since channels are resized independently; the deeper planar formats refuse all three as P010 does.
``run_chunked(frames, chunk_pairs=64)`` is ``run()`` over an iterable of unknown length - a pipe - in bounded memory: at most
``chunk_pairs * frame_interval + 1`` source frames are held, and the yielded sequence is ``run(list(frames))``'s byte for byte.
``evaluate(frames, every=1)`` scores the model by the held-out protocol instead of emitting frames: every target frame ``t`` is interpolated
from ``t - 1`` and ``t + 1`` and compared with the true ``t`` on the device (the frame-metric definition of include/emavfi.h: per-channel sum
of squared differences and 11 x 11 Gaussian-window SSIM); only the metric words travel to the host, behind the ``done`` event the drain
waits for anyway.
``mode="resample"`` (opt-in, not in the reference, whose ``--target-fps`` only multiplies the rate by an integer) converts the stream from
``rate_in`` to ANY ``rate_out >= rate_in`` - 24 -> 60, 25 -> 60, 30000/1001 -> 60 (both: anything ``fractions.Fraction`` accepts; pass decimals as
strings).  Output ``k`` sits at source time ``k * rate_in / rate_out`` (the temporal resample definition of include/emavfi.h, all integer) and is
served from the dyadic tree of recursive midpoints of its pair, ``resample_depth`` (1..5, default 3) levels deep: ``resample_method="nearest"``
(default) takes the closest node, ``"blend"`` mixes the two nodes around the output time per sample, as emitted.  ``run()`` yields frames in
TEMPORAL order - a source frame, then the in-betweens that follow it.  Only the nodes a pair's outputs use are computed (``resample_plan``), one
model call per tree level per batch; every node is post-processed once, and one ``emavfi_resample_frames`` call on the post lane assembles the
batch's output frames - source frames included - into the buffer that leaves for the host, holding the earlier frame of a flagged pair when
``scene_threshold`` is set.  ``run_chunked`` and ``run(frames, rank, world)`` work as before on the global time grid.  Needs
``reference_quirks=False`` (the constructor's default is the reference's behaviour, which this is not), ``frame_interval=1``, the default
``interpolation_factor`` and ``zero_copy=False``; all pixel formats work, ``scale`` / ``size`` on the byte formats; ``evaluate()`` is unaffected.
``shutter`` (opt-in, mode "resample" only; degrees in (0, 360]: 180, 172.8, "1080/7") adds motion blur: every output frame is the weighted
integer mean of the tree nodes inside its exposure window of ``shutter / 360`` of an OUTPUT frame period (the shutter definition of
include/emavfi.h; ``shutter_taps``, ``shutter_plan``), summed on the device by ``emavfi_accumulate_frames`` in place of the selection above,
so that only the accumulated frames cross PCIe.  ``rate_out`` must be an integer multiple of ``rate_in`` (1 included: the frame rate stays
and blur is added) - windows then never leave their pair, and chunks, ranks, scene holds and the static guard work as without it.  The
output on the last frame of the clip is that frame.  Excludes ``resample_method="blend"``, ``dedup_threshold`` and ``evaluate()``.
``light`` (opt-in, mode "resample" with a ``shutter`` or ``resample_method="blend"``; "srgb", "bt709" or "hlg") takes those means in linear
light instead of on the coded samples (the linear light definition of include/emavfi.h): the table of the transfer function - full range
for ``bgr24``, ``yuv_full_range`` otherwise - is built and uploaded once here, every batch is assembled by
``emavfi_accumulate_frames_linear`` (a blend ``(a, b, w)`` as the taps ``(a, b)`` with the weights ``(256 - w, w)``), the same forwards are
issued and nothing else changes.  ``bgr24`` is mixed whole; of a Y'CbCr frame the Y plane is mixed in light and chroma stays coded: a
luma-linear approximation, exact for greys.  The 16-bit formats are refused; ``evaluate()`` mixes nothing and ignores it.
``dedup_threshold`` (opt-in, mode "resample" only; a fraction in [0, 1], 0 = bit-identical luma) drops frames that copy the frame before them -
24 fps film in a 30 fps stream, animation on twos, screen captures - and interpolates across the gap instead of yielding the copy again (the
duplicate-frame definition of include/emavfi.h: per cell of the 32 x 32 scene grid the mean absolute luma difference, the MAXIMUM over the
cells; all ten pixel formats, scored as staged, at source size).  Output count and times do not change; an output inside a gap of ``m``
source intervals comes from that gap's tree, ``ceil(log2 m)`` levels deeper (``dedup_kept``, ``resample_plan_dedup``).  ``dedup_max_run``
(default 3) bounds the dropped frames in a row, ``dedup_span`` (default 64) keeps every frame whose global index it divides, so that
``run_chunked`` with a ``chunk_pairs`` that is a multiple of it sees what the whole clip would.  The set of forwards depends on the flags, so
- unlike the scene decision - the host reads them before it plans: a pre-pass uploads the call's frames in slot-sized batches, scores the
consecutive pairs and waits ONCE per ``run()`` call (once per chunk in ``run_chunked``); the source frames cross PCIe twice.  ``duplicates``
lists ``(t, score)`` of the dropped frames, ``dedup_scores`` of every scored pair ``(t - 1, t)``, with global indices.  One process only.
``static_guard=r`` (opt-in, an int radius in 0..16; not in the reference, which writes the prediction as it comes) holds the static regions
of a pair - channel logos, subtitles, scoreboards, letterbox bars, the unchanged background of screen captures: a pixel whose whole window of
radius ``r``, clipped to the frame, is the same in both source frames keeps the EARLIER frame's samples in every prediction of the pair (the
static region definition of include/emavfi.h; 4:2:0 chroma where all four luma pixels it covers qualify).  ``static_tolerance`` (a fraction of
full scale in [0, 1], default 0: bit-equal samples only; ``lib.static_tolerance_units``) widens "the same".  No default radius or tolerance is
claimed.  The guard runs on the post lane, on the frames AS EMITTED, at the size the model runs at: the prediction bytes are compared with the
staged source bytes (with ``scale`` / ``size``: the device-resized ones) by one ``emavfi_static_guard_frames`` call per batch, ahead of the
scene hold (the order cannot change the result: a held frame is the earlier frame everywhere); in mode "resample" every node frame is guarded
against its gap's two kept source frames before ``emavfi_resample_frames`` selects or blends.  The recursion's fp32 inputs stay unguarded.
``static_share`` lists, per emitted prediction of the last ``run()`` (mode "resample": per emitted frame made of node frames), the share of
its pixels that were held; the counts ride to a small pinned buffer behind the frames and are read after the ``done`` wait the drain already
performs - no new synchronisation point.  Refused with ``reference_quirks=True`` (exact source pixels pasted into the quirk's de-normalised
prediction would show as patches) and with ``zero_copy=True``; ``evaluate()`` is unaffected.  All ten pixel formats work.
``ensemble="reverse" | "flip" | "full"`` (opt-in; not in the reference, which calls the model once per pair) runs EVERY forward the harness
issues - all three modes, the recursion's inner midpoints, ``evaluate()``, with any of the options above - as the test-time ensemble of
include/emavfi.h ("ENSEMBLE DEFINITION"; ``EMA_VFI.ensemble``): 2, 4 or 8 plain forwards of the same batch, averaged on the device.  It is
passed with each call, so the model's own attribute is neither read nor changed; ``None`` (default) leaves the decision to that attribute.
With "reverse" or "full" every prediction is exactly symmetric in time: the reversed clip yields the reversed predictions, byte for byte.
``agreement=tol`` with ``agreement_radius=r`` (opt-in; not in the reference) runs EVERY forward the harness issues - all three modes, the
recursion's inner midpoints, ``evaluate()`` - under the agreement guard of include/emavfi.h ("AGREEMENT GUARD DEFINITION";
``EMA_VFI.agreement``): where the time-forward and the time-reversed half of the ensemble differ by more than ``tol`` of full scale within
``r`` pixels, the plain blend of the two source frames is emitted.  It needs ``ensemble="reverse"`` or ``"full"`` (given here, or the
model's attribute) and is refused otherwise, and with ``reference_quirks=True`` (a [0, 1] blend pasted into the quirk's de-normalised
prediction would show as patches).  ``agreement_share`` lists, per emitted prediction of the last ``run()`` (mode "resample": per emitted
frame made of node frames, the share of the first node frame it names), the share of its pixels the guard held; the counts follow the
frames to pinned memory and are read after the ``done`` wait the drain already performs - no new synchronisation point.
``flow_scale=2 | 4 | 8`` (opt-in; not in the reference, whose ``--scale`` shrinks the output as well) runs EVERY forward the harness issues -
all three modes, the recursion's inner midpoints, ``evaluate()``, the members of an ensemble, with any of the options above - with the flow
estimated on the pair reduced by that factor and everything else at full size (include/emavfi.h, "COARSE FLOW DEFINITION";
``EMA_VFI.flow_scale``).  It is passed with each call, as ``ensemble`` is; ``None`` (default) leaves the decision to the model's attribute.
No quality claim is made: ``evaluate()`` says what it buys on a clip.
``align=R_px`` with ``align_ratio=q`` (opt-in; not in the reference; both or neither, no default is claimed) runs EVERY forward the harness
issues - all three modes, the recursion's inner midpoints, ``evaluate()``, with any of the options above and below - on the pair with its
global translation removed (include/emavfi.h, "ALIGN DEFINITION"; ``EMA_VFI.align``): one shift per pair, a multiple of 4 pixels per axis
within ``R_px`` (a multiple of 4 in 4..128), found on the device from 4 x 4 cell sums and kept only where it lowers the mean absolute
difference to ``q`` (in [0, 1]) of the unshifted one; both frames are moved by half of it and the model sees the moved pair.  Like
``ensemble`` it is passed with each call.  ``align_shifts`` lists, per emitted prediction of the last ``run()`` (mode "resample": per emitted
frame made of node frames, the first node frame it names), the (dy, dx) in pixels; the records follow the frames to pinned memory as the
agreement counts do - no new synchronisation point.  With ``active_area`` the model, and so the search, sees the active picture.

``border=N`` with ``border_mode="replicate" | "reflect"`` (opt-in; not in the reference) runs EVERY forward the harness issues - all three
modes, the recursion's inner midpoints, ``evaluate()``, with any of the options above, the ensemble included - on frames extended by N
pixels past each edge and crops the prediction back (include/emavfi.h, "BORDER DEFINITION"; ``EMA_VFI.border``): the forward takes the outside
of the picture as zero, which is mean grey after normalisation, so the in-between frames carry an edge band where the picture continues past
the frame.  Like ``ensemble`` it is passed with each call: the model's own attribute is neither read nor changed, ``None`` (default) leaves the
decision to that attribute.  Everything behind the model - the post kernels, the static guard, scene holds, the resample assembly, the
metrics - works on the cropped frames and is untouched.
``active_area="auto" | (top, left, height, width)`` (opt-in; not in the reference, which interpolates the whole frame) runs every forward
of ``run()`` on the active picture alone - a 2.39:1 film in a 16:9 container is a quarter black bars - and puts the bars back (the active
area definition of include/emavfi.h): the pre / post kernels read and write views of the rectangle inside the staged and emitted frames
(``bgr24``: emavfi_preprocess_u8_pitched / _postprocess_u8_pitched; the Y'CbCr entries are pitched already), the slots' fp32 tensors and the
forward have the rectangle's size, and one ``emavfi_fill_outside_frames`` call per batch on the post lane copies the bars of the pair's
EARLIER frame around every prediction (mode "resample": around every node frame) ahead of the static guard, the scene hold and the
assembly, which see whole frames as before.  ``ensemble``, ``border``, ``flow_scale`` and ``agreement`` act on the cropped tensors; source
frames are emitted untouched.  An explicit rectangle needs an even top and bottom and a left and right that are multiples of 16 (a bottom
/ right edge may be the frame's) and costs no scan and no host wait; content outside it is not interpolated.  ``"auto"`` finds it in a
pre-pass like ``dedup_threshold``'s, with which it shares the upload and the ONE host wait per ``run()`` (``prepass_waits``): every frame's
bounds of samples above black + ``active_tolerance`` (a fraction of full scale; black is 16 << (depth - 8) for limited-range Y'CbCr, which
is scanned on its Y plane; ``lib.active_level_units``) are taken by ``emavfi_active_bounds`` and joined and rounded on the host
(``lib.active_rect``).  No bars, or none found: the plain path, byte for byte.  ``active_rect`` / ``active_share`` report the rectangle in
force and its share of the frame's pixels.  Refused with ``reference_quirks=True``, ``scale`` / ``size``, ``zero_copy=True``, in
``evaluate()`` and, for ``"auto"``, with ``world != 1``: out of scope, not for ever.  No quality claim is made: the model sees zero padding
at the rectangle's edge where it saw the bar before (``border`` replicates the picture there instead).
"""
from __future__ import annotations

import functools
import os
from fractions import Fraction
from math import gcd
from types import SimpleNamespace
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import formats as _formats
from . import lib as _lib


class FrameScore(NamedTuple):
    """One held-out target of ``FrameInterpolator.evaluate``: frame ``t`` interpolated from ``t - 1`` and ``t + 1`` against the true ``t``.
    ``sse`` / ``ssimq``: the device's integers per channel; ``psnr`` / ``ssim``: the figures per channel; ``sse_all`` / ``psnr_all``: over
    all channels' samples; ``ssim_all``: the mean over the channels (nan below 11 pixels per side)."""
    t: int
    sse: Tuple[int, ...]
    ssimq: Tuple[int, ...]
    psnr: Tuple[float, ...]
    ssim: Tuple[float, ...]
    sse_all: int
    psnr_all: float
    ssim_all: float


class Evaluation:
    """What ``FrameInterpolator.evaluate`` returns: ``size`` = (H, W) the frames were scored at, ``channels`` (1 for NV12: the Y plane),
    ``targets`` = one ``FrameScore`` per target in order, and the clip means ``psnr`` / ``ssim`` of the targets' overall figures (nan for an
    empty clip).  Iterating or indexing goes over ``targets``."""

    def __init__(self, size, channels, targets=()):
        self.size, self.channels, self.targets = (int(size[0]), int(size[1])), int(channels), list(targets)

    def add(self, t, words):
        """words: [channels][2] integers {sse, ssimq} as emavfi_frame_metrics_u8 wrote them"""
        (H, W), C = self.size, self.channels
        sse, ssimq = tuple(int(w[0]) for w in words), tuple(int(w[1]) for w in words)
        ssim = tuple(_lib.ssim(q, H, W) for q in ssimq)
        self.targets.append(FrameScore(int(t), sse, ssimq, tuple(_lib.psnr(v, H * W) for v in sse), ssim, sum(sse),
                                       _lib.psnr(sum(sse), H * W * C), sum(ssim) / C))

    def __len__(self):
        return len(self.targets)

    def __iter__(self):
        return iter(self.targets)

    def __getitem__(self, k):
        return self.targets[k]

    @property
    def psnr(self):
        return sum(r.psnr_all for r in self.targets) / len(self.targets) if self.targets else float("nan")

    @property
    def ssim(self):
        return sum(r.ssim_all for r in self.targets) / len(self.targets) if self.targets else float("nan")

    def __repr__(self):
        return f"Evaluation({len(self.targets)} targets at {self.size[0]} x {self.size[1]} x {self.channels}: psnr {self.psnr:.3f} dB, ssim {self.ssim:.5f})"


class ResamplePlan(NamedTuple):
    """What ``FrameInterpolator.resample_plan`` returns.  ``outputs``: ``(k, s, j0, j1, w)`` per output frame in emission order - output
    ``k`` lies in the pair ``(s, s + 1)`` and is node ``j0`` (``w`` = 0, then ``j1 == j0``) or the blend of nodes ``j0`` and ``j1`` with
    weight ``w`` in 1..255 (a ``w`` of 256 is normalised to node ``j1`` alone); node 0 is source ``s``, node ``G`` source ``s + 1``.
    ``pairs``: ``{s: levels}`` for every pair this rank computes, ``levels[l]`` = the needed nodes of recursion level ``l + 1`` (level 1 is
    the midpoint ``G / 2``), ascending - one forward each.  ``P`` / ``Q``: ``rate_in / rate_out`` in lowest terms; ``G`` = 2^depth."""
    outputs: List[Tuple[int, int, int, int, int]]
    pairs: Dict[int, List[List[int]]]
    P: int
    Q: int
    G: int

    @property
    def forwards(self) -> int:
        return sum(len(lv) for levels in self.pairs.values() for lv in levels)


class DedupPlan(NamedTuple):
    """What ``FrameInterpolator.resample_plan_dedup`` returns.  ``outputs``: ``(k, t_i, m, j0, j1, w)`` per output frame in emission order -
    output ``k`` is served from the gap of ``m`` source intervals that starts at the kept frame ``t_i`` (a global index) and is node ``j0``
    (``w`` = 0, then ``j1 == j0``) or the blend of nodes ``j0`` and ``j1`` of that gap's tree of depth ``D + ceil(log2 m)``; node 0 is source
    ``t_i``, node ``2^(D + ceil(log2 m))`` source ``t_i + m``.  ``gaps``: ``{t_i: (m, levels)}``, ``levels[l]`` = the needed nodes of
    recursion level ``l + 1``, ascending - one forward each.  ``P`` / ``Q``: ``rate_in / rate_out`` in lowest terms; ``D``: the depth asked for."""
    outputs: List[Tuple[int, int, int, int, int, int]]
    gaps: Dict[int, Tuple[int, List[List[int]]]]
    P: int
    Q: int
    D: int

    @property
    def forwards(self) -> int:
        return sum(len(lv) for _, levels in self.gaps.values() for lv in levels)


class ShutterPlan(NamedTuple):
    """What ``FrameInterpolator.shutter_plan`` returns.  ``outputs``: ``(k, s, taps)`` per output frame in emission order - output ``k``
    lies in the pair ``(s, s + 1)`` and is the weighted mean of its ``taps`` ``((j, w), ...)``, nodes of that pair's tree (node 0 is source
    ``s``, node ``G`` source ``s + 1``); the output on the last frame of the clip is that frame alone, ``((0, 1),)``.  ``pairs``:
    ``{s: levels}`` as in ``ResamplePlan`` - one forward per listed node.  ``Q``: ``rate_out / rate_in``; ``G`` = 2^depth."""
    outputs: List[Tuple[int, int, Tuple[Tuple[int, int], ...]]]
    pairs: Dict[int, List[List[int]]]
    Q: int
    G: int

    @property
    def forwards(self) -> int:
        return sum(len(lv) for levels in self.pairs.values() for lv in levels)


class FrameInterpolator:
    shutter = None   # the shutter angle in degrees as a Fraction (include/emavfi.h, "SHUTTER DEFINITION"); None: instantaneous frames
    light = None     # the transfer function blends and shutter means are taken in light with (include/emavfi.h, "LINEAR LIGHT DEFINITION"); None: coded
    dedup = None   # the duplicate threshold in score units (lib.dedup_threshold_units); None: duplicates are not looked for
    dedup_max_run, dedup_span = 3, 64
    static_guard = None   # the radius of the static-region guard (include/emavfi.h, "STATIC REGION DEFINITION"); None: off
    static_tol = 0        # its tolerance in sample units (lib.static_tolerance_units)
    ensemble = None       # test-time ensembling of every forward (EMA_VFI.ensemble); None: what the model's attribute says
    border = None         # (N, mode) of the frame border of every forward (EMA_VFI.border); None: what the model's attribute says
    agreement = None      # (tol, radius) of the agreement guard of every forward (EMA_VFI.agreement); None: what the model's attribute says
    flow_scale = None     # the scale the flow of every forward is estimated at (EMA_VFI.flow_scale); None: what the model's attribute says
    active = None         # "auto" or an explicit (top, left, height, width) (include/emavfi.h, "ACTIVE AREA DEFINITION"); None: the whole frame
    active_rect = None    # the rectangle in force in the last run(): (top, left, height, width); None before a run and with active_area=None
    active_share = 1.0    # its share of the frame's pixels
    prepass_waits = 0     # host waits of the last run()'s pre-pass (dedup_threshold and active_area="auto" share one)
    _act = None           # the rectangle in force where it is smaller than the frame, else None: the plain path
    align = None          # (R_px, ratio) of the global motion compensated before every forward (EMA_VFI.align); None: what the model's attribute says
    _al = None   # under `align`: the records of the batch just predicted, int32 [.., 4] on the device, in prediction order
    _ag = None   # under `agreement`: the held pixel counts of the batch just predicted, int32 on the device, in prediction order
    fmt = _formats.FORMATS["bgr24"]   # the record of `pixel_format` (formats.PixelFormat): what the frames are, asked here and nowhere by name
    mode = "reference"

    def __init__(self, model, interpolation_factor: int = 1, frame_interval: int = 1, batch_pairs: int = 8,
                 reference_quirks: bool = True, mode: str = "reference", device=None, copy_out: bool = True, zero_copy: bool = False,
                 numa: str = "off", pixel_format: str = "bgr24", yuv_standard: str = "bt601", yuv_full_range: bool = False,
                 scale: Optional[float] = None, size=None, scene_threshold: Optional[float] = None,
                 rate_in=None, rate_out=None, resample_depth: int = 3, resample_method: str = "nearest",
                 dedup_threshold: Optional[float] = None, dedup_max_run: int = 3, dedup_span: int = 64,
                 static_guard: Optional[int] = None, static_tolerance: float = 0.0, ensemble: Optional[str] = None,
                 border: Optional[int] = None, border_mode: str = "replicate",
                 agreement: Optional[float] = None, agreement_radius: Optional[int] = None, shutter=None,
                 flow_scale: Optional[int] = None, light: Optional[str] = None, active_area=None, active_tolerance: float = 0.0,
                 align: Optional[int] = None, align_ratio: Optional[float] = None):
        if shutter is not None and mode != "resample":
            raise ValueError("shutter belongs to mode='resample': the exposure window is accumulated over the nodes of its time grid")
        if light is not None:
            if not isinstance(light, str) or light not in _lib.TRANSFERS:
                raise ValueError(f"light must be one of {_lib.TRANSFERS} (None: coded samples are mixed), got {light!r}")
            if mode != "resample":
                raise ValueError("light belongs to mode='resample': only its blends and shutter means mix frames")
        if interpolation_factor < 0 or frame_interval < 1 or batch_pairs < 1:
            raise ValueError("interpolation_factor >= 0, frame_interval >= 1, batch_pairs >= 1 required")
        if mode not in ("reference", "recursive", "resample"):
            raise ValueError("mode must be 'reference' (the reference's repeated identical prediction), 'recursive' or 'resample' (any output "
                             "frame rate: rate_in, rate_out)")
        if mode == "resample":
            if reference_quirks:
                raise ValueError("mode='resample' with reference_quirks=True: frame-rate conversion is not the reference's behaviour (pass "
                                 "reference_quirks=False)")
            if frame_interval != 1:
                raise ValueError("mode='resample' with frame_interval != 1: the time grid counts every source frame")
            if interpolation_factor != 1:
                raise ValueError("mode='resample' with an interpolation_factor: the number of in-between frames follows from rate_in and rate_out")
            if zero_copy:
                raise ValueError("mode='resample' with zero_copy=True: the output frames are assembled in device memory and leave by copy")
            if rate_in is None or rate_out is None:
                raise ValueError("mode='resample' needs rate_in and rate_out")
            self._ratio = self.resample_ratio(rate_in, rate_out)
            self.resample_depth, self.resample_method = self._resample_args(resample_depth, resample_method)
            if shutter is not None:
                P, Q = self._ratio
                if P != 1:
                    raise ValueError(f"shutter with rate_in / rate_out = {P}/{Q}: exposure windows would cross pair boundaries unless rate_out "
                                     "is an integer multiple of rate_in (P > 1 is not supported)")
                if resample_method == "blend":
                    raise ValueError("shutter with resample_method='blend': the window's weights already say how the nodes are mixed")
                if dedup_threshold is not None:
                    raise ValueError("shutter with dedup_threshold: a window over a gap of dropped frames is not defined")
                self._taps = [self.shutter_taps(Q, self.resample_depth, shutter, r) for r in range(Q)]     # refuses what the rule refuses
                self.shutter = self._exposure(shutter)[2]
            elif light is not None and resample_method != "blend":
                raise ValueError("light without a shutter or resample_method='blend': nothing is mixed, every output frame is one node")
        elif rate_in is not None or rate_out is not None:
            raise ValueError("rate_in / rate_out belong to mode='resample'")
        if mode != "resample" and (dedup_threshold is not None or dedup_max_run != 3 or dedup_span != 64):
            raise ValueError("dedup_threshold / dedup_max_run / dedup_span belong to mode='resample': dropped frames are replaced on its time grid")
        if mode == "recursive" and (interpolation_factor + 1) & interpolation_factor:
            raise ValueError("recursive midpoints need interpolation_factor = 2^k - 1 (1, 3, 7, ...)")
        if numa not in ("off", "auto"):
            raise ValueError("numa must be 'off' or 'auto'")
        if ensemble is not None and (not isinstance(ensemble, str) or ensemble not in _lib.ENSEMBLES):
            raise ValueError(f"ensemble must be one of {_lib.ENSEMBLES} (None: what the model's attribute says), got {ensemble!r}")
        self.ensemble = ensemble
        if not isinstance(border_mode, str) or border_mode not in _lib.BORDER_MODES:
            raise ValueError(f"border_mode must be one of {_lib.BORDER_MODES}, got {border_mode!r}")
        if border is None and border_mode != _lib.BORDER_MODES[0]:
            raise ValueError(f"border_mode={border_mode!r} needs a border (border=N, 1..{_lib.BORDER_MAX})")
        if border is not None and (isinstance(border, bool) or not isinstance(border, int) or not 1 <= border <= _lib.BORDER_MAX):
            raise ValueError(f"border must be an int in 1..{_lib.BORDER_MAX} (None: what the model's attribute says), got {border!r}")
        self.border = None if border is None else (border, border_mode)
        # what rides on every forward: only what was given here, so that a model without these arguments still serves a plain harness
        self._forward_kw = {**({"ensemble": ensemble} if ensemble is not None else {}), **({"border": self.border} if border is not None else {})}
        if agreement is None:
            if agreement_radius is not None:
                raise ValueError("agreement_radius without agreement: the radius belongs to the agreement guard (pass a tolerance)")
        else:
            self.agreement = _lib.agreement_args(agreement, 0 if agreement_radius is None else agreement_radius, "agreement / agreement_radius")
            if reference_quirks:
                raise ValueError("agreement with reference_quirks=True: a [0, 1] blend of the sources pasted into the quirk's de-normalised "
                                 "prediction would show as patches (pass reference_quirks=False)")
            runs = ensemble if ensemble is not None else getattr(model, "ensemble", None)
            if runs not in _lib.AGREEMENT_ENSEMBLES:
                raise ValueError(f"agreement with ensemble={runs!r}: the guard compares the two time directions and needs an ensemble that "
                                 f"runs both, one of {_lib.AGREEMENT_ENSEMBLES} (it is not chosen for you)")
            self._forward_kw["agreement"] = self.agreement
        self.agreement_share = []   # per emitted prediction of the last run(): the share of its pixels the agreement guard held
        if flow_scale is not None:
            self.flow_scale = _lib.flow_scale_arg(flow_scale, "flow_scale")
            if getattr(model, "pack_adapt", None) is not None:
                raise ValueError("flow_scale with a model under pack_adapt: the adaptive route has no given-flow form (unset one of them)")
            self._forward_kw["flow_scale"] = self.flow_scale
        if (align is None) != (align_ratio is None):
            raise ValueError("align and align_ratio belong together: the search radius in pixels and the acceptance ratio (no default is "
                             "claimed for either)")
        if align is not None:
            _lib.align_args(align, align_ratio, "align / align_ratio")
            self.align = (align, float(align_ratio))
            self._forward_kw["align"] = self.align
        self.align_shifts = []      # per emitted prediction of the last run(): the (dy, dx) in pixels its pair was aligned by
        fmt = self.fmt = _formats.lookup(pixel_format)   # refuses an unknown name; from here on the record answers what the format is
        if light is not None and not fmt.light_table_fits:
            raise ValueError(f"light with pixel_format={pixel_format!r}: a table of 2^16 values of light does not fit LDS (8-, 10- and 12-bit "
                             "formats only)")
        # raises on an unknown standard; only the high-bit-depth definition knows "bt2020"
        (_lib.yuv_standard_code_deep if fmt.takes_bt2020 else _lib.yuv_standard_code)(yuv_standard, yuv_full_range)
        if not fmt.byte_kernels:
            if scale is not None or size is not None:
                raise ValueError(f"pixel_format={pixel_format!r} with scale / size: the resize kernels read bytes (16-bit frames are not resized)")
            if scene_threshold is not None:
                raise ValueError(f"pixel_format={pixel_format!r} with scene_threshold: the signature kernel reads bytes (16-bit frames are not "
                                 "scanned for cuts)")
        if mode == "resample":
            self.dedup_max_run, self.dedup_span = self._dedup_args(dedup_max_run, dedup_span,
                                                                   self.resample_depth if dedup_threshold is not None else None)
            if dedup_threshold is not None:
                if isinstance(dedup_threshold, bool) or not isinstance(dedup_threshold, (int, float)) or not 0 <= dedup_threshold <= 1:
                    raise ValueError("dedup_threshold must be None (off) or a number in [0, 1]: the largest mean absolute luma difference of a "
                                     "cell, as a fraction of full scale, at which a frame still counts as a copy of the frame before it (0: "
                                     "bit-identical luma only)")
                self.dedup = _lib.dedup_threshold_units(dedup_threshold, fmt.depth)
        self.duplicates, self.dedup_scores = [], []   # (t, score) of the dropped frames / of every scored pair (t - 1, t), global indices
        if isinstance(static_tolerance, bool) or not isinstance(static_tolerance, (int, float)) or not 0 <= static_tolerance <= 1:
            raise ValueError("static_tolerance must be a number in [0, 1]: the largest difference of two samples, as a fraction of full scale, "
                             "at which they still count as the same (0: bit-equal only)")
        if static_guard is None:
            if static_tolerance != 0:
                raise ValueError("static_tolerance without static_guard: the tolerance belongs to the static-region guard (pass a radius)")
        else:
            if isinstance(static_guard, bool) or not isinstance(static_guard, int) or not 0 <= static_guard <= _lib.STATIC_MAX_RADIUS:
                raise ValueError(f"static_guard must be None (off) or an integer radius in 0..{_lib.STATIC_MAX_RADIUS}")
            if reference_quirks:
                raise ValueError("static_guard with reference_quirks=True: exact source pixels pasted into the quirk's de-normalised prediction "
                                 "would show as patches (pass reference_quirks=False)")
            if zero_copy:
                raise ValueError("static_guard with zero_copy=True: the guard compares and patches frames in device memory, which leave by copy")
            self.static_guard = static_guard
            self.static_tol = _lib.static_tolerance_units(static_tolerance, fmt.depth)
        self.static_share = []   # per emitted prediction of the last run(): the share of its pixels the guard held
        if isinstance(active_tolerance, bool) or not isinstance(active_tolerance, (int, float)) or not 0 <= active_tolerance <= 1:
            raise ValueError("active_tolerance must be a number in [0, 1]: how far above black, as a fraction of full scale, a sample of the "
                             "bars may lie (0: black itself only)")
        if active_area is None:
            if active_tolerance != 0:
                raise ValueError("active_tolerance without active_area: the tolerance belongs to the search for the bars (pass active_area='auto')")
        else:
            if isinstance(active_area, str):
                if active_area != "auto":
                    raise ValueError(f"active_area must be None (the whole frame), 'auto' or a rectangle (top, left, height, width), got {active_area!r}")
                self.active = "auto"
            else:
                # the frame is not known yet: what can be said of the rectangle alone, the rest when the first frame arrives
                self.active = _lib.active_rect_check(active_area, None, None, "active_area")
                if active_tolerance != 0:
                    raise ValueError("active_tolerance with an explicit active_area: nothing is searched for (the tolerance belongs to 'auto')")
            if reference_quirks:
                raise ValueError("active_area with reference_quirks=True: the bars are the exact source samples, which the quirk's de-normalised "
                                 "frames are not (pass reference_quirks=False)")
            if scale is not None or size is not None:
                raise ValueError("active_area with scale / size: the rectangle is found and cut on the frames as staged, a resize in between "
                                 "is not supported")
            if zero_copy:
                raise ValueError("active_area with zero_copy=True: the bars are put back in device memory around frames that leave by copy")
            self._active_level = _lib.active_level_units(active_tolerance, fmt.depth, fmt.yuv, bool(yuv_full_range))
        if scale is not None and size is not None:
            raise ValueError("scale and size are mutually exclusive")
        if scale is not None and not scale > 0:
            raise ValueError("scale must be positive")
        if size is not None:
            size = self.output_size(0, 0, size=size, pixel_format=pixel_format)   # validates; the source size does not matter here
        if scene_threshold is not None and (isinstance(scene_threshold, bool) or not isinstance(scene_threshold, (int, float))
                                            or not 0 < scene_threshold <= 1):
            raise ValueError("scene_threshold must be None (off) or a float in (0, 1]: the mean absolute thumbnail difference, as a fraction "
                             "of full scale, at which a pair counts as a cut")
        self.scene = float(scene_threshold) if scene_threshold is not None else None
        self.scene_cuts, self.scene_scores = [], []   # (i1, i2, score) of the flagged pairs / of every pair of the last run()
        self.scale, self.size = scale, size
        self._resize = scale is not None or size is not None
        self.pixel_format = pixel_format
        self.yuv = {"standard": yuv_standard, "full_range": bool(yuv_full_range)}
        self.model = model
        self.factor = int(interpolation_factor)
        self.interval = int(frame_interval)
        self.batch_pairs = int(batch_pairs)
        self.quirks = bool(reference_quirks)
        self.mode = mode
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("FrameInterpolator needs the model on a ROCm device (no CPU path)")
        if light is not None:
            # built, checked and uploaded once: full range for bgr24, the Y'CbCr range otherwise.  The bits of the uint32 table as int32.
            table = _lib.transfer_table(light, fmt.depth, not fmt.yuv or bool(yuv_full_range))
            _lib.transfer_table_check(table, fmt.depth)
            self.light = light
            self._lin = torch.from_numpy(table.view(np.int32)).to(self.device)
        self._shape = None
        self._per = 0
        self._norm = None
        # False: yield views into the pinned result buffers instead of fresh arrays (valid until the generator is
        # advanced again - enough for a writer that consumes each frame at once; saves a page-faulting 2.8-6 MB
        # allocation + copy per frame)
        self.copy_out = bool(copy_out)
        # True: the round-1..4 transport (the pre / post kernels read / write the pinned host buffers in place) instead of SDMA copies
        self.zero_copy = bool(zero_copy)
        # "auto": the device's NUMA plan, computed once (None when "off"); its `bind` flag says whether the host work is placed
        if numa == "auto":
            from .dist import numa_plan
            self.numa = numa_plan(self.device)
        else:
            self.numa = None

    # ---- the size the model runs at (inference.py:93-94: width = int(w * scale), height = int(h * scale))
    @staticmethod
    def output_size(H: int, W: int, scale=None, size=None, pixel_format: str = "bgr24"):
        """(Hd, Wd) of H x W source frames: ``size`` itself, ``(int(H * scale), int(W * scale))`` as the reference truncates, or (H, W).
        ValueError for both arguments, a size outside 1..16384 and, for NV12, an odd destination H or W.  Pure host logic."""
        if scale is not None and size is not None:
            raise ValueError("scale and size are mutually exclusive")
        if size is not None:
            try:
                Hd, Wd = (int(v) for v in size)
            except (TypeError, ValueError):
                raise ValueError("size must be (Hd, Wd)") from None
        elif scale is not None:
            Hd, Wd = int(H * scale), int(W * scale)
        else:
            return int(H), int(W)
        if not (1 <= Hd <= _lib.RESIZE_MAX_DIM and 1 <= Wd <= _lib.RESIZE_MAX_DIM):
            raise ValueError(f"the resized frame {(Hd, Wd)} must lie in 1..{_lib.RESIZE_MAX_DIM} per dimension")
        if _formats.lookup(pixel_format).even_resize and (Hd % 2 or Wd % 2):
            raise ValueError(f"pixel_format={pixel_format!r}: the packed [H*3/2, W] layout needs an even destination H and W, got {(Hd, Wd)}")
        return Hd, Wd

    # ---- the reference's frame selection (inference.py:158-201), as (pairs, tail) over frame indices
    @staticmethod
    def schedule(n_frames: int, frame_interval: int):
        """Returns (pairs, last, last_roundtrip): pairs = [(i1, i2)] in processing order, last = index of the frame
        written at the end (None for an empty input), last_roundtrip = the loop ended in the skip branch
        (inference.py:198-201), where the reference writes denormalize_frame(frame1_tensor) - the float32 normalise ->
        float64 de-normalise -> truncate round trip, which changes some pixels by one count - instead of the raw frame."""
        if n_frames <= 0:
            return [], None, False
        pairs, cur, frame_num, nxt = [], 0, 0, 1
        while True:
            frame_num += 1
            if nxt >= n_frames:          # cap.read() fails: both branches write frame1 and stop
                return pairs, cur, frame_num % frame_interval != 0
            if frame_num % frame_interval == 0:
                pairs.append((cur, nxt))
            cur, nxt = nxt, nxt + 1      # in the skip branch the reference also advances frame1

    def count_outputs(self, n_frames: int) -> int:
        if self.mode == "resample":
            P, Q = self._ratio
            return 0 if n_frames <= 0 else ((n_frames - 1) * Q) // P + 1
        pairs, last, _ = self.schedule(n_frames, self.interval)
        return 0 if last is None else len(pairs) * (self.factor + 1) + 1

    # ---- frame-rate conversion (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION"): the schedule, pure host logic over integers
    @staticmethod
    def resample_ratio(rate_in, rate_out):
        """(P, Q) with P / Q = rate_in / rate_out in lowest terms.  Each rate: anything ``fractions.Fraction`` accepts (60, "59.94",
        "60000/1001", Fraction(30000, 1001), ...; a float is taken at its exact binary value, so pass decimals as strings).  ValueError for a
        rate that is no positive rational and for ``rate_out < rate_in``."""
        try:
            fi, fo = Fraction(rate_in), Fraction(rate_out)
        except (TypeError, ValueError, ZeroDivisionError):
            raise ValueError(f"rate_in / rate_out must be rationals (60, '59.94', '60000/1001', ...), got {rate_in!r} and {rate_out!r}") from None
        if fi <= 0 or fo <= 0:
            raise ValueError(f"rate_in and rate_out must be positive, got {rate_in!r} and {rate_out!r}")
        if fo < fi:
            raise ValueError(f"rate_out {fo} lies below rate_in {fi}: frames are interpolated, never dropped")
        ratio = fi / fo
        return ratio.numerator, ratio.denominator

    @staticmethod
    def _resample_args(depth, method):
        if isinstance(depth, bool) or not isinstance(depth, int) or not 1 <= depth <= _lib.RESAMPLE_MAX_DEPTH:
            raise ValueError(f"resample_depth must be an integer in 1..{_lib.RESAMPLE_MAX_DEPTH} (the dyadic tree has 2^depth - 1 nodes per pair)")
        if method not in ("nearest", "blend"):
            raise ValueError("resample_method must be 'nearest' (the closest node) or 'blend' (the two nodes around the output time, mixed)")
        return depth, method

    @staticmethod
    def resample_span(P: int, Q: int, depth: int, method: str, lo: int, hi: int):
        """The outputs ``(k, s, j0, j1, w)`` whose pair index ``s = k P / Q`` lies in ``[lo, hi)``, in order (``ResamplePlan.outputs``).  The
        grid is global: a span needs neither the clip's length nor the spans before it."""
        G, outs = 1 << depth, []
        for k in range(-((-lo * Q) // P), -((-hi * Q) // P)):      # ceil(lo Q / P) .. ceil(hi Q / P) - 1
            s = (k * P) // Q
            r = k * P - s * Q
            if method == "nearest":
                j = (2 * r * G + Q) // (2 * Q)
                outs.append((k, s, j, j, 0))
            else:
                j0 = (r * G) // Q
                w = (256 * (r * G - j0 * Q) + Q // 2) // Q
                outs.append((k, s, j0 + 1, j0 + 1, 0) if w == 256 else (k, s, j0, j0, 0) if w == 0 else (k, s, j0, j0 + 1, w))
        return outs

    @staticmethod
    def resample_needed(nodes, depth: int):
        """The nodes to compute for a pair whose outputs use ``nodes``: those in 1..G-1, closed under parents (``j -+ (j & -j)``), by level -
        ``levels[l]`` holds the needed nodes ``j`` with ``j & -j == G >> (l + 1)``, ascending."""
        G, need, todo = 1 << depth, set(), [j for j in nodes if 0 < j < (1 << depth)]
        while todo:
            j = todo.pop()
            if j not in need:
                need.add(j)
                todo += [p for p in (j - (j & -j), j + (j & -j)) if 0 < p < G]
        return [sorted(j for j in need if j & -j == G >> (l + 1)) for l in range(depth)]

    @staticmethod
    def resample_plan(n_frames: int, rate_in, rate_out, depth: int = 3, method: str = "nearest", rank: int = 0, world: int = 1) -> ResamplePlan:
        """What ``run(frames, rank, world)`` yields in mode "resample", symbolically and in order, and what it computes: a ``ResamplePlan``.
        A rank emits the outputs whose pair lies in its contiguous slice of the ``n_frames - 1`` pairs (``dist.shard_range``); the last rank
        also emits the output that falls on the last frame, if there is one.  Pure host logic (no device needed)."""
        from .dist import shard_range
        P, Q = FrameInterpolator.resample_ratio(rate_in, rate_out)
        depth, method = FrameInterpolator._resample_args(depth, method)
        if n_frames <= 0:
            return ResamplePlan([], {}, P, Q, 1 << depth)
        a, b = shard_range(n_frames - 1, rank, world)
        outs = FrameInterpolator.resample_span(P, Q, depth, method, a, b)
        pairs = {s: FrameInterpolator.resample_needed({j for _, s2, j0, j1, _ in outs if s2 == s for j in (j0, j1)}, depth) for s in range(a, b)}
        if rank == world - 1 and ((n_frames - 1) * Q) % P == 0:
            outs.append((((n_frames - 1) * Q) // P, n_frames - 1, 0, 0, 0))
        return ResamplePlan(outs, pairs, P, Q, 1 << depth)

    # ---- motion blur (include/emavfi.h, "SHUTTER DEFINITION"): the taps of an exposure window, pure host logic over integers
    @staticmethod
    def _exposure(shutter):
        """(n, d, degrees): e = shutter / 360 = n / d in lowest terms.  An int, a Fraction, a string Fraction accepts ("172.8", "1080/7") or
        a float, taken at its shortest decimal form."""
        try:
            if isinstance(shutter, bool):
                raise TypeError
            deg = Fraction(str(shutter)) if isinstance(shutter, float) else Fraction(shutter)
        except (TypeError, ValueError, ZeroDivisionError):
            raise ValueError(f"shutter must be an angle in degrees (180, 172.8, '1080/7', Fraction(1080, 7)), got {shutter!r}") from None
        if not 0 < deg <= 360:
            raise ValueError(f"shutter {deg} lies outside (0, 360] degrees")
        return (deg / 360).numerator, (deg / 360).denominator, deg

    @staticmethod
    def shutter_taps(Q: int, depth: int, shutter, r: int):
        """``[(j, w)]``: the nodes of a pair's tree of depth ``depth`` inside the exposure window of its output ``r`` (0 .. Q - 1) at the
        rate ratio ``Q`` and the angle ``shutter``, with their reduced integer weights, ascending in ``j``.  ValueError where the definition
        refuses: an exposure shorter than one node spacing, weights that sum to more than 65535."""
        n, d, deg = FrameInterpolator._exposure(shutter)
        depth, _ = FrameInterpolator._resample_args(depth, "nearest")
        if any(isinstance(v, bool) or not isinstance(v, int) for v in (Q, r)) or Q < 1 or not 0 <= r < Q:
            raise ValueError(f"shutter_taps: integers Q >= 1 and 0 <= r < Q expected, got Q = {Q!r}, r = {r!r}")
        G = 1 << depth
        if G * n < Q * d:
            raise ValueError(f"shutter {deg} at rate ratio {Q}: the exposure of {Fraction(n, d * Q)} of a source interval is shorter than one "
                             f"node spacing 1/{G}; raise resample_depth")
        lo, half = 2 * G * d * r, Q * d
        hi = lo + 2 * G * n
        taps = [(j, min(2 * j * half + half, hi) - max(2 * j * half - half, lo)) for j in range(G + 1)]
        taps = [(j, w) for j, w in taps if w > 0]
        g = 0
        for _, w in taps:
            g = gcd(g, w)
        taps = [(j, w // g) for j, w in taps]
        if sum(w for _, w in taps) > _lib.ACCUMULATE_MAX_SUM:
            raise ValueError(f"shutter {deg} at rate ratio {Q} and depth {depth}: the weights sum to {sum(w for _, w in taps)}, above "
                             f"{_lib.ACCUMULATE_MAX_SUM}; use an angle with a smaller denominator")
        return taps

    @staticmethod
    def shutter_plan(n_frames: int, rate_in, rate_out, depth: int = 3, shutter=180, rank: int = 0, world: int = 1) -> ShutterPlan:
        """What ``run(frames, rank, world)`` yields in mode "resample" under a shutter, symbolically and in order, and what it computes: a
        ``ShutterPlan``.  Ranks share the pairs as in ``resample_plan``: windows never leave their pair.  Pure host logic (no device needed)."""
        from .dist import shard_range
        P, Q = FrameInterpolator.resample_ratio(rate_in, rate_out)
        if P != 1:
            raise ValueError(f"shutter_plan: rate_in / rate_out = {P}/{Q}: rate_out must be an integer multiple of rate_in (P > 1 is not supported)")
        taps = [tuple(FrameInterpolator.shutter_taps(Q, depth, shutter, r)) for r in range(Q)]
        if n_frames <= 0:
            return ShutterPlan([], {}, Q, 1 << depth)
        a, b = shard_range(n_frames - 1, rank, world)
        outs = [(s * Q + r, s, taps[r]) for s in range(a, b) for r in range(Q)]
        levels = FrameInterpolator.resample_needed({j for t in taps for j, _ in t}, depth)
        if rank == world - 1:
            outs.append(((n_frames - 1) * Q, n_frames - 1, ((0, 1),)))
        return ShutterPlan(outs, {s: levels for s in range(a, b)}, Q, 1 << depth)

    # ---- duplicate frames (include/emavfi.h, "DUPLICATE FRAME DEFINITION", Schedule): pure host logic over integers
    @staticmethod
    def _dedup_args(max_run, span, depth=None):
        for name, v in (("dedup_max_run", max_run), ("dedup_span", span)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1")
        if depth is not None and depth + max_run.bit_length() > _lib.RESAMPLE_MAX_DEPTH:
            raise ValueError(f"resample_depth {depth} with dedup_max_run {max_run}: a gap of {max_run + 1} intervals needs a tree of depth "
                             f"{depth + max_run.bit_length()}, above the deepest one ({_lib.RESAMPLE_MAX_DEPTH}); lower either")
        return max_run, span

    @staticmethod
    def dedup_kept(flags, n_frames: int, base: int = 0, max_run: int = 3, span: int = 64):
        """The kept frames (local indices, ascending) of ``n_frames`` source frames whose first has the global index ``base``:
        ``flags[t - 1]`` says that the pair ``(t - 1, t)`` was flagged as duplicates.  Frame ``t`` is dropped when its pair is flagged, unless it
        is frame 0, the last frame, a frame with ``(base + t) % span == 0``, or the frame that follows ``max_run`` dropped frames in a row."""
        max_run, span = FrameInterpolator._dedup_args(max_run, span)
        flags, n = [bool(f) for f in flags], int(n_frames)
        if n < 0 or base < 0 or len(flags) != max(n - 1, 0):
            raise ValueError(f"dedup_kept: {n} frames have {max(n - 1, 0)} pairs, got {len(flags)} flags (n_frames >= 0, base >= 0)")
        kept, run = [], 0
        for t in range(n):
            if t == 0 or t == n - 1 or (base + t) % span == 0 or run >= max_run or not flags[t - 1]:
                kept.append(t)
                run = 0
            else:
                run += 1
        return kept

    @staticmethod
    def resample_gap(P: int, Q: int, depth: int, method: str, t0: int, t1: int):
        """The outputs ``(k, t0, m, j0, j1, w)`` served from the gap of ``m = t1 - t0`` source intervals between the kept frames ``t0 < t1``
        (global indices): those with ``t0 <= k P / Q < t1``, at ``R = k P - t0 Q`` over ``m Q`` in a tree of depth ``depth + ceil(log2 m)``.
        With ``m`` = 1 these are ``resample_span``'s."""
        m = t1 - t0
        G, den, outs = 1 << (depth + (m - 1).bit_length()), m * Q, []
        for k in range(-((-t0 * Q) // P), -((-t1 * Q) // P)):      # ceil(t0 Q / P) .. ceil(t1 Q / P) - 1
            R = k * P - t0 * Q
            if method == "nearest":
                j = (2 * R * G + den) // (2 * den)
                outs.append((k, t0, m, j, j, 0))
            else:
                j0 = (R * G) // den
                w = (256 * (R * G - j0 * den) + den // 2) // den
                outs.append((k, t0, m, j0 + 1, j0 + 1, 0) if w == 256 else (k, t0, m, j0, j0, 0) if w == 0 else (k, t0, m, j0, j0 + 1, w))
        return outs

    @staticmethod
    def resample_plan_dedup(kept, rate_in, rate_out, depth: int = 3, method: str = "nearest", base: int = 0, tail: bool = True) -> DedupPlan:
        """What ``run(frames)`` yields in mode "resample" once the frames outside ``kept`` (``dedup_kept``: local indices, the first frame has
        the global index ``base``) are dropped, symbolically and in order, and what it computes: a ``DedupPlan`` on the global grid.  The
        output count and times are ``resample_plan``'s; ``tail``: the output that falls on the last kept frame, if there is one, is part of
        the plan (``run_chunked`` emits it with the final chunk only).  Pure host logic (no device needed)."""
        P, Q = FrameInterpolator.resample_ratio(rate_in, rate_out)
        depth, method = FrameInterpolator._resample_args(depth, method)
        kept = [int(t) for t in kept]
        if base < 0 or any(t < 0 for t in kept[:1]) or any(b <= a for a, b in zip(kept, kept[1:])):
            raise ValueError("resample_plan_dedup: kept must be ascending frame indices >= 0, base >= 0")
        outs, gaps = [], {}
        for t0, t1 in zip(kept, kept[1:]):
            dm = depth + (t1 - t0 - 1).bit_length()
            if dm > _lib.RESAMPLE_MAX_DEPTH:
                raise ValueError(f"resample_plan_dedup: the gap ({t0}, {t1}) needs a tree of depth {dm}, above the deepest one "
                                 f"({_lib.RESAMPLE_MAX_DEPTH}): lower depth or dedup_max_run")
            mine = FrameInterpolator.resample_gap(P, Q, depth, method, base + t0, base + t1)
            outs += mine
            gaps[base + t0] = (t1 - t0, FrameInterpolator.resample_needed({j for o in mine for j in o[3:5]}, dm))
        if tail and kept and ((base + kept[-1]) * Q) % P == 0:
            outs.append((((base + kept[-1]) * Q) // P, base + kept[-1], 1, 0, 0, 0))
        return DedupPlan(outs, gaps, P, Q, depth)

    # ---- segment sharding (BASELINE configs[4]): one process per GPU, each with a contiguous
    # run of the stream's frame pairs.  No exchange between ranks: a pair's two frames are all a forward needs.
    @staticmethod
    def segment(n_frames: int, frame_interval: int, rank: int = 0, world: int = 1):
        """Rank ``rank``'s share of a stream of ``n_frames`` frames: ``(pairs, lo, hi, tail)``.

        ``pairs``: its contiguous slice of ``schedule()``'s pair list (sizes differ by at most one, earlier ranks take
        the remainder: ``dist.shard_range``); ``[lo, hi)``: the frame indices it has to read - with ``frame_interval`` 1 its
        last frame is the next rank's first (segment boundaries share one frame); ``tail``: it writes the stream's final
        frame (the highest rank does, also when it owns no pair).  Concatenating the ranks' outputs in rank order gives
        exactly the single-process sequence (``tests/test_stream.py``)."""
        from .dist import shard_range
        pairs, last, _ = FrameInterpolator.schedule(n_frames, frame_interval)
        a, b = shard_range(len(pairs), rank, world)
        mine = pairs[a:b]
        tail = last is not None and rank == world - 1
        need = [f for p in mine for f in p] + ([last] if tail else [])
        return mine, (min(need) if need else 0), (max(need) + 1 if need else 0), tail

    @staticmethod
    def emission_plan(n_frames: int, interpolation_factor: int, frame_interval: int, rank: int = 0, world: int = 1,
                      reference_quirks: bool = True):
        """What ``run(frames, rank, world)`` yields, symbolically and in order: ("pred", i1, i2, j) - prediction j of the
        pair (identical for every j in reference mode) -, ("src", i1) - the earlier frame of the pair, round-tripped when
        ``reference_quirks`` -, ("tail", index, roundtrip).  Pure host logic (no device needed)."""
        mine, _, _, tail = FrameInterpolator.segment(n_frames, frame_interval, rank, world)
        _, last, last_roundtrip = FrameInterpolator.schedule(n_frames, frame_interval)
        plan = []
        for i1, i2 in mine:
            plan += [("pred", i1, i2, j) for j in range(interpolation_factor)]
            plan.append(("src", i1))
        if tail:
            plan.append(("tail", last, bool(last_roundtrip and reference_quirks)))
        return plan

    @staticmethod
    def evaluation_plan(n_frames: int, every: int = 1, rank: int = 0, world: int = 1):
        """What ``evaluate(frames, every, rank, world)`` scores, in order: ``(t, t - 1, t + 1)`` - target ``t`` interpolated from its two
        neighbours - for this rank's contiguous share (``dist.shard_range``) of the targets ``t = 1, 1 + every, ...`` with ``t <= n_frames - 2``.
        Concatenating the ranks' plans in rank order gives the single-process plan.  Pure host logic (no device needed)."""
        from .dist import shard_range
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError("evaluate: every must be an integer >= 1")
        if n_frames < 0:
            raise ValueError("evaluate: n_frames must be >= 0")
        targets = list(range(1, n_frames - 1, every))
        a, b = shard_range(len(targets), rank, world)
        return [(t, t - 1, t + 1) for t in targets[a:b]]

    # ---- buffers: two slots of pinned host memory the kernels read / write in place, the preprocessed frames of a slot in HBM
    def _alloc(self, shape, per=2):
        """`per`: staged frames per item of a batch - 2 for run()'s pairs, 3 for evaluate()'s (earlier, target, later); buffers made for
        evaluate() also serve run()"""
        if self._shape == shape and self._per >= per:
            return
        self._per = per
        Hs, Ws, C = self.fmt.geometry(shape)
        fin = tuple(shape)                               # the bytes of a frame as it arrives: [Hs, Ws, C] or [Hs*3/2, Ws (* 2)]
        H, W = self.output_size(Hs, Ws, self.scale, self.size, self.fmt.name)
        self._dst = (H, W)
        fs = self.fmt.byte_shape(H, W)                   # and as it leaves, at the size the model runs at
        nb, nout = self.batch_pairs, max(self.factor if self.mode == "recursive" else 1, 1)
        self._shape = shape
        self._slots = []
        for _ in range(2):
            if self._bound():
                # pinned and first touched on a thread of the device's node (on the hosts measured the runtime already put pinned
                # pages on the GPU's node whichever CPU asked: profiles/r09_numa_stream_ab.md)
                pinned = self._copy_pool().submit(self._pinned_local, [(per * nb, *fin), (nb * nout, *fs), (nb, *fs)]).result()
            else:
                pinned = [torch.empty(per * nb, *fin, dtype=torch.uint8).pin_memory(),
                          torch.empty(nb * nout, *fs, dtype=torch.uint8).pin_memory(),
                          torch.empty(nb, *fs, dtype=torch.uint8).pin_memory()]
            self._slots.append({
                "h_in": pinned[0], "h_pred": pinned[1], "h_src": pinned[2],
                "x": torch.empty(per * nb, C, H, W, dtype=torch.float32, device=self.device),
                # device-side images of the three pinned buffers (the SDMA copies' other end)
                "d_in": torch.empty(per * nb, *fin, dtype=torch.uint8, device=self.device),
                # the resized bytes of the slot's frames, where frames leave as they arrived (reference_quirks=False) and arrive at another size
                "d_rs": torch.empty(per * nb, *fs, dtype=torch.uint8, device=self.device) if self._resize and not self.quirks else None,
                # without a fused resize frames are resized into a buffer of their own ahead of the preprocess kernel: this one where neither d_rs nor e_rs serves
                "p_rs": torch.empty(per * nb, *fs, dtype=torch.uint8, device=self.device) if not self.fmt.fused_resize and self._resize and self.quirks else None,
                "d_pred": torch.empty(nb * nout, *fs, dtype=torch.uint8, device=self.device),
                "d_src": torch.empty(nb, *fs, dtype=torch.uint8, device=self.device),
                # consumed: the preprocess kernel has read h_in (the host may restage it); pre: x is ready; fwd: the forward has read x
                # and written its predictions; done: the postprocess kernels have written h_pred / h_src (the host may drain them)
                "consumed": torch.cuda.Event(), "pre": torch.cuda.Event(), "fwd": torch.cuda.Event(), "done": torch.cuda.Event(),
                "src": torch.cuda.Event(),
            })
            if per > 2:
                # evaluate(): the resized bytes of the staged frames whatever reference_quirks says (the ground truth at the size the model
                # runs at), and the metric words {sse, ssimq} per target and channel, on the device and pinned
                mc = 1 if self.fmt.yuv else C
                self._slots[-1].update({"e_rs": torch.empty(per * nb, *fs, dtype=torch.uint8, device=self.device) if self._resize else None,
                                        "met": torch.zeros(nb, mc, 2, dtype=torch.int64, device=self.device),
                                        "h_met": torch.zeros(nb, mc, 2, dtype=torch.int64).pin_memory()})
            if self.static_guard is not None:
                # core pixel counts of the slot's prediction frames, on the device and pinned
                self._slots[-1].update({"sg": torch.zeros(nb * nout, dtype=torch.int32, device=self.device),
                                        "h_sg": torch.zeros(nb * nout, dtype=torch.int32).pin_memory()})
            if self.agreement is not None:
                # held pixel counts of the slot's predictions, pinned (the device side is the model's own tensor per forward)
                self._slots[-1]["h_ag"] = torch.zeros(nb * nout, dtype=torch.int32).pin_memory()
            if self.scene is not None:
                # signatures of the slot's staged frames; flags (row 0) and scores (row 1) of its pairs, on the device and pinned
                self._slots[-1].update({"sig": torch.empty(per * nb, _lib.SCENE_SIG_WORDS, dtype=torch.int32, device=self.device),
                                        "fs": torch.zeros(2, nb, dtype=torch.int32, device=self.device),
                                        "h_fs": torch.zeros(2, nb, dtype=torch.int32).pin_memory()})
        self._scene_units = _lib.scene_threshold_units(self.scene, Hs, Ws) if self.scene is not None else None
        # high-priority lanes: a 9-frame preprocess needs < 1 % of the CUs' time, the priority gets its workgroups dispatched between
        # those of the compute kernels (torch: lower number = higher priority)
        self._pre = _lib.side_stream(self.device, which=2, priority=-1)
        self._post = _lib.side_stream(self.device, which=3, priority=-1)

    # ---- the two device kernels of a frame format: uint8 frames (a slot buffer's rows, device or pinned) <-> normalised fp32 NCHW
    def _resize_planes(self, src, dst, device=None):
        """the planes of the byte frames `src` resized into those of `dst`, each as an image of its own (4:2:0 chroma to H/2 x W/2)"""
        for a, b in zip(self.fmt.planes(src), self.fmt.planes(dst)):
            a, b = (a, b) if a.dim() == 4 else (a.unsqueeze(-1), b.unsqueeze(-1))
            _lib.resize_u8(a, (b.shape[1], b.shape[2]), out=b, device=device)

    def _yuv_entry(self, which):
        """the format's lib function, `which` = "preprocess" or "postprocess" of nv12, p010 or yuv420p, and the colour arguments that follow
        its planes or its fp32 frames: the depth where the function takes one, the standard and the range"""
        family = self.fmt.family
        return getattr(_lib, which + "_" + family), (*(() if family == "nv12" else (self.fmt.depth,)), self.yuv["standard"], self.yuv["full_range"])

    def _cropped(self, luma, *chroma):
        """the planes of whole frames - [n,H,W(,C)], 4:2:0 chroma [n,H/2,W/2(,2)] - cut to the active rectangle in force: views, whose
        pitches the kernels take from .stride(); no rectangle in force: the planes as they are"""
        if self._act is None:
            return (luma, *chroma)
        t, l, h, w = self._act
        return (luma[:, t:t + h, l:l + w], *(c[:, t // 2:(t + h) // 2, l // 2:(l + w) // 2] for c in chroma))

    def _x(self, slot, n):
        """the normalised frames of a slot's first n staged frames: fp32 [n,C,H,W], or with an active rectangle in force [n,C,h,w] at the
        front of the same storage"""
        if self._act is None:
            return slot["x"][:n]
        C, (_, _, h, w) = slot["x"].shape[1], self._act
        return slot["x"].view(-1)[:n * C * h * w].view(n, C, h, w)

    def _set_active(self, rect):
        """puts `rect` = (top, left, height, width) in force for the frames the slots were made for; a rectangle that is the frame is the
        plain path"""
        H, W = self._dst
        rect = tuple(int(v) for v in rect)
        self.active_rect, self.active_share = rect, rect[2] * rect[3] / float(H * W)
        self._act = None if rect == (0, 0, H, W) else rect

    def _bars(self, dst, srcs, table):
        """on the post lane: frame k of `dst` (whole frames whose rectangle the post kernel has just written) receives the samples outside
        the rectangle of frame table[k] of `srcs`, the source frames as staged"""
        if self._act is not None and len(table):
            layout, C, sb, _, _ = self.fmt.frame_format
            _lib.fill_outside_frames(dst[:len(table)], srcs, table, self._dst, self._act, layout=layout, C=C, sample_bytes=sb)

    def _pre_kernel(self, buf, out=None, device=None, resized=None):
        """`resized`: with scale / size, a buffer of frames at the destination size that also receives the resized bytes (planar frames
        are resized into it first: without one, a fresh buffer is made).  With an active rectangle in force the kernels read views of it."""
        fmt, size = self.fmt, self._dst if self._resize else None
        if size is not None and not fmt.fused_resize:
            if resized is None:
                resized = torch.empty(buf.shape[0], *fmt.byte_shape(*size), dtype=torch.uint8, device=device if device is not None else buf.device)
            self._resize_planes(buf, resized, device)
            buf, size = resized, None
        planes = self._cropped(*fmt.planes(buf))
        if not fmt.yuv:
            # bgr24 has two entries: the dense one, which also resizes, and under an active rectangle the pitched one
            if self._act is not None:
                return _lib.preprocess_u8_pitched(*planes, device=device, out=out)
            return _lib.preprocess_u8(buf, device=device, out=out, size=size, resized_out=resized)
        # NV12's fused resize: the one 4:2:0 entry that takes a size
        fused = {"size": size, "resized_out": fmt.planes(resized) if resized is not None else None} if size is not None else {}
        entry, colour = self._yuv_entry("preprocess")
        return entry(*planes, *colour, device=device, out=out, **fused)

    # ---- scene cuts (include/emavfi.h, "SCENE CUT DEFINITION"): signatures and flags on the pre lane, the hold on the post lane
    @staticmethod
    def _run(buf, idx):
        """buf[idx] as ONE strided view when idx is an arithmetic run with a positive step, else None"""
        step = idx[1] - idx[0] if len(idx) > 1 else 1
        if step < 1 or any(idx[k + 1] - idx[k] != step for k in range(len(idx) - 1)):
            return None
        return buf[idx[0]:idx[-1] + 1:step]

    def _scene_decide(self, slot, buf, ia, ib):
        """signatures of the staged frames `buf` (source size; NV12: the Y plane as a 1-channel image of pitch W), then every pair's flag and score"""
        n, sig = len(ia), slot["sig"][:buf.shape[0]]
        img = self.fmt.luma(buf)
        _lib.luma_signature_u8(img, out=sig, device=self.device)
        size = (img.shape[1], img.shape[2])
        a, b = self._run(sig, ia), self._run(sig, ib)
        if a is not None and b is not None:
            _lib.scene_flags(a, b, size, self._scene_units, flags=slot["fs"][0, :n], scores=slot["fs"][1, :n])
        else:
            for k in range(n):
                _lib.scene_flags(sig[ia[k]], sig[ib[k]], size, self._scene_units, flags=slot["fs"][0, k:k + 1], scores=slot["fs"][1, k:k + 1])

    def _scene_hold(self, slot, dst, alt_buf, idx, rep):
        """flagged pairs: frame alt_buf[idx[k]] over the `rep` frames of pair k in dst"""
        n, flags = len(idx), slot["fs"][0]
        alt = self._run(alt_buf, idx)
        if alt is not None:
            _lib.hold_frames_u8(dst[:n * rep], alt, flags[:n], rep)
        else:
            for k in range(n):
                _lib.hold_frames_u8(dst[k * rep:(k + 1) * rep], alt_buf[idx[k]:idx[k] + 1], flags[k:k + 1], rep)

    def _static_hold(self, slot, dst, srcs, table):
        """the static regions of the pairs `table` = [(a, b)] (rows of `srcs`, the source frames as emitted) held in the prediction frames
        `dst`; the core pixel counts follow the frames to the slot's pinned buffer"""
        n = len(table)
        if slot["sg"].shape[0] < n:     # mode "resample": a batch has as many node frames as its plan needs
            slot["sg"] = torch.zeros(n, dtype=torch.int32, device=self.device)
            slot["h_sg"] = torch.zeros(n, dtype=torch.int32).pin_memory()
        layout, C, sb, depth, shift = self.fmt.frame_format
        _lib.static_guard_frames(dst[:n], srcs, table, self._dst, layout=layout, C=C, sample_bytes=sb, depth=depth, shift=shift,
                                 radius=self.static_guard, tol=self.static_tol, counts=slot["sg"][:n])
        slot["h_sg"][:n].copy_(slot["sg"][:n], non_blocking=True)

    def _resized_bytes(self, frame):
        """one source frame (numpy) at the destination size, as the device resizes it"""
        src = torch.from_numpy(frame).unsqueeze(0).to(self.device)
        out = torch.empty(1, *self.fmt.byte_shape(*self._dst), dtype=torch.uint8, device=self.device)
        self._resize_planes(src, out)
        return out.cpu().numpy()[0]

    def _post_kernel(self, x, denormalize, out=None):
        """with an active rectangle in force `x` has its size and `out`, whole frames, is written inside it only"""
        if self._act is not None and out is None:
            raise ValueError("_post_kernel: with an active rectangle the frames to write into must be given")
        fmt = self.fmt
        if not fmt.yuv and self._act is None:     # bgr24 has two entries: this is the dense one, below the pitched one
            return _lib.postprocess_u8(x, denormalize=denormalize, out=out)
        if out is None:
            out = torch.empty(x.shape[0], *fmt.byte_shape(x.shape[2], x.shape[3]), dtype=torch.uint8, device=x.device)
        planes = self._cropped(*fmt.planes(out))
        if fmt.yuv:
            entry, colour = self._yuv_entry("postprocess")
            entry(x, *colour, denormalize=denormalize, out=planes)
        else:
            _lib.postprocess_u8_pitched(x, *planes, denormalize=denormalize)
        return out

    _pool = None
    _bound_pools = {}   # (node, cpus) -> a pool whose threads run on those CPUs only; the unbound pool above stays as it is

    def _bound(self):
        return self.numa is not None and self.numa["bind"]

    @staticmethod
    def _pinned_local(shapes):
        bufs = [torch.empty(s, dtype=torch.uint8, pin_memory=True) for s in shapes]
        for b in bufs:
            b.numpy().fill(0)     # first touch, on this (bound) thread
        return bufs

    @staticmethod
    def _bind_thread(cpus):
        os.sched_setaffinity(0, cpus)   # pid 0: the calling thread (a new pool worker), not the process

    def _copy_pool(self):
        cls = type(self)
        if self._bound():
            key = (self.numa["numa_node"], tuple(self.numa["cpus"]))
            pool = cls._bound_pools.get(key)
            if pool is None:
                from concurrent.futures import ThreadPoolExecutor
                pool = cls._bound_pools[key] = ThreadPoolExecutor(max_workers=8, thread_name_prefix=f"emavfi-stage-n{key[0]}",
                                                                  initializer=cls._bind_thread, initargs=(key[1],))
            return pool
        if cls._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            cls._pool = ThreadPoolExecutor(max_workers=8, thread_name_prefix="emavfi-stage")
        return cls._pool

    def _stage(self, slot, frames, chunk):
        """Copy the distinct frames of `chunk` into the slot's pinned input buffer.
        Returns (number of staged frames, positions of each pair's first / second frame); a chunk of triples: three position lists."""
        order, pos = [], {}
        for item in chunk:
            for f in item:
                if f not in pos:
                    pos[f] = len(order)
                    order.append(f)
        slot["consumed"].synchronize()    # the preprocess kernel of this slot's previous batch has read the buffer
        # plain single-threaded memcpy: a torch CPU copy_ fans out over the intra-op thread pool, which on a
        # CPU-share-limited box (more threads than granted cores) was seen to stall for 40-160 ms at a time
        h_in = slot["h_in"].numpy()
        if len(order) >= 4 and h_in[0].nbytes >= (1 << 20):
            # a few plain memcpy threads (numpy releases the GIL inside copyto): the FIRST batch's staging is the one piece of host work
            # nothing overlaps (2.5-5 ms for nine 720p frames on one thread = 4-6 % of a 64-pair run)
            list(self._copy_pool().map(lambda t: np.copyto(h_in[t[0]], frames[t[1]]), enumerate(order)))
        else:
            for i, f in enumerate(order):
                np.copyto(h_in[i], frames[f])
        # positions stay on the host: a device index tensor would be a synchronous pageable copy on the
        # main stream, i.e. the host would block behind the compute it has just enqueued
        return (len(order), *([pos[item[k]] for item in chunk] for k in range(len(chunk[0]))))

    @staticmethod
    def _rows(x, idx):
        """x[idx] without a device index tensor: a view when idx is a run of consecutive rows (the usual case:
        consecutive pairs share frames), otherwise a stack of row views.  The forward takes 16-byte aligned tensors
        (include/emavfi.h): where a frame is no multiple of four floats (C*H*W % 4 != 0, e.g. 23 x 37) a run that starts at
        an odd row lies off that boundary and is copied into a fresh (aligned) tensor instead."""
        if all(idx[k + 1] == idx[k] + 1 for k in range(len(idx) - 1)):
            rows = x[idx[0]:idx[0] + len(idx)]
            return rows if rows.data_ptr() % 16 == 0 else rows.clone()
        return torch.stack([x[i] for i in idx])

    def _forward(self, a, b):
        """One forward of the model, every mode's and evaluate()'s: under the harness's own `ensemble` and `border` where given - for this
        call alone, the model's attributes stay as they are -, else as the model's attributes say."""
        return self.model(a, b, **self._forward_kw)

    def _held(self):
        """under `agreement`: the held pixel counts of the forward just issued - int32 [n] on the device, that forward's own tensor"""
        return self.model.agreement_counts if self.agreement is not None else None

    def _moved(self):
        """under `align`: the records of the forward just issued - int32 [n, 4] on the device, that forward's own tensor"""
        return self.model.align_shifts if self.align is not None else None

    def _moved_to_host(self, slot, shifts):
        """on the post lane: the records follow the frames into the slot's pinned buffer, ahead of `done`"""
        n = shifts.shape[0]
        if slot.get("h_al") is None or slot["h_al"].shape[0] < n:
            slot["h_al"] = torch.zeros(n, 4, dtype=torch.int32).pin_memory()
        shifts.record_stream(self._post)
        slot["h_al"][:n].copy_(shifts, non_blocking=True)

    def _held_to_host(self, slot, counts):
        """on the post lane: the counts follow the frames into the slot's pinned buffer, ahead of `done`"""
        n = counts.shape[0]
        if slot["h_ag"].shape[0] < n:       # mode "resample": a batch has as many node frames as its plan needs
            slot["h_ag"] = torch.zeros(n, dtype=torch.int32).pin_memory()
        counts.record_stream(self._post)
        slot["h_ag"][:n].copy_(counts, non_blocking=True)

    def _norm_constants(self, device):
        """(mean, std) of the model's input as [1, 3, 1, 1] device tensors, created once: torch.tensor(..., device=) is a synchronous
        pageable copy, i.e. the host would block behind the forward it has just enqueued and stop staging / draining beside it."""
        if self._norm is None:
            self._norm = (torch.tensor(_lib.IMAGENET_MEAN, device=device).view(1, 3, 1, 1),
                          torch.tensor(_lib.IMAGENET_STD, device=device).view(1, 3, 1, 1))
        return self._norm

    # ---- what a run reports beside its frames; run_chunked accumulates these over its chunks
    _REPORTS = ("scene_cuts", "scene_scores", "duplicates", "dedup_scores", "static_share", "agreement_share", "align_shifts")

    def _reset_reports(self):
        for name in self._REPORTS:
            setattr(self, name, [])

    def _note_scenes(self, slot, chunk):
        """on the drain: the scores and flags of the batch's pairs, written behind the frames, ahead of `done`"""
        fs = slot["h_fs"].numpy()
        for k, (a, b) in enumerate(chunk):
            self.scene_scores.append((a, b, int(fs[1, k])))
            if fs[0, k]:
                self.scene_cuts.append((a, b, int(fs[1, k])))

    def _shares(self, counts, idx):
        """on the drain: the held pixel counts `counts[i]` (a slot's pinned buffer, written behind the frames, ahead of `done`) for i in
        `idx`, as shares of a frame at the size the model runs at"""
        counts, area = counts.numpy(), float(self._dst[0] * self._dst[1])
        return [int(counts[i]) / area for i in idx]     # of the whole frame, also where the forward saw the active rectangle only

    # ---- the three lanes: the one place that orders a slot's readers and writers across the streams and the host
    def _lane_in(self, slot, nup, upload=True):
        """The pre lane's prologue for a slot, under ``self._pre``.  The slot's x was last read by the forward of the batch two before
        (`fwd`), and its x, d_in and resized bytes by that batch's post lane - the round trip of the earlier frames, the guards and holds, the
        resample assembly, the metric kernel (`done`).  `upload`: the `nup` staged frames then travel pinned -> HBM by hipMemcpyAsync (SDMA),
        after which the host may restage h_in (`consumed`)."""
        self._pre.wait_event(slot["fwd"])
        self._pre.wait_event(slot["done"])
        if upload:
            slot["d_in"][:nup].copy_(slot["h_in"][:nup], non_blocking=True)
            slot["consumed"].record(self._pre)

    def _batches(self, frames, chunks, pre, forward, post, drain, upload=True, early=None):
        """The batch pipeline of run(), mode "resample" and evaluate(): owns the order across the lanes and the host, and nothing else.
        Per batch ``b`` (``slot``, ``chunk``, ``n`` items, ``nup`` staged frames, ``rows`` = _stage's position lists; a step leaves what
        the later steps of its batch need as further attributes of ``b``):
          pre lane        wait `fwd`, `done` (_lane_in; `upload`: and the SDMA copy) -> ``pre(b)`` -> record `pre` -> ``early(b)``: what
                          depends on the preprocess only and leaves from this lane, ahead of the forward
          caller's stream wait `pre` -> ``forward(b)`` -> record `fwd`
          post lane       wait `fwd` -> ``post(b)`` -> record `done`
          host            stage batch ci + 1 into the other slot, then wait for `done` of batch ci - 1 and yield from its ``drain(b)``
        in exactly that order: staging and draining overlap the compute just enqueued, and a slot is restaged only behind its `consumed`
        (_stage) and rewritten only behind the readers above."""
        if not chunks:
            return
        main = torch.cuda.current_stream(self.device)

        def drained(b):
            b.slot["done"].synchronize()           # this batch's bytes and words have been written into the pinned buffers
            return drain(b) or ()

        staged = self._stage(self._slots[0], frames, chunks[0])
        prev = None
        for ci, chunk in enumerate(chunks):
            b = SimpleNamespace(slot=self._slots[ci & 1], chunk=chunk, n=len(chunk), nup=staged[0], rows=staged[1:])
            with torch.cuda.stream(self._pre):
                self._lane_in(b.slot, b.nup, upload)
                pre(b)
                b.slot["pre"].record(self._pre)
                if early is not None:
                    early(b)
            main.wait_event(b.slot["pre"])
            forward(b)
            b.slot["fwd"].record(main)
            with torch.cuda.stream(self._post):
                self._post.wait_event(b.slot["fwd"])
                post(b)
                b.slot["done"].record(self._post)
            if ci + 1 < len(chunks):                  # host-side staging of the next batch overlaps this batch's compute
                staged = self._stage(self._slots[(ci + 1) & 1], frames, chunks[ci + 1])
            if prev is not None:                      # emit the previous batch (its slot is reused only after this)
                yield from drained(prev)
            prev = b
        yield from drained(prev)

    def _predict(self, x1, x2):
        """[n, k, 3, H, W] predictions per pair: k = 1 (reference mode) or `factor` recursive midpoints."""
        with torch.no_grad():
            if self.mode == "reference" or self.factor <= 1:
                out = self._forward(x1, x2).unsqueeze(1)
                self._ag, self._al = self._held(), self._moved()
                return out
            # the model consumes normalised frames and returns [0,1] images: re-normalise midpoints to recurse
            mean, std = self._norm_constants(x1.device)

            def rec(a, b, depth):
                m = (self._forward(a, b), self._held(), self._moved())
                if depth == 1:
                    return [m]
                mn = (m[0] - mean) / std
                return rec(a, mn, depth - 1) + [m] + rec(mn, b, depth - 1)

            levels = (self.factor + 1).bit_length() - 1
            mids = rec(x1, x2, levels)
            # [n, k] flattened: the counts in the order of the predictions
            self._ag = torch.stack([c for _, c, _ in mids], dim=1).reshape(-1) if self.agreement is not None else None
            self._al = torch.stack([s for _, _, s in mids], dim=1).reshape(-1, 4) if self.align is not None else None
            return torch.stack([m for m, _, _ in mids], dim=1)

    def _check_frames(self, frames, first, what):
        self.fmt.check_frames(frames.values(), first, f"FrameInterpolator.{what}")

    def run(self, frames, rank: int = 0, world: int = 1, *, _emit_tail: bool = True, _base: int = 0, _rect=None) -> Iterator[np.ndarray]:
        """Yields uint8 HWC frames (``pixel_format="nv12"``: uint8 [H*3/2, W] frames; ``"p010"`` / ``"p012"`` / ``"p016"``: uint16 [H*3/2, W]
        frames) in the order the reference's writer receives them.

        ``frames``: the whole stream - an iterable, or (sharded use) any object with ``len()`` and integer indexing, of which
        only this rank's segment ``[lo, hi)`` (``segment()``) is touched, e.g. a lazy video reader.  ``rank`` / ``world``:
        this process's share (one process per GPU); the default is the whole stream.

        ``mode="resample"``: the frames of the stream at ``rate_out`` in TEMPORAL order - a source frame before the in-between frames that
        follow it, not the reference's predictions-first order (``resample_plan``)."""
        if not (hasattr(frames, "__len__") and hasattr(frames, "__getitem__")):
            frames = list(frames)
        if self.active == "auto" and world != 1:
            raise ValueError("run: world > 1 with active_area='auto': a shard sees only its segment, and the ranks' rectangles would differ "
                             "(pass the rectangle explicitly)")
        if self.mode == "resample":
            if self.dedup is not None and world != 1:
                raise ValueError("run: world > 1 with dedup_threshold: a shard boundary is no anchor of the duplicate schedule (one process)")
            yield from self._run_resample(frames, rank, world, _emit_tail, _base, _rect)
            return
        n_total = len(frames)
        mine, lo, hi, tail = self.segment(n_total, self.interval, rank, world)
        pairs, last, last_roundtrip = self.schedule(n_total, self.interval)
        if last is None or (not mine and not tail):
            return
        pairs = mine
        frames = {i: np.ascontiguousarray(frames[i]) for i in range(lo, hi)}   # this rank's segment only
        first = frames[lo]
        self._check_frames(frames, first, "run")
        # from here on a frame is its bytes (of words: [H*3/2, 2 W]); `words` turns what is yielded back into samples (views: no copy)
        frames = {i: self.fmt.as_bytes(f) for i, f in frames.items()}
        first, words = frames[lo], self.fmt.as_samples
        self._alloc(first.shape)
        self._reset_reports()
        self.prepass_waits = 0
        if self.active is not None:
            # "auto": the size of the forwards depends on the bounds, so the host reads them before it plans (one wait per run() call)
            scan = self.active == "auto" and hi - 1 > lo and bool(pairs)
            self._active_setup(self._prepass(frames, lo, hi - 1, False, True)[2] if scan else None, _rect)
        # ramp-up: with three or more batches to come the FIRST one is half-size - the GPU starts after five staged frames instead of
        # nine, and (64 pairs at batch 8: 4 + 7 x 8 + 4) the last one's drain is half as long; every other batch is full.  Per-sample
        # results do not depend on the batch a pair travels in (tests/test_gpu_parity.py::test_forward_config2_batch16_256)
        bp = self.batch_pairs
        head = bp // 2 if (bp >= 2 and len(pairs) > 2 * bp) else 0
        chunks = ([pairs[:head]] if head else []) + [pairs[i:i + bp] for i in range(head, len(pairs), bp)]
        npred = self.factor if self.mode == "recursive" else 1

        def pre(b):
            slot, nup, (ia, ib) = b.slot, b.nup, b.rows
            b.rs = rs = slot["d_rs"][:nup] if slot["d_rs"] is not None else None
            rz = slot["p_rs"][:nup] if slot["p_rs"] is not None else rs   # where the preprocess leaves resized bytes; `rs`: they are emitted
            if self.zero_copy:
                b.x = self._pre_kernel(slot["h_in"][:nup], device=self.device, out=slot["x"][:nup], resized=rz)   # distinct frames, read over PCIe, normalised once
                if self.scene is not None:
                    self._scene_decide(slot, slot["h_in"][:nup], ia, ib)
                    if not self.quirks and rs is None:
                        # the bytes a held frame is made of are the staged input rows, which the host restages once `consumed` fires
                        for k in range(b.n):
                            slot["d_src"][k].copy_(slot["h_in"][ia[k]], non_blocking=True)
                slot["consumed"].record(self._pre)
            else:                                  # the staged frames are in d_in (the driver's upload)
                b.x = self._pre_kernel(slot["d_in"][:nup], out=self._x(slot, nup), resized=rz)          # distinct frames, normalised once
                if self.scene is not None:
                    self._scene_decide(slot, slot["d_in"][:nup], ia, ib)
            b.src_here = self.quirks and not self.zero_copy and all(ia[k + 1] == ia[k] + 1 for k in range(b.n - 1))

        def early(b):
            slot, n, ia = b.slot, b.n, b.rows[0]
            if b.rs is not None:
                # reference_quirks=False with a resize: every pair's earlier frame leaves as the preprocess kernel resized it
                for k in range(n):
                    slot["h_src"][k].copy_(b.rs[ia[k]], non_blocking=True)
                slot["src"].record(self._pre)
            if b.src_here:
                # the reference's round trip of every pair's earlier frame (inference.py:187-188) depends on the preprocess only:
                # it leaves from this lane, ahead of the forward, instead of queueing behind the predictions at the end of the batch
                self._post_kernel(b.x[ia[0]:ia[0] + n], True, out=slot["d_src"][:n])
                slot["h_src"][:n].copy_(slot["d_src"][:n], non_blocking=True)
                slot["src"].record(self._pre)

        def forward(b):
            b.x1, x2 = self._rows(b.x, b.rows[0]), self._rows(b.x, b.rows[1])
            b.pred = self._predict(b.x1, x2)                                  # [n, k, 3, H, W], on the caller's stream
            b.held = self._ag                                                 # int32 [n k] on the device, or None
            b.moved = self._al                                                # int32 [n k, 4] on the device, or None

        def post(b):
            slot, n, nup, (ia, ib), rs, x1 = b.slot, b.n, b.nup, b.rows, b.rs, b.x1
            flat = b.pred.reshape(-1, *b.pred.shape[2:])
            flat.record_stream(self._post)                                # allocated on the caller's stream, read on this one
            if b.held is not None:
                self._held_to_host(slot, b.held)
            if b.moved is not None:
                self._moved_to_host(slot, b.moved)
            if self.quirks and (x1.data_ptr() < slot["x"].data_ptr() or x1.data_ptr() >= slot["x"].data_ptr() + slot["x"].numel() * 4):
                x1.record_stream(self._post)                              # a gathered copy (non-consecutive rows), not a view of the slot
            if self.zero_copy:
                self._post_kernel(flat, self.quirks, out=slot["h_pred"][:n * npred])
                if self.quirks:
                    self._post_kernel(x1, True, out=slot["h_src"][:n])
            else:
                self._post_kernel(flat, self.quirks, out=slot["d_pred"][:n * npred])
                # with an active rectangle: the bars of the pair's earlier frame around every prediction, ahead of the guard and the hold
                self._bars(slot["d_pred"], slot["d_in"][:nup], [ia[k] for k in range(n) for _ in range(npred)])
                if self.static_guard is not None:
                    # every prediction of pair k against the pair's two source frames as emitted; d_in / d_rs are complete: the
                    # forward waited for the preprocess
                    self._static_hold(slot, slot["d_pred"], rs if rs is not None else slot["d_in"][:nup],
                                      [(ia[k], ib[k]) for k in range(n) for _ in range(npred)])
                if self.scene is None:
                    slot["h_pred"][:n * npred].copy_(slot["d_pred"][:n * npred], non_blocking=True)   # HBM -> pinned (SDMA)
                if self.quirks and not b.src_here:
                    self._post_kernel(x1, True, out=slot["d_src"][:n])
                    slot["h_src"][:n].copy_(slot["d_src"][:n], non_blocking=True)
                if b.src_here:
                    self._post.wait_event(slot["src"])                    # the drain's wait covers both lanes' writes into the pinned buffers
            if rs is not None:
                self._post.wait_event(slot["src"])
            if self.scene is not None:
                # every source of a held frame is complete here: d_src / h_src (this lane, or the `src` event above), d_rs and d_in (the
                # preprocess the forward waited for).  The prediction frames of a flagged pair become the bytes emitted as its earlier frame
                dst = slot["h_pred"] if self.zero_copy else slot["d_pred"]
                if self.quirks:
                    self._scene_hold(slot, dst, slot["h_src"] if self.zero_copy else slot["d_src"], list(range(n)), npred)
                elif rs is not None:
                    self._scene_hold(slot, dst, rs, ia, npred)
                elif self.zero_copy:
                    self._scene_hold(slot, dst, slot["d_src"], list(range(n)), npred)
                else:
                    self._scene_hold(slot, dst, slot["d_in"], ia, npred)
                if not self.zero_copy:
                    slot["h_pred"][:n * npred].copy_(slot["d_pred"][:n * npred], non_blocking=True)   # HBM -> pinned (SDMA), after the hold
                slot["h_fs"].copy_(slot["fs"], non_blocking=True)

        def drain(b):
            slot = b.slot
            pred_h, src_h = slot["h_pred"].numpy(), slot["h_src"].numpy()
            own = (lambda v: words(v).copy()) if self.copy_out else words
            if self.scene is not None:
                self._note_scenes(slot, b.chunk)
            sg = self._shares(slot["h_sg"], range(b.n * npred)) if self.static_guard is not None else None
            ag = self._shares(slot["h_ag"], range(b.n * npred)) if self.agreement is not None else None
            al = slot["h_al"].numpy() if self.align is not None else None
            for k, (a, _) in enumerate(b.chunk):
                for j in range(self.factor):
                    i = k * npred + j % npred     # reference mode: the pair's one prediction, `factor` times; recursive: its j-th midpoint
                    if sg is not None:
                        self.static_share.append(sg[i])
                    if ag is not None:
                        self.agreement_share.append(ag[i])
                    if al is not None:
                        self.align_shifts.append((int(al[i, 0]), int(al[i, 1])))
                    yield own(pred_h[i])
                yield own(src_h[k]) if (self.quirks or self._resize) else words(frames[a])

        yield from self._batches(frames, chunks, pre, forward, post, drain, upload=not self.zero_copy, early=early)
        if not tail or not _emit_tail:       # the stream's final frame belongs to the highest rank (run_chunked: to the last chunk)
            return
        if last_roundtrip and self.quirks:   # skip-branch ending: the reference writes the round-tripped frame
            src = torch.from_numpy(frames[last]).unsqueeze(0).to(self.device)
            yield words(self._post_kernel(self._pre_kernel(src), True).cpu().numpy()[0])
        else:
            yield self._resized_bytes(frames[last]) if self._resize else words(frames[last])

    # ---- mode "resample": forwards level by level over the pairs that need the node, nodes post-processed once, outputs assembled on the post lane
    def _resample_forwards(self, x, ia, ib, levels, depths):
        """levels[l] = [(pair of the batch, node)] of recursion level l + 1, in node-buffer order -> the model's output per non-empty level
        ([len(levels[l]), 3, H, W]); depths[k]: the depth of pair k's tree (a gap of m source intervals: D + ceil(log2 m)).  The recursion and
        the re-normalisation of a midpoint are ``_predict``'s."""
        outs, norm, held, moved = [], {}, [], []
        mean, std = self._norm_constants(x.device)

        def node(k, j):
            return x[ia[k]] if j == 0 else x[ib[k]] if j == 1 << depths[k] else norm[(k, j)]

        with torch.no_grad():
            for l, items in enumerate(levels):
                if not items:
                    break                    # a needed node has needed parents: below an empty level there is nothing
                step = [(1 << depths[k]) >> (l + 1) for k, _ in items]
                if l == 0:
                    x1, x2 = self._rows(x, [ia[k] for k, _ in items]), self._rows(x, [ib[k] for k, _ in items])
                else:
                    x1 = torch.stack([node(k, j - st) for (k, j), st in zip(items, step)])
                    x2 = torch.stack([node(k, j + st) for (k, j), st in zip(items, step)])
                m = self._forward(x1, x2)
                outs.append(m)
                held.append(self._held())
                moved.append(self._moved())
                if l + 1 < len(levels) and levels[l + 1]:
                    mn = (m - mean) / std
                    for i, item in enumerate(items):
                        norm[item] = mn[i]
        # the counts in node-buffer order, as the node frames are
        self._ag = torch.cat(held) if self.agreement is not None and held else None
        self._al = torch.cat(moved) if self.align is not None and moved else None
        return outs

    def _resample_batch(self, chunk, outs_of, ia, ib):
        """One batch's host-side schedule: (levels, table, n_nodes, depths).  `chunk`: its pairs (s, s + m) of kept frames, local frame indices
        (m = 1 unless duplicates were dropped between them); `outs_of[s]`: the outputs (R, j0, j1, w) - under a shutter (r, taps) - of pair s
        in order; ia / ib: the staged rows of each pair's frames.  A pair's tree has depth D + ceil(log2 m); the levels run to the deepest tree of the batch.  Node frames
        are numbered level by level, pair by pair - the order the forwards produce them in."""
        depths = [self.resample_depth + (s2 - s - 1).bit_length() for s, s2 in chunk]
        needed = [self.resample_needed({j for o in outs_of[s] for j in self._out_nodes(o)}, depths[k]) for k, (s, _) in enumerate(chunk)]
        levels = [[(k, j) for k in range(len(chunk)) if l < depths[k] for j in needed[k][l]] for l in range(max(depths))]
        index = {item: i for i, item in enumerate(item for lv in levels for item in lv)}
        table = []
        for k, (s, _) in enumerate(chunk):
            ref = lambda j: ia[k] if j == 0 else ib[k] if j == 1 << depths[k] else _lib.RESAMPLE_NODES | index[(k, j)]
            if self.shutter is not None:      # (taps, weights, f, h) of accumulate_frames: every output of a flagged pair is held, r = 0 too
                table += [([ref(j) for j, _ in taps], [w for _, w in taps], k + 1 if self.scene is not None else 0, ia[k])
                          for _, taps in outs_of[s]]
                continue
            for r, j0, j1, w in outs_of[s]:
                f = k + 1 if (self.scene is not None and r > 0) else 0
                if self.light is None:
                    table.append((ref(j0), ref(j1), w, f, ia[k]))
                elif w in (0, 256):           # in light a blend is an accumulate entry: the single tap, or ((a, b), (256 - w, w))
                    table.append(([ref(j1 if w else j0)], [256], f, ia[k]))
                else:
                    table.append(([ref(j0), ref(j1)], [256 - w, w], f, ia[k]))
        return levels, table, len(index), depths

    def _out_nodes(self, out):
        """the nodes an output of ``outs_of`` uses: (r, j0, j1, w), or under a shutter (r, taps)"""
        return [j for j, _ in out[1]] if self.shutter is not None else out[1:3]

    def _entry_nodes(self, entry):
        """the node frames a table entry names, in order: an entry of resample_frames, or under a shutter of accumulate_frames"""
        taps = entry[0] if self.shutter is not None or self.light is not None else entry[:2]
        return [t & ~_lib.RESAMPLE_NODES for t in taps if t & _lib.RESAMPLE_NODES]

    def _prepass(self, frames, lo, hi, dedup, active):
        """The pre-pass of a run() whose plan depends on the frames - dedup_threshold (`dedup`), active_area="auto" (`active`) or both:
        frames lo .. hi (hi > lo) go to the device in slot-sized batches (consecutive batches share one frame), every consecutive pair is
        scored and / or every frame's bounds are taken, and the words come back with ONE host wait whichever were asked for.  Returns
        (flags, scores, bounds): flags and scores of the pairs (lo, lo + 1) .. (hi - 1, hi), the bounds {top, bottom, left, right} of the frames
        lo .. hi; what was not asked for is None.  The frames cross PCIe here and again in the batch loop that follows."""
        n = hi - lo
        cap = self._slots[0]["d_in"].shape[0]                   # >= 2 frames
        dd = getattr(self, "_dd", None)
        if dd is None or dd["cap"] < cap or dd["fs"].shape[1] < n:
            size = max(n, dd["fs"].shape[1] if dd is not None else 0)
            dd = self._dd = {"cap": cap, "cells": torch.empty(cap - 1, _lib.SCENE_SIG_WORDS, dtype=torch.int32, device=self.device),
                             "fs": torch.zeros(2, size, dtype=torch.int32, device=self.device),
                             "h_fs": torch.zeros(2, size, dtype=torch.int32).pin_memory(),
                             "ab": torch.zeros(size + 1, 4, dtype=torch.int32, device=self.device),
                             "h_ab": torch.zeros(size + 1, 4, dtype=torch.int32).pin_memory(), "ready": torch.cuda.Event()}
        _, depth, shift = self.fmt.sample_format
        self._pre.wait_stream(torch.cuda.current_stream(self.device))     # buffers made on the caller's stream are used on the pre lane
        for bi, f0 in enumerate(range(lo, hi, cap - 1)):
            f1 = min(f0 + cap - 1, hi)
            nfr, slot = f1 - f0 + 1, self._slots[bi & 1]
            self._stage(slot, frames, [tuple(range(f0, f1 + 1))])           # waits until the slot's previous upload has been read
            with torch.cuda.stream(self._pre):
                self._lane_in(slot, nfr)
                img = self.fmt.luma(slot["d_in"][:nfr])    # as staged, at source size
                if dedup:
                    cells = _lib.frame_diff_cells(img[:-1], img[1:], depth=depth, shift=shift, out=dd["cells"][:nfr - 1])
                    _lib.duplicate_flags(cells, self.dedup, flags=dd["fs"][0, f0 - lo:f1 - lo], scores=dd["fs"][1, f0 - lo:f1 - lo])
                if active:                                                  # the shared frame of two batches is written twice, alike
                    _lib.active_bounds(img, self._active_level, depth=depth, shift=shift, out=dd["ab"][f0 - lo:f1 - lo + 1])
        with torch.cuda.stream(self._pre):
            if dedup:
                dd["h_fs"].copy_(dd["fs"], non_blocking=True)
            if active:
                dd["h_ab"].copy_(dd["ab"], non_blocking=True)
            dd["ready"].record(self._pre)
        dd["ready"].synchronize()                                         # the one host wait: the plan depends on these words
        self.prepass_waits += 1
        got, ab = dd["h_fs"].numpy(), dd["h_ab"].numpy()
        return ([int(v) for v in got[0, :n]] if dedup else None, [int(v) & 0xFFFFFFFF for v in got[1, :n]] if dedup else None,
                [tuple(int(v) & 0xFFFFFFFF for v in row) for row in ab[:n + 1]] if active else None)

    def _active_setup(self, bounds, carry):
        """Puts the rectangle of this run() in force: the explicit one, now validated against the frame, or under "auto" the rectangle of
        `bounds` (the pre-pass's; None: no pair to predict) joined with `carry`, the rectangle run_chunked carries from the chunks before."""
        H, W = self._dst
        if self.active != "auto":
            self._set_active(_lib.active_rect_check(self.active, H, W, "active_area"))
            return
        held = [(carry[0], carry[0] + carry[2], carry[1], carry[1] + carry[3])] if carry is not None else []
        self._set_active(_lib.active_rect(list(bounds or ()) + held, H, W))

    def _run_resample(self, frames, rank, world, emit_tail, base, rect=None):
        from .dist import shard_range
        n_total = len(frames)
        if n_total <= 0:
            return
        (P, Q), D, G = self._ratio, self.resample_depth, 1 << self.resample_depth
        a, b = shard_range(n_total - 1, rank, world)
        last = n_total - 1
        tail = emit_tail and rank == world - 1 and ((base + last) * Q) % P == 0     # an output falls on the last frame: r = 0, the frame itself
        if b <= a and not tail:
            return
        frames = {i: np.ascontiguousarray(frames[i]) for i in sorted(set(range(a, b + 1) if b > a else ()) | ({last} if tail else set()))}
        first = next(iter(frames.values()))
        self._check_frames(frames, first, "run")
        frames = {i: self.fmt.as_bytes(f) for i, f in frames.items()}
        first, words = next(iter(frames.values())), self.fmt.as_samples
        self._alloc(first.shape)
        self._reset_reports()
        kept = list(range(a, b + 1)) if b > a else []
        self.prepass_waits = 0
        flags = scores = bounds = None
        if b > a and (self.dedup is not None or self.active == "auto"):
            # the set of forwards depends on the flags, their size on the bounds: the host reads both before it plans (one wait per run() call)
            flags, scores, bounds = self._prepass(frames, a, b, self.dedup is not None, self.active == "auto")
        if self.active is not None:
            self._active_setup(bounds, rect)
        if flags is not None:
            kept = [a + t for t in self.dedup_kept(flags, b - a + 1, base + a, self.dedup_max_run, self.dedup_span)]
            self.dedup_scores = [(base + a + 1 + i, sc) for i, sc in enumerate(scores)]
            keep = set(kept)
            self.duplicates = [(base + t, scores[t - a - 1]) for t in range(a + 1, b + 1) if t not in keep]
        gaps = list(zip(kept, kept[1:]))          # without duplicates: the pairs (s, s + 1), and resample_gap is resample_span
        if self.shutter is not None:              # P = 1: every pair has the outputs r = 0 .. Q - 1, each (r, the taps of its window)
            outs_of = {t0: list(enumerate(self._taps)) for t0, _ in gaps}
        else:
            outs_of = {t0: [(k * P - (base + t0) * Q, j0, j1, w) for k, _, _, j0, j1, w in
                            self.resample_gap(P, Q, D, self.resample_method, base + t0, base + t1)] for t0, t1 in gaps}
        bp = self.batch_pairs
        chunks = [gaps[i:i + bp] for i in range(0, len(gaps), bp)]
        fmt = self.fmt.sample_format
        if chunks:
            # the node and emission buffers of a slot hold the largest batch of this run
            sizes = [(sum(len(outs_of[s]) for s, _ in c), sum(len(lv) for s, s2 in c for lv in self.resample_needed(
                {j for o in outs_of[s] for j in self._out_nodes(o)}, D + (s2 - s - 1).bit_length()))) for c in chunks]
            n_emit, n_node = max(o for o, _ in sizes), max(1, max(n for _, n in sizes))
            for slot in self._slots:
                fs = tuple(slot["d_src"].shape[1:])
                if "d_emit" not in slot or slot["d_emit"].shape[0] < n_emit or slot["d_node"].shape[0] < n_node:
                    slot.update({"d_node": torch.empty(n_node, *fs, dtype=torch.uint8, device=self.device),
                                 "d_emit": torch.empty(n_emit, *fs, dtype=torch.uint8, device=self.device),
                                 "h_emit": torch.empty(n_emit, *fs, dtype=torch.uint8).pin_memory()})

        def pre(b):
            slot, nup, (ia, ib) = b.slot, b.nup, b.rows
            b.levels, b.table, b.n_nodes, b.depths = self._resample_batch(b.chunk, outs_of, ia, ib)
            b.rs = slot["d_rs"][:nup] if slot["d_rs"] is not None else None
            b.x = self._pre_kernel(slot["d_in"][:nup], out=self._x(slot, nup), resized=b.rs)
            if self.scene is not None:
                self._scene_decide(slot, slot["d_in"][:nup], ia, ib)

        def forward(b):
            b.preds = self._resample_forwards(b.x, *b.rows, b.levels, b.depths)                       # on the caller's stream
            b.held = self._ag                                                                         # int32 [n_nodes] on the device, or None
            b.moved = self._al                                                                        # int32 [n_nodes, 4] on the device, or None

        def post(b):
            slot, nup, (ia, ib), rs, table = b.slot, b.nup, b.rows, b.rs, b.table
            if b.held is not None:
                self._held_to_host(slot, b.held)
            if b.moved is not None:
                self._moved_to_host(slot, b.moved)
            off = 0
            for m in b.preds:                                                                         # every node becomes bytes once
                m.record_stream(self._post)
                self._post_kernel(m, False, out=slot["d_node"][off:off + m.shape[0]])
                off += m.shape[0]
            assert off == b.n_nodes
            b.first_node = []
            gap_of = [k for lv in b.levels for k, _ in lv]
            # with an active rectangle: the bars of its gap's earlier kept frame around every node frame, ahead of the guard and the assembly
            self._bars(slot["d_node"], slot["d_in"][:nup], [ia[k] for k in gap_of])
            if self.static_guard is not None and off:
                # every node frame against its gap's two kept source frames, before the outputs are selected or blended
                self._static_hold(slot, slot["d_node"], rs if rs is not None else slot["d_in"][:nup], [(ia[k], ib[k]) for k in gap_of])
                first = {}
                for i, k in enumerate(gap_of):
                    first.setdefault(k, i)
                # an entry's last field is its gap's first staged row, ia[k]: distinct per gap
                b.first_node = [first[ia.index(e[-1])] for e in table if self._entry_nodes(e)]
            # the source frames as emitted: the staged bytes, or the bytes the preprocess kernel resized them to
            assemble = _lib.accumulate_frames if self.shutter is not None else _lib.resample_frames
            if self.light is not None:       # in light: the whole bgr24 frame, the Y plane (the first two thirds) of a 4:2:0 frame
                fb = slot["d_emit"][0].numel()
                assemble = functools.partial(_lib.accumulate_frames_linear, lin=self._lin,
                                             linear_bytes=self.fmt.luma_bytes(fb))
            assemble(slot["d_emit"][:len(table)], rs if rs is not None else slot["d_in"][:nup], slot["d_node"][:off] if off else None, table,
                     flags=slot["fs"][0] if self.scene is not None else None, sample_bytes=fmt[0], depth=fmt[1], shift=fmt[2])
            slot["h_emit"][:len(table)].copy_(slot["d_emit"][:len(table)], non_blocking=True)         # HBM -> pinned (SDMA)
            if self.scene is not None:
                slot["h_fs"].copy_(slot["fs"], non_blocking=True)

        def drain(b):
            slot = b.slot
            emit_h = slot["h_emit"].numpy()
            if self.agreement is not None:
                # an emitted frame made of node frames has the share of the first node frame its entry names
                self.agreement_share += self._shares(slot["h_ag"], [self._entry_nodes(e)[0] for e in b.table if self._entry_nodes(e)])
            if self.align is not None:
                # likewise: the shift of the first node frame its entry names
                named = [self._entry_nodes(e)[0] for e in b.table if self._entry_nodes(e)]
                al = slot["h_al"].numpy() if named else None           # a batch without a node issued no forward
                self.align_shifts += [(int(al[i, 0]), int(al[i, 1])) for i in named]
            if self.static_guard is not None:
                # an emitted frame made of node frames has its gap's share (core depends on the two sources only)
                self.static_share += self._shares(slot["h_sg"], b.first_node)
            own = (lambda v: words(v).copy()) if self.copy_out else words
            if self.scene is not None:
                self._note_scenes(slot, b.chunk)
            for i in range(len(b.table)):
                yield own(emit_h[i])

        yield from self._batches(frames, chunks, pre, forward, post, drain)
        if tail:
            yield self._resized_bytes(frames[last]) if self._resize else words(frames[last])

    @staticmethod
    def chunk_plan(n_frames: int, frame_interval: int, chunk_pairs: int = 64):
        """How ``run_chunked`` cuts a stream of ``n_frames`` frames: ``[(lo, hi, final)]`` - chunk c holds the global frames ``[lo, hi)`` =
        ``[c L, c L + L]`` with ``L = chunk_pairs * frame_interval`` (consecutive chunks share one frame; every chunk starts on a multiple of
        ``frame_interval``, which keeps the reference's ``frame_num % frame_interval`` phase), runs through ``run()`` on its own, and only the
        ``final`` one emits its tail frame.  A stream that ends on a chunk boundary has a final chunk of one frame: the tail alone.  Pure host
        logic (no device needed)."""
        if frame_interval < 1 or chunk_pairs < 1:
            raise ValueError("frame_interval >= 1 and chunk_pairs >= 1 required")
        L, lo, plan = chunk_pairs * frame_interval, 0, []
        while lo < n_frames:
            if lo + L + 1 <= n_frames:
                plan.append((lo, lo + L + 1, False))
                lo += L
            else:
                plan.append((lo, n_frames, True))
                break
        return plan

    def run_chunked(self, frames: Iterable[np.ndarray], chunk_pairs: int = 64) -> Iterator[np.ndarray]:
        """``run(list(frames))``, byte for byte, over any iterable - no ``len()``, so a pipe works - holding at most
        ``chunk_pairs * frame_interval + 1`` source frames: the stream is cut as ``chunk_plan`` says, each chunk goes through ``run()``,
        and the tail frame of every chunk but the last is neither yielded nor computed.  ``scene_cuts`` / ``scene_scores`` (and ``duplicates`` /
        ``dedup_scores``) accumulate over the chunks with global frame indices.  With ``dedup_threshold`` set, ``chunk_pairs`` must be a
        multiple of ``dedup_span``, and every chunk costs one host wait.  Single process: a stream of unknown length cannot be sharded over ranks.
        With an explicit ``active_area`` the yielded bytes are always ``run()``'s.  With ``active_area="auto"`` every chunk is scanned on its
        own (one host wait each, shared with ``dedup_threshold``'s) and its rectangle is joined with the one carried from the chunks before:
        the rectangle never shrinks, and content that first appears outside it lies inside the rectangle of its own chunk, so none is lost.
        The yielded bytes then equal ``run()``'s exactly when the first chunk already shows the final rectangle; ``active_rect`` /
        ``active_share`` are the last chunk's."""
        if isinstance(chunk_pairs, bool) or not isinstance(chunk_pairs, int) or chunk_pairs < 1:
            raise ValueError("run_chunked: chunk_pairs must be an integer >= 1")
        if self.dedup is not None and chunk_pairs % self.dedup_span:
            raise ValueError(f"run_chunked: chunk_pairs = {chunk_pairs} with dedup_threshold must be a multiple of dedup_span = {self.dedup_span}: "
                             "every chunk then starts and ends on a frame that is kept regardless, and sees what the whole clip would")
        L, it, held, lo = chunk_pairs * self.interval, iter(frames), [], 0
        carry, waits = None, 0
        total = {name: [] for name in self._REPORTS}
        self._reset_reports()
        while True:
            for f in it:
                held.append(f)
                if len(held) == L + 1:
                    break
            final = len(held) < L + 1          # the stream ended inside this chunk (a full chunk is never final: its last frame starts the next)
            if held:
                self._reset_reports()                           # this chunk's own, whatever run() does with them
                # mode "resample": the time grid is global, so a chunk is told where it starts
                # active_area="auto": the rectangle in force so far is joined with this chunk's, so it never shrinks
                yield from self.run(held, _emit_tail=final, **({"_base": lo} if self.mode == "resample" else {}),
                                    **({"_rect": carry} if self.active == "auto" else {}))
                carry, waits = self.active_rect, waits + self.prepass_waits
                self.prepass_waits = waits
                for name in self._REPORTS:
                    mine = getattr(self, name)
                    if name in ("scene_cuts", "scene_scores"):  # the chunk's own frame indices; duplicates / dedup_scores are global already
                        mine = [(a + lo, b + lo, sc) for a, b, sc in mine]
                    total[name] += mine
                    setattr(self, name, list(total[name]))
            if final:
                return
            held, lo = held[-1:], lo + L

    def evaluate(self, frames, every: int = 1, rank: int = 0, world: int = 1) -> Evaluation:
        """Scores the model on a clip by the held-out protocol and returns an ``Evaluation``: every target ``t = 1, 1 + every, ...`` with
        ``t <= n - 2`` is interpolated from frames ``t - 1`` and ``t + 1`` and compared with the true frame ``t`` (``evaluation_plan``).

        Everything is decided on the device.  The forwards are batched through ``run()``'s slots and lanes, by the same driver (``_batches``;
        ``batch_pairs`` targets per batch); the prediction is turned into bytes by the postprocess kernel with ``denormalize`` off - the
        model's output lies in [0, 1], and de-normalising it as ``reference_quirks`` does would score the reference's quirk instead of the
        model - and scored by ``emavfi_frame_metrics_u8`` against the bytes of frame ``t`` as they sit on the device at the size the
        model runs at (with ``scale`` / ``size``: the device-resized bytes).  ``pixel_format="nv12"``: the Y planes are scored as a
        one-channel image (PSNR-Y / SSIM-Y); chroma is not scored.  Only the metric words travel to a small pinned buffer, read after the
        ``done`` wait of the drain; no frame returns to the host.  The staged frames always reach the device by copy (``zero_copy`` is a
        property of ``run()``'s transport).  ``interpolation_factor``, ``mode``, ``reference_quirks``, ``frame_interval`` and
        ``scene_threshold`` do not affect ``evaluate``: a target has one midpoint and is never held.  ``static_guard`` does not either: the
        model's own prediction is scored, not the guarded frame.  ``agreement`` DOES: that guard is part of the forward, so the guarded
        prediction is what is scored (``agreement_share`` is ``run()``'s and is left alone here).

        ``frames`` / ``rank`` / ``world`` as for ``run()``: a rank touches only the frames of its contiguous share of the targets, and
        the ranks' ``targets`` concatenated in rank order are the single-process result."""
        if not self.fmt.byte_kernels:
            raise ValueError(f"evaluate() with pixel_format={self.fmt.name!r}: the metric kernel reads bytes (16-bit frames are not scored)")
        if self.active is not None:
            raise ValueError("evaluate() with active_area: a held-out frame is scored whole, and the bars would score as perfect (use a "
                             "harness without it)")
        if self.shutter is not None:
            raise ValueError("evaluate() with a shutter: a held-out frame is an instantaneous sample, an accumulated one is not comparable to it")
        if not (hasattr(frames, "__len__") and hasattr(frames, "__getitem__")):
            frames = list(frames)
        plan = self.evaluation_plan(len(frames), every, rank, world)
        if not plan:                               # fewer than three frames, or a rank without a share: nothing is touched, size (0, 0)
            return Evaluation((0, 0), 1 if self.fmt.yuv else 3)
        frames = {i: np.ascontiguousarray(frames[i]) for i in sorted({f for item in plan for f in item})}   # this rank's frames only
        first = frames[plan[0][1]]
        self._check_frames(frames, first, "evaluate")
        self._alloc(first.shape, per=3)
        H, W = self._dst
        result = Evaluation((H, W), 1 if self.fmt.yuv else first.shape[2])
        image = self.fmt.luma                     # the scored image of frames at the size the model runs at: of 4:2:0 frames the Y plane as one channel
        bp = self.batch_pairs
        chunks = [[(a, t, b) for t, a, b in plan[i:i + bp]] for i in range(0, len(plan), bp)]

        def pre(b):
            slot, nup = b.slot, b.nup
            b.rs = slot["e_rs"][:nup] if slot["e_rs"] is not None else None
            b.x = self._pre_kernel(slot["d_in"][:nup], out=slot["x"][:nup], resized=b.rs)

        def forward(b):
            with torch.no_grad():
                b.pred = self._forward(self._rows(b.x, b.rows[0]), self._rows(b.x, b.rows[2]))   # [n, 3, H, W], on the caller's stream

        def post(b):
            slot, n, it = b.slot, b.n, b.rows[1]
            b.pred.record_stream(self._post)
            self._post_kernel(b.pred, False, out=slot["d_pred"][:n])
            truth = image(b.rs if b.rs is not None else slot["d_in"][:b.nup])
            step = it[1] - it[0] if n > 1 else 1                          # the targets' rows are an arithmetic run: frames are staged in order
            _lib.frame_metrics_u8(image(slot["d_pred"][:n]), truth[it[0]:it[-1] + 1:step], out=slot["met"][:n])
            slot["h_met"][:n].copy_(slot["met"][:n], non_blocking=True)

        def drain(b):                             # only the metric words came back
            words = b.slot["h_met"].numpy()
            for k, (_, t, _) in enumerate(b.chunk):
                result.add(t, words[k].tolist())

        for _ in self._batches(frames, chunks, pre, forward, post, drain):
            pass
        return result
