"""``python -m emavfi IN.y4m OUT.y4m``: the reference's command line (inference.py) around the device-side harness.

A YUV4MPEG2 stream goes in, the interpolated stream comes out; ``-`` is stdin / stdout, so any video file reaches it through ffmpeg pipes
(INTEGRATION.md).  The pixel format comes from the stream's colour-space tag; frames travel through ``FrameInterpolator.run_chunked`` in
bounded memory, planar 4:2:0 all the way (``emavfi.y4m``).  Single process, single GPU.  ``--evaluate`` is the exception to the bound:
``FrameInterpolator.evaluate`` indexes its clip, so the whole clip is read into host memory first.

Defaults that DIFFER from inference.py, on purpose:
  * no resize: the reference halves every frame (``--scale 0.5``); here ``--scale`` / ``--size`` are opt-in;
  * ``reference_quirks`` off: the reference de-normalises a model output that is already in [0, 1];
    ``--reference-quirks`` brings that back.
"""
from __future__ import annotations

import argparse
import sys

from . import formats, y4m

_EPILOG = """defaults that differ from the reference's inference.py: frames are NOT resized (the reference halves them: pass --scale 0.5 for
that) and --reference-quirks is off (the reference de-normalises a model output that is already in [0, 1])."""


def _size(text):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("HxW expected, e.g. 360x640") from None
    return h, w


def _active_area(text):
    if text == "auto":
        return text
    try:
        t, l, h, w = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("auto or T,L,H,W expected, e.g. 88,0,544,1280") from None
    return t, l, h, w


def _rate(text):
    try:
        return y4m.parse_rate(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m emavfi", description="Interpolate a YUV4MPEG2 (.y4m) stream on an MI355X.", epilog=_EPILOG)
    p.add_argument("input", help="input .y4m ('-': stdin)")
    p.add_argument("output", nargs="?", help="output .y4m ('-': stdout); not needed with --evaluate")
    w = p.add_mutually_exclusive_group(required=True)
    w.add_argument("--weights", metavar="FILE", help="a state_dict with the reference's keys (torch.save)")
    w.add_argument("--synthetic-weights", metavar="SEED", type=int, help="deterministic synthetic weights (the reference ships none)")
    p.add_argument("--dtype", default="bf16", help="compute dtype of the forward (default: bf16)")
    p.add_argument("--mid-channels", type=int, default=64)
    p.add_argument("--target-fps", type=float, default=None, help="as in inference.py: factor = round(target / fps - 1)")
    p.add_argument("--max-interpolation-factor", type=int, default=4, help="without --target-fps: the factor in 1..MAX that brings the rate closest to 60")
    p.add_argument("--factor", type=int, default=None, help="the interpolation factor itself (overrides --target-fps)")
    p.add_argument("--frame-interval", type=int, default=1)
    p.add_argument("--mode", choices=("reference", "recursive"), default=None, help="default: reference")
    p.add_argument("--output-fps", type=_rate, default=None, metavar="RATE",
                   help="convert to exactly this frame rate (60, 59.94, 60000/1001 or 60000:1001; at least the stream's): frames in temporal "
                        "order, assembled from recursive midpoints; excludes --target-fps, --factor, --mode, --reference-quirks and a "
                        "--frame-interval other than 1")
    p.add_argument("--resample", choices=("nearest", "blend"), default="nearest",
                   help="with --output-fps: the closest midpoint (default), or the two around the output time mixed")
    p.add_argument("--resample-depth", type=int, default=3, metavar="D", help="with --output-fps: midpoints down to 1 / 2^D of a frame interval (1..5, default 3)")
    p.add_argument("--shutter", default=None, metavar="DEGREES",
                   help="with --output-fps at an integer multiple of the stream's rate (the rate itself included: blur is added, the rate "
                        "stays): motion blur - every output frame is the mean of the midpoints inside an exposure of DEGREES / 360 of its "
                        "frame period (180, 172.8 or 1080/7; at most 360), summed on the device; no quality claim is made; excludes "
                        "--resample blend, --dedup and --evaluate")
    p.add_argument("--light", choices=("srgb", "bt709", "hlg"), default=None,
                   help="with --shutter or --resample blend: mix the frames in linear light through this transfer function instead of "
                        "averaging the coded samples (of a Y'CbCr stream the luma plane only: a luma-linear approximation, exact for greys; "
                        "8-, 10- and 12-bit streams); Y4M carries no transfer tag, so there is no default")
    p.add_argument("--dedup", type=float, default=None, metavar="FRACTION",
                   help="with --output-fps: drop frames that copy the frame before them and interpolate across the gap; a frame is a copy when no "
                        "cell's mean absolute luma difference exceeds FRACTION of full scale (0: bit-identical luma only; no default is claimed)")
    p.add_argument("--dedup-max-run", type=int, default=None, metavar="N", help="with --dedup: at most N frames in a row are dropped (default 3)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--scale", type=float, default=None, help="resize every frame on the device (default: no resize; the reference: 0.5)")
    g.add_argument("--size", type=_size, default=None, metavar="HxW", help="resize every frame on the device to H x W")
    p.add_argument("--scene-threshold", type=float, default=None, help="hold the earlier frame across cuts (8-bit streams)")
    p.add_argument("--static-guard", type=int, default=None, metavar="R",
                   help="hold static regions (overlays, subtitles, letterbox bars): a pixel whose window of radius R (0..16) is the same in both "
                        "source frames keeps the earlier frame's samples (no default is claimed); excludes --reference-quirks")
    p.add_argument("--static-tolerance", type=float, default=None, metavar="FRACTION",
                   help="with --static-guard: samples that differ by at most FRACTION of full scale count as the same (default 0: bit-equal only)")
    p.add_argument("--active-area", type=_active_area, default=None, metavar="auto|T,L,H,W",
                   help="run the model on the active picture only and put the bars of the earlier frame back around every in-between frame: "
                        "the rectangle top,left,height,width (top and bottom even, left and right multiples of 16 unless they are the frame's "
                        "edge), or auto: black bars are found on the device, per chunk, and the rectangle only grows; excludes --scale / "
                        "--size, --reference-quirks and --evaluate; no quality claim is made")
    p.add_argument("--active-tolerance", type=float, default=None, metavar="FRACTION",
                   help="with --active-area auto: samples up to FRACTION of full scale above black still count as bar (default 0)")
    p.add_argument("--ensemble", choices=("reverse", "flip", "full"), default=None,
                   help="test-time ensembling of every forward: the pair and the reversed pair (reverse: 2 forwards, symmetric in time), the "
                        "pair under the four mirrorings (flip: 4 forwards, equivariant under flips) or both (full: 8 forwards); no quality "
                        "claim is made, --evaluate tells what it buys on a clip")
    p.add_argument("--border", type=int, default=None, metavar="N",
                   help="extend every frame by N pixels (1..64) past each edge before every forward and crop the prediction back: the model "
                        "takes the outside of the picture as mean grey, which shows as an edge band in the in-between frames wherever the "
                        "picture continues past the frame; no quality claim is made, --evaluate tells what it buys on a clip")
    p.add_argument("--border-mode", choices=("replicate", "reflect"), default=None,
                   help="with --border: repeat the edge pixel (replicate, the default) or mirror the picture about it (reflect)")
    p.add_argument("--agreement", type=float, default=None, metavar="TOL",
                   help="with --ensemble reverse or full: where the forward and the time-reversed prediction differ by more than TOL of full "
                        "scale (0..1) the plain blend of the two source frames is written instead; no default and no quality claim is made, "
                        "--evaluate tells what it buys on a clip; excludes --reference-quirks")
    p.add_argument("--agreement-radius", type=int, default=None, metavar="R",
                   help="with --agreement: a disagreeing pixel holds its neighbours within R pixels (0..16) as well (default 0)")
    p.add_argument("--flow-scale", type=int, choices=(2, 4, 8), default=None, metavar="{2,4,8}",
                   help="estimate the flow of every forward on frames reduced by this factor and run everything else at full size: the "
                        "model's flow sees 7 pixels, this multiplies that reach; the output keeps its size (--scale shrinks it); no quality "
                        "claim is made, --evaluate tells what it buys on a clip")
    p.add_argument("--align", type=int, default=None, metavar="PIXELS",
                   help="with --align-ratio: remove the global translation of every pair before every forward - one shift per pair, a "
                        "multiple of 4 pixels per axis within PIXELS (a multiple of 4 in 4..128), found on the device; the model's flow sees 7 "
                        "pixels, a pan is tens; no default and no quality claim is made, --evaluate tells what it buys on a clip")
    p.add_argument("--align-ratio", type=float, default=None, metavar="FRACTION",
                   help="with --align: a shift is kept only where it lowers the mean absolute difference of the pair to at most FRACTION "
                        "(0..1) of the unshifted one")
    p.add_argument("--batch-pairs", type=int, default=8)
    p.add_argument("--chunk-pairs", type=int, default=64, help="frame pairs per chunk: at most chunk_pairs * frame_interval + 1 source frames are held")
    p.add_argument("--yuv-standard", default="bt601", help="bt601, bt709 or (10 / 12 / 16-bit streams) bt2020")
    p.add_argument("--full-range", action="store_true")
    p.add_argument("--reference-quirks", action="store_true", help="de-normalise the model output as the reference does (default: off)")
    p.add_argument("--evaluate", action="store_true", help="score the model on the clip (held-out PSNR / SSIM of the Y plane); writes no video; holds the WHOLE clip in host memory")
    p.add_argument("--every", type=int, default=1, help="with --evaluate: every N-th frame is a target")
    return p


def _run(args) -> int:
    import torch
    from . import EMA_VFI, FrameInterpolator, synth

    if not args.evaluate and args.output is None:
        raise ValueError("an output stream is needed (or --evaluate)")
    resample = args.output_fps is not None
    if resample:
        for given, name in ((args.target_fps is not None, "--target-fps"), (args.factor is not None, "--factor"),
                            (args.mode is not None, "--mode"), (args.reference_quirks, "--reference-quirks"),
                            (args.frame_interval != 1, "--frame-interval other than 1")):
            if given:
                raise ValueError(f"--output-fps excludes {name}: the output rate alone decides which frames are written")
    else:
        for given, name in ((args.dedup is not None, "--dedup"), (args.dedup_max_run is not None, "--dedup-max-run")):
            if given:
                raise ValueError(f"{name} needs --output-fps: dropped frames are replaced on the resampler's time grid")
        if args.shutter is not None:
            raise ValueError("--shutter needs --output-fps (the stream's own rate adds blur and keeps the rate): the exposure window is "
                             "accumulated on the resampler's time grid")
    if args.shutter is not None:
        for given, name, why in ((args.resample == "blend", "--resample blend", "the window's weights already say how the midpoints are mixed"),
                                 (args.dedup is not None, "--dedup", "a window over a gap of dropped frames is not defined"),
                                 (args.evaluate, "--evaluate", "a held-out frame is an instantaneous sample")):
            if given:
                raise ValueError(f"--shutter excludes {name}: {why}")
    if args.light is not None:
        if args.shutter is None and not (resample and args.resample == "blend"):
            raise ValueError("--light needs --shutter or --output-fps with --resample blend: nothing else mixes frames")
    if args.static_tolerance is not None and args.static_guard is None:
        raise ValueError("--static-tolerance needs --static-guard R")
    if args.static_guard is not None and args.reference_quirks:
        raise ValueError("--static-guard excludes --reference-quirks: exact source pixels pasted into the quirk's de-normalised prediction would "
                         "show as patches")
    if args.static_guard is not None and not 0 <= args.static_guard <= 16:
        raise ValueError("--static-guard R: the radius must lie in 0..16")
    if args.static_tolerance is not None and not 0.0 <= args.static_tolerance <= 1.0:
        raise ValueError("--static-tolerance FRACTION: a fraction of full scale in 0..1")
    if args.active_tolerance is not None:
        if args.active_area != "auto":
            raise ValueError("--active-tolerance needs --active-area auto: the tolerance belongs to the search for the bars")
        if not 0.0 <= args.active_tolerance <= 1.0:     # false for a NaN
            raise ValueError("--active-tolerance FRACTION: a fraction of full scale in 0..1")
    if args.active_area is not None:
        for given, name, why in ((args.scale is not None or args.size is not None, "--scale / --size", "the rectangle is cut from the frames as "
                                  "staged"), (args.reference_quirks, "--reference-quirks", "the bars are exact source samples, which the "
                                  "quirk's de-normalised frames are not"), (args.evaluate, "--evaluate", "a held-out frame is scored whole")):
            if given:
                raise ValueError(f"--active-area excludes {name}: {why}")
    if args.dedup_max_run is not None and args.dedup is None:
        raise ValueError("--dedup-max-run needs --dedup FRACTION")
    if args.border_mode is not None and args.border is None:
        raise ValueError("--border-mode needs --border N")
    if args.border is not None and not 1 <= args.border <= 64:
        raise ValueError("--border N: the border must lie in 1..64")
    if args.agreement_radius is not None and args.agreement is None:
        raise ValueError("--agreement-radius needs --agreement TOL")
    if args.agreement is not None:
        if not 0.0 <= args.agreement <= 1.0:     # false for a NaN
            raise ValueError("--agreement TOL: a fraction of full scale in 0..1")
        if args.agreement_radius is not None and not 0 <= args.agreement_radius <= 16:
            raise ValueError("--agreement-radius R: the radius must lie in 0..16")
        if args.ensemble not in ("reverse", "full"):
            raise ValueError("--agreement needs --ensemble reverse or --ensemble full: the guard compares the two time directions")
        if args.reference_quirks:
            raise ValueError("--agreement excludes --reference-quirks: a [0, 1] blend pasted into the quirk's de-normalised prediction would "
                             "show as patches")
    if (args.align is None) != (args.align_ratio is None):
        raise ValueError("--align PIXELS and --align-ratio FRACTION belong together: no default is claimed for either")
    if args.align is not None:
        if args.align % 4 or not 4 <= args.align <= 128:
            raise ValueError("--align PIXELS: the radius must be a multiple of 4 in 4..128")
        if not 0.0 <= args.align_ratio <= 1.0:     # false for a NaN
            raise ValueError("--align-ratio FRACTION: a fraction in 0..1")
    mode = "resample" if resample else (args.mode or "reference")
    with y4m.Y4MReader(args.input) as reader:
        head = reader.header
        if resample:
            factor = 1
            if args.output_fps < head.rate:
                raise ValueError(f"--output-fps {args.output_fps} lies below the stream's {head.rate} fps: frames are interpolated, never dropped")
            if args.shutter is not None:      # what the shutter definition refuses is said before a device is asked for
                FrameInterpolator.shutter_plan(0, head.rate, args.output_fps, args.resample_depth, args.shutter)
        elif args.factor is not None:
            factor = args.factor
        else:
            factor, _ = y4m.choose_factor(head.fps, args.target_fps, args.max_interpolation_factor)
        if args.light is not None and not formats.lookup(head.pixel_format).light_table_fits:
            raise ValueError(f"--light on a 16-bit stream ({head.pixel_format}): linear light takes 8-, 10- and 12-bit streams")
        if factor < 0:
            raise ValueError(f"the interpolation factor {factor} is negative (the target rate lies below the stream's {head.fps:g} fps)")
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device: this project has no CPU path")
        dev = torch.device("cuda")
        if args.weights is not None:
            sd = torch.load(args.weights, map_location="cpu", weights_only=True)   # a plain state_dict: nothing else is unpickled
        else:
            sd = synth.synthetic_state_dict(seed=args.synthetic_weights, mid_channels=args.mid_channels)
        model = EMA_VFI(mid_channels=args.mid_channels, compute_dtype=args.dtype).to(dev).eval()
        model.load_state_dict(sd, strict=True)
        fi = FrameInterpolator(model, interpolation_factor=factor, frame_interval=args.frame_interval, batch_pairs=args.batch_pairs,
                               reference_quirks=args.reference_quirks, mode=mode, pixel_format=head.pixel_format,
                               yuv_standard=args.yuv_standard, yuv_full_range=args.full_range, scale=args.scale, size=args.size,
                               scene_threshold=args.scene_threshold, copy_out=False,
                               **(dict(rate_in=head.rate, rate_out=args.output_fps, resample_depth=args.resample_depth,
                                       resample_method=args.resample, shutter=args.shutter) if resample else {}),
                               **(dict(dedup_threshold=args.dedup, dedup_max_run=3 if args.dedup_max_run is None else args.dedup_max_run)
                                  if args.dedup is not None else {}),
                               **(dict(static_guard=args.static_guard, static_tolerance=args.static_tolerance or 0.0)
                                  if args.static_guard is not None else {}),
                               ensemble=args.ensemble,
                               **(dict(border=args.border, border_mode=args.border_mode or "replicate") if args.border is not None else {}),
                               **(dict(agreement=args.agreement, agreement_radius=args.agreement_radius) if args.agreement is not None else {}),
                               flow_scale=args.flow_scale, **(dict(light=args.light) if args.light is not None else {}),
                               **(dict(active_area=args.active_area, active_tolerance=args.active_tolerance or 0.0)
                                  if args.active_area is not None else {}),
                               **(dict(align=args.align, align_ratio=args.align_ratio) if args.align is not None else {}))
        if args.evaluate:
            print(fi.evaluate(list(reader), every=args.every))      # evaluate() indexes the clip: all of it is held
            return 0
        dst = fi.output_size(head.height, head.width, args.scale, args.size, head.pixel_format)
        out_size = dst if (args.scale is not None or args.size is not None) else None
        out_head = head.for_output_rate(args.output_fps, out_size) if resample else head.for_output(factor, out_size)
        with y4m.Y4MWriter(args.output, out_head) as writer:
            for frame in fi.run_chunked(reader, chunk_pairs=args.chunk_pairs):
                writer.write(frame)
        if args.output != "-":
            print(f"{reader.frames_read} frames in, {writer.frames_written} frames out at {out_head.fps_num}:{out_head.fps_den} fps "
                  f"({out_head.width} x {out_head.height}, {head.pixel_format}, "
                  + (f"{args.resample} at depth {args.resample_depth})" if resample else f"factor {factor})")
                  + (f", shutter {fi.shutter} degrees" if args.shutter is not None else "")
                  + (f", mixed in linear light ({args.light})" if args.light is not None else "")
                  + (f", {len(fi.duplicates)} duplicate frames dropped" if args.dedup is not None else "")
                  + (f", static guard held {100.0 * sum(fi.static_share) / max(len(fi.static_share), 1):.2f} % of the predictions' pixels on average"
                     if args.static_guard is not None else "")
                  + (f", active area {fi.active_rect} = {100.0 * fi.active_share:.1f} % of the frame" if args.active_area is not None else "")
                  + (f", ensemble {args.ensemble}" if args.ensemble is not None else "")
                  + (f", border {args.border} {args.border_mode or 'replicate'}" if args.border is not None else "")
                  + (f", flow scale {args.flow_scale}" if args.flow_scale is not None else "")
                  + (f", agreement guard held {100.0 * sum(fi.agreement_share) / max(len(fi.agreement_share), 1):.2f} % of the predictions' "
                     f"pixels on average" if args.agreement is not None else "")
                  + (f", align {args.align} px at ratio {args.align_ratio:g} shifted "
                     f"{100.0 * sum(1 for d in fi.align_shifts if d != (0, 0)) / max(len(fi.align_shifts), 1):.2f} % of the predictions"
                     if args.align is not None else ""), file=sys.stderr)
    return 0


def main(argv=None) -> int:
    """Runs the command line in-process; returns the exit code (0, or non-zero with the message on stderr for refused input)."""
    try:
        args = parser().parse_args(argv)
    except SystemExit as e:      # argparse has printed its message
        return int(e.code or 0)
    try:
        return _run(args)
    except (ValueError, RuntimeError, OSError) as e:
        print(f"emavfi: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
