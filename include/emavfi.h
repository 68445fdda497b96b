/*
 * emavfi.h - C-ABI of libemavfi.so, the MI355X-native (gfx950) EMA-VFI
 * inference path.
 *
 * The reference (424635328/video-frame-interpolation) has no FFI layer: its hot
 * path is the Python class EMA_VFI in src/models/ema_vfi.py, whose work is done
 * by torch / torchvision operators.  Each entry below replaces the operator
 * call sites cited next to it.  The Python mirror of the reference class
 * (video-frame-interpolation_amd/emavfi/model.py) binds these with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer on the current HIP device, 16-byte
 *    aligned, to a dense tensor.  Image tensors crossing this boundary are
 *    NCHW fp32, exactly what the reference's forward() receives and returns.
 *  - The library never allocates, frees or retains device memory and never
 *    synchronises the device: the caller owns inputs, outputs, the packed
 *    weight blob and the workspace (sized by the *_bytes queries) and all work
 *    is enqueued on the hipStream_t passed as `stream` (void* here so the
 *    header needs no HIP include; NULL = the default stream).
 *  - Every int-returning entry returns 0 on success and a negative EMAVFI_E_*
 *    code on failure; emavfi_last_error() then holds a thread-local message.
 *    Nothing aborts the process (the reference wraps its loop in try/except,
 *    inference.py:207-208).
 *  - `dtype` selects the arithmetic of the contractions: EMAVFI_F32 computes
 *    every convolution with fp32-input MFMA (exact fp32 FMA chains; this is the
 *    parity mode, <= 1e-3 max-abs vs the reference's CPU forward);
 *    EMAVFI_BF16 stores activations and weights in bf16 and accumulates in
 *    fp32 (BASELINE.json configs[2]: "bf16 convs + fp32 warp").  One stage
 *    leaves bf16: the one-launch ModulatedDeformConvPack kernel (mid_channels
 *    64) works on the IEEE f16 image of its input window - bf16 values convert
 *    exactly inside f16's normal range, keep 11 instead of 8 significant bits
 *    through the bilinear blend, lose trailing bits below 6.1e-5 and SATURATE
 *    at +-65504 (v_cvt_pkrtz; no infinities are produced) - contracts bf16-
 *    rounded weights stored as f16 (weights below 6.1e-5 in magnitude are f16
 *    subnormals there: absolute error <= 3e-8 each), and hands the tensor
 *    between two consecutive packs on as f16 bit patterns.  Since round 3 the feature map
 *    that enters the fusion stage (`feat`, and the warped frame beside it) is
 *    itself stored as f16 in this mode, saturating the same way, and its two
 *    other readers (context_encoding.0, motion_estimation.0) contract it with
 *    bf16-rounded weights stored as f16.  Activations beyond +-65504 in `feat`
 *    and in the fusion stage are therefore clamped there, not propagated
 *    (tests/test_gpu_parity.py::test_bf16_pack_saturates_at_the_f16_range).
 *    EMAVFI_F16 is the same data flow in IEEE half precision - the arithmetic
 *    torch.cuda.amp.autocast() gives the reference's convolutions on a GPU
 *    (inference.py:159); its fused deformable kernel blends the four corners
 *    in packed f16; values beyond +-65504 overflow to inf exactly as they
 *    would there.  NON-FINITE ACTIVATIONS inside the one-launch pack (reachable only through such an
 *    f16 overflow): the reference confines an Inf / NaN sample to the output pixels that sample it; this
 *    kernel may also turn channels 64..66 of the pixel 16 columns to the left / right in the same 2 x 16
 *    fragment row into NaN (its third output fragment contracts two pixels per MFMA column and separates
 *    them by zero weights: 0 x Inf), and a lane whose sample is parked for the fix-up pass reads window
 *    offset 0 / the arena's zero slot against zero weights.  Finite inputs are unaffected; a frame that
 *    contains any non-finite value is garbage in the reference as well.  A NaN / infinite flow (or one whose `2 * v` overflows)
 *    warps to NaN in every channel, a finite flow far outside to 0 - what
 *    the reference's CPU grid_sample returns (ema_vfi.py:169).  Flow, warp coordinates,
 *    deformable offsets / masks / sampling positions, the pooled context
 *    vector and the output are fp32 in every mode.
 *  - The model is identified by the reference constructor's three integers
 *    (ema_vfi.py:64): in_channels, mid_channels, num_blocks.
 */
#ifndef EMAVFI_H
#define EMAVFI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMAVFI_VERSION 403 /* 0.4.3: emavfi_align_signature_f32, emavfi_align_workspace_bytes, emavfi_align_search, emavfi_shift_f32 added (global motion compensated before the forward: one translation per pair, found and applied on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_active_bounds, emavfi_fill_outside_frames, emavfi_preprocess_u8_pitched, emavfi_postprocess_u8_pitched added (the forward run on the active picture only: black bars found on the device and put back around every prediction; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_transfer_table, emavfi_transfer_table_check, emavfi_accumulate_frames_linear added (blended and motion-blurred frames mixed in linear light through a transfer table, on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_downscale_f32, emavfi_upsample_flow_f32, emavfi_forward_flow, emavfi_forward_given_flow (and their two launch lists) added (the flow estimated on frames reduced by 2, 4 or 8 for motion beyond seven pixels, the forward split at its flow; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_accumulate_frames added (motion blur from a shutter angle: every output frame the weighted integer mean of the node frames inside its exposure window, on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_agreement_guard_f32 added (where the two time directions of the ensemble disagree the plain blend of the source frames is emitted, decided on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_border_pad_f32, emavfi_border_crop_f32 added (frames extended past their edges by replication or reflection before the forward and cropped after it, on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_flip_f32, emavfi_ensemble_mean_f32 added (test-time ensembling over time reversal and flips: the mirrored inputs and the tree mean of the members on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_static_guard_frames added (static regions of a pair held on the device: overlays, subtitles, letterbox bars; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_frame_diff_cells, emavfi_duplicate_flags added (duplicate frames found on the device, so that the resampler interpolates across the gap; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_resample_frames added (output frames at any rate assembled from source and node frames on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_preprocess_yuv420p, emavfi_postprocess_yuv420p added (planar 4:2:0 frames, 8 / 10 / 12 / 16 bits, as software decoders and Y4M hold them; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_frame_metrics_workspace_bytes, emavfi_frame_metrics_u8 added (held-out PSNR / SSIM scored on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_luma_signature_u8, emavfi_scene_flags, emavfi_hold_frames_u8 added (scene cuts decided and applied on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_resize_u8, emavfi_preprocess_u8_resized, emavfi_preprocess_nv12_resized added (frames resized on the device; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_yuv_coefficients, emavfi_preprocess_nv12, emavfi_postprocess_nv12 added (NV12 frames; same version: the packed layout is unchanged, cached blobs stay valid); emavfi_forward_census, emavfi_mdcn_census (round 6; the workspace grows by 8 KiB, the packed layout is unchanged); emavfi_forward_profiled / _staged and emavfi_mdcn_profiled later folded into emavfi_forward_routed / emavfi_mdcn_routed (same version: the packed layout is unchanged); 0.4.2: emavfi_forward_staged, emavfi_mdcn_profiled (round 5; the packed layout is 0.4.1's, but a blob says which library packed it: re-pack); 0.4.1: context_encoding.1 / .2 re-packed for conv_wreg.inl; 0.4.0: the packed blob starts with a 256-byte self-describing header, emavfi_forward takes packed_bytes (round 4): re-pack */

#define EMAVFI_F32 0
#define EMAVFI_BF16 1
#define EMAVFI_F16 2
/* The reference's forward under torch.cuda.amp.autocast() (inference.py:159), op policy restated: fp16 nn.Conv2d /
 * nn.Linear (input, weight AND bias cast to fp16, fp32 accumulation, fp16 result), fp16 tensors between those layers,
 * but grid_sample (ema_vfi.py:169; promotes to its widest argument, and frame2 and the grid are fp32) in fp32 on the
 * fp16-valued flow and torchvision's deform_conv2d (ema_vfi.py:60)
 * in fp32 on the UNROUNDED fp32 fusion tensor with the fp32 master weights (its Autocast kernel casts every argument
 * to float and the result back to the input's dtype, which is fp32 because cat(feat, warped) promotes), offsets /
 * sigmoid(mask) as fp16 values, tanh and (t+1)/2 in fp16.  The frame holds fp16-representable values.  Since 0.4.3 the fp32 deform_conv2d
 * of THIS mode contracts as a three-term f16 split (22 bits of each operand, exact products, fp32 accumulation: 3e-7 .. 1.4e-6 relative,
 * the spread between two fp32 summation orders - which is what separates any GPU run of the reference from its CPU run anyway); its
 * sampling positions, corner weights and blend are fp32 as before.  EMAVFI_F32 is the mode with exact fp32 FMA chains.
 * EMAVFI_F16 stays the FAST half-precision mode (DCN contraction and blend in fp16 too). */
#define EMAVFI_AMP16 3
/* fp32-ACCURATE contractions on the 16-bit matrix pipe (round 6; gfx950 has no TF32 and its fp32 MFMA runs at 1/16 of the f16 rate):
 * every nn.Conv2d computes x_hi w_hi + x_hi w_lo + x_lo w_hi with x = x_hi + x_lo, w = w_hi + w_lo in IEEE f16 (up to 22 significant
 * bits of each operand, see below; the products are exact in fp32, accumulation in fp32, biases and activations in fp32), activations
 * between the layers are stored as the two f16 halves of the fp32 value; the nn.Linear of context_encoding and the context half of
 * motion_estimation.0 (a per-border-class bias) are fp32 FMA chains on the fp32 weights; flow, warp, the pooled context and the sampling
 * geometry (positions, corner weights, blend) of the three deform_conv2d are the fp32 ones of EMAVFI_F32.  The deform_conv2d
 * CONTRACTION: at mid_channels + 3 = 65..68 (mid_channels 64: the LDS-window kernel, deform_f32w.inl) it is the same three-term f16
 * split as EMAVFI_AMP16's (above) - in the launch list "fp32 sampling, three-term f16 split contraction" -; at every other width the
 * generic fp32 kernel runs and it is exact fp32.  Passes the fp32 mode's parity gates (<= 1e-3 on the frame, <= 5e-4 relative on every
 * stage) on every reference-run fixture; a SEPARATELY NAMED mode: EMAVFI_F32 stays the exact-fp32 parity mode.
 * ACCURACY AS A FUNCTION OF MAGNITUDE (derived, and checked per element: tests/rounding_model.py, conv_model_x3 / accuracy_bound_x3;
 * tests/test_gpu_fp32x3_rounding_model.py).  An operand v is carried as hi = f16(v), lo = f16(v - hi).  While lo is a NORMAL f16
 * number (|lo| >= 2^-14 = 6.1e-5; |lo| <= 2^-11 |v|, so every |v| < 2^-3 has a subnormal lo) hi + lo is v to 2^-22 |v|: 22 bits.  A
 * subnormal lo is a multiple of 2^-24: hi + lo is v to 2^-25 = 3e-8 ABSOLUTELY, i.e. 2^-25 (|w| + |x|) per product - Kaiming-scale
 * weights of 0.02 are carried to about 19 bits, an operand of 1e-3 to 15.  Per output element, against the float64 convolution of
 * the unsplit operands: <= 3 * 2^-22 sum|w x| + 2^-25 (sum|w| + sum|x|) over the receptive field, plus the fp32 accumulation of the
 * 27 Cin + 1 terms and the output's own split.
 * RANGE: every |input| and |activation| must stay <= 65504 (the largest f16 number).  An accumulator v of magnitude 65520 or more
 * (what rounds to infinity in f16) stores hi = +-inf with the sign of v and lo = v - hi = -+inf with the opposite one (v >= 65520:
 * hi = inf, lo = -inf; v <= -65520: hi = -inf, lo = inf): that ONE element is non-finite (NaN once hi + lo is formed) and poisons
 * what reads it; no other element is affected and no address depends on a value.  Stage entries: emavfi_conv3x3 only. */
#define EMAVFI_F32X3 4

#define EMAVFI_OK 0
#define EMAVFI_E_ARG (-1)         /* bad shape / dtype / null pointer / misaligned pointer */
#define EMAVFI_E_UNSUPPORTED (-2) /* model widths this build has no kernel instantiation for */
#define EMAVFI_E_WORKSPACE (-3)   /* workspace or packed buffer too small */
#define EMAVFI_E_LAUNCH (-4)      /* hipGetLastError() after a launch */

/*
 * SIZE LIMITS (the one place).  Sample bases, batch strides and every pitched 8 / 16-bit entry's pitches and strides are 64-bit.  INSIDE
 * one sample the kernels keep narrow arithmetic on purpose: 32-bit byte offsets, 24-bit pixel indices.  The entries check what that needs
 * BEFORE any pointer is touched and return EMAVFI_E_ARG with the limit in the message; the *_workspace_bytes queries and the launch lists
 * are size_t / double throughout and exceed 2^32 at ordinary 4K batches.
 *   "plane" = H * W * (channels padded as the kernels store them) * (bytes of the WIDEST element the mode keeps of that tensor): the
 *   fusion tensor of mid_channels + 3 channels padded to a multiple of 16 (80 at the reference width), 2 bytes in EMAVFI_BF16 /
 *   EMAVFI_F16, 4 bytes in EMAVFI_F32, EMAVFI_AMP16 and EMAVFI_F32X3 (which also keep it in fp32).
 *     emavfi_forward*, emavfi_mdcn*, emavfi_context, emavfi_reconstruct (+ their queries, launch lists and census entries):
 *                          B*H*W < 2^31, H*W < 2^24, plane < 4 GiB.  At the reference width: 16-bit modes up to 2^24 - 1 pixels a frame
 *                          (4095 x 4096: a 2.4 GB plane), 4-byte modes up to 13 421 772 pixels (3840 x 2160 is 8 294 400).
 *     emavfi_conv3x3:      INPUT plane (Cin padded to 16; fp32 65..72 -> 72) < 4 GiB; no limit on H*W or B*H*W; no limit on the output
 *                          plane - every kernel writes through 64-bit addresses.  EMAVFI_F32X3 runs the tile kernel alone, whose input
 *                          addresses are 64-bit as well: its plane is counted in f16 halves (2 bytes), i.e. the real [hi | lo] plane is
 *                          < 8 GiB.
 *     emavfi_deform_conv2d: H*W < 2^24, input plane (C padded to the kernel's width: 80 for 65..80) < 4 GiB.
 *     emavfi_warp:         H*W < 2^31 (32-bit pixel offsets inside one fp32 plane); B and C are not limited.
 *   Of these, two statements rest on READING the kernels, not on a run: "no limit on the output plane" was run for the tile kernel
 *   (6 -> 64, a 4.3 GB output plane) - for the other families (an output larger than a < 4 GiB input needs Cout > Cin: conv_wreg's 128 ->
 *   256 at stride 1) it follows from `obase` / `orow` being size_t arithmetic in conv_wreg.inl, conv_ring*.inl and conv3x3.inl; and the
 *   EMAVFI_F32X3 plane was run just under and just over 4 GiB (4.0004 GiB), not between there and 8 GiB.
 * Run at these sizes, with offsets past 2^31 inside a sample and past 2^32 in total: tests/test_gpu_large.py; the limits themselves, last
 * admitted and first refused value: tests/test_cabi_cpu.py, tests/host/host_check.cpp.
 */

/* Activation selector of emavfi_conv3x3 (conv vs conv_block, ema_vfi.py:7-14). */
#define EMAVFI_ACT_NONE 0
#define EMAVFI_ACT_RELU 1
#define EMAVFI_ACT_TANH01 2 /* tanh then (t+1)/2: reconstruction tail, ema_vfi.py:106,146 */

int emavfi_version(void);
const char *emavfi_last_error(void);

/* 0 if (in_channels, mid_channels, num_blocks, dtype) has kernels in this build. */
int emavfi_supported(int in_channels, int mid_channels, int num_blocks, int dtype);

/* Number of tensors in the reference state_dict (ema_vfi.py:63-107): 16 + 8*num_blocks... see
 * emavfi_param_count(); order = the reference's registration order:
 *   feat_ext_conv1.0.{weight,bias}; feat_ext_blocks.conv_block_i.0.{w,b} (i < num_blocks);
 *   context_encoding.{0.0,1.0,2.0}.{w,b}; context_encoding.5.{w,b};
 *   motion_estimation.{0.0,1.0,2}.{w,b};
 *   attention_blocks.i.offset_conv.{w,b}, attention_blocks.i.dcn_v2.{w,b} (i < num_blocks);
 *   reconstruction.{0.0,1.0,2}.{w,b}. */
int emavfi_param_count(int num_blocks);

/* Re-pack the fp32 OIHW parameters into the MFMA fragment order the kernels stream
 * (replaces nothing in the reference: torch keeps OIHW; this runs once after
 * load_state_dict, inference.py:69).  `params[i]` are device pointers in the order above. */
size_t emavfi_packed_bytes(int in_channels, int mid_channels, int num_blocks, int dtype);
int emavfi_pack_weights(int in_channels, int mid_channels, int num_blocks,
                        const void *const *params, int n_params,
                        void *packed, size_t packed_bytes, int dtype, void *stream);

/* The packed blob is self-describing.  Bytes [0, 256): header, little endian -
 *   char magic[8] = "EMAVFIPK"; u32 version (EMAVFI_VERSION); u32 header_bytes (256); u32 in_channels, mid_channels, num_blocks;
 *   u32 dtype (as requested: EMAVFI_AMP16 is a layout of its own); u32 layout_tag (emavfi_layout_tag() of the packing process);
 *   u32 reserved; u64 total_bytes (= emavfi_packed_bytes); u64 checksum; zeros up to byte 256;
 * bytes [256, total_bytes): the payload.  checksum = sum over the payload's 32-bit words w[i] of (w[i] + 0x9E3779B9) * (2 i + 1)
 * mod 2^64.  The reference has no counterpart (torch.load of a state_dict, inference.py:69); the blob is what this library
 * caches on disk and broadcasts between ranks, so it has to say what it is.
 *
 * emavfi_layout_tag: bit mask of the process-wide environment switches the packed LAYOUT depends on (read once per process):
 *   1 EMAVFI_CONV_MFMA16=0, 2 EMAVFI_CONV_RING=0, 4 EMAVFI_CONV_S2RING=0, (8: unused since 0.4.1), 16 EMAVFI_PACK_F16_CHAIN=0,
 *   32 EMAVFI_NO_FUSED_OFFSET, 64 EMAVFI_CONV_WREG=0.  Cache keys must use it (not the environment, which may have changed since the library latched it).
 * emavfi_packed_check: verifies header (magic, version, model, dtype, layout tag, size) and checksum of a blob in device OR host
 *   memory; EMAVFI_E_ARG with a message naming the mismatch.  THE ONE ENTRY THAT SYNCHRONISES: for a device blob it makes the
 *   blob's device current, waits for EVERY stream of that device (hipDeviceSynchronize - the producer may have been the pack
 *   kernels, an RCCL broadcast or a cache upload on any stream, also a non-blocking one), copies the blob to the host and restores
 *   the caller's device.  Host memory is read in place: the caller orders its own writes.  Call it when a blob arrives - from a
 *   file, another rank, another process - not per frame.
 * emavfi_forward itself (a) returns EMAVFI_E_ARG when packed_bytes is smaller than the model / dtype needs and (b) compares the
 *   header ON THE DEVICE with what the call expects, in its LAST launch (blob_guard, ~2 us): for a blob of another version /
 *   model / dtype / layout tag every kernel still runs on the foreign bytes, and that last launch then overwrites `out` with NaN -
 *   an all-NaN frame, never plausible garbage; it cannot return a code for device-resident bytes without synchronising.
 *   The `taps` (a test hook) are NOT guarded: they hold whatever the kernels computed from the foreign bytes. */
int emavfi_layout_tag(void);
int emavfi_packed_check(int in_channels, int mid_channels, int num_blocks, int dtype, const void *packed, size_t packed_bytes);

/* EMA_VFI.forward(frame1, frame2) -> out, ema_vfi.py:110-147.
 * frame1, frame2: [B, in_channels, H, W] fp32; out: [B, in_channels, H, W] fp32 in [0,1].
 * `taps` is NULL, or 5 + num_blocks device pointers (any may be NULL) that receive NCHW fp32
 * copies of the intermediates the golden vectors hold:
 *   [0] feat [B,mid,H,W]  [1] ctx [B,mid]  [2] flow [B,2,H,W]  [3] warped [B,in_channels,H,W]
 *   [4] reserved  [5+i] output of attention block i [B,mid+3,H,W].
 *
 * THE WORKSPACE CONTRACT, for this and every other entry that takes (workspace, workspace_bytes) - emavfi_forward*, emavfi_conv3x3,
 * emavfi_deform_conv2d, emavfi_mdcn*, emavfi_context, emavfi_reconstruct, emavfi_frame_metrics_u8 - with the size its
 * *_workspace_bytes function reports for the same arguments:
 *   - the contents of the workspace on entry are ARBITRARY: hipMalloc'ed and never written, another call's activations, NaN bit
 *     patterns (0 x NaN is NaN on the matrix pipe, so "finite data against zero weights" is not a property the caller owes);
 *   - an entry reads no byte of the workspace that the same call has not written, and no byte outside any buffer it is given, that
 *     can change a result: whatever a kernel over-fetches (pad lanes, spare tap slots, slack behind the last pixel) is either
 *     written by the call first or discarded before it meets arithmetic; no index, bound or route is ever taken from such a byte;
 *   - an entry writes nothing outside [workspace, workspace + the reported size) and outside the outputs' own shapes; fewer bytes
 *     than reported are refused with EMAVFI_E_WORKSPACE before any device work;
 *   - on exit only the census (emavfi_forward_census, emavfi_mdcn_census) is defined, until the next call on that workspace; every
 *     other byte is scratch.
 * tests/test_gpu_workspace.py holds every entry to this: exact-size, guard-banded workspaces pre-filled with 0x00, 0xFF and 0x7B must
 * give bit-identical outputs, taps and census words. */
size_t emavfi_workspace_bytes(int in_channels, int mid_channels, int num_blocks,
                              int B, int H, int W, int dtype);
int emavfi_forward(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes,
                   const float *frame1, const float *frame2, float *out,
                   void *workspace, size_t workspace_bytes,
                   int B, int H, int W, int dtype, float *const *taps, void *stream);

/* Measurement hooks (no reference counterpart: the reference has no profiling).
 * emavfi_forward_launches enumerates the kernel launches one forward enqueues, in order: returns
 * their number (also when capacity == 0), and for capacity >= that number fills `names`
 * (newline-separated, "kernel<instantiation> reference-layer"), and each launch's ALGORITHMIC
 * flops and bytes (real, unpadded channels; every tensor touched once).  emavfi_forward_routed
 * below brackets these launches with events. */
int emavfi_forward_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                            char *names, size_t names_bytes, double *flops, double *bytes, int capacity);

/* Per-block route of the 16-bit attention blocks.  The one-launch pack exists as two kernels with the same operands,
 * weights (the blob and emavfi_layout_tag() do not change) and output:
 *   EMAVFI_ROUTE_WINDOW  deform_pack3_kernel: stages a 23 x 23 window (+-2 px beyond every tap); samples that leave it take a fix-up pass,
 *                        so its cost grows with the offsets (the census below counts them).  What every entry without a route runs.
 *   EMAVFI_ROUTE_GATHER  deform_gather3_kernel: stages only offset_conv's 18 x 18 tile, gathers every corner from global memory; its cost
 *                        does not depend on the offsets.  Bit-identical to the window route wherever that one's census shows no fix-up group.
 * The gather route exists exactly where the one-launch pack runs (EMAVFI_BF16 / EMAVFI_F16 at mid_channels + 3 = 65..67); fp32,
 * EMAVFI_AMP16, EMAVFI_F32X3 and other widths refuse it with EMAVFI_E_UNSUPPORTED.  Workspace sizes are the same for both routes.
 * emavfi_forward_routed: emavfi_forward (`taps` may be NULL) plus
 *   `events` / `n_events`  NULL (n_events ignored), or caller-created hipEvent_t (timing enabled) with n_events >= 2, else EMAVFI_E_ARG:
 *                          launch i of emavfi_forward_launches_routed's list is bracketed by hipEventRecord on events[2i] / events[2i+1]
 *                          on `stream` (the launches with 2i + 1 >= n_events are not bracketed);
 *   `stage_events`         NULL or three caller-created hipEvent_t (any may be NULL), for a caller that pipelines pieces of a batch over
 *                          several streams (frame pairs are independent, ema_vfi.py:110-147 has no cross-sample op; emavfi/model.py,
 *                          EMAVFI_PIPELINE), recorded on `stream` behind
 *                            [0] the front of the forward - feature extraction, context encoding, motion estimation, warp (ema_vfi.py:112-130),
 *                            [1] the last attention block (:136-138),   [2] the reconstruction (:144-146; the forward's last launch);
 *   `gather_blocks`        bit i routes attention block i to EMAVFI_ROUTE_GATHER; bits at or above num_blocks are EMAVFI_E_ARG.
 * With NULL events and mask 0 it is emavfi_forward exactly (same launches, same results).  emavfi_forward_launches_routed lists the
 * launches of such a forward: a gathered block's launch is named "deform_gather<...> offset_conv+dcn_v2", a windowed one
 * "deform<...> offset_conv+dcn_v2". */
#define EMAVFI_ROUTE_WINDOW 0
#define EMAVFI_ROUTE_GATHER 1
int emavfi_forward_routed(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes,
                          const float *frame1, const float *frame2, float *out,
                          void *workspace, size_t workspace_bytes,
                          int B, int H, int W, int dtype, float *const *taps, void *const *stage_events, void *const *events, int n_events,
                          unsigned gather_blocks, void *stream);
int emavfi_forward_launches_routed(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, unsigned gather_blocks,
                                   char *names, size_t names_bytes, double *flops, double *bytes, int capacity);

/* Adaptive per-block route: the route of every 16-bit attention block is chosen ON THE DEVICE from the census of the
 * previous forward, so neither the caller nor a captured graph ever reads a counter back.  Each such block runs the ROUTED pack
 * (deform_pack3_kernel<Route3<T>, true>): one launch that reads the block's route word in `route_state` and runs the window body or the
 * gather body above - same operands, output and census as the plain kernel of that route, bit for bit.  After the last attention block
 * one route_select launch reads this forward's census, records per block the route that ran and its fix-up share (fix-up wave-taps /
 * all wave-taps, the fixup_share of emavfi_forward_census) and writes the route of the NEXT forward with hysteresis:
 *   on EMAVFI_ROUTE_WINDOW: switch to gather when share >= enter_share;  on EMAVFI_ROUTE_GATHER: back to window when share <= leave_share.
 * route_state: caller-owned DEVICE memory of emavfi_route_state_bytes() (<= 256) bytes, 16-byte aligned, one per stream of forwards;
 * u32 words:
 *   [0] EMAVFI_ROUTE_MAGIC   [1] num_blocks   [2] next mask (bit i: block i runs gather in the next adaptive forward)
 *   [3] ran mask (bit i: block i ran gather in the last adaptive forward)   [4] adaptive forwards whose census was read   [5..7] 0
 *   [8 + i]  route word of block i (EMAVFI_ROUTE_*; the routed pack reads it; always bit i of the next mask)
 *   [16 + i] float: block i's fix-up share in the last adaptive forward (-1 before the first one)
 *   [24 + i] switches of block i since the state was initialised
 * emavfi_route_state_init writes a fresh state on `stream` (start_gather_mask: the starting routes; bits at or above num_blocks are
 * EMAVFI_E_ARG).  emavfi_forward_adaptive takes emavfi_forward_routed's arguments with gather_blocks replaced by the state and the two
 * thresholds (0 <= leave_share < enter_share <= 1, else EMAVFI_E_ARG).  The entry never reads the state back (no host sync): the library
 * remembers the states emavfi_route_state_init wrote, and a null state, one it did not write (wrong magic) or one written for another
 * num_blocks is EMAVFI_E_ARG.  On the device the selector also checks words [0] and [1] and leaves a state that fails them untouched.
 * In modes and widths without a one-launch pack (fp32, EMAVFI_AMP16, EMAVFI_F32X3, other widths) emavfi_forward_adaptive is exactly
 * emavfi_forward: same launches, same frame, no selector, the state untouched (adaptation is a preference, unlike
 * EMAVFI_ROUTE_GATHER).  emavfi_forward_launches_adaptive lists such a forward's launches: "deform_routed<...> offset_conv+dcn_v2" per
 * routed block and one final "route_select".  The thresholds of DESIGN 4.1 (0.75 / 0.65) come from one block at B = 8 x 720p. */
#define EMAVFI_ROUTE_MAGIC 0x52544531u /* "1ETR" */
size_t emavfi_route_state_bytes(void);
int emavfi_route_state_init(void *route_state, int num_blocks, unsigned start_gather_mask, void *stream);
int emavfi_forward_adaptive(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes,
                            const float *frame1, const float *frame2, float *out,
                            void *workspace, size_t workspace_bytes,
                            int B, int H, int W, int dtype, float *const *taps, void *const *stage_events, void *const *events, int n_events,
                            void *route_state, float enter_share, float leave_share, void *stream);
int emavfi_forward_launches_adaptive(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                                     char *names, size_t names_bytes, double *flops, double *bytes, int capacity);

/* EMA_VFI.warp(frame2, feature, flow), ema_vfi.py:149-171 (grid build + normalise +
 * F.grid_sample bilinear/zeros/align_corners=True), fused into one HBM-bound kernel.
 * frame2 [B,C,H,W], flow [B,2,H,W] (channel 0 = dx, 1 = dy, pixels), out [B,C,H,W]; fp32.
 * NON-FINITE VALUES, as ATen's CPU grid_sample (the same contract holds for the warp step inside every forward):
 *   flow:   a finite coordinate outside the image samples zeros; a NaN or infinite flow - or one so large that the reference's own
 *           2 * (x + flow) overflows - gives NaN in every channel of that pixel.
 *   frame2: a corner of the bilinear footprint that lies outside [0, size - 1] contributes exactly nothing, whatever frame2 holds
 *           anywhere: a sample with all four corners outside is 0 even beside a NaN or an infinity.  A corner INSIDE multiplies in
 *           IEEE arithmetic, a zero weight included: a NaN or infinite pixel reaches every output whose footprint covers it
 *           (NaN * 0 = Inf * 0 = NaN).  Finite frames: four fp32 products summed in the order nw, ne, sw, se, no contraction. */
int emavfi_warp(const float *frame2, const float *flow, float *out,
                int B, int C, int H, int W, void *stream);

/* Frame pre/post-processing around the forward (the reference does both on the host, per frame).
 * emavfi_preprocess_u8: transforms.ToTensor() + Normalize(mean, std), inference.py:38-41 / :44-48
 *   (cv2.resize excluded): frames_hwc uint8 [B,H,W,C] -> out_nchw fp32 [B,C,H,W] = ((u8/255) - mean[c]) / std[c].
 * emavfi_postprocess_u8: denormalize_frame, inference.py:51-58: frames_nchw fp32 [B,C,H,W] -> out_hwc uint8
 *   [B,H,W,C] = uint8(clip(x * std[c] + mean[c], 0, 1) * 255) (truncation; float64 arithmetic as numpy's
 *   promotion makes it there).  denormalize = 0 skips the x*std+mean step, which the reference applies to an
 *   output that is already in [0,1].
 * `mean` and `std` are HOST pointers to C values (C <= 4): fp32 for preprocess (torchvision builds fp32
 * tensors), float64 for postprocess (numpy's np.array([...]) constants); the frame pointers are device pointers -
 * the uint8 side may also be pinned (device-mapped) host memory, which the kernel then reads / writes over PCIe. */
int emavfi_preprocess_u8(const unsigned char *frames_hwc, float *out_nchw, int B, int H, int W, int C,
                         const float *mean, const float *std, void *stream);
int emavfi_postprocess_u8(const float *frames_nchw, unsigned char *out_hwc, int B, int H, int W, int C,
                          const double *mean, const double *std, int denormalize, void *stream);

/* NV12 frames, in and out: what video decoders produce - a full-resolution Y plane [H][W] and a half-resolution plane of interleaved
 * U,V byte pairs [ceil(H/2)][ceil(W/2)][2], 1.5 bytes per pixel.  Both planes have their own pointer, their own row pitch and their own
 * batch stride (bytes): the pitched surfaces of a hardware decoder are read / written in place.  Odd H and W are valid.  C = 3 only.
 *
 * COLOUR DEFINITION (the one place).  THIS IS THE PROJECT'S OWN DEFINITION: IT MAKES NO CLAIM OF BYTE PARITY WITH ANY OUTSIDE LIBRARY
 * (swscale, OpenCV, a vendor's colour-conversion block ...); those differ among themselves in rounding and chroma siting.
 * Standards: BT.601 Kr = 0.299, Kb = 0.114; BT.709 Kr = 0.2126, Kb = 0.0722; Kg = 1 - Kr - Kb.  All arithmetic is signed 32-bit integer
 * fixed point with 20 fractional bits: every coefficient is floor(k * 2^20 + 0.5) of its real value k computed in double, `>> 20` is
 * floor division by 2^20, clip is to 0..255.
 *   Decode (NV12 -> bytes): pixel (y, x) uses the chroma pair (y >> 1, x >> 1) (nearest upsampling); u = U - 128, v = V - 128;
 *     limited range: l = max(Y - 16, 0), CY = 255/219, s = 255/224;  full range: l = Y, CY = 1, s = 1;
 *     CVR = 2(1-Kr)s, CUG = -2Kb(1-Kb)s/Kg, CVG = -2Kr(1-Kr)s/Kg, CUB = 2(1-Kb)s;
 *     R = clip((CY l + CVR v + 2^19) >> 20), G = clip((CY l + CUG u + CVG v + 2^19) >> 20), B = clip((CY l + CUB u + 2^19) >> 20).
 *   Encode (bytes -> NV12): limited range: t = 219/255, s' = 224/255, yoff = 16;  full range: t = 1, s' = 1, yoff = 0;
 *     Y = clip(((YR R + YG G + YB B + 2^19) >> 20) + yoff) per pixel, (YR, YG, YB) = (Kr, Kg, Kb) t;
 *     chroma from the rounded mean of the 2x2 block: each of r, g, b = (sum of 4 + 2) >> 2, coordinates past the last row / column
 *     clamped (an odd edge block still has four samples);
 *     U = clip(((UR r + UG g + UB b + 2^19) >> 20) + 128), (UR, UG, UB) = (-Kr/(2(1-Kb)), -Kg/(2(1-Kb)), 0.5) s';
 *     V = clip(((VR r + VG g + VB b + 2^19) >> 20) + 128), (VR, VG, VB) = (0.5, -Kg/(2(1-Kr)), -Kb/(2(1-Kr))) s'.
 *   The integer tables, decode {CY, CVR, CUG, CVG, CUB} and encode {YR, YG, YB, UR, UG, UB, VR, VG, VB} (the worst intermediate,
 *   CY 239 + CUB 128 + 2^19 at BT.709 limited, is 5.8e8 < 2^31):
 *     EMAVFI_YUV_BT601_LIMITED decode {1220945, 1673555, -410793, -852458, 2115221}
 *                              encode {269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897}
 *     EMAVFI_YUV_BT601_FULL    decode {1048576, 1470104, -360853, -748826, 1858077}
 *                              encode {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}
 *     EMAVFI_YUV_BT709_LIMITED decode {1220945, 1879825, -223607, -558796, 2215014}
 *                              encode {191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230}
 *     EMAVFI_YUV_BT709_FULL    decode {1048576, 1651297, -196424, -490864, 1945738}
 *                              encode {222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074}
 *   emavfi_yuv_coefficients (host only) returns them.
 * `order`: which byte is channel 0 of the decoded / encoded pixel, i.e. which colour mean[0] / std[0] and plane 0 of the fp32 tensor
 *   belong to.  EMAVFI_ORDER_BGR is what cv2 hands the reference - which then normalises BGR with RGB statistics; that quirk is kept,
 *   it is the default of the Python layer -, EMAVFI_ORDER_RGB the alternative.
 * emavfi_preprocess_nv12 is DEFINED as emavfi_preprocess_u8 (C = 3) applied to the decoded bytes (the same fp32 /255, - mean, / std with
 *   true divisions in that order: bit for bit), emavfi_postprocess_nv12 as the encode of the bytes emavfi_postprocess_u8 would write (the
 *   same float64 arithmetic, truncation and NaN -> 0).
 * EMAVFI_E_ARG (never an abort): null pointers, y_pitch < W, uv_pitch < 2 ceil(W/2), for B > 1 a batch stride smaller than its plane, a
 *   zero std, an unknown standard or order, a Y or UV pointer that is not 2-byte aligned.  The Y and UV pointers are device pointers or
 *   pinned (device-mapped) host memory, as for the u8 entries; `mean` / `std`: host pointers to 3 values, fp32 / float64 as there.
 * Nothing is allocated, nothing synchronises, all work goes on `stream`.  Access width: with both byte pointers, pitches and batch
 *   strides multiples of 16, a 16-byte aligned fp32 pointer and W % 4 == 0, every full 2-row x 16-column block moves with 16-byte
 *   accesses; everything else (and the right / bottom remainders) takes a scalar path with the same per-element arithmetic. */
#define EMAVFI_YUV_BT601_LIMITED 0
#define EMAVFI_YUV_BT601_FULL 1
#define EMAVFI_YUV_BT709_LIMITED 2
#define EMAVFI_YUV_BT709_FULL 3
#define EMAVFI_ORDER_BGR 0
#define EMAVFI_ORDER_RGB 1
int emavfi_yuv_coefficients(int standard, int decode[5], int encode[9]);
int emavfi_preprocess_nv12(const unsigned char *y, size_t y_pitch, size_t y_batch_stride, const unsigned char *uv, size_t uv_pitch,
                           size_t uv_batch_stride, float *out_nchw, int B, int H, int W, int standard, int order,
                           const float *mean, const float *std, void *stream);
int emavfi_postprocess_nv12(const float *frames_nchw, unsigned char *y, size_t y_pitch, size_t y_batch_stride, unsigned char *uv,
                            size_t uv_pitch, size_t uv_batch_stride, int B, int H, int W, int standard, int order,
                            const double *mean, const double *std, int denormalize, void *stream);

/* HIGH BIT DEPTH frames, in and out: P010, P012 and P016 - what decoders of HEVC Main10, AV1 10-bit and HDR / UHD material produce.  NV12's
 * layout with 16-bit little-endian words: a Y plane [H][W] of words and a plane of interleaved U,V word pairs [ceil(H/2)][ceil(W/2)][2], each
 * plane with its own pointer, row pitch and batch stride, all in BYTES.  `depth` d is 10, 12 or 16; the sample of a word is word >> (16 - d):
 * the low 16 - d bits are ignored on read and written as zero.  Odd H and W are valid.  The reference has no counterpart (cv2 is 8-bit).
 *
 * HIGH BIT DEPTH COLOUR DEFINITION (the one place).  THE PROJECT'S OWN DEFINITION, AS FOR NV12: NO CLAIM OF PARITY WITH ANY OUTSIDE LIBRARY.
 * Constants: P = 2^d - 1, mid = 2^(d-1); limited range: yoff = 16 2^(d-8), Yr = 219 2^(d-8), Cr = 224 2^(d-8); full range: yoff = 0, Yr = Cr = P.
 * Standards: the four codes of NV12 plus EMAVFI_YUV_BT2020_LIMITED / _FULL (BT.2020 non-constant luminance: Kr = 0.2627, Kb = 0.0593), which
 *   only the entries of this section accept: the 8-bit entries and emavfi_yuv_coefficients keep refusing them.
 * Coefficients: the NV12 formulas above with 255/219 -> P/Yr, 255/224 -> P/Cr, 219/255 -> Yr/P, 224/255 -> Cr/P, each floor(k 2^20 + 0.5) of
 *   its real value k computed in double.  emavfi_yuv_coefficients_depth (host only) returns them as decode {CY, CVR, CUG, CVG, CUB} and encode
 *   {YR, YG, YB, UR, UG, UB, VR, VG, VB}; it also takes depth 8, where it returns exactly emavfi_yuv_coefficients' tables.  For
 *     EMAVFI_YUV_BT2020_LIMITED at depth 10: decode {1224536, 1765394, -197003, -684025, 2252416}
 *                                            encode {235879, 608777, 53246, -128236, -330964, 459200, 459200, -422268, -36933}
 * Arithmetic: signed 64-BIT integer fixed point with 20 fractional bits (the worst decode intermediate is 3.6e9 at depth 10 and 2.3e11 at
 *   depth 16: NV12's 32 bits do not hold it); `>> 20` is floor division by 2^20, clip is to 0..P.
 *   Decode, per pixel: the chroma pair of pixel (y, x) is (y >> 1, x >> 1); l = max(Y - yoff, 0), u = U - mid, v = V - mid;
 *     R = clip((CY l + CVR v + 2^19) >> 20), G = clip((CY l + CUG u + CVG v + 2^19) >> 20), B = clip((CY l + CUB u + 2^19) >> 20):
 *     three d-bit integers, not bytes.
 *   Encode: Y = clip(((YR R + YG G + YB B + 2^19) >> 20) + yoff) per pixel; chroma from the rounded mean of the 2x2 block of d-bit integers,
 *     each of r, g, b = (sum of 4 + 2) >> 2, coordinates past the last row / column clamped;
 *     U = clip(((UR r + UG g + UB b + 2^19) >> 20) + mid), V = clip(((VR r + VG g + VB b + 2^19) >> 20) + mid).
 * emavfi_preprocess_p010 is DEFINED as fp32 ((float(v) / float(P)) - mean[c]) / std[c] of the decoded integers v: true divisions in that
 *   order, emavfi_preprocess_u8's arithmetic with 255 -> P.  emavfi_postprocess_p010 is DEFINED as the encode of the integers
 *   trunc(clip(x std + mean, 0, 1) P) in float64, NaN -> 0, `denormalize` = 0 skipping the affine step: emavfi_postprocess_u8's arithmetic
 *   with 255 -> P.  `order`, `mean`, `std`: as for NV12.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer; depth outside {10, 12, 16}; a standard outside 0..5; an
 *   unknown order; y_pitch < 2 W or odd; uv_pitch < 4 ceil(W/2) or no multiple of 4; a Y pointer that is not 2-byte, a UV pointer that is not
 *   4-byte aligned; for B > 1 a batch stride smaller than its plane (or one that breaks its plane's alignment); a zero std; B, H or W below 1.
 * The Y and UV pointers are device pointers or pinned (device-mapped) host memory.  Nothing is allocated, nothing synchronises, all work goes
 *   on `stream`.  Access width: with both word pointers, pitches and batch strides multiples of 16, a 16-byte aligned fp32 pointer and
 *   W % 4 == 0, every full 2-row x 8-column block moves with 16-byte accesses (two of Y, one of UV, twelve of fp32); everything else (and the
 *   right / bottom remainders) takes a scalar path with the same per-element arithmetic (csrc/p010_elem.h). */
#define EMAVFI_YUV_BT2020_LIMITED 4
#define EMAVFI_YUV_BT2020_FULL 5
int emavfi_yuv_coefficients_depth(int standard, int depth, int decode[5], int encode[9]);
int emavfi_preprocess_p010(const void *y, size_t y_pitch, size_t y_batch_stride, const void *uv, size_t uv_pitch, size_t uv_batch_stride,
                           float *out_nchw, int B, int H, int W, int depth, int standard, int order, const float *mean, const float *std,
                           void *stream);
int emavfi_postprocess_p010(const float *frames_nchw, void *y, size_t y_pitch, size_t y_batch_stride, void *uv, size_t uv_pitch,
                            size_t uv_batch_stride, int B, int H, int W, int depth, int standard, int order, const double *mean,
                            const double *std, int denormalize, void *stream);

/* PLANAR 4:2:0 frames, in and out: what software decoders produce (yuv420p, yuv420p10le ...) and what a YUV4MPEG2 stream holds - a Y plane
 * [H][W], a U plane and a V plane of [ceil(H/2)][ceil(W/2)] samples each.  Every plane has its own pointer, row pitch and batch stride, all in
 * BYTES; odd H and W are valid; YV12 is the caller swapping the U and V arguments.  `depth` is 8, 10, 12 or 16.  Depth 8: one byte per sample.
 * Depth d > 8: one 16-bit little-endian word per sample with the sample in the word's LOW d bits (the yuv420p10le convention, Y4M's C420p10;
 * P010 keeps it in the top bits): a word is masked to its low d bits on read, the high 16 - d bits are written as zero.
 *
 * DEFINITION BY COMPOSITION: there is no new colour definition.
 *   depth 8:  emavfi_preprocess_yuv420p / emavfi_postprocess_yuv420p are DEFINED as emavfi_preprocess_nv12 / emavfi_postprocess_nv12 on the
 *     chroma plane uv[i][j] = {U[i][j], V[i][j]}, bit for bit.  Standards 0..3.
 *   depth d > 8: they are DEFINED as emavfi_preprocess_p010 / emavfi_postprocess_p010 at that depth on the words (w & (2^d - 1)) << (16 - d);
 *     the written words are those entries' words >> (16 - d).  Standards 0..5 (BT.2020 included).
 *   `order`, `mean`, `std`, NaN -> 0, truncation and `denormalize`: as in those entries.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer; depth outside {8, 10, 12, 16}; a standard outside its range
 *   for that depth; an unknown order; y_pitch / u_pitch / v_pitch smaller than its row (W, ceil(W/2), ceil(W/2) samples); at depth > 8 an odd
 *   pitch or a Y / U / V pointer that is not 2-byte aligned; for B > 1 a batch stride smaller than its plane (at depth > 8: or odd); a zero std;
 *   B, H or W below 1; an fp32 pointer that is not 4-byte aligned.
 * The Y, U and V pointers are device pointers or pinned (device-mapped) host memory.  Nothing is allocated, nothing synchronises, all work goes
 *   on `stream`.  Access width: with the Y pointer, its pitch and (B > 1) its batch stride multiples of 16, those of U and of V multiples of 8,
 *   a 16-byte aligned fp32 pointer and W % 4 == 0, every full block of 2 rows x 16 BYTES of Y (NV12's / P010's block: 16 columns at depth 8, 8
 *   above) moves with two 16-byte accesses of Y, twelve / twenty-four of fp32 and one 8-BYTE access of U and of V - a planar chroma row is half
 *   as wide as NV12's; chroma is 0.5 - 1 of the 13.5 - 15 bytes per pixel, so it takes the narrower access and the fp32 side, which carries 12,
 *   keeps NV12's / P010's pattern (profiles/r15_yuv420p_y4m.md times this block beside one twice as wide with 16-byte chroma accesses; 1280 x 720 and 1920 x 1080 frames stored densely plane after plane qualify at every depth); everything else (and the
 *   right / bottom remainders) takes a scalar path with the same per-element arithmetic.  Pitch padding is never read or written. */
int emavfi_preprocess_yuv420p(const void *y, size_t y_pitch, size_t y_batch_stride, const void *u, size_t u_pitch, size_t u_batch_stride,
                              const void *v, size_t v_pitch, size_t v_batch_stride, float *out_nchw, int B, int H, int W, int depth,
                              int standard, int order, const float *mean, const float *std, void *stream);
int emavfi_postprocess_yuv420p(const float *frames_nchw, void *y, size_t y_pitch, size_t y_batch_stride, void *u, size_t u_pitch,
                               size_t u_batch_stride, void *v, size_t v_pitch, size_t v_batch_stride, int B, int H, int W, int depth,
                               int standard, int order, const double *mean, const double *std, int denormalize, void *stream);

/* Frames resized on the device: the reference's `--scale` step, cv2.resize(frame, (int(w * scale), int(h * scale))), inference.py:46 / :93-94,
 * which it applies to every decoded frame before ToTensor / Normalize.
 *
 * RESIZE DEFINITION (the one place).  THIS IS THE PROJECT'S OWN DEFINITION: IT MAKES NO CLAIM OF BYTE PARITY WITH ANY OUTSIDE LIBRARY (OpenCV,
 * swscale, ...).  The geometry is that of cv2.resize's default INTER_LINEAR and of F.interpolate(mode="bilinear", align_corners=False):
 * half-pixel centres, clamped at the edges; the weights are quantised to 11 bits and all arithmetic is signed 32-bit integer, so host, oracle
 * and device agree bit for bit.  Per axis, for destination length nd, source length ns and destination index d (`/` is floor division):
 *     num = clamp((2d + 1) ns - nd, 0, 2 nd (ns - 1))
 *     i0  = num / (2 nd)
 *     fr  = num - i0 2 nd
 *     w   = (fr 2048 + nd) / (2 nd)          (0 .. 2048)
 *     i1  = min(i0 + 1, ns - 1)
 * Per byte, with wx / wy the column / row weights and (x0, x1) / (y0, y1) the column / row indices:
 *     v = ( (2048 - wy) ((2048 - wx) p[y0][x0] + wx p[y0][x1])
 *         +         wy  ((2048 - wx) p[y1][x0] + wx p[y1][x1]) + 2^21 ) >> 22
 * Each channel of an interleaved image is resized independently.  Every dimension is at most 16384 (EMAVFI_RESIZE_MAX_DIM): the largest
 * intermediates, (2d + 1) ns and 2048 * 2048 * 255 + 2^21, then stay below 2^31.  Up-scaling and down-scaling both use this formula; there is
 * no antialias filter (INTER_LINEAR has none either).  Consequences the tests pin: equal sizes return the input bytes; an exact 2:1 reduction
 * is (a + b + c + d + 2) >> 2 of each 2x2 block; a constant image stays constant; |byte - real-valued bilinear| <= 0.5 + 255 * 2 * (0.5 / 2048)
 * = 0.6245.
 *
 * emavfi_resize_u8: the primitive.  src [B][Hs][Ws][C] -> dst [B][Hd][Wd][C], interleaved bytes, C in 1..4 (1: a Y plane, 2: a UV plane, 3: a
 *   BGR frame); each side has its own row pitch and batch stride in bytes.  Bytes between the rows of a pitched destination are left as they were.
 * emavfi_preprocess_u8_resized: dense frames_hwc [B,Hs,Ws,C] -> out_nchw fp32 [B,C,Hd,Wd]; DEFINED as emavfi_preprocess_u8 applied to
 *   emavfi_resize_u8's bytes, bit for bit.  ONE launch that reads the source once and never writes the resized bytes to memory - unless
 *   `resized_hwc` (dense [B,Hd,Wd,C]; NULL skips it) asks for them: the frame the reference writes "as read" (inference.py:167) is the resized one.
 * emavfi_preprocess_nv12_resized: pitched Y / UV planes at Hs x Ws -> out_nchw fp32 [B,3,Hd,Wd]; DEFINED as emavfi_preprocess_nv12 applied to
 *   the Y plane resized as a 1-channel image to Hd x Wd and the UV plane resized as a 2-channel image from ceil(Hs/2) x ceil(Ws/2) to
 *   ceil(Hd/2) x ceil(Wd/2), bit for bit.  ONE launch; optional pitched `y_out` / `uv_out` receive the resized planes (NULL skips either).
 * EMAVFI_E_ARG (never an abort): a pitch smaller than its row, for B > 1 a batch stride smaller than its plane, a dimension below 1 or above
 *   16384, C outside 1..4, a null required pointer, a zero std; for NV12 an unknown standard or order and planes that are not 2-byte aligned.
 * The byte pointers are device pointers or pinned (device-mapped) host memory, as for the u8 entries; `mean` / `std`: host pointers, fp32.
 * Nothing is allocated, nothing synchronises, all work goes on `stream`.  Access width: a workgroup stages the source span of its tile of the
 *   destination in LDS - with 16-byte loads when the source pointer, pitch and batch stride are multiples of 16 - and stores fp32 with 16-byte
 *   accesses when Wd % 4 == 0 and the fp32 pointer is 16-byte aligned; everything else takes byte / dword accesses with the same per-element
 *   arithmetic. */
#define EMAVFI_RESIZE_MAX_DIM 16384
int emavfi_resize_u8(const unsigned char *src, size_t src_pitch, size_t src_batch_stride, unsigned char *dst, size_t dst_pitch,
                     size_t dst_batch_stride, int B, int Hs, int Ws, int Hd, int Wd, int C, void *stream);
int emavfi_preprocess_u8_resized(const unsigned char *frames_hwc, float *out_nchw, unsigned char *resized_hwc, int B, int Hs, int Ws, int Hd,
                                 int Wd, int C, const float *mean, const float *std, void *stream);
int emavfi_preprocess_nv12_resized(const unsigned char *y, size_t y_pitch, size_t y_batch_stride, const unsigned char *uv, size_t uv_pitch,
                                   size_t uv_batch_stride, float *out_nchw, unsigned char *y_out, size_t y_out_pitch, size_t y_out_batch_stride,
                                   unsigned char *uv_out, size_t uv_out_pitch, size_t uv_out_batch_stride, int B, int Hs, int Ws, int Hd, int Wd,
                                   int standard, int order, const float *mean, const float *std, void *stream);

/* Scene cuts, decided and applied on the device.  When frame a ends one shot and frame b starts the next, a motion-compensated blend of the two
 * is a ghosted mixture; a video tool holds the earlier frame instead.  The reference has no such guard (inference.py:173-188 interpolates every
 * pair); this is an addition, off unless asked for.  The decision is made from the frame bytes already on the device and applied there: the
 * host learns of it only together with the frames it waits for anyway.
 *
 * SCENE CUT DEFINITION (the one place).  This is the project's own definition: it follows no outside tool's scene detector (Practical-RIFE,
 * ffmpeg's minterpolate scd, ...) and claims agreement with none.  All arithmetic is unsigned 32-bit integer, `/` is floor division: host,
 * oracle and device agree bit for bit.
 *   Luma of a pixel.  C = 1: the byte itself (a Y plane, as NV12 stores it).  C = 3: (313524 R + 615514 G + 119538 B + 2^19) >> 20 - the
 *     encode row of EMAVFI_YUV_BT601_FULL above; it sums to 2^20, so the result is 0..255 with no clip.  `order` (EMAVFI_ORDER_BGR /
 *     EMAVFI_ORDER_RGB) says which byte is R; it is ignored (but still validated) at C = 1.
 *   Signature of a frame: EMAVFI_SCENE_GRID x EMAVFI_SCENE_GRID = 32 x 32 cells, EMAVFI_SCENE_SIG_WORDS = 1024 u32.  Cell (i, j) covers rows
 *     [i H / 32, (i + 1) H / 32) and columns [j W / 32, (j + 1) W / 32); with H < 32 or W < 32 some cells hold no pixel (empty cells).
 *     sig[i 32 + j] = the sum of the luma over the cell, 0 for an empty cell.  H and W are 1..16384: the largest cell is 512 x 512 pixels,
 *     so 16 sum + n / 2 <= 16 * 255 * 2^18 + 2^17 < 2^31.
 *   Score of a pair: for every non-empty cell of n pixels m = (16 sum + n / 2) / n (the cell's mean in sixteenths of a count, 0..4080);
 *     score = the sum over the cells of |m_a - m_b|, 0 .. 4080 cells with cells = min(H, 32) min(W, 32);  flag = score >= threshold.
 *     `threshold` is in score units.  A caller who thinks of "the mean absolute difference of the two 32 x 32 thumbnails as a fraction of
 *     full scale" passes ceil(fraction * 4080 * cells) (the Python layer's scene_threshold_units does).
 *
 * emavfi_luma_signature_u8: src [B][H][W][C] bytes, C = 1 or 3, rows `pitch` bytes apart, frames `batch_stride` bytes apart -> sig [B][1024]
 *   u32 in device memory.  EVERY one of the B * 1024 words is written, whatever the buffer held before (empty cells: 0); a workgroup owns
 *   the cells it stores, so there are no global atomics and nothing has to be zeroed first.
 * emavfi_scene_flags: pair k < n compares the signatures at sig_a + k stride_a_words and sig_b + k stride_b_words (strides in u32 words: 0 -
 *   every pair against the one signature - or at least 1024) of H x W frames; writes flags[k] = 0 / 1 and, unless `scores` is NULL, scores[k].
 * emavfi_hold_frames_u8: for every k < n with flags[k] != 0 the frame_bytes bytes at alt + k alt_stride are copied over each of the `rep`
 *   frames at dst + (k rep + r) dst_stride, r < rep.  Frames of unflagged pairs and bytes between frames are left as they were.
 * EMAVFI_E_ARG (never an abort): a null required pointer, B, n or rep below 1 (or above 65535: B, n of emavfi_hold_frames_u8, rep), a
 *   dimension below 1 or above 16384, C outside {1, 3}, an unknown order, a pitch smaller than its row, for B > 1 a batch stride smaller
 *   than its plane, a u32 pointer that is not 4-byte aligned, a signature stride between 1 and 1023 words, frame_bytes of 0 or above
 *   2^40, for n rep > 1 a dst_stride or alt_stride smaller than frame_bytes, size arithmetic that overflows size_t.
 * The byte pointers are device pointers or pinned (device-mapped) host memory, as for the u8 entries; sig, flags and scores: device memory
 *   (or pinned).  Nothing is allocated, nothing synchronises, all work goes on `stream`.  Access width: the signature kernel reads 16 pixels
 *   per lane with 16-byte loads when the source pointer, the pitch and (B > 1) the batch stride are multiples of 16, and the right remainder
 *   of a row - or everything, otherwise - byte by byte with the same per-element functions (csrc/scene_elem.h); the hold kernel copies
 *   with 16-byte accesses when both frame addresses are 16-byte aligned (the last frame_bytes % 16 bytes: byte accesses), else byte by byte;
 *   a workgroup whose pair is not flagged leaves at once. */
#define EMAVFI_SCENE_GRID 32
#define EMAVFI_SCENE_SIG_WORDS 1024
int emavfi_luma_signature_u8(const unsigned char *src, size_t pitch, size_t batch_stride, int B, int H, int W, int C, int order, unsigned *sig,
                             void *stream);
int emavfi_scene_flags(const unsigned *sig_a, size_t stride_a_words, const unsigned *sig_b, size_t stride_b_words, int n, int H, int W,
                       unsigned threshold, unsigned *flags, unsigned *scores, void *stream);
int emavfi_hold_frames_u8(unsigned char *dst, size_t dst_stride, int rep, const unsigned char *alt, size_t alt_stride, const unsigned *flags, int n,
                          size_t frame_bytes, void *stream);

/* Frame-rate conversion.  The model produces midpoints only, so an output frame at an arbitrary time is assembled from the dyadic tree of
 * recursive midpoints between two source frames: a schedule the host knows ahead of time, and a selection or blend of already emitted frames
 * on the device.  The reference multiplies a frame rate by an integer and nothing else (inference.py:117: `--target-fps 60` on a 24 fps clip
 * writes 72 fps); this is an addition, off unless asked for.
 *
 * TEMPORAL RESAMPLE DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool (ffmpeg's
 * fps / minterpolate / framerate filters, ...).  All arithmetic is integer, `/` is floor division: host, oracle and device agree bit for bit.
 *   Time grid.  The input rate Fi and the output rate Fo are positive rationals with Fo >= Fi; P / Q = Fi / Fo in lowest terms (P <= Q).
 *     Output frame k = 0, 1, ... sits at source time k P / Q, in source-frame intervals: s = k P / Q, r = k P - s Q (0 <= r < Q).  A clip of
 *     n frames yields k = 0 .. ((n - 1) Q) / P, that is ((n - 1) Q) / P + 1 frames; n = 0 yields nothing, n = 1 the one frame.  r = 0 is
 *     source frame s itself.
 *   Nodes.  Depth D in 1..5, G = 2^D.  Node j (0 < j < G) of the pair (s, s + 1) is the recursive midpoint the harness's mode "recursive"
 *     with factor G - 1 emits as its j-th prediction: the model's midpoint of node j - (j & -j) and node j + (j & -j) (its parents), with
 *     the same fp32 recursion and the same re-normalisation of a midpoint before it is fed back.  Node 0 is source s, node G source s + 1.
 *   method "nearest": j = (2 r G + Q) / (2 Q) (0..G; a tie goes to the later node).  The output is node j.
 *   method "blend": j0 = (r G) / Q, e = r G - j0 Q, w = (256 e + Q / 2) / Q (0..256).  Per sample out = ((256 - w) A + w B + 128) >> 8 with
 *     A = node j0, B = node j0 + 1.  w = 0 is A alone and w = 256 is B alone: the other frame is not needed.  A sample is a byte, or the
 *     depth-bit value (word >> shift) & (2^depth - 1) of a 16-bit little-endian word, written back as v << shift.  The blend acts on the
 *     frames AS EMITTED: it is the same arithmetic for bgr24, NV12, P01x (shift = 16 - depth) and the planar formats (shift = 0), and it
 *     ignores the plane structure.  A blend mixes two model outputs 1 / G of a source interval apart; it is no motion compensation.
 *   Needed nodes of a pair: the nodes its outputs use, closed under parents; only these are computed.  24 -> 60 (P / Q = 2 / 5), D = 3,
 *     n = 5, blend, as (k, s, j0, j1, w) - j1 = j0 where w = 0:
 *       (0,0,0,0,0) (1,0,3,4,51) (2,0,6,7,102) (3,1,1,2,154) (4,1,4,5,205) (5,2,0,0,0) (6,2,3,4,51) (7,2,6,7,102) (8,3,1,2,154) (9,3,4,5,205)
 *       (10,4,0,0,0); needed nodes {2,3,4,6,7} for even pairs, {1,2,4,5,6} for odd pairs: 5 forwards per pair.  Nearest picks nodes 3, 6 | 2, 5
 *       and needs {2,3,4,6} / {2,4,5,6}: 4 per pair.  30 -> 60 needs one forward per pair at any D, a ratio of 1 none.
 *   Scene cuts (SCENE CUT DEFINITION above).  Every output with r > 0 of a flagged pair is source frame s.
 *
 * emavfi_resample_frames assembles n_out output frames, in emission order, at dst + k dst_stride from two pools of dense frames of
 *   frame_bytes bytes each: `srcs` (n_srcs source frames as emitted, src_stride bytes apart) and `nodes` (n_nodes post-processed node
 *   frames, node_stride apart; a pool of 0 frames may be NULL).  `table` is a HOST pointer to n_out entries {a, b, w, f, h}: a, b = a frame
 *   index, plus EMAVFI_RESAMPLE_NODES when it counts in `nodes`; w = 0..256; f = 0, or 1 + an index into the device array `flags` of
 *   n_flags u32 (may be NULL: then no entry is held); h = the index in `srcs` of the frame to hold.  The table is read and validated
 *   before the call returns and nothing of it is retained: it travels as kernel arguments, EMAVFI_RESAMPLE_LAUNCH_CAP = 64 entries per
 *   launch, so n_out entries take ceil(n_out / 64) launches.  Per entry:
 *     flags != NULL, f != 0 and flags[f - 1] != 0: srcs[h] is copied;  else w = 0: a is copied;  else w = 256: b is copied;  else every
 *     sample is blended.  A copy never reads (nor forms the address of) the frame it does not use; bytes between output frames are left as
 *     they were.  sample_bytes 1 takes depth 8 and shift 0; sample_bytes 2 takes depth 10, 12 or 16 and shift 0 .. 16 - depth.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null dst or table, a null pool or flags with a count above 0, n_out below
 *   1, a negative count, sample_bytes outside {1, 2}, a depth or shift outside the above, frame_bytes of 0 or above 2^40 or odd at
 *   sample_bytes 2, a stride (of dst, or of a pool that has frames) below frame_bytes or odd at sample_bytes 2, size arithmetic that
 *   overflows size_t, a dst / srcs / nodes pointer that is not 2-byte aligned at sample_bytes 2, a flags pointer that is not 4-byte aligned,
 *   dst overlapping either pool, and per entry an a or b outside its pool (also where w makes it unused), w above 256, f beyond n_flags,
 *   for f != 0 an h outside srcs.
 * The frame pointers are device pointers or pinned (device-mapped) host memory, `flags` device (or pinned) memory.  Nothing is allocated,
 *   nothing synchronises, all work goes on `stream`.  Access width: an entry moves 16 bytes per lane where every frame address IT USES
 *   (dst and a, b or srcs[h]) is 16-byte aligned - the last frame_bytes % 16 bytes: bytes / words -, else bytes (sample_bytes 1) or words
 *   throughout; all forms run the same per-element functions (csrc/resample_elem.h).  The kernel is short-lived and waits on nothing. */
#define EMAVFI_RESAMPLE_NODES 0x80000000u
#define EMAVFI_RESAMPLE_LAUNCH_CAP 64
typedef struct { unsigned a, b, w, f, h; } emavfi_resample_entry;
int emavfi_resample_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                           const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_resample_entry *table,
                           const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift, void *stream);

/* Motion blur.  Every frame the resampler emits is an instantaneous sample of the motion; a camera frame integrates light while the shutter
 * is open.  With a shutter angle every output frame becomes the weighted mean of the tree nodes inside its exposure window, summed on the
 * device: only the accumulated frames leave it.  The reference has nothing of the kind; this is an addition, off unless asked for.
 *
 * SHUTTER DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.  It extends the
 * TEMPORAL RESAMPLE DEFINITION; all arithmetic is integer, `/` is floor division: host, oracle and device agree bit for bit.
 *   Scope.  P = 1 only: the output rate is an integer multiple Q >= 1 of the input rate (Q = 1, "add motion blur", included), so that every
 *     window stays inside its pair.  P > 1 (24 -> 60) would cross pair and batch boundaries and is refused.
 *   Exposure.  e = shutter / 360 = n / d in lowest terms, 0 < e <= 1.  Output k has s = k / Q, r = k - s Q; it opens at source time s + r / Q
 *     and stays open for e / Q of a source interval: the angle refers to the OUTPUT frame period.
 *   Weights, in units of 1 / (2 G Q d) of a source interval, G = 2^D: the window is [2 G d r, 2 G d r + 2 G n]; node j (0 .. G; 0 and G are
 *     the two source frames) owns the cell [(2 j - 1) Q d, (2 j + 1) Q d]; w_j = max(0, min(cell_hi, win_hi) - max(cell_lo, win_lo)).  The
 *     nonzero weights are contiguous and sum to 2 G n: the trapezoid rule on the node lattice.  They are divided by their gcd; the taps of the
 *     output are the (j, w_j) with w_j > 0, S = sum w_j.  Refused: S > 65535 after the reduction, and an exposure shorter than one node
 *     spacing (e / Q < 1 / G, that is G n < Q d: raise the depth).
 *   Per sample out = (sum w_j s_j + S / 2) / S, s_j the sample of node j: a byte, or (word >> shift) & (2^depth - 1) of a 16-bit
 *     little-endian word, written back as v << shift.  The largest intermediate is 65535 * 65535 + 32767 < 2^32: unsigned 32-bit holds
 *     everything.  The mean acts on the frames AS EMITTED, the same arithmetic for every pixel format, as the blend above; it averages the
 *     coded samples (in light: emavfi_accumulate_frames_linear below).  A single tap copies its frame byte for byte; a single-tap output with j = 0 is the source frame.
 *   Scene cuts.  Every output of a flagged pair is source frame s, those with r = 0 and those whose taps reach node G (the next shot) included.
 *   The last frame.  The output that falls on the last source frame of a clip has no pair to integrate over: it is that frame itself.
 *   Needed nodes of a pair: the taps of its outputs, closed under parents; only these are computed.
 *   Known answers, (Q, D, shutter, r) -> (j,w) ...:  (1, 2, 180, 0) -> (0,1) (1,2) (2,1);  (1, 2, 360, 0) -> (0,1) (1,2) (2,2) (3,2) (4,1);
 *     (1, 1, 180, 0) -> (0,1) (1,1);  (2, 2, 180, 0) -> (0,1) (1,1);  (2, 2, 180, 1) -> (2,1) (3,1);  (3, 3, 270, 1) -> (3,5) (4,6) (5,1),
 *     needed nodes {2,3,4,5,6};  (1, 1, 90, 0) is refused.  At 180 degrees and D = 3 a pair needs nodes {1,2,3,4}: 4 forwards instead of 7.
 *
 * emavfi_accumulate_frames assembles n_out output frames at dst + k dst_stride from the two pools of emavfi_resample_frames, under the same
 *   contract: `table` is a HOST pointer to n_out entries {n, f, h, tap[33], w[33]}, read and validated before the call returns, nothing of it
 *   retained; it travels as kernel arguments, EMAVFI_ACCUMULATE_LAUNCH_CAP = 8 entries per launch.  tap[i] (i < n) = a frame index in
 *   `srcs`, or EMAVFI_RESAMPLE_NODES + an index in `nodes`; w[i] its weight; f, h the resample entry's hold: flags != NULL, f != 0 and
 *   flags[f - 1] != 0 copies srcs[h].  Else n = 1 copies tap[0]; else every sample is the mean above.  An entry never reads (nor forms the
 *   address of) a frame it does not use; bytes between output frames are left as they were; dst must not overlap a pool.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: every refusal of emavfi_resample_frames that applies (all but its a, b and
 *   w), and per entry n outside 1..33, a tap[i] (i < n) outside its pool, a w[i] of zero, weights that sum to more than 65535, f beyond
 *   n_flags, for f != 0 an h outside srcs.
 * Nothing is allocated, nothing synchronises, all work goes on `stream`.  Access width: an entry moves 16 bytes per lane and tap where every
 *   frame address IT USES is 16-byte aligned - the last frame_bytes % 16 bytes: bytes / words -, else bytes / words throughout; all forms
 *   run the same per-element functions (csrc/shutter_elem.h), the division by S as a multiply and a correction proven equal to `/` by
 *   tests/host/host_check_shutter.cpp.  The kernel is short-lived and waits on nothing. */
#define EMAVFI_ACCUMULATE_MAX_TAPS 33
#define EMAVFI_ACCUMULATE_LAUNCH_CAP 8
typedef struct { unsigned n, f, h; unsigned tap[EMAVFI_ACCUMULATE_MAX_TAPS]; unsigned w[EMAVFI_ACCUMULATE_MAX_TAPS]; } emavfi_accumulate_entry;
int emavfi_accumulate_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                             const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_accumulate_entry *table,
                             const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift, void *stream);

/* Linear light.  The blend and the shutter above average CODED samples.  A camera integrates light, and a coded sample is a gamma-like
 * function of light: a bright object blurred over a dark ground comes out too dark and too thin, and an even mix of black and white comes
 * out as code 128 where the light says 188 (sRGB).  With a transfer table the same taps are averaged in light, on the device.  The reference
 * has nothing of the kind; this is an addition, off unless asked for.
 *
 * LINEAR LIGHT DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.  It extends the
 * temporal resample and shutter definitions above; all device arithmetic is integer, `/` is floor division, floating point only builds a
 * table on the host: oracle and device agree bit for bit.
 *   Table.  lin[0 .. 2^depth - 1], unsigned 32-bit, depth 8, 10 or 12: lin[v] = BIAS + round(ONE g(x)), ONE = 2^28, BIAS = 2^26,
 *     x = (v - lo) / (hi - lo), (lo, hi) = (0, 2^depth - 1) at full range and (16, 235) << (depth - 8) at limited range.  g is the inverse
 *     transfer function on x >= 0 and -g(-x) on x < 0 (the odd extension): codes below black and above white keep distinct, ordered values.
 *     Built in:  EMAVFI_TRANSFER_SRGB: x / 12.92 for x <= 0.04045, else ((x + 0.055) / 1.055)^2.4.  EMAVFI_TRANSFER_BT709: the inverse OETF
 *     with BT.2020's precise constants alpha = 1.09929682680944, beta = 0.018053968510807: x / 4.5 below 4.5 beta, else
 *     ((x + alpha - 1) / alpha)^(1 / 0.45) (the rounded 1.099 / 0.081 are discontinuous at the knee: the 12-bit full-range table would not be
 *     monotone).  EMAVFI_TRANSFER_HLG: the inverse HLG OETF, x^2 / 3 for x <= 0.5, else (exp((x - c) / a) + b) / 12 with a = 0.17883277,
 *     b = 0.28466892, c = 0.55991073.  A VALID table is strictly increasing with every value below 2^30.  The three built-ins are valid at
 *     depths 8, 10 and 12 in both ranges (smallest step 5: HLG, 12-bit, full range; largest value 520 767 148); lin[lo] = BIAS exactly, lin[hi]
 *     within 8 of BIAS + ONE (HLG's rounded constants: + 7).  Depth 16 is refused: 256 KiB of table exceed the 160 KiB of LDS, and the built-ins
 *     lose strictness there.  PQ and a pure power law lose it at 12 bits and are not built in; the entry takes any table that passes the check.
 *   Encode.  enc(L) = the largest v with v = 0 or lin[v - 1] + lin[v] <= 2 L: the code nearest in light, a tie going up, found by a
 *     depth-step binary search.  enc(lin[v]) = v for every valid table.
 *   Mean.  For an entry with taps (j, w_j), S = sum w_j <= 65535, every sample below linear_bytes is
 *     out = enc((sum w_j lin[s_j] + S / 2) / S); the largest intermediate, 65535 * (2^30 - 1) + 32767, is below 2^46: unsigned 64-bit.  A
 *     sample is extracted and written back as in the shutter definition: (word >> shift) & mask, then v << shift.
 *   linear_bytes.  The first linear_bytes bytes of every frame are mixed in light, the rest by the shutter definition's coded mean, word for
 *     word.  A multiple of sample_bytes, at most frame_bytes.  bgr24: the whole frame.  NV12, P010 / P012 and the planar formats: the Y
 *     plane, which comes first in the emitted frame; chroma stays coded.  For Y'CbCr THIS IS A LUMA-LINEAR APPROXIMATION, exact for greys:
 *     true RGB linear light for 4:2:0 would need chroma resampling and is out of scope.
 *   Copies.  As above: a flagged hold copies srcs[h], a single tap copies its frame byte for byte; an entry never reads (nor forms the
 *     address of) a frame it does not use.
 *   Consequences.  Taps that all hold sample v give v.  linear_bytes = 0 is emavfi_accumulate_frames byte for byte.  The affine table
 *     lin[v] = BIAS + 65536 v reproduces the coded mean bit for bit (S < 65536 keeps every tie where it was).
 *   Known answers, table: taps (sample, weight) -> linear light (coded mean):  sRGB 8-bit full: (0,1) (255,1) -> 188 (128);
 *     (0,3) (255,1) -> 137 (64).  bt709 8-bit limited: (16,1) (235,1) -> 170 (126);  (16,3) (235,1) -> 123 (71).
 *
 * emavfi_transfer_table builds a built-in table into lin_host (HOST memory, 2^depth words; pure host code).  EMAVFI_E_ARG: an unknown
 *   transfer, a depth outside {8, 10, 12}, a null pointer.
 * emavfi_transfer_table_check checks a host table: strictly increasing, every value below 2^30.  EMAVFI_E_ARG, the message naming the first
 *   offending index; also a depth outside {8, 10, 12} and a null pointer.
 * emavfi_accumulate_frames_linear is emavfi_accumulate_frames - the same entry struct, the same HOST table that travels as kernel arguments,
 *   EMAVFI_ACCUMULATE_LAUNCH_CAP entries per launch, every one of its refusals - plus `lin`, a DEVICE pointer (4-byte aligned) to the 2^depth
 *   words of a table, and linear_bytes.  It refuses as well: a null or misaligned lin, a depth outside {8, 10, 12}, linear_bytes above
 *   frame_bytes or no multiple of sample_bytes.  Never an abort; nothing is allocated, nothing synchronises, all work goes on `stream`.
 *   The device table is NOT validated on the device: the contract is that it passed emavfi_transfer_table_check.  The kernel is memory-safe
 *   for ANY table content: the decode index is masked to 2^depth, the search is bounded to the table.  A table that is not valid gives wrong
 *   samples and never an out-of-range access.
 * The kernel keeps the coded kernel's shape: grid (32 KiB pieces of a frame, entries of this launch), 256 threads, 16-byte accesses where
 *   every frame address an entry uses is 16-byte aligned, bytes / words otherwise.  A workgroup first copies lin into LDS (1, 4 or 16 KiB);
 *   decode is one LDS gather per sample and tap, encode `depth` steps over LDS.  A 16-byte piece across linear_bytes goes sample by sample,
 *   each by its own rule.  All forms run the same per-element functions (csrc/light_elem.h); the 46-bit quotient is three steps of schoolbook
 *   division in base 2^16 over shutter_div, proven equal to `/` on unsigned long long by tests/host/host_check_light.cpp. */
#define EMAVFI_TRANSFER_SRGB 0
#define EMAVFI_TRANSFER_BT709 1
#define EMAVFI_TRANSFER_HLG 2
#define EMAVFI_LIGHT_ONE (1u << 28)
#define EMAVFI_LIGHT_BIAS (1u << 26)
#define EMAVFI_LIGHT_LIMIT (1u << 30)
int emavfi_transfer_table(int transfer, int depth, int full_range, unsigned *lin_host);
int emavfi_transfer_table_check(const unsigned *lin_host, int depth);
int emavfi_accumulate_frames_linear(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                                    const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_accumulate_entry *table,
                                    const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift,
                                    const unsigned *lin, size_t linear_bytes, void *stream);

/* Duplicate frames.  The resampler above puts every output frame at its true time and assumes that every INPUT frame sits at its true time
 * too.  24 fps film in a 30 fps stream, animation drawn on twos, screen captures and anything that went through a frame-rate filter break
 * that: some frames are copies of the frame before them, an (A, A) pair yields A again, and the motion A -> B is squeezed into one interval.
 * The reference has no guard for this (inference.py:173-188 interpolates every pair); this is an addition, off unless asked for.  The copies
 * are found on the device, dropped, and the resampler interpolates across the gap they leave.
 *
 * DUPLICATE FRAME DEFINITION (the one place).  This is the project's own definition: it follows no outside tool's de-duplication (ffmpeg's
 * mpdecimate, ...) and claims agreement with none.  All arithmetic is integer, `/` is floor division: host, oracle and device agree bit for bit.
 *   Sample.  A byte, or (word >> shift) & (2^depth - 1) of a 16-bit little-endian word: depth 10, 12 or 16 and shift 0 .. 16 - depth, the
 *     triple emavfi_resample_frames takes (sample_bytes 1: depth 8, shift 0).
 *   Luma.  C = 1: the sample itself.  C = 3 (bytes only): the luma of the SCENE CUT DEFINITION, with the same `order` argument.
 *   Cells.  The scene grid: EMAVFI_SCENE_GRID x EMAVFI_SCENE_GRID = 32 x 32 cells with the same bounds - cell (i, j) covers rows
 *     [i H / 32, (i + 1) H / 32) and columns [j W / 32, (j + 1) W / 32); with H < 32 or W < 32 some cells hold no pixel (empty cells).
 *   Per cell of n pixels.  sad = the sum of |luma_a - luma_b|, an unsigned 64-bit integer: at most 65535 * 2^18, so 16 sad < 2^38.
 *     m = (16 sad + n - 1) / n: the CEILING of the cell's mean absolute difference in sixteenths of a count.  m = 0 exactly when the cell's
 *     luma is identical; m <= 16 (2^depth - 1) <= 1 048 560 fits u32.  An empty cell gives 0.
 *   Score of a pair: the MAXIMUM of m over the cells.  (The sum would let coding noise spread over 1024 cells outvote the one cell in which
 *     something moved; the scene signature, which compares cell means, cannot see a small moving object at all.)
 *   Duplicate: score <= threshold, `threshold` in score units.  A caller who thinks of a fraction f of full scale passes
 *     floor(f * 16 * (2^depth - 1)), depth 8 for bytes (the Python layer's dedup_threshold_units does).  A threshold of 0 flags exactly the
 *     pairs whose luma is bit-identical.
 *   Schedule (extends the TEMPORAL RESAMPLE DEFINITION; host-side integers).  Of n source frames, frame t >= 1 is DROPPED when the pair
 *     (t - 1, t) is flagged, unless it is KEPT regardless: t = 0, the last frame, t % span = 0 (span: 64 by default, on the global frame index -
 *     a chunk of a chunked run then sees exactly what the whole clip would), and the frame that follows max_run dropped frames in a row
 *     (max_run: 3 by default; it bounds the drift and the gap).  Consecutive kept frames t_i < t_i+1 form a gap of m = t_i+1 - t_i intervals,
 *     1 <= m <= max_run + 1.  The output count and times are unchanged: output k has s = k P / Q, r = k P - s Q, and is served from the gap
 *     with t_i <= s < t_i+1 at R = (s - t_i) Q + r over the denominator m Q, in a tree of depth D_m = D + ceil(log2 m), G_m = 2^D_m - never
 *     coarser than 1 / 2^D of a SOURCE interval.  The formulas above apply with r -> R, Q -> m Q, G -> G_m:
 *       nearest: j = (2 R G_m + m Q) / (2 m Q);  blend: j0 = (R G_m) / (m Q), e = R G_m - j0 m Q, w = (256 e + m Q / 2) / (m Q).
 *     R = 0 is source t_i itself; m = 1 is the TEMPORAL RESAMPLE DEFINITION word for word.  Needed nodes are closed under parents, as before.
 *     D + ceil(log2(max_run + 1)) must not exceed 5, the deepest tree.  Scene cuts are decided on the kept pair (t_i, t_i+1): a flagged gap
 *     yields t_i for every output with R > 0.  A ratio of 1 is valid: the dropped frames are replaced by interpolated ones.
 *
 * emavfi_frame_diff_cells: pair k < n compares image k of `a` ([n][H][W][C] samples, rows a_pitch BYTES apart, images a_batch_stride BYTES
 *   apart) with image k of `b` and writes cells[k][1024] = m.  EVERY one of the n * 1024 words is written, whatever the buffer held before
 *   (empty cells: 0); a workgroup owns the cells it stores, so there are no global atomics and nothing has to be zeroed first.  `a` and `b`
 *   may overlap - both are only read: the consecutive frames of one buffer of B frames are b = a + batch_stride, n = B - 1.
 * emavfi_duplicate_flags: pair k < n reads the 1024 words at cells + k stride_words; writes flags[k] = 0 / 1 and, unless `scores` is NULL,
 *   scores[k] = the maximum.
 * EMAVFI_E_ARG (never an abort): the refusals of emavfi_luma_signature_u8 (a null required pointer, n below 1, n of emavfi_frame_diff_cells
 *   above 65535, a dimension below 1 or above 16384, C outside {1, 3}, an unknown order, a pitch smaller than its row, for n > 1 a batch
 *   stride smaller than its plane, a u32 pointer that is not 4-byte aligned, size arithmetic that overflows size_t), and: sample_bytes outside
 *   {1, 2}, a depth or shift outside the above, C = 3 at sample_bytes 2, and at sample_bytes 2 an odd pitch, (n > 1) an odd batch stride or an
 *   image pointer that is not 2-byte aligned; for emavfi_duplicate_flags a stride below 1024 words.
 * The image pointers are device pointers or pinned (device-mapped) host memory; cells, flags and scores: device memory (or pinned).  Nothing
 *   is allocated, nothing synchronises, all work goes on `stream`.  Access width, per image: 16 pixels per lane with 16-byte loads when that
 *   image's pointer, pitch and (n > 1) batch stride are multiples of 16, and the right remainder of a row - or everything, otherwise - byte by
 *   byte with the same per-element functions (csrc/dedup_elem.h, csrc/scene_elem.h).  Per-lane partial sums are 32-bit (at most 8240 pixels
 *   per lane), a cell's total is 64-bit.  Both kernels are short-lived and wait on nothing. */
int emavfi_frame_diff_cells(const unsigned char *a, size_t a_pitch, size_t a_batch_stride, const unsigned char *b, size_t b_pitch,
                            size_t b_batch_stride, int n, int H, int W, int C, int order, int sample_bytes, int depth, int shift,
                            unsigned *cells, void *stream);
int emavfi_duplicate_flags(const unsigned *cells, size_t stride_words, int n, unsigned threshold, unsigned *flags, unsigned *scores, void *stream);

/* Static regions.  Channel logos, subtitles, scoreboards, game HUDs, letterbox bars and the unchanged background of screen captures and
 * animation are bit-identical, or nearly so, in both frames of a pair, yet the forward pushes them through a flow warp and three deformable
 * convolutions, and whatever the model does next to a moving object leaks into pixels whose true midpoint is known exactly: the pixel itself.
 * The reference has no guard for this (inference.py:173-188 writes the prediction as it comes); this is an addition, off unless asked for.
 *
 * STATIC REGION DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.  All arithmetic is
 * integer: host, oracle and device agree bit for bit.
 *   Frame layouts.  A frame is dense, with no pitch, as the harness emits it; sample_bytes is 1 or 2.
 *     EMAVFI_LAYOUT_INTERLEAVED: [H][W][C] samples, C in 1..4.
 *     EMAVFI_LAYOUT_NV12: [H][W] Y samples, then [H/2][W/2] pairs {U, V}.
 *     EMAVFI_LAYOUT_I420: the Y plane, then the U plane [H/2][W/2], then the V plane [H/2][W/2].
 *     The two 4:2:0 layouts need an even H and W.
 *   Sample.  A byte, or (word >> shift) & (2^depth - 1) of a 16-bit little-endian word: depth 10, 12 or 16 and shift 0 .. 16 - depth, the
 *     triple emavfi_resample_frames / emavfi_frame_diff_cells take (sample_bytes 1: depth 8, shift 0).
 *   same(y, x) of two frames a, b with `tol` in sample units.  Interleaved: every one of the C samples of the pixel has |sa - sb| <= tol.
 *     4:2:0: the Y sample at (y, x) is within tol, and the U and the V sample at (y >> 1, x >> 1) are within tol.
 *   core(y, x) for a radius r in 0..EMAVFI_STATIC_MAX_RADIUS: same(y', x') holds for every y' in [max(0, y - r), min(H - 1, y + r)] and every
 *     x' in [max(0, x - r), min(W - 1, x + r)].  The window is clipped to the frame: the frame edge never erodes, so letterbox bars survive.
 *   Applied to a destination frame d (a post-processed prediction for the pair (a, b)).  Interleaved: at every core pixel the C samples of d
 *     become a's.  4:2:0, luma: the Y sample of d becomes a's at every core pixel.  4:2:0, chroma: the chroma sample (i, j), U and V alike,
 *     becomes a's exactly when all four luma pixels (2 i + {0, 1}, 2 j + {0, 1}) are core.  A replaced 16-bit sample receives a's WHOLE word
 *     (the bits outside the sample included).  Every other byte of d is left as it was, and d is never read.
 *   Consequences: r = 0 gives core == same; a == b makes d a copy of a; one differing sample in otherwise equal frames leaves a hole of
 *     (2 r + 1)^2 pixels clipped at the frame; core is monotone: it shrinks as r grows and grows with tol.
 *
 * emavfi_static_guard_frames applies the definition to n_dst destination frames at dst + k dst_stride; entry k of `table`, a HOST pointer to
 *   n_dst entries {a, b}, names the two frames of `srcs` (n_srcs dense frames, src_stride bytes apart) that frame k is guarded against.  The
 *   table is read and validated before the call returns and nothing of it is retained: it travels as kernel arguments,
 *   EMAVFI_RESAMPLE_LAUNCH_CAP = 64 entries per launch.  counts (device memory, n_dst u32; may be NULL): counts[k] = the number of core
 *   pixels of entry k.  EVERY one of the n_dst words is defined on exit whatever the buffer held before: a launch ahead of the guard clears
 *   them on `stream` and the workgroups add their tiles' integer sums - the order does not matter.  C is ignored, but still validated (it
 *   must be 1), at a 4:2:0 layout, as `order` is where C = 1 elsewhere.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null dst, srcs or table; n_dst or n_srcs below 1; H or W outside 1..16384,
 *   or odd at a 4:2:0 layout; an unknown layout; C outside 1..4, or other than 1 at a 4:2:0 layout; sample_bytes, depth or shift outside the
 *   above; a radius outside 0..16; a tol above 2^depth - 1; a stride below the frame's bytes, or odd at sample_bytes 2; a dst / srcs pointer
 *   that is not 2-byte aligned at sample_bytes 2, a counts pointer that is not 4-byte aligned; size arithmetic that overflows size_t; dst
 *   overlapping srcs; an entry index outside srcs.
 * The frame pointers are device pointers or pinned (device-mapped) host memory.  Nothing is allocated, nothing synchronises, there is no
 *   workspace, all work goes on `stream`.  A workgroup owns a tile of 64 x 128 pixels of one destination frame, reads a and b there plus an
 *   r-wide halo, clipped to the frame - no byte beyond a frame is read -, erodes in LDS, rows then columns, and stores a's samples (read a
 *   second time, from cache) at the replaced positions.  Access width: 16-byte loads and stores where the three frame addresses of the entry,
 *   every plane's offset and every plane's row bytes are multiples of 16, else bytes / words throughout; both forms run the same per-element
 *   functions (csrc/static_elem.h).  The kernel is short-lived and waits on nothing. */
#define EMAVFI_LAYOUT_INTERLEAVED 0
#define EMAVFI_LAYOUT_NV12 1
#define EMAVFI_LAYOUT_I420 2
#define EMAVFI_STATIC_MAX_RADIUS 16
typedef struct { unsigned a, b; } emavfi_static_entry;   /* indices into srcs */
int emavfi_static_guard_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, int n_srcs,
                               const emavfi_static_entry *table, int H, int W, int layout, int C, int sample_bytes, int depth, int shift,
                               int radius, unsigned tol, unsigned *counts, void *stream);

/* The active picture.  A 2.39:1 film in a 16:9 container, 4:3 material pillarboxed into 16:9: a quarter of the pixels of such a frame are
 * black bars, and the forward's cost is proportional to the pixels it is given.  The static guard above keeps the bars, but after the
 * forward has paid for them.  The reference interpolates the whole frame (inference.py); this is an addition, off unless asked for: the bars
 * are found on the device, the forward runs on the picture alone, and the bars are put back around every prediction.
 *
 * ACTIVE AREA DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool (ffmpeg's
 * cropdetect and the like).  All arithmetic is integer: host, oracle and device agree bit for bit.
 *   Sample.  A byte, or (word >> shift) & (2^depth - 1) of a 16-bit little-endian word: the (sample_bytes, depth, shift) triple
 *     emavfi_frame_diff_cells takes.
 *   Content.  A pixel of an image [H][W][C] has content when ANY of its C samples is GREATER than `level`; a sample equal to `level` is not
 *     content.  C = 1: the Y plane of a Y'CbCr frame - chroma is not looked at.  C = 3: bytes only (bgr24); any channel counts, so a
 *     saturated blue pixel is content although its luma is low.
 *   Bounds of a frame.  Four u32 words {top, bottom, left, right}: top = the smallest y with content, bottom = the largest such y plus 1,
 *     left and right the same in x.  A frame with no content: {H, 0, W, 0}.
 *   Rectangle of a set of frames (host integers).  The union of the bounds, grown outward so that top and bottom are multiples of 2 and left
 *     and right multiples of 16, clipped to the frame.  The multiples of 2 make the 4:2:0 chroma planes crop at whole samples; the multiples
 *     of 16 keep the 16-byte paths of every pitched entry at every sample size.  An empty union, or a rectangle that covers the frame, means
 *     "the whole frame".
 *   A prediction with an active rectangle R for the pair (a, b).  Inside R: the samples of the forward run on the two frames cropped to R.
 *     Outside R: the samples of frame a as emitted.  4:2:0: the chroma sample (i, j) belongs to R exactly when its 2 x 2 luma block does -
 *     R's even edges make that unambiguous.  A replaced 16-bit sample receives a's WHOLE word, as the static guard's does.
 *   Consequences.  R = frame is the plain path byte for byte.  Content outside an explicitly given R is not interpolated: it shows frame a.
 *     The model sees zero padding (mean grey) at R's edge where it saw the bar before; a border (BORDER DEFINITION below) replicates the
 *     picture there instead.  No quality claim is made.
 *
 * emavfi_active_bounds writes the bounds of n images (img + k batch_stride, rows `pitch` bytes apart, [H][W][C] samples: C = 1, or C = 3 at
 *   sample_bytes 1) to bounds[4 k ..] (device memory).  EVERY one of the 4 n words is defined on exit whatever the buffer held before: a launch
 *   ahead of the scan initialises them on `stream`, then lanes keep their extremes in registers, waves fold them, a workgroup folds its waves'
 *   and issues atomicMin / atomicMax on the frame's words - order-free, so exact.  Access width: 16-byte loads where pointer, pitch and (n > 1) batch stride are
 *   multiples of 16, else - and for a row's remainder - bytes through the same per-element functions (csrc/active_elem.h); pitch padding is
 *   never read.  The image may be pinned host memory.
 * emavfi_fill_outside_frames: destination frame k (dst + k dst_stride) receives the samples OUTSIDE the rectangle (top, left, height, width) of
 *   frame table[k] of `srcs`; bytes inside the rectangle are neither read nor written, and a rectangle that is the frame leaves dst untouched.
 *   Frames are dense, in the layouts of the STATIC REGION DEFINITION, sample_bytes 1 or 2.  `table` is a HOST pointer to n_dst indices, read and
 *   validated before the call returns and passed on as kernel arguments, EMAVFI_RESAMPLE_LAUNCH_CAP entries per launch.  Only the bar bytes
 *   move: 16-byte accesses on aligned units that lie wholly outside, samples elsewhere.
 * emavfi_preprocess_u8_pitched / emavfi_postprocess_u8_pitched are emavfi_preprocess_u8 / emavfi_postprocess_u8 on the dense copy of the
 *   frames, bit for bit, for frames whose rows are `pitch` and whose frames are `batch_stride` bytes apart (a sub-rectangle of a larger
 *   frame); pitch padding is never read or written; 16-byte accesses where pointer, pitch and stride allow.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer; n, n_dst, n_srcs or B below 1, n or B above 65535; H or W
 *   outside 1..16384, or odd at a 4:2:0 layout; an unknown layout; C outside {1, 3} (bounds; 3 at sample_bytes 1 only) or 1..4 (the others; 1
 *   at a 4:2:0 layout); sample_bytes, depth or shift outside the above; a level above 2^depth - 1; a pitch below the row, a stride below the
 *   plane or frame, either odd at sample_bytes 2; a frame pointer that is not 2-byte aligned there, a u32 / fp32 pointer that is not 4-byte
 *   aligned; size arithmetic that overflows size_t; a rectangle that leaves the frame, has no area, or is odd at a 4:2:0 layout; a table
 *   index outside srcs; dst overlapping srcs; a zero std.  Nothing is allocated, nothing synchronises, all work goes on `stream`. */
int emavfi_active_bounds(const unsigned char *img, size_t pitch, size_t batch_stride, int n, int H, int W, int C, int sample_bytes, int depth,
                         int shift, unsigned level, unsigned *bounds /* n x 4 */, void *stream);
int emavfi_fill_outside_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, int n_srcs,
                               const unsigned *table /* n_dst indices into srcs, HOST */, int H, int W, int layout, int C, int sample_bytes,
                               int top, int left, int height, int width, void *stream);
int emavfi_preprocess_u8_pitched(const unsigned char *frames, size_t pitch, size_t batch_stride, float *out_nchw, int B, int H, int W, int C,
                                 const float *mean, const float *std, void *stream);
int emavfi_postprocess_u8_pitched(const float *frames_nchw, unsigned char *out, size_t pitch, size_t batch_stride, int B, int H, int W, int C,
                                  const double *mean, const double *std, int denormalize, void *stream);

/* Test-time ensembling.  The forward estimates one flow and warps only frame2 (ema_vfi.py:130), so F(a, b) and F(b, a) are two different
 * "midpoints" of the same pair, and its stride-2 context path and zero padding make it non-equivariant under mirroring.  The usual remedy
 * (RIFE: --ensemble; EMA-VFI's authors: TTA) runs the pair reversed and / or mirrored, maps each prediction back and averages.  The reference
 * has none (inference.py:158-160 calls the model once); this is an addition, off unless asked for.  No quality claim is made: what the
 * definition below buys, bit for bit, is an interpolator that is exactly symmetric in time and exactly equivariant under flips.  The
 * composition (which forwards run, on which inputs) lives in the Python layer (EMA_VFI.ensemble); the two entries here are the device work
 * a C integrator needs beside emavfi_forward_routed.
 *
 * ENSEMBLE DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.
 *   Flip codes.  EMAVFI_FLIP_H = 1 maps column x to W - 1 - x; EMAVFI_FLIP_V = 2 maps row y to H - 1 - y; 3 applies both; 0 is the identity.
 *     phi_f is the map on fp32 [planes][H][W] tensors: (phi_f t)[p][y][x] = t[p][f & 2 ? H - 1 - y : y][f & 1 ? W - 1 - x : x].  Every
 *     phi_f is its own inverse.
 *   F(a, b) is the plain forward's fp32 result (under EMAVFI_AMP16: before the final conversion of the frame to fp16).
 *   A member is a pair (tensor m_k, flip f_k); its value at output position p is m_k[phi_{f_k} p].
 *   The mean of n in {1, 2, 4, 8} members is a balanced pairwise tree in the order given; every + is one IEEE fp32 addition, and the tree is
 *     then multiplied ONCE by the exact constant 1 / n (n = 1: the member's value itself):
 *       n = 1: m0        n = 2: m0 + m1        n = 4: (m0 + m1) + (m2 + m3)        n = 8: ((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))
 *     No reassociation, no contraction, no fast-math.  A NaN in any member gives NaN.
 *   The ensembles, with P_f(a, b) = F(phi_f a, phi_f b) read through flip f (the member (F(phi_f a, phi_f b), f)):
 *       "reverse":  (F(a, b), 0), (F(b, a), 0)
 *       "flip":     P_0(a, b), P_3(a, b), P_1(a, b), P_2(a, b)
 *       "full":     the four of "flip" for (a, b), then the same four for (b, a)
 *   Why this order, and why nobody may tidy it.  fp32 addition is commutative but not associative, so a symmetry of the inputs leaves the
 *     bits alone only if it maps the tree onto itself.  (1) Swapping a and b swaps the two members of "reverse" - one commutative addition -
 *     and swaps the two halves of "full" - its top addition.  (2) Flipping both inputs by g turns P_f into P_{f ^ g} read at the flipped
 *     position (phi_f phi_g = phi_{f ^ g}).  The pairing {identity, HV}, {H, V} is closed under that: g = HV (3) swaps the members WITHIN
 *     each pair, g = H (1) or V (2) swaps the two pairs whole.  Either way every addition sees the same two operands, perhaps exchanged.
 *     (The flips form a group under xor and two pairs are always the cosets of one of its subgroups, so another pairing would be
 *     equivariant too - with other bits: the order above is the definition.)  What is NOT equivariant is an unbalanced sum: left to
 *     right, ((P_0 + P_3) + P_1) + P_2 turns under g = H into ((P_1 + P_2) + P_0) + P_3, other additions altogether.
 *     Hence "reverse" and "full" give ens(a, b) == ens(b, a) and "flip" and "full" give ens(phi_g a, phi_g b) == phi_g ens(a, b), bit for bit,
 *     for any deterministic F at all - which the plain forward is for a fixed route (EMA_VFI.pack_adapt unset).
 *
 * emavfi_flip_f32: dst = phi_flip src; flip = 0 is a copy.
 * emavfi_ensemble_mean_f32: out = the tree mean above of the n members (members[k], flips[k]).  `members` and `flips` are HOST arrays of n
 *   entries, read and validated before the call returns; they travel as kernel arguments and nothing of them is retained.
 * Both: dense fp32 [planes][H][W], H and W in 1..16384; planes * H * W is addressed with 64 bits (indices inside a plane are 32-bit).  The
 *   tensors are device pointers or pinned (device-mapped) host memory.  Nothing is allocated, nothing synchronises, there is no workspace,
 *   all work goes on `stream`; every word of dst / out is written and nothing else is.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer (src, dst, out, members, flips or a members[k]); n outside
 *   {1, 2, 4, 8}; a flip outside 0..3; planes of 0; a dimension outside 1..16384; a pointer that is not 4-byte aligned; size arithmetic
 *   that overflows size_t; dst overlapping src, or out overlapping any member.
 * Access width: 16-byte loads and stores, 4 consecutive output columns per lane, when W % 4 == 0 and every pointer of the call is 16-byte
 *   aligned; a member flipped along H is then read as the mirrored 16-byte unit with its four lanes reversed in registers.  Everything else
 *   takes a scalar path built from the same per-element functions (csrc/ensemble_elem.h).  Both kernels are pure streaming and short-lived:
 *   the grid follows the element count, nothing waits on anything. */
#define EMAVFI_FLIP_H 1
#define EMAVFI_FLIP_V 2
#define EMAVFI_ENSEMBLE_MAX_MEMBERS 8
int emavfi_flip_f32(const float *src, float *dst, size_t planes, int H, int W, int flip, void *stream);
int emavfi_ensemble_mean_f32(const float *const *members, const int *flips, int n, float *out, size_t planes, int H, int W, void *stream);

/* Frame borders.  Every operator of the forward takes the outside of the picture as zero: the backward warp is grid_sample with zeros
 * padding (ema_vfi.py:162-169), the deformable blocks return 0 for a sample at h <= -1 || h >= H, and every convolution zero-pads.  In the
 * normalised domain zero is the mean grey, so wherever the picture continues past the frame (a pan, an object entering or leaving) the
 * in-between frames carry a band along the edge that the source frames do not.  The usual remedy of interpolation tools is to extend the
 * frame past its edge, run the model on the larger frame and crop.  The reference has no such step; this is an addition, off unless asked
 * for, and no quality claim is made.  The composition lives in the Python layer (EMA_VFI.border); the two entries here are the device work
 * a C integrator needs beside emavfi_forward_routed.
 *
 * BORDER DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool (the two index maps
 *   happen to be numpy.pad's "edge" and "reflect", which the tests use to check their oracle).
 *   A border is (N, mode): N pixels added on each of the four sides, N in 0..EMAVFI_BORDER_MAX.
 *   pad_{N,mode} maps fp32 [planes][H][W] to [planes][H + 2N][W + 2N]:  dst[p][y][x] = src[p][iy(y - N)][ix(x - N)], with the index map
 *   i -> index in 0..n - 1 of an axis of n samples (n = H for iy, n = W for ix):
 *     EMAVFI_BORDER_REPLICATE = 0:  min(max(i, 0), n - 1).
 *     EMAVFI_BORDER_REFLECT = 1 (the edge sample is not repeated):  n == 1: 0.  Otherwise p = 2 (n - 1), m = ((i mod p) + p) mod p, and
 *       the index is m where m <= n - 1, else p - m.  The periodic form stays defined for N > n - 1 (several reflections).
 *   crop_N maps [planes][H + 2N][W + 2N] back to [planes][H][W]:  dst[p][y][x] = src[p][y + N][x + N].  Hence crop_N pad_{N,mode} is the
 *     identity, and N = 0 makes both a copy.
 *   Both are pure moves of 32-bit words: every bit pattern survives (NaN payloads, -0.0, infinities).
 *   The bordered forward is crop_N(G(pad a, pad b)), G being the plain forward F of the ENSEMBLE DEFINITION, or the ensemble of it where
 *     one is set.  Everything is taken in fp32, before the final conversion of the frame (fp16 under EMAVFI_AMP16, the input dtype
 *     otherwise).  The padded frame is an ordinary frame to the forward: the SIZE LIMITS apply to (H + 2N) x (W + 2N).
 *   Padding commutes with the four mirrorings, pad(phi_f t) = phi_f pad(t) - both index maps are symmetric under i -> n - 1 - i -, cropping
 *     likewise, and neither looks at which input it is given.  So a flip of both inputs, or their exchange, reaches the ensemble as the
 *     same flip or exchange of the padded inputs, and the ensemble's exact symmetry in time and exact flip equivariance carry over to
 *     the bordered ensemble bit for bit.
 *
 * emavfi_border_pad_f32: dst = pad_{N,mode} src.  emavfi_border_crop_f32: dst = crop_N src.  H and W are the size of the PICTURE (the
 *   unpadded tensor) in both entries: the source of a pad, the destination of a crop.
 * Both: dense fp32 tensors; every dimension of either tensor in 1..16384 (so H + 2N and W + 2N are bounded as well); planes * H * W is
 *   addressed with 64 bits (indices inside a plane are 32-bit).  The tensors are device pointers or pinned (device-mapped) host memory.
 *   Nothing is allocated, nothing synchronises, there is no workspace, all work goes on `stream`; every word of dst is written and
 *   nothing else is.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer; N outside 0..EMAVFI_BORDER_MAX; a mode other than the
 *   two above; planes of 0; a dimension of either tensor outside 1..16384; a pointer that is not 4-byte aligned; size arithmetic that
 *   overflows size_t; dst overlapping src.
 * Access width: one 16-byte store of 4 consecutive destination columns per lane when the destination's row length % 4 == 0 and dst is
 *   16-byte aligned; the four values are one 16-byte load where the unit lies wholly inside the picture and src is 16-byte aligned, the
 *   source's row length % 4 == 0 and N % 4 == 0, and four scalar loads through the index map otherwise (the border columns, the units that
 *   straddle the picture's edge, a misaligned interior).  Everything else takes a scalar path built from the same per-element functions
 *   (csrc/border_elem.h).  Both kernels are pure streaming and short-lived: the grid follows the destination's element count, nothing
 *   waits on anything. */
#define EMAVFI_BORDER_REPLICATE 0
#define EMAVFI_BORDER_REFLECT 1
#define EMAVFI_BORDER_MAX 64
int emavfi_border_pad_f32(const float *src, float *dst, size_t planes, int H, int W, int N, int mode, void *stream);
int emavfi_border_crop_f32(const float *src, float *dst, size_t planes, int H, int W, int N, void *stream);

/* Coarse flow.  The forward's flow comes from seven stride-1 3 x 3 convolutions between the frames and the flow field (feat_ext_conv1, three
 * feat_ext_blocks, motion_estimation.0/.1/.2; ema_vfi.py:73-76, :89-92) plus the context vector, a global mean that carries no position: a
 * flow value can depend on nothing farther than 7 pixels away.  At 720p and above ordinary motion is tens of pixels per frame.  The
 * reference's answer is --scale 0.5, which halves the OUTPUT as well.  The entries here estimate the flow on frames reduced by s and run
 * everything else at full size: the "flow scale" of flow-based interpolators.  The reference has no such step; this is an addition, off
 * unless asked for, and no quality claim is made (the reference ships no weights).  The composition lives in the Python layer
 * (EMA_VFI.flow_scale); the entries are the device work a C integrator needs.
 *
 * COARSE FLOW DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.
 *   s is 2, 4 or 8;  Hs = ceil(H / s), Ws = ceil(W / s).  All arithmetic is IEEE fp32 without contraction, in exactly the stated order.
 *   F_s(a, b), for two normalised fp32 batches [B][3][H][W], in four steps:
 *   1. Downscale.  a_s = down_s(a), b_s = down_s(b), each [B][3][Hs][Ws].  Block (i, j) has s x s leaves
 *        L(r, c) = x[min(s i + r, H - 1)][min(s j + c, W - 1)]
 *      - the clamp is applied once, at the leaves: an edge block still has s^2 of them -, reduced by the balanced quadtree
 *        T_1 = L,   T_2m(r, c) = ((T_m(2r, 2c) + T_m(2r, 2c+1)) + (T_m(2r+1, 2c) + T_m(2r+1, 2c+1))) * 0.25f,
 *      and the result is T_s(0, 0).  The multiplications are exact (up to underflow): host, oracle and device agree bit for bit.
 *   2. Coarse flow.  flow_s = the flow of the plain forward of (a_s, b_s) at Hs x Ws: bit for bit what taps[2] of emavfi_forward holds for
 *      those arguments, in the same mode and from the same packed blob (the weights do not depend on the resolution).
 *   3. Upsample.  flow_up[b][c][y][x] = (float)s * v, v being the bilinear sample at half-pixel centres.  Per axis, with destination index
 *      d and coarse length n:  num = 2 d + 1 - s (an integer, possibly negative);  i0 = floor(num / (2 s));
 *      w = (float)(num - 2 s i0) / (float)(2 s) (dyadic, exact);  j0 = clamp(i0, 0, n - 1), j1 = clamp(i0 + 1, 0, n - 1).  Then
 *        top = (1 - wx) p[y0][x0] + wx p[y0][x1],  bot the same on row y1,  v = (1 - wy) top + wy bot.
 *      Both flow channels are scaled by s.  The block geometry is s even where H or W is not a multiple of s.
 *   4. Fine forward.  F_s(a, b) = the plain forward of (a, b) with flow_up in place of motion_estimation's output: feature extraction,
 *      warp, attention blocks and reconstruction run exactly as in emavfi_forward; context encoding and motion estimation, which have no
 *      consumer but the flow, are not launched.
 *   Consequences:
 *     - A forward given its own plain flow is the plain forward, bit for bit.
 *     - A zero flow makes warped == frame2.
 *     - down_s of a constant is that constant (x + x and 2x + 2x are exact, as is * 0.25f).
 *     - up of a constant flow c is exactly s c wherever the two products with the dyadic weights are exact (c of at most 20 significant
 *       bits: the weights have at most 4), and in particular at every position whose weights are 0 and 1.
 *     - The first s / 2 rows and columns of flow_up have i0 = -1: both taps clamp to coarse row / column 0.
 *   Ensemble members, border padding and the agreement halves (the definitions above) receive F_s wherever they say F: the padded frame is
 *   the frame that is reduced.
 *
 * emavfi_downscale_f32: dst [planes][ceil(H / s)][ceil(W / s)] = down_s of src [planes][H][W].
 * emavfi_upsample_flow_f32: flow [planes][H][W] = step 3 of flow_s [planes][Hs][Ws]; Hs and Ws must be the ceilings.
 * Both: dense fp32 tensors, device pointers or pinned (device-mapped) host memory; H, W (and Hs, Ws) in 1..16384; planes * H * W is
 *   addressed with 64 bits (indices inside a plane are 32-bit).  Nothing is allocated, nothing synchronises, there is no workspace, there
 *   are no atomics, all work goes on `stream`; every word of the destination is written and nothing else is.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null pointer; s outside {2, 4, 8}; planes of 0; a dimension outside
 *   1..16384; Hs or Ws that is not the ceiling; a pointer that is not 4-byte aligned; size arithmetic that overflows size_t; the
 *   destination overlapping the source.
 * Access width.  Down: 16-byte loads of the leaves when src is 16-byte aligned and W % 4 == 0 (a unit of 4 results for s = 2 and 4, of 1
 *   for s = 8; a unit whose leaves reach past column W - 1 takes the scalar path), one 16-byte store per 4 results when dst is 16-byte
 *   aligned and Ws % 4 == 0.  Up: one 16-byte store of 4 destination columns when flow is 16-byte aligned and W % 4 == 0; the coarse samples
 *   are scalar loads.  Everything else takes a scalar path built from the same per-element functions (csrc/coarse_elem.h).
 *
 * emavfi_forward_flow: the launches of emavfi_forward up to and including the one that writes the flow (step 2), then a device-to-device
 *   copy of it to flow_out [B][2][H][W] fp32 (16-byte aligned).  No attention block runs and no census is produced.  The workspace is
 *   emavfi_workspace_bytes' for the same arguments, under THE WORKSPACE CONTRACT.
 * emavfi_forward_given_flow: step 4.  The arguments of emavfi_forward_routed plus `flow` [B][2][H][W] fp32, 16-byte aligned, read in place
 *   (it must stay unchanged until the call's work on `stream` is done and may not overlap out or the workspace).  taps[1] (ctx) and
 *   taps[2] (flow) must be NULL, else EMAVFI_E_ARG: this forward computes neither; the other taps work.  stage_events[0] is recorded behind
 *   the warp.  Same workspace size and contract; the census is that of the attention blocks, as for emavfi_forward_routed.
 * emavfi_forward_flow_launches / emavfi_forward_given_flow_launches list the launches of the two, as emavfi_forward_launches does: the
 *   first is the prefix of the plain list through the flow's launch, the second the plain (routed) list without the context_encoding and
 *   motion_estimation launches; names, flops and bytes of the launches that remain are unchanged.
 * The adaptive route (emavfi_forward_adaptive) has no given-flow form. */
int emavfi_downscale_f32(const float *src, float *dst, size_t planes, int H, int W, int s, void *stream);
int emavfi_upsample_flow_f32(const float *flow_s, float *flow, size_t planes, int Hs, int Ws, int H, int W, int s, void *stream);
int emavfi_forward_flow(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes,
                        const float *frame1, const float *frame2, float *flow_out,
                        void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype, void *stream);
int emavfi_forward_given_flow(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes,
                              const float *frame1, const float *frame2, const float *flow, float *out,
                              void *workspace, size_t workspace_bytes,
                              int B, int H, int W, int dtype, float *const *taps, void *const *stage_events, void *const *events, int n_events,
                              unsigned gather_blocks, void *stream);
int emavfi_forward_flow_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                                 char *names, size_t names_bytes, double *flops, double *bytes, int capacity);
int emavfi_forward_given_flow_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, unsigned gather_blocks,
                                       char *names, size_t names_bytes, double *flops, double *bytes, int capacity);

/* Global motion.  A flow value of the forward depends on nothing farther than 7 pixels away (see "Coarse flow" above), while the largest
 * motion of real video is usually the camera's - a pan, a tilt, a tracking shot - and that motion is global.  It can be removed exactly, by
 * integer moves of words, before the model sees the pair; what is left (a residual of at most 2 pixels per axis, plus the objects' own
 * motion) is what the 7-pixel reach was built for.  The reference has no such step; this is an addition, off unless asked for, and no quality
 * claim is made.  The composition lives in the Python layer (EMA_VFI.align); the four entries here are the device work a C integrator needs
 * beside emavfi_forward_routed.  Nothing waits on the host: the shift is decided on the device and read there by the kernel that applies it.
 *
 * ALIGN DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.  Every decision is
 *   taken in integers, so host, oracle and device agree bit for bit.  The inputs are two normalised fp32 batches a, b of [B][3][H][W].
 *   EMAVFI_ALIGN_CELL = 4.  Hc = H / 4, Wc = W / 4 (floor): the remainder rows and columns at the bottom and right are not looked at.
 *   1. Signature.  Per pixel l = (x0 + x1) + x2 of its three channels in fp32, in that order, then t = l * 64.0f.  q = 0 where !(t >= -512)
 *      (a NaN included), q = 1023 where t >= 512, else q = (int)floorf(t) + 512.  G[i][j] is the sum of the 16 q of cell (i, j): 0..16368,
 *      stored as uint16, dense [B][Hc][Wc].
 *   2. Scores.  The radius R is in cells: R in 1..EMAVFI_ALIGN_MAX_RADIUS = 32 and 2 R <= min(Hc, Wc), so every candidate keeps at least
 *      half of each axis.  Candidates are d = (dy, dx), each component in [-R, R].  SAD(d) = sum |Ga[i][j] - Gb[i + dy][j + dx]| over the
 *      cells where both indices are inside the grid; N(d) = (Hc - |dy|)(Wc - |dx|); m(d) = floor(SAD(d) * 256 / N(d)) in unsigned 64-bit
 *      (SAD <= 16368 * 4096 * 4096, m <= 4 190 208).  d is the displacement of the content from a to b.
 *   3. Choice.  Of the candidates with the least m take those with the least |dy| + |dx|, of these those with the least |dy|.  If more
 *      than one is left (they differ only in signs), d* = (0, 0).  Acceptance: a non-zero d* is kept only if m(d*) * 1024 <= m(0) * ratio,
 *      ratio in 0..EMAVFI_ALIGN_MAX_RATIO = 1024; otherwise d* = (0, 0).  The record of a sample is four int32 words
 *      {4 dy*, 4 dx*, m(d*), m(0)}: the first two are pixels.
 *   4. Shift.  h = d_px / 2, exact since d_px is a multiple of 4.  a'[c][y][x] = a[c][cy(y - hy)][cx(x - hx)] and
 *      b'[c][y][x] = b[c][cy(y + hy)][cx(x + hx)], cy and cx clamping to 0..H-1 and 0..W-1 (replication).  Pure moves of 32-bit words:
 *      every bit pattern survives.  Both frames are moved into the midpoint's coordinates, so the output needs no shift back, and every
 *      sample of a batch keeps H x W whatever its own shift is.
 *   5. The aligned forward is M(a', b'), M being the forward the model would otherwise run (plain, ensembled, bordered, coarse, guarded)
 *      with (a', b') as its pair in every role, the agreement guard's source blend included.
 *   Consequences (each one is tested):
 *   - SAD_(b,a)(d) = SAD_(a,b)(-d), N and the order of step 3 are symmetric under negation, so d*(b, a) = -d*(a, b) and forward(b, a) runs
 *     on (b', a'): the exact time symmetry of the "reverse" and "full" ensembles survives bit for bit.
 *   - If b is a translated by a multiple of 4 pixels within the radius, a' == b' bit for bit at every position whose source indices were
 *     not clamped.
 *   - A rejected or zero shift is the plain path, byte for byte.
 *   - A constant frame, or a pattern whose minima tie under sign changes (stripes of period 2 cells), gives d* = 0.
 *
 * emavfi_align_signature_f32: sig = G of step 1 for the B samples of x.  H and W in 8..16384; x fp32 [B][3][H][W], 4-byte aligned; sig
 *   uint16 [B][H / 4][W / 4], 2-byte aligned.  16-byte loads of the three planes where W % 4 == 0 and x is 16-byte aligned, scalar loads
 *   through the same per-element functions (csrc/align_elem.h) otherwise.
 * emavfi_align_workspace_bytes: the bytes emavfi_align_search needs for B samples at radius R (B (2R + 1)^2 64-bit sums); 0 for a B < 1
 *   or an R outside 1..32.
 * emavfi_align_search: shifts[b] = the record of steps 2 and 3 for sample b of the two signature batches.  Hc, Wc in 2..4096 cells;
 *   workspace 8-byte aligned; shifts device int32 [B][4].  The entry clears its workspace on `stream` itself: the result does not depend
 *   on what the workspace held before.  The sums are integer atomics: the result is the same in every run.
 * emavfi_shift_f32: dst[b] = src[b] moved by sign * (shifts[4b] >> 1, shifts[4b + 1] >> 1) as in step 4: dst[b][c][y][x] =
 *   src[b][c][cy(y - sign * hy)][cx(x - sign * hx)]; sign = +1 makes a' of a, sign = -1 makes b' of b.  H, W in 1..16384.  `shifts` is read
 *   from DEVICE memory by the kernel; words 2 and 3 of a record are not looked at.  The kernel is memory-safe for any content of `shifts`:
 *   the half-shift is clamped to +-16384 before any index arithmetic.  dst may not overlap src.
 * All: nothing is allocated, nothing synchronises, all work goes on `stream`.  EMAVFI_E_ARG (never an abort), the message naming the
 *   argument: a null or misaligned pointer; B or C below 1; a dimension out of range; R outside 1..32 or 2 R > min(Hc, Wc); ratio outside
 *   0..1024; a workspace that is too small; sign other than +-1; dst overlapping src; size arithmetic that overflows size_t. */
#define EMAVFI_ALIGN_CELL 4
#define EMAVFI_ALIGN_MAX_RADIUS 32
#define EMAVFI_ALIGN_MAX_RATIO 1024
int emavfi_align_signature_f32(const float *x, unsigned short *sig, int B, int H, int W, void *stream);
size_t emavfi_align_workspace_bytes(int B, int R);
int emavfi_align_search(const unsigned short *sig_a, const unsigned short *sig_b, int B, int Hc, int Wc, int R, int ratio, void *workspace,
                        size_t workspace_bytes, int *shifts, void *stream);
int emavfi_shift_f32(const float *src, float *dst, int B, int C, int H, int W, const int *shifts, int sign, void *stream);

/* Agreement guard.  Every other guard here decides from the SOURCE frames (cuts, duplicates, static regions, borders); nothing protects
 * against the model being wrong.  The forward estimates one flow and warps only frame2, and on large motion, occlusions and repetitive
 * texture it tears or smears.  The "reverse" and "full" ensembles already compute F(a, b) and F(b, a), two midpoints of the same pair, and
 * then average away where they differ; their per-pixel disagreement is a reliability map that costs no forward.  This entry keeps it:
 * where the two time directions disagree, within a small window, the plain blend of the two source frames is emitted instead.  The
 * reference has no such step; this is an addition, off unless asked for, and no quality claim is made.  The composition (which forwards
 * make u and v) lives in the Python layer (EMA_VFI.agreement); the entry is the device work a C integrator needs beside
 * emavfi_forward_routed and emavfi_ensemble_mean_f32.
 *
 * AGREEMENT GUARD DEFINITION (the one place).  This is the project's own definition: it claims agreement with no outside tool.
 *   Inputs, all fp32, dense, [B][C][H][W], C in 1..4, H and W in 1..16384, B in 1..EMAVFI_AGREEMENT_MAX_BATCH:
 *     u: the mean of the time-forward members of the ensemble; v: the mean of the time-reversed members (ENSEMBLE DEFINITION);
 *     a, b: the two NORMALISED source batches exactly as the forward received them; mean[C], std[C]: the normalisation, HOST pointers to
 *     fp32, as for the preprocess entries.
 *   Disagreement.  d(b, c, y, x) = |u - v|: one IEEE fp32 subtraction, then the sign bit cleared.
 *   Flagged.  A pixel (b, y, x) is flagged when, for some channel c, NOT (d <= tol).  tol is fp32, 0 <= tol <= 1, in units of the output's
 *     full scale.  The negated form is the definition: a NaN in u or v (and inf - inf) flags the pixel.
 *   Held.  A pixel (y, x) is held, for a radius r in 0..EMAVFI_STATIC_MAX_RADIUS, when some pixel (y', x') of the same sample with
 *     y' in [max(0, y - r), min(H - 1, y + r)] and x' in [max(0, x - r), min(W - 1, x + r)] is flagged.  The window is clipped to the frame,
 *     as the static guard's is.
 *   Output, per channel.  Not held:  out = (u + v) * 0.5f - one fp32 addition and one exact multiplication.
 *     Held:  h = (a + b) * 0.5f;  t = h * std[c];  t = t + mean[c]  (three roundings: no contraction);  out = t < 0 ? 0 : (t > 1 ? 1 : t).
 *     Both comparisons fail for a NaN, so a NaN source stays NaN; a NaN in u or v at a held pixel does not reach the output.
 *   Counts.  counts[b] = the number of held pixels of sample b.
 *   Consequences:
 *     - Exchanging u with v together with a with b leaves every output bit unchanged: |u - v| == |v - u|, and `+` is commutative.
 *     - Flipping all four inputs by phi_g (ENSEMBLE DEFINITION) flips the output and the hold map: the clipped window is symmetric under
 *       y -> H - 1 - y and x -> W - 1 - x, and everything else is per element.
 *     - One flagged pixel in otherwise agreeing inputs holds a (2 r + 1)^2 square clipped at the frame.
 *     - tol = 1 with finite inputs in [0, 1] holds nothing and yields (u + v) * 0.5f everywhere.
 *     - The hold map is monotone: it grows with r and shrinks as tol grows.
 *   Composition (EMA_VFI.agreement; G_4(x, y) = the tree mean of the four "flip" members of (x, y), emavfi_ensemble_mean_f32 with n = 4):
 *       "reverse":  u = F(a, b), v = F(b, a).  With nothing held the result IS the "reverse" ensemble, bit for bit: the same two operations.
 *       "full":     u = G_4(a, b), v = G_4(b, a).  With nothing held the result is (s_ab * 0.25f + s_ba * 0.25f) * 0.5f against the "full"
 *                   ensemble's (s_ab + s_ba) * 0.125f, s being the four-member sums.  Scaling by a power of two is exact unless it
 *                   underflows, and a frame's values are far from that, so the two are equal bit for bit wherever no intermediate is
 *                   subnormal; that is asserted by the tests on their fixtures and is not part of the definition.
 *     The guard needs both time directions: without an ensemble, or with "flip", it is refused, never upgraded silently.  With a border
 *     (BORDER DEFINITION) the forwards run on the padded pair, u and v are cropped, and the guard runs on the picture with the UNPADDED
 *     a and b: window and counts refer to the picture, and since cropping commutes with flips the symmetries carry over.  Under
 *     EMAVFI_AMP16 everything above is fp32, ahead of the final conversion.  As for the ensemble, the symmetries hold for a deterministic
 *     F, which the plain forward is for a fixed route (EMA_VFI.pack_adapt unset).
 *
 * emavfi_agreement_guard_f32 applies the definition.  counts (device memory, B u32; may be NULL): EVERY one of the B words is defined on
 *   exit whatever the buffer held before: a launch ahead of the guard clears them on `stream` and the workgroups add their tiles' integer
 *   sums - the order does not matter.  Every word of out is written and nothing else is; out may overlap none of u, v, a, b (those four may
 *   alias one another).  mean and std are read before the call returns and travel as kernel arguments.
 * EMAVFI_E_ARG (never an abort), the message naming the argument: a null u, v, a, b, out, mean or std; B outside
 *   1..EMAVFI_AGREEMENT_MAX_BATCH; C outside 1..4; H or W outside 1..16384; a radius outside 0..16; a tol outside 0..1 or NaN; a std[c] that
 *   is zero or not finite, a mean[c] that is not finite; a tensor pointer that is not 4-byte aligned, a counts pointer likewise; size
 *   arithmetic that overflows size_t (a tensor that wraps the address space); out overlapping u, v, a or b.
 * The tensors are device pointers or pinned (device-mapped) host memory.  Nothing is allocated, nothing synchronises, there is no
 *   workspace, all work goes on `stream`.  A workgroup owns a tile of 64 x 128 pixels of one sample.  It reads u and v there plus an r-wide
 *   halo, clipped to the frame - nothing outside a tensor is read -, stores (u + v) * 0.5f for the tile's own elements as it goes, reduces
 *   over the channels to one flag per pixel in LDS, dilates rows then columns, and then reads a and b and stores the blend ONLY where
 *   held.  Access width: 16-byte loads and stores, 4 columns per lane, when W % 4 == 0 and every tensor pointer of the call is 16-byte
 *   aligned (a halo unit may then reach past the halo but never past its row); a scalar path otherwise.  Both run the same per-element
 *   functions (csrc/agreement_elem.h).  The kernel is short-lived and waits on nothing. */
#define EMAVFI_AGREEMENT_MAX_BATCH 65535
int emavfi_agreement_guard_f32(const float *u, const float *v, const float *a, const float *b, float *out, int B, int C, int H, int W,
                               int radius, float tol, const float *mean, const float *std, unsigned *counts, void *stream);

/* Frame metrics on the device: how close is image a (an interpolated frame) to image b (the held-out true frame)?  The reference has no
 * evaluation script (its README names PSNR and SSIM against held-out ground-truth frames as the way to judge a model and calls an eval.py a
 * future improvement); this is an addition.  Two byte images stay where they are; a few 64-bit words per image pair come back.
 *
 * FRAME METRIC DEFINITION (the one place).  Inputs: two byte images a, b [B][H][W][C], C = 1..4, H and W 1..16384, each side with its own row
 * pitch and batch stride; every channel is scored on its own.  Host, oracle and device agree bit for bit.
 *   SSE.  sse[c] = the sum over the H W pixels of (a - b)^2, an unsigned 64-bit integer (at most 255^2 * 16384^2 < 2^46).  PSNR is host
 *     arithmetic on it: 10 log10(255^2 n / sse) over n samples, inf for sse == 0.
 *   SSIM follows Wang et al. 2004: an 11 x 11 Gaussian window of sigma 1.5 (EMAVFI_METRICS_WINDOW), K1 = 0.01, K2 = 0.03, L = 255, population
 *     covariance, only windows that lie wholly inside the image, the mean over the (H - 10)(W - 10) windows.  The weights are quantised so
 *     that the moments are exact integers: per axis g = {67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67}, which is
 *     floor(g_real 65536 + 0.5) of the normalised Gaussian with the centre raised by one so that the sum is exactly 65536; the 2-D weight is
 *     w = g[i] g[j], summing to 2^32.  Per window the moments are
 *         A = sum w a,  B = sum w b,  Axx = sum w a^2,  Ayy = sum w b^2,  Axy = sum w a b.
 *     After one axis each fits 32 bits unsigned (65025 * 65536 < 2^32); after both each is below 65025 * 2^32 < 2^48, so its conversion to
 *     double is exact.  The tail runs in IEEE double precision, no contraction, in exactly this operation order:
 *         a = A 2^-32; b = B 2^-32; axx = Axx 2^-32; ayy = Ayy 2^-32; axy = Axy 2^-32        (exact)
 *         aa = a a; bb = b b; ab = a b
 *         sx = axx - aa; sy = ayy - bb; sxy = axy - ab
 *         num = (2 ab + C1) (2 sxy + C2)
 *         den = ((aa + bb) + C1) ((sx + sy) + C2)
 *         m = num / den
 *         q = (int64) floor(m 4294967296.0)
 *     with C1, C2 the doubles nearest 6.5025 and 58.5225.  ssimq[c] = the sum of q over the windows, a signed 64-bit integer of magnitude at
 *     most 2^32 * 16384^2 = 2^60; an integer sum, so it does not depend on the order or grouping of the reduction.  The SSIM of a channel is
 *     ssimq / (2^32 windows).  With H < 11 or W < 11 there is no window: ssimq = 0 (the Python layer reports nan); this is not an error.
 *     Against the real-valued-Gaussian SSIM the quantised weights moved the result by at most 4.8e-6 on the four 40 x 56 image pairs of
 *     tests/test_metrics_cpu.py.
 *
 * emavfi_frame_metrics_u8: out [B][C][2] 64-bit words {sse, ssimq} in device or pinned memory.  EVERY one of the B C 2 words is written,
 *   whatever the buffer held before; the caller zeroes nothing.  `workspace`: at least emavfi_frame_metrics_workspace_bytes(B, H, W, C) bytes
 *   of device memory (0 from that query: arguments it refuses); it receives each workgroup's partial sums, which a small second launch adds
 *   - no atomics, and integer sums are the same in any grouping.  Nothing is allocated, nothing synchronises, all work goes on `stream`.
 * EMAVFI_E_ARG (never an abort): a null pointer, B below 1 (or above 65535), a dimension outside 1..16384, C outside 1..4, a pitch smaller
 *   than its row, for B > 1 a batch stride smaller than its plane, an `out` or workspace that is not 8-byte aligned, size arithmetic that
 *   overflows size_t.  EMAVFI_E_WORKSPACE: a workspace that is too small.
 * a and b are device pointers or pinned (device-mapped) host memory, as for the other u8 entries.  Access width: a workgroup stages its tile of
 *   an image with 16-byte loads when that image's pointer, pitch and (B > 1) batch stride are multiples of 16 (only units that end inside the
 *   row: pitch padding is never read), else byte by byte; both forms feed the same per-element functions (csrc/metrics_elem.h). */
#define EMAVFI_METRICS_WINDOW 11
size_t emavfi_frame_metrics_workspace_bytes(int B, int H, int W, int C);
int emavfi_frame_metrics_u8(const unsigned char *a, size_t a_pitch, size_t a_batch_stride, const unsigned char *b, size_t b_pitch,
                            size_t b_batch_stride, int B, int H, int W, int C, long long *out, void *workspace, size_t workspace_bytes,
                            void *stream);

/* One conv / conv_block (ema_vfi.py:7-14): Conv2d(k=3, p=1, stride 1 or 2) + activation.
 * x [B,Cin,H,W], weight [Cout,Cin,3,3], bias [Cout], y [B,Cout,ceil(H/stride),ceil(W/stride)]. */
size_t emavfi_conv3x3_workspace_bytes(int B, int Cin, int Cout, int H, int W, int stride, int dtype);
int emavfi_conv3x3(const float *x, const float *weight, const float *bias, float *y,
                   int B, int Cin, int Cout, int H, int W, int stride, int act, int dtype,
                   void *workspace, size_t workspace_bytes, void *stream);

/* torchvision.ops.deform_conv2d(x, offset, weight, bias, padding=1, mask=mask) as configured
 * at ema_vfi.py:45-51 / :60 (3x3, stride 1, pad 1, one offset group, one weight group).
 * x [B,C,H,W], offset [B,18,H,W] (2k = dy, 2k+1 = dx of tap k = 3i+j), mask [B,9,H,W],
 * weight [O,C,3,3], bias [O], y [B,O,H,W]. */
size_t emavfi_deform_conv2d_workspace_bytes(int B, int C, int O, int H, int W, int dtype);
int emavfi_deform_conv2d(const float *x, const float *offset, const float *mask,
                         const float *weight, const float *bias, float *y,
                         int B, int C, int O, int H, int W, int dtype,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ModulatedDeformConvPack.forward(x), ema_vfi.py:53-60, as one stage:
 *   raw = offset_conv(x) (3x3, pad 1, C -> 27, :35-43); offset = cat(raw[:, 0:9], raw[:, 18:27]); mask = sigmoid(raw[:, 9:18]) (:56-59);
 *   y = dcn_v2(x, offset, mask) (:60).
 * x, y [B,C,H,W] fp32 NCHW; offset_weight [27,C,3,3], offset_bias [27], dcn_weight [C,C,3,3], dcn_bias [C] (may be NULL).
 * C must be mid_channels + 3 of a supported model (the only width the reference builds the pack at, ema_vfi.py:97).
 * Routed exactly as one attention block of emavfi_forward: EMAVFI_BF16 / EMAVFI_F16 at C = 67 run the ONE-LAUNCH kernel
 * (offset_conv on the staged window, offsets / masks in registers, DCN, fix-up loop for samples that leave the window); EMAVFI_F32
 * runs conv3x3 + the fp32 LDS-window DCN; EMAVFI_AMP16 the fp16 offset_conv + fp32 DCN pair; other widths conv3x3 + the
 * global-gather DCN.  `flags` reproduce the forms the forward hands the tensor over in (one-launch kernel only):
 *   EMAVFI_MDCN_IN_F16 / _OUT_F16  bf16 model: x is stored / y is produced as IEEE f16 bit patterns (hand-off between packs, `feat`);
 *   EMAVFI_MDCN_SPLIT_TAIL         channels mid.. of x reach the kernel through the compact tail buffer - 4 channels per pixel - (the first pack's input). */
#define EMAVFI_MDCN_IN_F16 1
#define EMAVFI_MDCN_OUT_F16 2
#define EMAVFI_MDCN_SPLIT_TAIL 4
size_t emavfi_mdcn_workspace_bytes(int B, int C, int H, int W, int dtype, int flags);
int emavfi_mdcn(const float *x, const float *offset_weight, const float *offset_bias, const float *dcn_weight, const float *dcn_bias,
                float *y, int B, int C, int H, int W, int dtype, int flags, void *workspace, size_t workspace_bytes, void *stream);
/* emavfi_mdcn with a route (EMAVFI_ROUTE_WINDOW | EMAVFI_ROUTE_GATHER, see emavfi_forward_routed) and a measurement hook: `events` is
 * NULL, or n_events >= 2 caller-created hipEvent_t (else EMAVFI_E_ARG) and the stage's own launches (one in the 16-bit modes at C = 67,
 * else two) are bracketed by hipEventRecord on events[2i] / events[2i+1]; the layout conversions around them are not bracketed
 * (bench.py's also_pack_vs_offset_spread: what the dominant kernel costs when the offsets leave its staged window).  The window route
 * with NULL events is emavfi_mdcn exactly.  All flag combinations of the one-launch pack are valid on both routes; emavfi_mdcn_census
 * reads either route's counters. */
int emavfi_mdcn_routed(const float *x, const float *offset_weight, const float *offset_bias, const float *dcn_weight, const float *dcn_bias,
                       float *y, int B, int C, int H, int W, int dtype, int flags, int route, void *workspace, size_t workspace_bytes,
                       void *const *events, int n_events, void *stream);

/* Census of the one-launch ModulatedDeformConvPack kernel (measurement hook; the reference bounds its offsets nowhere, ema_vfi.py:55-60,
 * and the kernel stages a window that holds offsets up to +-2 px beyond the tap: samples that leave it take a fix-up pass).  The kernel
 * counts, while it runs: the (wave, tap) groups - 4 rows x 16 pixels x one tap - that took the fix-up, the samples outside the window and
 * the largest |offset| of the waves that had one (only those pay for the census: 0 = every sample was inside the window).  The gather route
 * (EMAVFI_ROUTE_GATHER) writes the same record with the same meaning - what WOULD have left the window - so both routes report identical
 * counts on the same input and a caller can route by it in either direction.  emavfi_forward_census reads the counters the LAST emavfi_forward* call on `workspace` left there
 * (same model, B, H, W, dtype; enqueue it on the same stream), emavfi_mdcn_census those of the last emavfi_mdcn* call:
 *   out[block][4] (unsigned 64-bit, DEVICE memory, num_blocks rows - one row for mdcn) =
 *     {fix-up wave-taps, all wave-taps (0: this block did not run the one-launch kernel, nothing was counted), samples outside the
 *      window (of B*H*W*9), max |offset| in px as fp32 bits}.
 * One tiny launch; nothing is synchronised. */
int emavfi_forward_census(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                          const void *workspace, size_t workspace_bytes, unsigned long long *out, void *stream);
int emavfi_mdcn_census(int B, int C, int H, int W, int dtype, int flags, const void *workspace, size_t workspace_bytes,
                       unsigned long long *out, void *stream);

/* context_encoding(feat) -> ctx, ema_vfi.py:79-86 (called at :120): conv stride 2 + ReLU, conv stride 2 + ReLU, conv + ReLU,
 * AdaptiveAvgPool2d(1), Flatten, Linear.  feat [B,mid,H,W]; params = 8 device pointers in the Sequential's registration order:
 * context_encoding.{0.0,1.0,2.0}.{weight,bias} ([2m,m,3,3] [2m] [4m,2m,3,3] [4m] [4m,4m,3,3] [4m]) and context_encoding.5.{weight [m,4m],
 * bias [m]}; ctx [B,mid] fp32.
 * reconstruction(fused) -> out, ema_vfi.py:102-107 (called at :144-146): conv + ReLU, conv + ReLU, conv, tanh, then (t + 1) / 2.
 * fused [B,mid+3,H,W]; params = 6 device pointers: reconstruction.{0.0,1.0,2}.{weight,bias}; out [B,3,H,W] in [0,1].
 * Both run the launches emavfi_forward runs for the stage (16-bit modes at mid_channels 64: the LDS-ring kernels, reconstruction.1 + .2
 * as ONE launch), on EMA_VFI(3, mid_channels, 3)'s plan; storage rounding of the inputs as the forward's tensors have it. */
size_t emavfi_context_workspace_bytes(int B, int mid_channels, int H, int W, int dtype);
int emavfi_context(const float *feat, const float *const *params, float *ctx, int B, int mid_channels, int H, int W, int dtype,
                   void *workspace, size_t workspace_bytes, void *stream);
size_t emavfi_reconstruct_workspace_bytes(int B, int mid_channels, int H, int W, int dtype);
int emavfi_reconstruct(const float *fused, const float *const *params, float *out, int B, int mid_channels, int H, int W, int dtype,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Test hook: the A/B switches of the launch sequence (EMAVFI_CONV_FIRST / _FIRSTRING / _HEAD / _TAILFUSE / _LIGHT / _RING2 /
 * _POOLFUSE = 0, EMAVFI_RING_CHUNK = 0, EMAVFI_NO_PERSISTENT_CONV) are read from the environment ONCE per process into one word; this replaces it by
 * (word & and_mask) | or_mask and returns the previous value (bits: 1 no conv_first, 2 no fused first two layers, 4 no fused flow
 * head, 8 no fused reconstruction tail, 16 no planar-head kernel, 32 no persistent conv, 64 no two-layer ring fusions, 128
 * context_encoding.2 stores its output instead of fusing the average pool, 256 (EMAVFI_RING_ONE_WG=1, a measurement switch) the
 * persistent LDS-ring kernels launch one workgroup per CU instead of two, 512 (EMAVFI_RING_CHUNK=0) they walk 45-row segments dealt
 * round-robin instead of one contiguous range of rows per workgroup).  None of them changes the packed layout.  Not for
 * production callers. */
int emavfi_debug_switches(int and_mask, int or_mask);

#ifdef __cplusplus
}
#endif
#endif /* EMAVFI_H */
