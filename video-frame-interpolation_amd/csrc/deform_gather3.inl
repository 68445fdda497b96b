// ModulatedDeformConvPack at the reference width, 16-bit storage types: the WINDOW-FREE one-launch route.
//
// A drop-in for deform_pack3_kernel<TS, true> - same DeformParams, same packed weights (the pack3 layout, blob untouched), same input
// forms (x at x_ps, the split tail x_tail / tail_ps, the bf16 model's f16 hand-off in_f16 / out_f16), same output, and `om` is not
// written - whose cost does not depend on the offsets:
//
//   * LDS holds only what offset_conv reads: the 16 x 16 tile plus a 1 px halo (18 x 18 pixels x 144 B = 46 656 B) and the 4.5 KiB
//     third-fragment table, 51 264 B in all (the pack: 81 312 B for its 23 x 23 window).  No sample ever "leaves" anything.
//   * offset_conv, the sigmoid, the sampling geometry, the tail contraction, the census record and the epilogue are the very
//     text the pack's body runs (deform3_stages.inl): one definition each, so the two routes cannot drift apart.
//   * Every tap gathers its corner pieces straight from global memory: lane (r, h) loads the four 16-byte corner pieces
//     (k-group kg, half h) of pixel r of fragment row m with raw buffer loads.  A corner outside the image gets an offset beyond the
//     buffer's range and reads 0 - exactly what the pack's window holds there (its DMA reads the zero page), so the blend runs on the
//     same values with the same (unmasked) weights.  The tail channels come from x_tail (or bytes 128.. of the pixel) the same way.
//   * The MFMA order per accumulator is the pack's: the three tail k-groups first, then taps 0..8 x k-groups 0..3.  Together with the
//     same f16 corner values (bf16 -> f16 by the same conversion, in registers instead of in LDS) and the same blend sequence the output
//     equals the pack's bit for bit wherever the pack has no sample outside its window (its census reports no fix-up group).
//   * Census: the same record as the pack's, with the same meaning - (wave, tap) groups and samples that WOULD have left the pack's
//     +-2 px window, the largest |offset| of the waves that had one - so both routes report identical counts on the same input.
//
// Latency: the corner loads of a step go out four steps (half a tap) ahead through a ring of four operand buffers, across the tap
// boundary; the sampling descriptors of all nine taps are computed up front as in the pack.
#pragma once
#include "deform_pack3.inl"

struct Gather3 {
    static constexpr int TROWS = 16, TCOLS = 16, WAVES = 4, THREADS = 256;
    static constexpr int TR = TROWS + 2, TC = TCOLS + 2;                                  // 18 x 18: the tile and offset_conv's 1 px halo
    static constexpr int SP = 9, PSB = SP * 16, ROWB = TC * PSB, WIN_BYTES = TR * ROWB;    // 144 B pixels, 2592 B rows, 46 656 B
    static constexpr int NPIECE = TR * TC * SP, NCHUNK = (NPIECE + 63) / 64;              // 2916 pieces, 46 wave-loads (64 lanes x 16 B)
    static constexpr int W3_OFF = WIN_BYTES, W3_TAP = Pack3::W3_TAP, W3_BYTES = Pack3::W3_BYTES;
    static constexpr int LDS_BYTES = W3_OFF + W3_BYTES;                                   // 51 264 B: LDS alone would admit three workgroups per CU
    static constexpr int DCN_TAP = Pack3::DCN_TAP, DCN_W3 = Pack3::DCN_W3, DCN_TAIL = Pack3::DCN_TAIL, OFF_TAIL = Pack3::OFF_TAIL;
    static constexpr unsigned BAD = 0xf0000000u;   // buffer offset of an out-of-image corner: beyond any plane (H*W < 2^24, 144 B pixels)
    static_assert(W3_OFF % 16 == 0 && 3 * LDS_BYTES <= 160 * 1024 && 27 * THREADS * 4 <= WIN_BYTES, "layout");
    static_assert((unsigned long long)(1u << 24) * PSB < BAD, "out-of-image offsets must lie beyond every plane");
};

template <typename TS>
__global__ __launch_bounds__(256, 2) void deform_gather3_kernel(const DeformParams p)
{
#include "deform_gather3_body.inl"
}

template <typename TS> static int launch_deform_gather3(const DeformParams &p, hipStream_t s)
{
    if (!p.off_w || p.pack3 != 1 || !deform_pack3_shape(p.ck, p.nf, p.cin_real, p.cout_real)) return -2;
    if ((long long)p.H * p.W >= (1LL << 24)) return (int)hipErrorInvalidValue;   // 24-bit pixel indices in the corner descriptors
    static PerDeviceOnce once;
    return deform3_launch<Gather3>(&deform_gather3_kernel<TS>, once, Gather3::LDS_BYTES, p, s);
}
