// ModulatedDeformConvPack (ema_vfi.py:23-60) at the reference width (67 -> 27 offsets/masks, 67 -> 67) as ONE launch,
// 16-bit storage types - round 3 rebuild of deform_pack.inl around what its counters and ISA showed:
// the kernel is bound by instruction issue at two waves per SIMD, so this version removes issued work.
//
//   * K = 64 + 3.  The three warped-frame channels (64..66) used to cost a fifth k-group in every tap (3 real of 16
//     input channels: 6 of 30 MFMAs, 6 of 15 weight-fragment loads, 8 corner reads and 16 blend instructions per tap).
//     Now every tap contracts exactly the 64 feature channels (4 k-groups), and the three tail channels of ALL NINE taps
//     are one im2col step at the end: each half-lane blends the tail of ITS OWN pixel per tap (4 eight-byte corner
//     reads, 8 packed FMAs), keeps the 9 x 3 values in registers, and three k-groups (K index = tap slot * 4 + channel,
//     27 real of 48) contract them after the tap loop.  The offset_conv does the same with the undeformed window.
//     Issued MFMAs per wave: 90 + 270 -> 78 + 234; blend instructions per tap 144 -> 136; LDS reads 40 -> 36.
//   * The third output fragment (channels 64..66: 3 real rows of 32) takes its A operand from a 4.5 KiB table in LDS
//     ([tap][k-group][row 0..2 | zero row][half][16 B], every lane of a zero row reads the same 16 bytes: a broadcast)
//     instead of a 1 KiB global fragment per k-group: weight-fragment traffic L2/L1 -> registers 15 -> 8 KiB per wave and tap
//     (64 B/clk per CU was a co-limit: 8 waves x 15 KiB per tap).
//   * Window DMA by rows: wave w owns pixels [7w, 7w+7) of every window row (wave 3: the last two), so a lane's
//     (pixel, piece) and its source pointer / row increment are computed ONCE and a DMA instruction costs one 64-bit add
//     and one select (was ~25 address instructions per DMA instruction, 6 200 cycles of issue per tile).
//   * The blend is issued corner-major (four independent chains), which hipcc's scheduler had turned back into four dependent
//     chains with a wait state behind every v_pk_fma_f16 (63 s_nop per tap); the sample-outside-the-window fix-up is a pass of its
//     own behind the tap loop (round 6: an arena in the then dead window, the same tap body), so the common path carries none of
//     its address arithmetic or EXEC regions.
//   * bf16 storage may hand f16 bit patterns between consecutive packs (DeformParams::in_f16 / out_f16): the window is f16 on
//     chip anyway (deform_pack.inl), so pack i+1 skips the in-LDS conversion pass and the intermediate fusion tensor keeps 11
//     significant bits instead of 8.
//
// Geometry, lane <-> pixel assignment, the f16 on-chip arithmetic and the fallback semantics are those of deform_pack.inl.
#pragma once
#include "deform_pack.inl"

// timing-only ablations (wrong results; the tap loop's, bits 0-3, 6, 7, leave the offsets alone: every sample stays in the window):
// bit 0 no weight-fragment loads in the tap loop, 1 undeformed (conflict-free) gathers, 2 no blend beyond its first four multiplies,
// 3 no 32x32x16 MFMAs in the tap loop, 4 no window DMA, 5 no offset_conv MFMAs, 6 no third-fragment MFMAs, 7 no corner reads
#ifndef EMAVFI_P3_ABL
#define EMAVFI_P3_ABL 0
#endif
// measurement build: request 100 KiB of LDS per workgroup = ONE workgroup (one wave per SIMD) per CU - what a wave's phases cost
// without a partner on its SIMD
#ifndef EMAVFI_P3_ONE_WG
#define EMAVFI_P3_ONE_WG 0
#endif
// A/B builds (round 6): what the census and the fix-up hand-shake cost a tile that has no sample outside its window.  NO_HANDSHAKE is
// only legal together with -DEMAVFI_DEFORM_ABL_NO_FALLBACK=1 (no wave ever waits): timing only, wrong results beyond the window.
#ifndef EMAVFI_P3_NO_CENSUS
#define EMAVFI_P3_NO_CENSUS 0
#endif
#ifndef EMAVFI_P3_NO_HANDSHAKE
#define EMAVFI_P3_NO_HANDSHAKE 0
#endif
struct Pack3 {
    static constexpr int R = 2, TROWS = 16, TCOLS = 16, WAVES = 4, THREADS = 256;
    static constexpr int TR = TROWS + 3 + 2 * R, TC = TCOLS + 3 + 2 * R;                 // 23 x 23 window pixels
    static constexpr int SP = 9, PSB = SP * 16, ROWB = TC * PSB, WIN_BYTES = TR * ROWB;  // 144 B pixels, 3312 B rows, 76 176 B
    static constexpr int SEG_PX = 7, SEG_BYTES = SEG_PX * PSB;                            // one DMA instruction = 7 pixels x 9 pieces
    static constexpr int LAST_PX = TC - 3 * SEG_PX;                                       // wave 3: the last 2 pixels of a row
    static constexpr int W3_OFF = WIN_BYTES, W3_TAP = 4 * 4 * 2 * 16, W3_BYTES = 9 * W3_TAP;  // third-fragment A operands
    // fix-up arena (round 6): once all four waves have left the tap loop the window is dead, and every wave owns a quarter of it as an
    // arena of 32 entries = {4 corners x 9 pieces | one pad slot} (an odd number of 16-byte slots: conflict-free like the window's pixels);
    // entry 31 is all zeros (what lanes without a sample in the round read against zero weights)
    // Layout: piece-major - row (2 i + hb) = 32 slots x 16 B holds piece i % 9 of corner (2 hb + i / 9) of every slot, i = 0..17 - because an
    // LDS-DMA instruction writes lane-linear: instruction i fetches row 2 i from lanes 0..31 and row 2 i + 1 from lanes 32..63, each lane
    // ONE slot's corner pair (2 hb, 2 hb + 1) for the whole round: a DMA instruction costs one 64-bit add.  Slot 31 is all zeros.
    static constexpr int NENT = 31, SLOTS = 32, AROW = SLOTS * 16, ADMA = 2 * SP;         // 512 B rows, 18 DMA instructions per round
    static constexpr int ARENA_BYTES = (WIN_BYTES / 4) & ~15;                             // 19 040 B per wave
    static constexpr int A_KG = 2 * 2 * AROW, A_H = 2 * AROW, A_C1 = SP * 2 * AROW, A_C2 = AROW;   // k-group / piece / corner strides
    static constexpr int SYNC_OFF = W3_OFF + W3_BYTES;                                    // u32: waves that have left the tap loop
    static constexpr int TAB_OFF = SYNC_OFF + 16, TAB_BYTES = 4 * 32 * 4;                 // per wave 32 corner descriptors
    static constexpr int LDS_BYTES = TAB_OFF + TAB_BYTES;                                 // 81 312 B: two workgroups per CU
    static_assert(4 * SP * AROW <= ARENA_BYTES && NENT < SLOTS, "arena");
    // packed weights (bytes): DCN = [tap][kg 4][nf 2][lane][16] | W3 table | tail [j 3][nf 3][lane][16]
    static constexpr int DCN_TAP = 4 * 2 * 1024, DCN_W3 = 9 * DCN_TAP, DCN_TAIL = DCN_W3 + W3_BYTES, DCN_BYTES = DCN_TAIL + 9 * 1024;
    // offset_conv = [tap][kg 4][lane][16] | tail [j 3][lane][16]
    static constexpr int OFF_TAP = 4 * 1024, OFF_TAIL = 9 * OFF_TAP, OFF_BYTES = OFF_TAIL + 3 * 1024;
    static_assert(SEG_PX * SP <= 64 && LAST_PX > 0 && LAST_PX <= SEG_PX, "row segments");
    static_assert(WIN_BYTES % 16 == 0 && 2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
    static_assert(ROWB + PSB + 8 * 16 + 15 < 65536, "corner offsets must fit the ds_read immediate");
};

// Pins a point of the hand-made schedule: an empty volatile asm that "rewrites" the four partial sums (instruction selection
// otherwise places plain arithmetic anywhere between its operands and its users, on either side of a scheduling fence - half of
// the steps came out with their blend sunk behind their MFMAs), then the fence for the machine scheduler.  The asm emits no
// instruction, so the hazard recogniser still sees the real producer of every MFMA operand.
#define PACK3_PIN(a)                                                                  \
    do {                                                                              \
        asm volatile("" : "+v"((a)[0]), "+v"((a)[1]), "+v"((a)[2]), "+v"((a)[3]));    \
        __builtin_amdgcn_sched_barrier(0);                                            \
    } while (0)

#include "deform3_shared.inl"   // the stages this kernel's body has in common with the window-free route's (deform_gather3.inl)

template <typename TS, bool FUSE_OFF>
__global__ __launch_bounds__(256, 2) void deform_pack3_kernel(const DeformParams p)
{
#include "deform_pack3_body.inl"
}

template <typename TS, bool FUSE_OFF> static int launch_deform_pack3(const DeformParams &p, hipStream_t s)
{
    static PerDeviceOnce once;
    return deform3_launch<Pack3>(&deform_pack3_kernel<TS, FUSE_OFF>, once, EMAVFI_P3_ONE_WG ? 100 * 1024 : Pack3::LDS_BYTES, p, s);
}
