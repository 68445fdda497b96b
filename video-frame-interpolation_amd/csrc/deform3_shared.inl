// What the two bodies of the one-launch ModulatedDeformConvPack have in common: the window body (deform_pack3_body.inl) and the
// window-free gather body (deform_gather3_body.inl), hence both branches of the routed kernel (deform_route3.inl).  The routes must stay
// bit-identical wherever the census shows no fix-up group and must report the same census row, so each stage they share has ONE
// definition and a body keeps only what its route does differently: how the window is staged, where a tap's corner pieces come from,
// the fix-up.
//
// The shared device code is STATEMENTS, not functions: deform3_stages.inl, included by a body once per stage, at the place where the
// stage runs.  Every stage was first tried as a force-inlined function; each of them changed the register allocation or the
// instruction order of at least one of the eight kernels (docs/LABBOOK.md), and these kernels' schedules are pinned by hand.  A stage
// included as text compiles to what the body spelled out before.  This file holds what is defined once per translation unit: the stage
// ids, the tap-offset function and the host-side launch.  Included by deform_pack3.inl.
#pragma once

// stage ids of deform3_stages.inl, in the order a body runs them
#define DEFORM3_TILE 1
#define DEFORM3_LANE 2
#define DEFORM3_LANE_CONST 3
#define DEFORM3_OFFSET_CONV 4
#define DEFORM3_ACC_INIT 5
#define DEFORM3_PICK 6
#define DEFORM3_SAMPLE 7
#define DEFORM3_CORNERS 8
#define DEFORM3_CORNER_DESC 9
#define DEFORM3_TAIL_MMA 10
#define DEFORM3_COUNT_PARKED 11
#define DEFORM3_CENSUS_RECORD 12
#define DEFORM3_EPILOGUE 13

// window byte offset of plain tap t relative to tap 0 in layout C (taps past 8 re-read tap 8: finite data against zero weights)
template <typename C> __host__ __device__ constexpr int deform3_tap_off(int t) { return t < 9 ? ((t / 3) * C::TC + (t % 3)) * C::PSB : (2 * C::TC + 2) * C::PSB; }

// host: the launch of any of the three kernels, in the caller's layout C (Pack3 / Gather3): one workgroup per C::TROWS x C::TCOLS tile
// and batch item.  `lds_bytes` is the kernel's dynamic LDS request, `once` the caller's per-kernel flag (the library is re-entrant and
// serves several devices per process).  Shape checks stay with the callers.
template <typename C, typename K> static int deform3_launch(K *kernel, PerDeviceOnce &once, int lds_bytes, const DeformParams &p, hipStream_t s)
{
    if (const hipError_t e_ = set_lds_limit(once, reinterpret_cast<const void *>(kernel), lds_bytes); e_ != hipSuccess) return (int)e_;
    const long long nwg = (long long)((p.W + C::TCOLS - 1) / C::TCOLS) * ((p.H + C::TROWS - 1) / C::TROWS) * p.B;
    if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    kernel<<<(unsigned)nwg, C::THREADS, lds_bytes, s>>>(p);
    return (int)hipGetLastError();
}
