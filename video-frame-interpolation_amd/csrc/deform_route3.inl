// The ROUTED one-launch ModulatedDeformConvPack (include/emavfi.h, emavfi_forward_adaptive): one kernel per 16-bit
// storage type that reads its block's route word in device memory (DeformParams::route) and runs either deform_pack3_kernel<TS, true>'s
// window body (EMAVFI_ROUTE_WINDOW = 0) or deform_gather3_kernel<TS>'s window-free body (EMAVFI_ROUTE_GATHER = 1), statement for statement
// (deform_pack3_body.inl / deform_gather3_body.inl, their common stages in deform3_stages.inl): same DeformParams forms, same output,
// same census record.  The word is written on
// the device by the adaptive forward's route selector (misc_kernels.hip, route_select_kernel), so a captured graph or a stream of
// batches changes routes without a host read.
//
// Geometry: both bodies use the same grid (16 x 16 tiles, the same XCD-aware order), 256 threads and __launch_bounds__(256, 2); the
// launch requests the window's 81 312 B of LDS (the gather body uses the first 51 264 B), still two workgroups per CU.
//
// The kernel is an explicit specialisation deform_pack3_kernel<Route3<TS>, true>: it belongs to the pack's family (its LDS-DMA is the
// window body's, tests/test_cabi_cpu.py), and the two plain kernels keep their code objects.  A specialisation is defined once per
// program, so each storage type's translation unit includes this file with DEFORM_ROUTE3_TS set (deform_bf16.hip, deform_f16.hip).
#pragma once
#include "deform_gather3.inl"

#ifndef DEFORM_ROUTE3_TS
#error "define DEFORM_ROUTE3_TS (bf16_t or half_t) before including deform_route3.inl: one translation unit per storage type"
#endif

template <typename TS> struct Route3 {};   // tag of the routed instantiation of deform_pack3_kernel

// The kernel's operands, read afresh in each branch: the kernel-argument pointer goes through an empty asm statement, so the compiler
// cannot hoist the argument loads both bodies share above the branch.  Hoisted, they stay live through either body and push the window
// body's scalar registers (101 of 102 on their own) into VGPR lanes - one VGPR fewer for the gather body, which has none to spare
// (hoisted: 6 SGPR and 5 VGPR spills in the bf16 kernel; as written: none and one, a census flag that only waves with a sample
// beyond the window read back; the f16 kernel has none).
__device__ __forceinline__ DeformParams route3_params()
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const DeformParams kparams_t;
    kparams_t *k = (kparams_t *)__builtin_amdgcn_kernarg_segment_ptr();   // (the kernel's only explicit argument, at offset 0)
    asm volatile("" : "+s"(k));
    return *k;
#else
    return DeformParams{};   // (host pass: never called)
#endif
}

template <>
__global__ __launch_bounds__(256, 2) void deform_pack3_kernel<Route3<DEFORM_ROUTE3_TS>, true>(const DeformParams args)
{
    using TS = DEFORM_ROUTE3_TS;
    constexpr bool FUSE_OFF = true;
    // one plain load of a word every lane reads: the branch is uniform over the launch
    if (__builtin_amdgcn_readfirstlane(*args.route) != 0u) {
        const DeformParams p = route3_params();
#include "deform_gather3_body.inl"
    } else {
        const DeformParams p = route3_params();
#include "deform_pack3_body.inl"
    }
}

static int launch_deform_route3(const DeformParams &p, hipStream_t s)
{
    using C = Pack3;
    using G = Gather3;
    static_assert(C::THREADS == G::THREADS && C::WAVES == G::WAVES && C::TROWS == G::TROWS && C::TCOLS == G::TCOLS && G::LDS_BYTES <= C::LDS_BYTES,
                  "the two bodies share the grid, the block and the LDS request");
    // what the shared stages (deform3_stages.inl) take from either layout: only the row pitch TC and W3_OFF may differ
    static_assert(C::SP == G::SP && C::PSB == G::PSB, "one pixel record: 9 pieces of 16 bytes");
    static_assert(C::W3_TAP == G::W3_TAP && C::W3_BYTES == G::W3_BYTES, "one third-fragment table");
    static_assert(C::DCN_TAP == G::DCN_TAP && C::DCN_W3 == G::DCN_W3 && C::DCN_TAIL == G::DCN_TAIL && C::OFF_TAIL == G::OFF_TAIL, "one weight blob");
    if (!p.route || !p.off_w || p.pack3 != 1 || !deform_pack3_shape(p.ck, p.nf, p.cin_real, p.cout_real)) return -2;
    if ((long long)p.H * p.W >= (1LL << 24)) return (int)hipErrorInvalidValue;   // the gather body's 24-bit pixel indices
    static PerDeviceOnce once;
    return deform3_launch<C>(&deform_pack3_kernel<Route3<DEFORM_ROUTE3_TS>, true>, once, C::LDS_BYTES, p, s);
}
