// The per-element functions of the temporal resample definition (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION"): the blend of one
// sample of two emitted frames.  One text for the kernel (misc_kernels.hip) and for the host check (tests/host/host_check_resample.cpp, a
// plain C++ program): all integer.
#pragma once

#ifdef __HIP__
#define RESAMPLE_HD __host__ __device__
#else
#define RESAMPLE_HD
#endif

constexpr unsigned RESAMPLE_POOL_NODES = 0x80000000u;   // EMAVFI_RESAMPLE_NODES: the pool bit of a table entry's a / b
constexpr int RESAMPLE_CAP = 64;                        // EMAVFI_RESAMPLE_LAUNCH_CAP: table entries per launch

// ((256 - w) a + w b + 128) >> 8 for samples a, b <= 65535 and w in 0..256: at most 256 * 65535 + 128 < 2^32, and the result never
// exceeds max(a, b)
RESAMPLE_HD inline unsigned resample_blend(unsigned a, unsigned b, unsigned w) { return ((256u - w) * a + w * b + 128u) >> 8; }
// one 16-bit little-endian word: the sample is (word >> shift) & mask, the result is written back as v << shift (the other bits: zero)
RESAMPLE_HD inline unsigned resample_blend_word(unsigned wa, unsigned wb, unsigned w, unsigned mask, int shift)
{
    return resample_blend((wa >> shift) & mask, (wb >> shift) & mask, w) << shift;
}
// four bytes / two words at once, as the 16-byte path of the kernel holds them: the same per-element function on every lane of the dword
RESAMPLE_HD inline unsigned resample_blend_dword(unsigned da, unsigned db, unsigned w, int sample_bytes, unsigned mask, int shift)
{
    if (sample_bytes == 1)
        return resample_blend(da & 255u, db & 255u, w) | (resample_blend((da >> 8) & 255u, (db >> 8) & 255u, w) << 8) |
               (resample_blend((da >> 16) & 255u, (db >> 16) & 255u, w) << 16) | (resample_blend(da >> 24, db >> 24, w) << 24);
    return resample_blend_word(da & 65535u, db & 65535u, w, mask, shift) | (resample_blend_word(da >> 16, db >> 16, w, mask, shift) << 16);
}
