// The per-element functions of the shutter definition (include/emavfi.h, "SHUTTER DEFINITION"): the weighted integer mean of one sample of
// up to SHUTTER_MAX_TAPS emitted frames.  One text for the kernel (misc_kernels.hip) and for the host check (tests/host/host_check_shutter.cpp,
// a plain C++ program): all integer, unsigned 32-bit throughout.
#pragma once

#ifdef __HIP__
#define SHUTTER_HD __host__ __device__
#else
#define SHUTTER_HD
#endif

constexpr int SHUTTER_MAX_TAPS = 33;          // EMAVFI_ACCUMULATE_MAX_TAPS: the nodes 0 .. G of the deepest tree (G = 32)
constexpr int SHUTTER_CAP = 8;                // EMAVFI_ACCUMULATE_LAUNCH_CAP: table entries per launch
constexpr unsigned SHUTTER_MAX_SUM = 65535u;  // the largest sum of an entry's weights

// x / S for every x < 2^32 and S in 1..65535 without a division: M = shutter_magic(S) = floor((2^32 - 1) / S) is computed once per entry
// on the host.  With 2^32 = M S + c, 1 <= c <= S: floor(x M / 2^32) = floor(x / S - x c / (S 2^32)), and x c / (S 2^32) < 1, so the
// estimate is the quotient or one below it; one comparison of the remainder settles which.  q S <= x: nothing wraps.
SHUTTER_HD inline unsigned shutter_magic(unsigned S) { return 0xffffffffu / S; }
SHUTTER_HD inline unsigned shutter_div(unsigned x, unsigned S, unsigned M)
{
    const unsigned q = (unsigned)(((unsigned long long)x * M) >> 32);
    return q + (x - q * S >= S ? 1u : 0u);
}
// (sum + S / 2) / S of a finished sum of w_j s_j: sum <= 65535 * 65535, so sum + S / 2 < 2^32
SHUTTER_HD inline unsigned shutter_mean(unsigned sum, unsigned S, unsigned M) { return shutter_div(sum + (S >> 1), S, M); }

// one 16-bit little-endian word (or a byte: mask 255, shift 0): the sample is (word >> shift) & mask
SHUTTER_HD inline unsigned shutter_sample(unsigned word, unsigned mask, int shift) { return (word >> shift) & mask; }

// four bytes / two words at once, as the 16-byte path of the kernel holds them: the sums of one dword's samples (words: s0 and s1 only) -
// named members, not an array, so that they are registers whatever the optimiser makes of the loop around them
struct ShutterSums { unsigned s0, s1, s2, s3; };
SHUTTER_HD inline void shutter_add_dword(ShutterSums &acc, unsigned d, unsigned w, int sample_bytes, unsigned mask, int shift)
{
    w &= 65535u;   // a validated weight is below 2^16 as every sample is: said here, the compiler multiplies at the 24-bit rate
    if (sample_bytes == 1) {
        acc.s0 += w * (d & 255u); acc.s1 += w * ((d >> 8) & 255u); acc.s2 += w * ((d >> 16) & 255u); acc.s3 += w * (d >> 24);
    } else {
        acc.s0 += w * shutter_sample(d & 65535u, mask, shift); acc.s1 += w * shutter_sample(d >> 16, mask, shift);
    }
}
// the dword of the means of those sums, each written back as v << shift (the other bits of a word: zero)
SHUTTER_HD inline unsigned shutter_mean_dword(const ShutterSums &acc, unsigned S, unsigned M, int sample_bytes, int shift)
{
    if (sample_bytes == 1)
        return shutter_mean(acc.s0, S, M) | (shutter_mean(acc.s1, S, M) << 8) | (shutter_mean(acc.s2, S, M) << 16) | (shutter_mean(acc.s3, S, M) << 24);
    return (shutter_mean(acc.s0, S, M) << shift) | (shutter_mean(acc.s1, S, M) << (shift + 16));
}
