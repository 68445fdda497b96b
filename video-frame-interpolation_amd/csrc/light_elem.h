// The per-element functions of the linear-light definition (include/emavfi.h, "LINEAR LIGHT DEFINITION"): one sample of up to SHUTTER_MAX_TAPS
// emitted frames decoded to light through a table, averaged there, and encoded back to the nearest code.  One text for the kernel
// (misc_kernels.hip) and for the host check (tests/host/host_check_light.cpp, a plain C++ program): all integer, the sums unsigned 64-bit.
// `lin` is the table of 2^depth words - in the kernel its copy in LDS; every index formed here is below 2^depth whatever the table holds.
#pragma once

#include "shutter_elem.h"

#ifdef __HIP__
#define LIGHT_HD __host__ __device__ __forceinline__
#else
#define LIGHT_HD inline
#endif

constexpr unsigned LIGHT_ONE = 1u << 28;     // the light of nominal white above that of nominal black
constexpr unsigned LIGHT_BIAS = 1u << 26;    // the light of nominal black: codes below it keep distinct, ordered values
constexpr unsigned LIGHT_LIMIT = 1u << 30;   // every value of a valid table lies below this

// x / S for x < 2^48 and S in 1..65535, M = shutter_magic(S): schoolbook division in base 2^16.  A remainder is below S < 2^16, so a
// partial dividend r 2^16 + digit is below 2^32 and shutter_div takes it.  The digits of the quotient: the first is below 2^16 as x's is,
// the others below 2^16 as r < S.  (A mean of table values is below 2^32: its first digit is zero.)
LIGHT_HD unsigned long long light_div(unsigned long long x, unsigned S, unsigned M)
{
    const unsigned x2 = (unsigned)(x >> 32), x1 = (unsigned)(x >> 16) & 65535u, x0 = (unsigned)x & 65535u;
    const unsigned q2 = shutter_div(x2, S, M);
    const unsigned d1 = ((x2 - q2 * S) << 16) | x1;
    const unsigned q1 = shutter_div(d1, S, M);
    const unsigned d0 = ((d1 - q1 * S) << 16) | x0;
    const unsigned q0 = shutter_div(d0, S, M);
    return ((unsigned long long)q2 << 32) + ((unsigned long long)q1 << 16) + q0;
}
// (sum + S / 2) / S of a finished sum of w_j lin[s_j]: below 2^46 for a valid table, below 2^48 for any
LIGHT_HD unsigned light_mean(unsigned long long sum, unsigned S, unsigned M) { return (unsigned)light_div(sum + (S >> 1), S, M); }

// enc(L): the largest v with v == 0 or lin[v - 1] + lin[v] <= 2 L - the code nearest in light, a tie going up.  `depth` steps, one bit of
// v each; the candidate c lies in 1 .. 2^depth - 1, so lin[c - 1] and lin[c] are inside the table.  The sums are taken in 32 bits: exact for
// a valid table (values and L below 2^30); a table that is not valid gives some code, never an index outside the table.
LIGHT_HD unsigned light_enc(unsigned L, const unsigned *lin, int depth)
{
    unsigned v = 0u;
    for (int bit = depth - 1; bit >= 0; --bit) {
        const unsigned c = v | (1u << bit);
        if (lin[c - 1u] + lin[c] <= 2u * L) v = c;
    }
    return v;
}

// four bytes / two words at once, as shutter_elem.h's ShutterSums: the light sums of one dword's samples (words: s0 and s1 only)
struct LightSums { unsigned long long s0, s1, s2, s3; };
LIGHT_HD void light_add_dword(LightSums &acc, unsigned d, unsigned w, const unsigned *lin, int sample_bytes, unsigned mask, int shift)
{
    w &= 65535u;   // a validated weight is below 2^16
    if (sample_bytes == 1) {   // mask = 255 here; said again so that the index is bounded whatever the caller passes
        acc.s0 += (unsigned long long)w * lin[d & 255u & mask]; acc.s1 += (unsigned long long)w * lin[(d >> 8) & 255u & mask];
        acc.s2 += (unsigned long long)w * lin[(d >> 16) & 255u & mask]; acc.s3 += (unsigned long long)w * lin[(d >> 24) & mask];
    } else {
        acc.s0 += (unsigned long long)w * lin[shutter_sample(d & 65535u, mask, shift)];
        acc.s1 += (unsigned long long)w * lin[shutter_sample(d >> 16, mask, shift)];
    }
}
// the dword of the codes of those sums' means, each written back as v << shift (the other bits of a word: zero)
LIGHT_HD unsigned light_mean_dword(const LightSums &acc, unsigned S, unsigned M, const unsigned *lin, int sample_bytes, int depth, int shift)
{
    if (sample_bytes == 1)
        return light_enc(light_mean(acc.s0, S, M), lin, depth) | (light_enc(light_mean(acc.s1, S, M), lin, depth) << 8) |
               (light_enc(light_mean(acc.s2, S, M), lin, depth) << 16) | (light_enc(light_mean(acc.s3, S, M), lin, depth) << 24);
    return (light_enc(light_mean(acc.s0, S, M), lin, depth) << shift) | (light_enc(light_mean(acc.s1, S, M), lin, depth) << (shift + 16));
}
