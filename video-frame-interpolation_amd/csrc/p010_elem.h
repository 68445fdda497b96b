// The per-element functions of the high-bit-depth colour definition (include/emavfi.h, "HIGH BIT DEPTH"): constants, decode, normalise,
// quantise, luma, chroma.  One text for the kernels (misc_kernels.hip: the Yuv16 formats of preprocess_yuv420_kernel / postprocess_yuv420_kernel) and for the host check (tests/host/host_check_p010.cpp, a plain
// C++ program).  Integers are signed 64-bit fixed point with 20 fractional bits: a coefficient fits 32 bits, its operand 18, so every
// product is one 32 x 32 -> 64 multiply-add; the float side is preprocess_u8's / postprocess_u8's arithmetic with 255 -> P.
#pragma once

#ifdef __HIP__
#define P010_HD __host__ __device__
#else
#define P010_HD
#endif

// tables of emavfi_yuv_coefficients_depth and the constants of one (standard, depth, order); shift = 16 - depth; rgb: channel 0 is R
struct P010Coef { int dec[5], enc[9], P, mid, yoff, shift, rgb; };

// P, mid, yoff, shift of a depth in {8, 10, 12, 16}; limited: the standard's code is even
P010_HD inline void p010_constants(int depth, int limited, P010Coef &k)
{
    k.P = (1 << depth) - 1;
    k.mid = 1 << (depth - 1);
    k.yoff = limited ? 16 << (depth - 8) : 0;
    k.shift = 16 - depth;
}
P010_HD inline int p010_clip(long long v, int P) { return v < 0 ? 0 : v > P ? P : (int)v; }
// the sample of a 16-bit word: its top `depth` bits
P010_HD inline int p010_sample(unsigned word, const P010Coef &k) { return (int)((word & 0xffffu) >> k.shift); }
// one pixel: samples (Y, U, V) -> three d-bit integers, ch[0] = channel 0 of `order`
P010_HD inline void p010_decode(int Y, int U, int V, const P010Coef &k, int ch[3])
{
    const int u = U - k.mid, v = V - k.mid, l = Y - k.yoff > 0 ? Y - k.yoff : 0;
    const long long yl = (long long)k.dec[0] * l + (1 << 19);
    const int r = p010_clip((yl + (long long)k.dec[1] * v) >> 20, k.P);
    const int g = p010_clip((yl + (long long)k.dec[2] * u + (long long)k.dec[3] * v) >> 20, k.P);
    const int b = p010_clip((yl + (long long)k.dec[4] * u) >> 20, k.P);
    ch[0] = k.rgb ? r : b; ch[1] = g; ch[2] = k.rgb ? b : r;
}
// preprocess_u8's two true divisions, same order, with 255 -> P
P010_HD inline float p010_norm(int value, float P, float mean, float stdv)
{
    const float v = (float)value / P;
    return (v - mean) / stdv;
}
// postprocess_u8's integer of one element with 255 -> P: float64, truncation, NaN -> 0
P010_HD inline int p010_quant(float x, double mean, double stdv, int denorm, double P)
{
    double v = (double)x;
    if (denorm) v = v * stdv + mean;
    v = v > 0.0 ? v : 0.0;        // NaN compares false: 0
    v = v < 1.0 ? v : 1.0;
    return (int)(v * P);
}
P010_HD inline int p010_luma(const int ch[3], const P010Coef &k)
{
    const int r = k.rgb ? ch[0] : ch[2], g = ch[1], b = k.rgb ? ch[2] : ch[0];
    return p010_clip((((long long)k.enc[0] * r + (long long)k.enc[1] * g + (long long)k.enc[2] * b + (1 << 19)) >> 20) + k.yoff, k.P);
}
// sum[c]: the 2x2 block's four integers of channel c added up
P010_HD inline void p010_chroma(const int sum[3], const P010Coef &k, int &U, int &V)
{
    const int m0 = (sum[0] + 2) >> 2, m1 = (sum[1] + 2) >> 2, m2 = (sum[2] + 2) >> 2;
    const int r = k.rgb ? m0 : m2, g = m1, b = k.rgb ? m2 : m0;
    U = p010_clip((((long long)k.enc[3] * r + (long long)k.enc[4] * g + (long long)k.enc[5] * b + (1 << 19)) >> 20) + k.mid, k.P);
    V = p010_clip((((long long)k.enc[6] * r + (long long)k.enc[7] * g + (long long)k.enc[8] * b + (1 << 19)) >> 20) + k.mid, k.P);
}
