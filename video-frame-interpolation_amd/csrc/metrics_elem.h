// The per-element functions of the frame-metric definition (include/emavfi.h, "FRAME METRIC DEFINITION"): the window weights, the squared
// difference, the row pass of the five moments at one position, one tap of the column pass and the double-precision tail.
// One text for the kernel (misc_kernels.hip) and for the host check (tests/host/host_check_metrics.cpp, a plain C++ program).  Everything
// up to the tail is unsigned integer; the tail is IEEE double in a fixed operation order and must be compiled with contraction off
// (-ffp-contract=off; the pragma below says the same for this function's own text).
#pragma once

#ifdef __HIP__
#define METRICS_HD __host__ __device__
#else
#define METRICS_HD
#endif

constexpr int METRICS_WIN = 11;        // EMAVFI_METRICS_WINDOW: the window is 11 x 11
constexpr int METRICS_HALO = 10;       // a tile of n windows along an axis reads n + 10 pixels

// per-axis weight j = 0..10: floor(g_real 65536 + 0.5) of the normalised Gaussian (sigma 1.5), the centre raised by one: the sum is 65536
METRICS_HD inline unsigned metrics_weight(int j)
{
    constexpr unsigned g[METRICS_WIN] = {67u, 498u, 2359u, 7167u, 13960u, 17434u, 13960u, 7167u, 2359u, 498u, 67u};
    return g[j];
}

// (a - b)^2 of two bytes, at most 65025
METRICS_HD inline unsigned metrics_sqdiff(unsigned a, unsigned b)
{
    const unsigned d = a > b ? a - b : b - a;
    return d * d;
}

// the row pass at one position: the 11 bytes pa[j stride], pb[j stride] -> {sum g a, sum g b, sum g a^2, sum g b^2, sum g a b};
// each is at most 65025 * 65536 < 2^32
METRICS_HD inline void metrics_row5(const unsigned char *pa, const unsigned char *pb, int stride, unsigned out[5])
{
    unsigned sa = 0u, sb = 0u, saa = 0u, sbb = 0u, sab = 0u;
#pragma unroll
    for (int j = 0; j < METRICS_WIN; ++j) {
        const unsigned g = metrics_weight(j), a = pa[j * stride], b = pb[j * stride];
        sa += g * a;
        sb += g * b;
        saa += g * (a * a);
        sbb += g * (b * b);
        sab += g * (a * b);
    }
    out[0] = sa; out[1] = sb; out[2] = saa; out[3] = sbb; out[4] = sab;
}

// one tap of the column pass: acc += g[j] * (a row-pass word); eleven of them stay below 65025 * 2^32 < 2^48
METRICS_HD inline unsigned long long metrics_col_tap(unsigned long long acc, int j, unsigned v) { return acc + (unsigned long long)metrics_weight(j) * v; }

// the tail: five exact moments (each < 2^48, scaled by 2^32) -> q = floor(ssim_of_the_window * 2^32), in exactly this operation order
METRICS_HD inline long long metrics_tail(unsigned long long A, unsigned long long B, unsigned long long Axx, unsigned long long Ayy, unsigned long long Axy)
{
#pragma clang fp contract(off)
    const double C1 = 6.5025, C2 = 58.5225, S = 1.0 / 4294967296.0;     // (0.01 * 255)^2, (0.03 * 255)^2, 2^-32
    const double a = (double)A * S, b = (double)B * S, axx = (double)Axx * S, ayy = (double)Ayy * S, axy = (double)Axy * S;   // exact
    const double aa = a * a, bb = b * b, ab = a * b;
    const double sx = axx - aa, sy = ayy - bb, sxy = axy - ab;
    const double num = (2.0 * ab + C1) * (2.0 * sxy + C2);
    const double den = ((aa + bb) + C1) * ((sx + sy) + C2);
    const double m = num / den;
    return (long long)__builtin_floor(m * 4294967296.0);
}
