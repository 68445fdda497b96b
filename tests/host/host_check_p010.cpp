// Host-only exercise of the high-bit-depth entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_nv12.cpp: the
// coefficient query against a recomputation, every argument guard of emavfi_preprocess_p010 / emavfi_postprocess_p010 (include/emavfi.h,
// "HIGH BIT DEPTH"; no kernel is launched: every call here is refused on the host), and the per-element functions of csrc/p010_elem.h -
// the text the kernels run - in a plain loop against a second restatement written here from the header's formulas.
// tests/test_p010_cpu.py::test_p010_host_check_runs_clean_under_asan_ubsan builds and runs it.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/p010_elem.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_p010: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)

// ---- the second restatement: floor division spelled out, 128-bit sums, no shared helper
static long long floor_div_2_20(__int128 a) { return (long long)(a >= 0 ? a / 1048576 : -((-a + 1048575) / 1048576)); }
static long long clipP(long long v, long long P) { return v < 0 ? 0 : v > P ? P : v; }
struct Ref { int dec[5], enc[9]; long long P, mid, yoff; bool rgb; };
static Ref ref_of(int st, int depth, int order)
{
    Ref k{};
    emavfi_yuv_coefficients_depth(st, depth, k.dec, k.enc);
    k.P = (1ll << depth) - 1; k.mid = 1ll << (depth - 1); k.yoff = (st & 1) ? 0 : 16ll << (depth - 8); k.rgb = order == EMAVFI_ORDER_RGB;
    return k;
}
static void ref_decode(long long Y, long long U, long long V, const Ref &k, long long ch[3])
{
    const long long l = Y - k.yoff > 0 ? Y - k.yoff : 0, u = U - k.mid, v = V - k.mid;
    const long long r = clipP(floor_div_2_20((__int128)k.dec[0] * l + (__int128)k.dec[1] * v + 524288), k.P);
    const long long g = clipP(floor_div_2_20((__int128)k.dec[0] * l + (__int128)k.dec[2] * u + (__int128)k.dec[3] * v + 524288), k.P);
    const long long b = clipP(floor_div_2_20((__int128)k.dec[0] * l + (__int128)k.dec[4] * u + 524288), k.P);
    ch[0] = k.rgb ? r : b; ch[1] = g; ch[2] = k.rgb ? b : r;
}
static long long ref_row(const int *c, long long r, long long g, long long b, long long off, long long P)
{
    return clipP(floor_div_2_20((__int128)c[0] * r + (__int128)c[1] * g + (__int128)c[2] * b + 524288) + off, P);
}
static long long ref_quant(float x, double mean, double sd, int denorm, long long P)
{
    double v = (double)x;
    if (denorm) v = v * sd + mean;
    if (std::isnan(v)) return 0;
    return (long long)std::trunc(std::fmin(std::fmax(v, 0.0), 1.0) * (double)P);
}

static void check_elements(int depth, int st, int order, int ystep, int cstep)
{
    const Ref R = ref_of(st, depth, order);
    P010Coef k{};
    emavfi_yuv_coefficients_depth(st, depth, k.dec, k.enc);
    p010_constants(depth, (st & 1) == 0, k);
    k.rgb = order == EMAVFI_ORDER_RGB;
    CHECK(k.P == R.P && k.mid == R.mid && k.yoff == R.yoff && k.shift == 16 - depth);
    const int P = k.P;
    int bad = 0;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    for (int Y = 0; Y <= P; Y += (Y + ystep > P && Y != P) ? P - Y : ystep)
        for (int U = 0; U <= P; U += (U + cstep > P && U != P) ? P - U : cstep)
            for (int V = 0; V <= P; V += (V + cstep > P && V != P) ? P - V : cstep) {
                int ch[3];
                long long want[3];
                // words with junk in the low bits decode as their top bits
                const unsigned junk = (unsigned)((Y * 7 + U * 3 + V) & ((1 << k.shift) - 1));
                p010_decode(p010_sample(((unsigned)Y << k.shift) | junk, k), p010_sample(((unsigned)U << k.shift) | junk, k),
                            p010_sample(((unsigned)V << k.shift) | junk, k), k, ch);
                ref_decode(Y, U, V, R, want);
                for (int c = 0; c < 3; ++c) {
                    bad += ch[c] != want[c];
                    const float n = p010_norm(ch[c], (float)P, mean[c], sd[c]), w = (((float)want[c] / (float)R.P) - mean[c]) / sd[c];
                    bad += std::memcmp(&n, &w, 4) != 0;
                }
                // the decoded pixel encoded again: luma of the pixel, chroma of a block of four such pixels and of a block with the P corner
                const long long r = R.rgb ? want[0] : want[2], g = want[1], b = R.rgb ? want[2] : want[0];
                bad += p010_luma(ch, k) != ref_row(R.enc, r, g, b, R.yoff, R.P);
                for (int corner = 0; corner < 2; ++corner) {
                    int sum[3], Ue, Ve;
                    long long m[3];
                    for (int c = 0; c < 3; ++c) {
                        sum[c] = 3 * ch[c] + (corner ? P : ch[c]);
                        m[c] = (3 * want[c] + (corner ? R.P : want[c]) + 2) / 4;
                    }
                    p010_chroma(sum, k, Ue, Ve);
                    const long long mr = R.rgb ? m[0] : m[2], mb = R.rgb ? m[2] : m[0];
                    bad += Ue != ref_row(R.enc + 3, mr, m[1], mb, R.mid, R.P);
                    bad += Ve != ref_row(R.enc + 6, mr, m[1], mb, R.mid, R.P);
                }
            }
    // quantisation: NaN, infinities, out-of-range values and the exact k / P boundaries with their neighbours
    const double m64[3] = {0.485, 0.456, 0.406}, s64[3] = {0.229, 0.224, 0.225};
    const float special[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             -1.0f, 2.0f, 0.0f, -0.0f, 1.0f, 1e-30f, -3.0f, 3.0f};
    for (int denorm = 0; denorm < 2; ++denorm)
        for (int c = 0; c < 3; ++c) {
            for (float x : special) bad += p010_quant(x, m64[c], s64[c], denorm, (double)P) != ref_quant(x, m64[c], s64[c], denorm, R.P);
            for (int q = 0; q <= P; q += (q + 37 > P && q != P) ? P - q : 37) {
                float x = (float)((double)q / P);
                if (denorm) x = (float)(((double)q / P - m64[c]) / s64[c]);
                for (float t : {std::nextafterf(x, -10.0f), x, std::nextafterf(x, 10.0f)}) {
                    const int got = p010_quant(t, m64[c], s64[c], denorm, (double)P);
                    bad += got != ref_quant(t, m64[c], s64[c], denorm, R.P) || got < 0 || got > P;
                }
            }
        }
    if (bad) { fprintf(stderr, "host_check_p010: depth %d standard %d order %d: %d element(s) differ\n", depth, st, order, bad); ++g_fail; }
}

int main()
{
    // the tables against their definition, recomputed here; depth 8 against the NV12 query
    for (int depth : {8, 10, 12, 16})
        for (int st = EMAVFI_YUV_BT601_LIMITED; st <= EMAVFI_YUV_BT2020_FULL; ++st) {
            int dec[5], enc[9];
            CHECK(emavfi_yuv_coefficients_depth(st, depth, dec, enc) == EMAVFI_OK);
            const bool full = st & 1;
            const int mat = st >> 1;
            const double kr = mat == 0 ? 0.299 : mat == 1 ? 0.2126 : 0.2627, kb = mat == 0 ? 0.114 : mat == 1 ? 0.0722 : 0.0593, kg = 1 - kr - kb;
            const double P = std::ldexp(1.0, depth) - 1, Yr = full ? P : std::ldexp(219.0, depth - 8), Cr = full ? P : std::ldexp(224.0, depth - 8);
            const double s = P / Cr, sp = Cr / P;
            CHECK(dec[0] == (int)floor(P / Yr * 1048576.0 + 0.5));
            CHECK(dec[1] == (int)floor(2 * (1 - kr) * s * 1048576.0 + 0.5) && dec[4] == (int)floor(2 * (1 - kb) * s * 1048576.0 + 0.5));
            CHECK(dec[2] < 0 && dec[3] < 0 && dec[2] == (int)floor(-2 * kb * (1 - kb) * s / kg * 1048576.0 + 0.5));
            CHECK(dec[3] == (int)floor(-2 * kr * (1 - kr) * s / kg * 1048576.0 + 0.5));
            CHECK(enc[0] == (int)floor(kr * (Yr / P) * 1048576.0 + 0.5) && enc[1] == (int)floor(kg * (Yr / P) * 1048576.0 + 0.5));
            CHECK(enc[5] == enc[6] && enc[5] == (int)floor(0.5 * sp * 1048576.0 + 0.5));
            CHECK(std::abs(enc[3] + enc[4] + enc[5]) <= 1 && std::abs(enc[6] + enc[7] + enc[8]) <= 1);   // grey has no chroma
            if (depth == 8 && st <= EMAVFI_YUV_BT709_FULL) {
                int d8[5], e8[9];
                CHECK(emavfi_yuv_coefficients(st, d8, e8) == EMAVFI_OK);
                CHECK(!memcmp(d8, dec, sizeof dec) && !memcmp(e8, enc, sizeof enc));
            }
        }
    int dec[5], enc[9];
    const int adec[5] = {1224536, 1765394, -197003, -684025, 2252416};
    const int aenc[9] = {235879, 608777, 53246, -128236, -330964, 459200, 459200, -422268, -36933};
    CHECK(emavfi_yuv_coefficients_depth(EMAVFI_YUV_BT2020_LIMITED, 10, dec, enc) == EMAVFI_OK && !memcmp(dec, adec, sizeof dec) && !memcmp(enc, aenc, sizeof enc));
    CHECK(emavfi_yuv_coefficients_depth(6, 10, dec, enc) == EMAVFI_E_ARG && strstr(emavfi_last_error(), "standard"));
    CHECK(emavfi_yuv_coefficients_depth(-1, 10, dec, enc) == EMAVFI_E_ARG);
    CHECK(emavfi_yuv_coefficients_depth(0, 9, dec, enc) == EMAVFI_E_ARG && strstr(emavfi_last_error(), "depth"));
    CHECK(emavfi_yuv_coefficients_depth(0, 10, nullptr, enc) == EMAVFI_E_ARG && emavfi_yuv_coefficients_depth(0, 10, dec, nullptr) == EMAVFI_E_ARG);
    CHECK(emavfi_yuv_coefficients(EMAVFI_YUV_BT2020_LIMITED, dec, enc) == EMAVFI_E_ARG);   // the 8-bit query keeps refusing BT.2020

    unsigned char *const yp = (unsigned char *)(uintptr_t)256, *const uvp = (unsigned char *)(uintptr_t)512;   // never dereferenced
    float *const f = (float *)(uintptr_t)1024;
    const float m32[3] = {0.485f, 0.456f, 0.406f}, s32[3] = {0.229f, 0.224f, 0.225f}, z32[3] = {0.229f, 0.224f, 0.0f};
    const double m64[3] = {0.485, 0.456, 0.406}, s64[3] = {0.229, 0.224, 0.225}, z64[3] = {0.0, 0.224, 0.225};
#define PRE(y, ypitch, ybs, uv, uvpitch, uvbs, out, B, H, W, d, st, od, mean, sd) \
    emavfi_preprocess_p010(y, ypitch, ybs, uv, uvpitch, uvbs, out, B, H, W, d, st, od, mean, sd, nullptr)
#define POST(y, ypitch, ybs, uv, uvpitch, uvbs, in, B, H, W, d, st, od, mean, sd) \
    emavfi_postprocess_p010(in, y, ypitch, ybs, uv, uvpitch, uvbs, B, H, W, d, st, od, mean, sd, 1, nullptr)
#define BOTH(word, y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, d, st, od, m_a, s_a, m_b, s_b)                                         \
    do {                                                                                                                                  \
        CHECK(PRE(y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, d, st, od, m_a, s_a) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word));  \
        CHECK(POST(y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, d, st, od, m_b, s_b) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word)); \
    } while (0)
    // a valid frame here: W = 64 words = 128 bytes per Y row and per UV row, H = 8: Y plane 1024 bytes, UV plane 512
    BOTH("null", nullptr, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, nullptr, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, uvp, 128, 512, nullptr, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, nullptr, s32, nullptr, s64);
    BOTH("null", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, nullptr, m64, nullptr);
    BOTH("depth", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 8, 0, 0, m32, s32, m64, s64);
    BOTH("depth", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 11, 0, 0, m32, s32, m64, s64);
    BOTH("depth", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 0, 0, 0, m32, s32, m64, s64);
    BOTH("standard", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 6, 0, m32, s32, m64, s64);
    BOTH("standard", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, -1, 0, m32, s32, m64, s64);
    BOTH("order", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 2, m32, s32, m64, s64);
    BOTH("y_pitch", yp, 126, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("y_pitch", yp, 129, 1032, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);       // odd
    BOTH("uv_pitch", yp, 130, 1040, uvp, 130, 520, f, 1, 8, 65, 10, 0, 0, m32, s32, m64, s64);      // odd W: 4 * ceil(65 / 2) = 132
    BOTH("uv_pitch", yp, 128, 1024, uvp, 130, 520, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);      // no multiple of 4
    BOTH("batch stride", yp, 128, 1022, uvp, 128, 512, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("batch stride", yp, 128, 1024, uvp, 128, 508, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("batch stride", yp, 128, 1025, uvp, 128, 512, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);  // large enough, misaligning frame 1
    BOTH("std[", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, z32, m64, z64);
    BOTH("2-byte", yp + 1, 128, 1024, uvp, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("4-byte", yp, 128, 1024, uvp + 2, 128, 512, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, uvp, 128, 512, f, 0, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, uvp, 128, 512, f, 1, -3, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, uvp, 128, 512, f, 1, 8, 0, 10, 0, 0, m32, s32, m64, s64);
    // huge shapes: the size arithmetic of the guards must not overflow
    BOTH("uv_pitch", yp, (size_t)1 << 32, 0, uvp, 64, 0, f, 1, 2147483647, 2147483647, 16, 5, 1, m32, s32, m64, s64);
    BOTH("batch stride", yp, (size_t)1 << 32, 64, uvp, (size_t)1 << 33, 64, f, 2, 2147483647, 2147483647, 12, 4, 0, m32, s32, m64, s64);
    BOTH("batch stride", yp, ~(size_t)1, ~(size_t)1, uvp, ~(size_t)3, ~(size_t)3, f, 2, 2147483647, 2147483647, 10, 0, 0, m32, s32, m64, s64);

    // the per-element functions: depth 10 over all 1024 luma values x a chroma lattice, depths 12 and 16 sampled (extremes included)
    for (int st = EMAVFI_YUV_BT601_LIMITED; st <= EMAVFI_YUV_BT2020_FULL; ++st) {
        check_elements(10, st, st & 1 ? EMAVFI_ORDER_RGB : EMAVFI_ORDER_BGR, 1, 31);
        check_elements(12, st, st & 2 ? EMAVFI_ORDER_RGB : EMAVFI_ORDER_BGR, 53, 211);
        check_elements(16, st, st & 1 ? EMAVFI_ORDER_BGR : EMAVFI_ORDER_RGB, 797, 3301);
    }
    if (g_fail) { fprintf(stderr, "host_check_p010: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_p010: ok\n");
    return 0;
}
