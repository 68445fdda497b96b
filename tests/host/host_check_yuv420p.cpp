// Host-only exercise of the planar 4:2:0 entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_nv12.cpp and
// host_check_p010.cpp: every argument guard of emavfi_preprocess_yuv420p / emavfi_postprocess_yuv420p (include/emavfi.h, "PLANAR 4:2:0"; no
// kernel is launched: every call here is refused on the host), and the per-element path of the kernels in a plain loop - what
// csrc/yuv420p_elem.h adds (where a sample sits in a word and in a row piece) feeding csrc/p010_elem.h, against the interleaved element
// functions on the words the definition names: (w & (2^d - 1)) << (16 - d) on the way in, the P010 word >> (16 - d) on the way out.  Depth 8
// runs through the same functions: there the depth tables are the NV12 tables (host_check_p010 pins that), and a byte is its own sample.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/yuv420p_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_yuv420p: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)

static P010Coef coef_of(int st, int depth, int order)
{
    P010Coef k{};
    emavfi_yuv_coefficients_depth(st, depth, k.dec, k.enc);
    p010_constants(depth, (st & 1) == 0, k);
    k.rgb = order == EMAVFI_ORDER_RGB;
    return k;
}

// one lane's block as the kernels walk it: NX = 16 / sizeof(sample) columns x 2 rows, samples fetched from / put into dword row pieces
template <int BITS> static void check_block(int depth, int st, int order, unsigned seed)
{
    constexpr int NX = 128 / BITS;
    const P010Coef k = coef_of(st, depth, order);
    const unsigned P = (unsigned)k.P, full = 0xffffffffu >> (32 - BITS);
    unsigned yw[2][4], uw[2], vw[2], x = seed * 2654435761u + 12345u;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (auto &row : yw) for (unsigned &w : row) w = next();      // garbage in the high bits of every word included
    for (unsigned &w : uw) w = next();
    for (unsigned &w : vw) w = next();
    int bad = 0;
    unsigned yo[2][4] = {}, uo[2] = {}, vo[2] = {};
    int px[2][NX][3];
    for (int r = 0; r < 2; ++r)
        for (int p = 0; p < NX; ++p) {
            const unsigned wy = yuv420p_get<BITS>(yw[r], p), wu = yuv420p_get<BITS>(uw, p >> 1), wv = yuv420p_get<BITS>(vw, p >> 1);
            // the row piece read as the memory it is
            const unsigned char *mem = (const unsigned char *)yw[r];
            unsigned direct = 0;
            memcpy(&direct, mem + p * (BITS / 8), BITS / 8);
            bad += wy != direct || wy > full;
            int ch[3], want[3];
            p010_decode(yuv420p_sample(wy, k.P), yuv420p_sample(wu, k.P), yuv420p_sample(wv, k.P), k, ch);
            // the definition: the interleaved entry on the masked word shifted to the top
            p010_decode(p010_sample((wy & P) << k.shift, k), p010_sample((wu & P) << k.shift, k), p010_sample((wv & P) << k.shift, k), k, want);
            for (int c = 0; c < 3; ++c) { bad += ch[c] != want[c]; px[r][p][c] = ch[c]; }
        }
    // encode the decoded block again: planar words against the interleaved words >> shift, and zero high bits
    for (int r = 0; r < 2; ++r)
        for (int p = 0; p < NX; ++p) yuv420p_put<BITS>(yo[r], p, (unsigned)p010_luma(px[r][p], k));
    for (int q = 0; q < NX / 2; ++q) {
        int sum[3], U, V;
        for (int c = 0; c < 3; ++c) sum[c] = px[0][2 * q][c] + px[0][2 * q + 1][c] + px[1][2 * q][c] + px[1][2 * q + 1][c];
        p010_chroma(sum, k, U, V);
        yuv420p_put<BITS>(uo, q, (unsigned)U);
        yuv420p_put<BITS>(vo, q, (unsigned)V);
        const unsigned pu = ((unsigned)U << k.shift) & 0xffffu, pv = ((unsigned)V << k.shift) & 0xffffu;   // the P010 words
        bad += yuv420p_get<BITS>(uo, q) != (pu >> k.shift) || yuv420p_get<BITS>(vo, q) != (pv >> k.shift);
        bad += (yuv420p_get<BITS>(uo, q) & ~P) != 0 || (yuv420p_get<BITS>(vo, q) & ~P) != 0;
    }
    for (int r = 0; r < 2; ++r)
        for (int p = 0; p < NX; ++p) {
            const unsigned got = yuv420p_get<BITS>(yo[r], p), word = ((unsigned)p010_luma(px[r][p], k) << k.shift) & 0xffffu;
            bad += got != (word >> k.shift) || (got & ~P) != 0;
        }
    if (bad) { fprintf(stderr, "host_check_yuv420p: depth %d standard %d order %d: %d element(s) differ\n", depth, st, order, bad); ++g_fail; }
}

int main()
{
    unsigned char *const yp = (unsigned char *)(uintptr_t)256, *const up = (unsigned char *)(uintptr_t)2048, *const vp = (unsigned char *)(uintptr_t)4096;
    float *const f = (float *)(uintptr_t)8192;   // never dereferenced
    const float m32[3] = {0.485f, 0.456f, 0.406f}, s32[3] = {0.229f, 0.224f, 0.225f}, z32[3] = {0.229f, 0.224f, 0.0f};
    const double m64[3] = {0.485, 0.456, 0.406}, s64[3] = {0.229, 0.224, 0.225}, z64[3] = {0.0, 0.224, 0.225};
#define BOTH(word, y, ypitch, ybs, u, upitch, ubs, v, vpitch, vbs, fp, B, H, W, d, st, od, m_a, s_a, m_b, s_b)                               \
    do {                                                                                                                                     \
        CHECK(emavfi_preprocess_yuv420p(y, ypitch, ybs, u, upitch, ubs, v, vpitch, vbs, fp, B, H, W, d, st, od, m_a, s_a, nullptr)          \
              == EMAVFI_E_ARG && strstr(emavfi_last_error(), word));                                                                         \
        CHECK(emavfi_postprocess_yuv420p(fp, y, ypitch, ybs, u, upitch, ubs, v, vpitch, vbs, B, H, W, d, st, od, m_b, s_b, 1, nullptr)      \
              == EMAVFI_E_ARG && strstr(emavfi_last_error(), word));                                                                         \
    } while (0)
    // a valid frame here: W = 64, H = 8.  Depth 10: 128 bytes per Y row, 64 per chroma row; Y plane 1024 bytes, U and V 256 each
    BOTH("null", nullptr, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, nullptr, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, up, 64, 256, nullptr, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, up, 64, 256, vp, 64, 256, nullptr, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, nullptr, s32, nullptr, s64);
    BOTH("null", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, nullptr, m64, nullptr);
    for (int d : {0, 9, 11, 14, 32, -8}) BOTH("depth", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, d, 0, 0, m32, s32, m64, s64);
    BOTH("standard", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 6, 0, m32, s32, m64, s64);
    BOTH("standard", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, -1, 0, m32, s32, m64, s64);
    BOTH("standard", yp, 64, 512, up, 32, 128, vp, 32, 128, f, 1, 8, 64, 8, 4, 0, m32, s32, m64, s64);          // BT.2020 is not an 8-bit standard
    BOTH("order", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 2, m32, s32, m64, s64);
    BOTH("y_pitch", yp, 126, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("y_pitch", yp, 129, 1032, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);        // odd at depth > 8
    BOTH("y_pitch", yp, 63, 512, up, 32, 128, vp, 32, 128, f, 1, 8, 64, 8, 0, 0, m32, s32, m64, s64);
    BOTH("u_pitch", yp, 128, 1024, up, 62, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("u_pitch", yp, 128, 1024, up, 65, 260, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);        // odd
    BOTH("v_pitch", yp, 128, 1024, up, 64, 256, vp, 62, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("v_pitch", yp, 128, 1024, up, 64, 256, vp, 67, 268, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);        // odd
    BOTH("v_pitch", yp, 130, 1040, up, 66, 264, vp, 64, 256, f, 1, 8, 65, 10, 0, 0, m32, s32, m64, s64);        // odd W: ceil(65 / 2) = 33 words
    BOTH("v_pitch", yp, 65, 520, up, 33, 132, vp, 32, 128, f, 1, 8, 65, 8, 0, 0, m32, s32, m64, s64);
    BOTH("y batch stride", yp, 128, 1022, up, 64, 256, vp, 64, 256, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("u batch stride", yp, 128, 1024, up, 64, 254, vp, 64, 256, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("v batch stride", yp, 128, 1024, up, 64, 256, vp, 64, 254, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("y batch stride", yp, 128, 1025, up, 64, 256, vp, 64, 256, f, 2, 8, 64, 10, 0, 0, m32, s32, m64, s64);  // large enough, misaligning frame 1
    BOTH("std[", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, z32, m64, z64);
    BOTH("y pointer", yp + 1, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH("u pointer", yp, 128, 1024, up + 1, 64, 256, vp, 64, 256, f, 1, 8, 64, 12, 0, 0, m32, s32, m64, s64);
    BOTH("v pointer", yp, 128, 1024, up, 64, 256, vp + 3, 64, 256, f, 1, 8, 64, 16, 0, 0, m32, s32, m64, s64);
    BOTH("fp32 pointer", yp, 128, 1024, up, 64, 256, vp, 64, 256, (float *)(uintptr_t)8194, 1, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    // depth 8 takes odd pitches and odd pointers: the next refusal is the last one
    BOTH("fp32 pointer", yp + 1, 65, 520, up + 1, 33, 132, vp + 3, 35, 140, (float *)(uintptr_t)8194, 1, 8, 64, 8, 3, 1, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 0, 8, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, -3, 64, 10, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 128, 1024, up, 64, 256, vp, 64, 256, f, 1, 8, 0, 10, 0, 0, m32, s32, m64, s64);
    // huge shapes: the size arithmetic of the guards must not overflow
    BOTH("u_pitch", yp, (size_t)1 << 32, 0, up, 64, 0, vp, 64, 0, f, 1, 2147483647, 2147483647, 16, 5, 1, m32, s32, m64, s64);
    BOTH("y batch stride", yp, (size_t)1 << 32, 64, up, (size_t)1 << 32, 64, vp, (size_t)1 << 32, 64, f, 2, 2147483647, 2147483647, 12, 4, 0, m32, s32, m64, s64);
    BOTH("y batch stride", yp, ~(size_t)1, ~(size_t)1, up, ~(size_t)1, ~(size_t)1, vp, ~(size_t)1, ~(size_t)1, f, 2, 2147483647, 2147483647, 10, 0, 0, m32, s32, m64, s64);

    // the per-element path: both sample widths, every depth and standard, many blocks of pseudo-random words
    for (unsigned seed = 0; seed < 200; ++seed) {
        for (int st = EMAVFI_YUV_BT601_LIMITED; st <= EMAVFI_YUV_BT709_FULL; ++st) check_block<8>(8, st, (int)(seed & 1), seed * 7 + (unsigned)st);
        for (int depth : {10, 12, 16})
            for (int st = EMAVFI_YUV_BT601_LIMITED; st <= EMAVFI_YUV_BT2020_FULL; ++st) check_block<16>(depth, st, (int)((seed >> 1) & 1), seed * 13 + (unsigned)(st + depth));
    }
    if (g_fail) { fprintf(stderr, "host_check_yuv420p: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_yuv420p: ok\n");
    return 0;
}
