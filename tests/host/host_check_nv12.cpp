// Host-only exercise of the NV12 entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check.cpp: the coefficient
// query and every argument guard of emavfi_preprocess_nv12 / emavfi_postprocess_nv12 (include/emavfi.h, "NV12").  No kernel is launched:
// every call here is refused on the host.  tests/test_nv12_cpu.py::test_nv12_guards_run_clean_under_asan_ubsan builds and runs it.
#include "../../include/emavfi.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_nv12: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)

int main()
{
    // the tables against their definition, recomputed here
    for (int st = EMAVFI_YUV_BT601_LIMITED; st <= EMAVFI_YUV_BT709_FULL; ++st) {
        int dec[5], enc[9];
        CHECK(emavfi_yuv_coefficients(st, dec, enc) == EMAVFI_OK);
        const bool full = st & 1, bt709 = st >> 1;
        const double kr = bt709 ? 0.2126 : 0.299, kb = bt709 ? 0.0722 : 0.114, kg = 1 - kr - kb, s = full ? 1.0 : 255.0 / 224, sp = full ? 1.0 : 224.0 / 255;
        CHECK(dec[0] == (int)floor((full ? 1.0 : 255.0 / 219) * 1048576.0 + 0.5));
        CHECK(dec[1] == (int)floor(2 * (1 - kr) * s * 1048576.0 + 0.5) && dec[4] == (int)floor(2 * (1 - kb) * s * 1048576.0 + 0.5));
        CHECK(dec[2] < 0 && dec[3] < 0 && dec[2] == (int)floor(-2 * kb * (1 - kb) * s / kg * 1048576.0 + 0.5));
        CHECK(enc[5] == enc[6] && enc[5] == (int)floor(0.5 * sp * 1048576.0 + 0.5));
        CHECK(std::abs(enc[3] + enc[4] + enc[5]) <= 1 && std::abs(enc[6] + enc[7] + enc[8]) <= 1);   // grey has no chroma
    }
    int dec[5], enc[9];
    CHECK(emavfi_yuv_coefficients(4, dec, enc) == EMAVFI_E_ARG && strstr(emavfi_last_error(), "standard"));
    CHECK(emavfi_yuv_coefficients(-1, dec, enc) == EMAVFI_E_ARG);
    CHECK(emavfi_yuv_coefficients(0, nullptr, enc) == EMAVFI_E_ARG && emavfi_yuv_coefficients(0, dec, nullptr) == EMAVFI_E_ARG);

    unsigned char *const yp = (unsigned char *)(uintptr_t)256, *const uvp = (unsigned char *)(uintptr_t)512;   // never dereferenced
    float *const f = (float *)(uintptr_t)1024;
    const float m32[3] = {0.485f, 0.456f, 0.406f}, s32[3] = {0.229f, 0.224f, 0.225f}, z32[3] = {0.229f, 0.224f, 0.0f};
    const double m64[3] = {0.485, 0.456, 0.406}, s64[3] = {0.229, 0.224, 0.225}, z64[3] = {0.0, 0.224, 0.225};
#define PRE(y, ypitch, ybs, uv, uvpitch, uvbs, out, B, H, W, st, od, mean, sd) \
    emavfi_preprocess_nv12(y, ypitch, ybs, uv, uvpitch, uvbs, out, B, H, W, st, od, mean, sd, nullptr)
#define POST(y, ypitch, ybs, uv, uvpitch, uvbs, in, B, H, W, st, od, mean, sd) \
    emavfi_postprocess_nv12(in, y, ypitch, ybs, uv, uvpitch, uvbs, B, H, W, st, od, mean, sd, 1, nullptr)
#define BOTH(word, y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, st, od, m_a, s_a, m_b, s_b)                                         \
    do {                                                                                                                               \
        CHECK(PRE(y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, st, od, m_a, s_a) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word));  \
        CHECK(POST(y, ypitch, ybs, uv, uvpitch, uvbs, fp, B, H, W, st, od, m_b, s_b) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word)); \
    } while (0)
    BOTH("null", nullptr, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 64, 512, nullptr, 64, 256, f, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 64, 512, uvp, 64, 256, nullptr, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("null", yp, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, nullptr, s32, nullptr, s64);
    BOTH("null", yp, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, m32, nullptr, m64, nullptr);
    BOTH("y_pitch", yp, 63, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("uv_pitch", yp, 65, 520, uvp, 65, 260, f, 1, 8, 65, 0, 0, m32, s32, m64, s64);        // odd W: 2 * ceil(65 / 2) = 66
    BOTH("batch stride", yp, 64, 511, uvp, 64, 256, f, 2, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("batch stride", yp, 64, 512, uvp, 64, 255, f, 2, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("std[", yp, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, m32, z32, m64, z64);
    BOTH("standard", yp, 64, 512, uvp, 64, 256, f, 1, 8, 64, 4, 0, m32, s32, m64, s64);
    BOTH("order", yp, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 2, m32, s32, m64, s64);
    BOTH("2-byte", yp + 1, 64, 512, uvp, 64, 256, f, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH("2-byte", yp, 64, 512, uvp + 1, 64, 256, f, 1, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 64, 512, uvp, 64, 256, f, 0, 8, 64, 0, 0, m32, s32, m64, s64);
    BOTH(">= 1", yp, 64, 512, uvp, 64, 256, f, 1, -3, 64, 0, 0, m32, s32, m64, s64);
    // huge shapes: the size arithmetic of the guards must not overflow
    BOTH("uv_pitch", yp, (size_t)1 << 31, 0, uvp, 64, 0, f, 1, 2147483647, 2147483647, 0, 0, m32, s32, m64, s64);
    BOTH("batch stride", yp, 2147483647, 64, uvp, (size_t)1 << 31, 64, f, 2, 2147483647, 2147483647, 0, 0, m32, s32, m64, s64);
    if (g_fail) { fprintf(stderr, "host_check_nv12: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_nv12: ok\n");
    return 0;
}
