// Host-only exercise of the resize entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check.cpp and
// host_check_nv12.cpp: every argument guard of emavfi_resize_u8 / emavfi_preprocess_u8_resized / emavfi_preprocess_nv12_resized
// (include/emavfi.h, "RESIZE DEFINITION").  No kernel is launched: every call here is refused on the host.
// tests/test_resize_cpu.py::test_resize_guards_run_clean_under_asan_ubsan builds and runs it.
#include "../../include/emavfi.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_resize: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

int main()
{
    unsigned char *const sp = (unsigned char *)(uintptr_t)256, *const dp = (unsigned char *)(uintptr_t)4096;   // never dereferenced
    unsigned char *const uvp = (unsigned char *)(uintptr_t)512, *const op = (unsigned char *)(uintptr_t)8192;
    float *const f = (float *)(uintptr_t)16384;
    const float m[4] = {0.485f, 0.456f, 0.406f, 0.5f}, s[4] = {0.229f, 0.224f, 0.225f, 0.5f}, z[4] = {0.229f, 0.224f, 0.0f, 0.5f};
    const int MAXD = EMAVFI_RESIZE_MAX_DIM;

    // emavfi_resize_u8(src, src_pitch, src_bs, dst, dst_pitch, dst_bs, B, Hs, Ws, Hd, Wd, C, stream)
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 0, 8, 64, 4, 32, 3, nullptr), ">= 1");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 1, 8, 64, 4, -32, 3, nullptr), ">= 1");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 1, MAXD + 1, 64, 4, 32, 3, nullptr), "16384");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 1, 8, 64, 4, 2147483647, 3, nullptr), "16384");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 2147483647, 8, 64, 4, 32, 3, nullptr), "65535");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 1, 8, 64, 4, 32, 0, nullptr), "1..4");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 384, 1, 8, 64, 4, 32, 2147483647, nullptr), "1..4");
    REFUSED(emavfi_resize_u8(sp, 191, 1536, dp, 96, 384, 1, 8, 64, 4, 32, 3, nullptr), "src_pitch");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 95, 384, 1, 8, 64, 4, 32, 3, nullptr), "dst_pitch");
    REFUSED(emavfi_resize_u8(sp, 192, 1535, dp, 96, 384, 2, 8, 64, 4, 32, 3, nullptr), "src batch stride");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, dp, 96, 383, 2, 8, 64, 4, 32, 3, nullptr), "dst batch stride");
    REFUSED(emavfi_resize_u8(nullptr, 192, 1536, dp, 96, 384, 1, 8, 64, 4, 32, 3, nullptr), "null");
    REFUSED(emavfi_resize_u8(sp, 192, 1536, nullptr, 96, 384, 1, 8, 64, 4, 32, 3, nullptr), "null");
    // the largest shapes and strides: the size arithmetic of the guards must not overflow
    REFUSED(emavfi_resize_u8(sp, (size_t)MAXD * 4, (size_t)MAXD * MAXD * 4 - 1, dp, (size_t)MAXD * 4, (size_t)MAXD * MAXD * 4, 65535, MAXD, MAXD, MAXD, MAXD,
                             4, nullptr), "src batch stride");
    REFUSED(emavfi_resize_u8(nullptr, SIZE_MAX, SIZE_MAX, dp, SIZE_MAX, SIZE_MAX, 1, MAXD, MAXD, MAXD, MAXD, 4, nullptr), "null");

    // emavfi_preprocess_u8_resized(frames, out, resized, B, Hs, Ws, Hd, Wd, C, mean, std, stream)
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 8, 64, 4, 32, 3, nullptr, s, nullptr), "null");
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 8, 64, 4, 32, 3, m, nullptr, nullptr), "null");
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 0, 64, 4, 32, 3, m, s, nullptr), ">= 1");
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 8, MAXD + 1, 4, 32, 3, m, s, nullptr), "16384");
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 8, 64, 4, 32, 5, m, s, nullptr), "1..4");
    REFUSED(emavfi_preprocess_u8_resized(sp, f, nullptr, 1, 8, 64, 4, 32, 3, m, z, nullptr), "std[2]");
    REFUSED(emavfi_preprocess_u8_resized(nullptr, f, dp, 1, 8, 64, 4, 32, 3, m, s, nullptr), "null");
    REFUSED(emavfi_preprocess_u8_resized(sp, nullptr, dp, 1, 8, 64, 4, 32, 3, m, s, nullptr), "null");
    REFUSED(emavfi_preprocess_u8_resized(sp, (float *)((uintptr_t)f + 2), dp, 1, 8, 64, 4, 32, 3, m, s, nullptr), "4-byte");

#define NV12R(y, ypitch, ybs, uv, uvpitch, uvbs, out, yo, yop, yobs, uvo, uvop, uvobs, B, Hs, Ws, Hd, Wd, st, od, mean, sd) \
    emavfi_preprocess_nv12_resized(y, ypitch, ybs, uv, uvpitch, uvbs, out, yo, yop, yobs, uvo, uvop, uvobs, B, Hs, Ws, Hd, Wd, st, od, mean, sd, nullptr)
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, nullptr, s), "null");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 0, 32, 0, 0, m, s), ">= 1");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, MAXD + 1, 0, 0, m, s), "16384");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 4, 0, m, s), "standard");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 2, m, s), "order");
    REFUSED(NV12R(sp, 63, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "y_pitch");
    REFUSED(NV12R(sp, 65, 520, uvp, 65, 260, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 65, 4, 32, 0, 0, m, s), "uv_pitch");   // odd Ws: 2 * ceil(65 / 2) = 66
    REFUSED(NV12R(sp, 64, 511, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 2, 8, 64, 4, 32, 0, 0, m, s), "batch stride");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 255, f, nullptr, 0, 0, nullptr, 0, 0, 2, 8, 64, 4, 32, 0, 0, m, s), "batch stride");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, z), "std[2]");
    REFUSED(NV12R(nullptr, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "null");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, nullptr, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "null");
    REFUSED(NV12R(sp + 1, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "2-byte");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, op, 31, 128, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "y_out_pitch");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, op, 31, 64, 1, 8, 64, 4, 31, 0, 0, m, s), "uv_out_pitch");   // odd Wd: 32 bytes
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, op, 32, 127, nullptr, 0, 0, 2, 8, 64, 4, 32, 0, 0, m, s), "y_out batch stride");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, nullptr, 0, 0, op, 32, 63, 2, 8, 64, 4, 32, 0, 0, m, s), "uv_out batch stride");
    REFUSED(NV12R(sp, 64, 512, uvp, 64, 256, f, op + 1, 32, 128, nullptr, 0, 0, 1, 8, 64, 4, 32, 0, 0, m, s), "2-byte");
    REFUSED(NV12R(sp, (size_t)MAXD, 0, uvp, (size_t)MAXD, 0, f, op, SIZE_MAX, SIZE_MAX, op, SIZE_MAX, SIZE_MAX, 65535, MAXD, MAXD, MAXD, MAXD, 0, 0, m, s),
            "batch stride");
    if (g_fail) { fprintf(stderr, "host_check_resize: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_resize: ok\n");
    return 0;
}
