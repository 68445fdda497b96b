// Host-only exercise of the scene-cut entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check.cpp, host_check_nv12.cpp
// and host_check_resize.cpp: every argument guard of emavfi_luma_signature_u8 / emavfi_scene_flags / emavfi_hold_frames_u8 (include/emavfi.h,
// "SCENE CUT DEFINITION") - no kernel is launched, every call here is refused on the host - and the per-element functions the kernels are
// made of (csrc/scene_elem.h, the same text) in a plain loop over a generated image: the checksums it prints are compared with the numpy
// oracle's by tests/test_scene_cpu.py::test_scene_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/scene_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_scene: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// the generated image of the test: byte c of pixel (y, x)
static unsigned gen(int y, int x, int c) { return (unsigned)(y * 131 + x * 31 + c * 17 + (y * x) % 7) & 255u; }

static void signature(int H, int W, int C, int rgb, std::vector<unsigned> &sig)
{
    sig.assign(EMAVFI_SCENE_SIG_WORDS, 0u);
    for (int i = 0; i < SCENE_GRID; ++i)
        for (int j = 0; j < SCENE_GRID; ++j)
            for (int y = scene_cell_bound(i, H); y < scene_cell_bound(i + 1, H); ++y)
                for (int x = scene_cell_bound(j, W); x < scene_cell_bound(j + 1, W); ++x)
                    sig[i * SCENE_GRID + j] += C == 1 ? gen(y, x, 0) : scene_luma3(gen(y, x, 0), gen(y, x, 1), gen(y, x, 2), rgb);
}

int main()
{
    unsigned char *const sp = (unsigned char *)(uintptr_t)256, *const dp = (unsigned char *)(uintptr_t)4096;   // never dereferenced
    unsigned *const up = (unsigned *)(uintptr_t)8192, *const uq = (unsigned *)(uintptr_t)16384, *const ur = (unsigned *)(uintptr_t)32768;
    unsigned *const odd = (unsigned *)(uintptr_t)8194;
    const int MAXD = 16384;
    static_assert(EMAVFI_SCENE_GRID == SCENE_GRID && EMAVFI_SCENE_SIG_WORDS == SCENE_GRID * SCENE_GRID, "header and scene_elem.h disagree");

    // emavfi_luma_signature_u8(src, pitch, batch_stride, B, H, W, C, order, sig, stream)
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 0, 8, 64, 3, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 2147483647, 8, 64, 3, 0, up, nullptr), "65535");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 0, 64, 3, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, -64, 3, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, MAXD + 1, 64, 3, 0, up, nullptr), "16384");
    REFUSED(emavfi_luma_signature_u8(sp, 1 << 20, 1 << 30, 1, 8, 2147483647, 3, 0, up, nullptr), "16384");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, 64, 2, 0, up, nullptr), "1 or 3");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, 64, 4, 0, up, nullptr), "1 or 3");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, 64, 3, 2, up, nullptr), "order");
    REFUSED(emavfi_luma_signature_u8(sp, 64, 512, 1, 8, 64, 1, -1, up, nullptr), "order");
    REFUSED(emavfi_luma_signature_u8(sp, 191, 1536, 1, 8, 64, 3, 0, up, nullptr), "pitch");
    REFUSED(emavfi_luma_signature_u8(sp, 63, 512, 1, 8, 64, 1, 0, up, nullptr), "pitch");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1535, 2, 8, 64, 3, 0, up, nullptr), "batch stride");
    REFUSED(emavfi_luma_signature_u8(nullptr, 192, 1536, 1, 8, 64, 3, 0, up, nullptr), "null");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, 64, 3, 0, nullptr, nullptr), "null");
    REFUSED(emavfi_luma_signature_u8(sp, 192, 1536, 1, 8, 64, 3, 0, odd, nullptr), "4-byte");
    // the largest shapes and strides: the guards' size arithmetic must not overflow silently
    REFUSED(emavfi_luma_signature_u8(sp, SIZE_MAX, SIZE_MAX, 2, MAXD, MAXD, 3, 0, up, nullptr), "overflows");
    REFUSED(emavfi_luma_signature_u8(sp, (size_t)MAXD * 3, SIZE_MAX, 65535, MAXD, MAXD, 3, 0, up, nullptr), "overflows");
    REFUSED(emavfi_luma_signature_u8(sp, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3 - 1, 65535, MAXD, MAXD, 3, 0, up, nullptr), "batch stride");
    REFUSED(emavfi_luma_signature_u8(nullptr, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3, 65535, MAXD, MAXD, 3, 0, up, nullptr), "null");

    // emavfi_scene_flags(sig_a, stride_a_words, sig_b, stride_b_words, n, H, W, threshold, flags, scores, stream)
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 0, 48, 64, 100, ur, nullptr, nullptr), ">= 1");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 2, 0, 64, 100, ur, nullptr, nullptr), ">= 1");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 2, 48, MAXD + 1, 100, ur, nullptr, nullptr), "16384");
    REFUSED(emavfi_scene_flags(up, 1023, uq, 1024, 2, 48, 64, 100, ur, nullptr, nullptr), "stride");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1, 2, 48, 64, 100, ur, nullptr, nullptr), "stride");
    REFUSED(emavfi_scene_flags(up, SIZE_MAX, uq, 1024, 3, 48, 64, 100, ur, nullptr, nullptr), "overflows");
    REFUSED(emavfi_scene_flags(up, 0, uq, SIZE_MAX / 4, 2147483647, 48, 64, 100, ur, nullptr, nullptr), "overflows");
    REFUSED(emavfi_scene_flags(nullptr, 1024, uq, 1024, 2, 48, 64, 100, ur, nullptr, nullptr), "null");
    REFUSED(emavfi_scene_flags(up, 1024, nullptr, 0, 2, 48, 64, 100, ur, nullptr, nullptr), "null");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 2, 48, 64, 100, nullptr, ur, nullptr), "null");
    REFUSED(emavfi_scene_flags(odd, 1024, uq, 1024, 2, 48, 64, 100, ur, nullptr, nullptr), "4-byte");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 2, 48, 64, 100, odd, nullptr, nullptr), "4-byte");
    REFUSED(emavfi_scene_flags(up, 1024, uq, 1024, 2, 48, 64, 100, ur, odd, nullptr), "4-byte");

    // emavfi_hold_frames_u8(dst, dst_stride, rep, alt, alt_stride, flags, n, frame_bytes, stream)
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4096, up, 0, 4096, nullptr), ">= 1");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 0, sp, 4096, up, 2, 4096, nullptr), ">= 1");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4096, up, 65536, 4096, nullptr), "65535");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 2147483647, sp, 4096, up, 2, 4096, nullptr), "65535");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4096, up, 2, 0, nullptr), "frame_bytes");
    REFUSED(emavfi_hold_frames_u8(dp, SIZE_MAX, 1, sp, SIZE_MAX, up, 1, SIZE_MAX, nullptr), "frame_bytes");
    REFUSED(emavfi_hold_frames_u8(dp, 4095, 1, sp, 4096, up, 2, 4096, nullptr), "smaller than frame_bytes");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4095, up, 2, 4096, nullptr), "smaller than frame_bytes");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 3, sp, 0, up, 1, 4096, nullptr), "smaller than frame_bytes");
    REFUSED(emavfi_hold_frames_u8(dp, SIZE_MAX, 3, sp, 4096, up, 2, 4096, nullptr), "overflows");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 3, sp, SIZE_MAX, up, 65535, 4096, nullptr), "overflows");
    REFUSED(emavfi_hold_frames_u8(nullptr, 4096, 1, sp, 4096, up, 2, 4096, nullptr), "null");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, nullptr, 4096, up, 2, 4096, nullptr), "null");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4096, nullptr, 2, 4096, nullptr), "null");
    REFUSED(emavfi_hold_frames_u8(dp, 4096, 1, sp, 4096, odd, 2, 4096, nullptr), "4-byte");

    // the per-element functions, in a plain loop: cells partition the frame, sums and means as the oracle computes them
    const int shapes[][3] = {{45, 100, 3}, {5, 7, 3}, {70, 130, 1}, {33, 47, 3}};
    for (const auto &sh : shapes) {
        const int H = sh[0], W = sh[1], C = sh[2];
        CHECK(scene_cell_bound(0, H) == 0 && scene_cell_bound(SCENE_GRID, H) == H && scene_cell_bound(SCENE_GRID, W) == W);
        for (int rgb = 0; rgb < (C == 3 ? 2 : 1); ++rgb) {
            std::vector<unsigned> sig;
            signature(H, W, C, rgb, sig);
            unsigned long long total = 0, want = 0;
            unsigned sum_ck = 0, mean_ck = 0;
            for (int k = 0; k < EMAVFI_SCENE_SIG_WORDS; ++k) {
                const int i = k / SCENE_GRID, j = k % SCENE_GRID;
                const unsigned n = (unsigned)((scene_cell_bound(i + 1, H) - scene_cell_bound(i, H)) * (scene_cell_bound(j + 1, W) - scene_cell_bound(j, W)));
                total += sig[k];
                sum_ck += sig[k] * (unsigned)(k + 1);
                if (n) {
                    const unsigned m = scene_cell_mean(sig[k], n);
                    CHECK(m <= 4080u);
                    mean_ck += m * (unsigned)(k + 1);
                } else {
                    CHECK(sig[k] == 0u);
                }
            }
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) want += C == 1 ? gen(y, x, 0) : scene_luma3(gen(y, x, 0), gen(y, x, 1), gen(y, x, 2), rgb);
            CHECK(total == want);
            printf("host_check_scene: %d x %d x %d order %d: sums %u means %u\n", H, W, C, rgb, sum_ck, mean_ck);
        }
    }
    CHECK(scene_luma3(255, 255, 255, 0) == 255u && scene_luma3(0, 0, 0, 1) == 0u && scene_cell_mean(255u * 512u * 512u, 512u * 512u) == 4080u);
    if (g_fail) { fprintf(stderr, "host_check_scene: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_scene: ok\n");
    return 0;
}
