// Host-only exercise of the duplicate-frame entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_scene.cpp and
// the others: every argument guard of emavfi_frame_diff_cells / emavfi_duplicate_flags (include/emavfi.h, "DUPLICATE FRAME DEFINITION") - no
// kernel is launched, every call here is refused on the host - and the per-element functions the kernels are made of (csrc/dedup_elem.h and
// csrc/scene_elem.h, the same text) in a plain loop over generated images, against closed forms; the checksums it prints are compared with
// the numpy oracle's by tests/test_dedup_cpu.py::test_dedup_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/scene_elem.h"
#include "../../video-frame-interpolation_amd/csrc/dedup_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_dedup: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// the generated images of the test: element c of pixel (y, x) of image `which`, a 16-bit word
static unsigned gen(int which, int y, int x, int c)
{
    const unsigned v = (unsigned)(y * 131 + x * 31 + c * 17 + (y * x) % 7) * 2654435761u;
    return ((which ? v * 40503u + 12345u : v) >> 9) & 65535u;
}

// cells of the generated pair through the per-element functions: C = 1 samples of (depth, shift) - bytes: depth 8 of the low byte - or C = 3 bytes
static void cells_of(int H, int W, int C, int rgb, unsigned mask, int shift, unsigned elem_mask, std::vector<unsigned> &out)
{
    out.assign(DEDUP_CELLS, 0u);
    for (int i = 0; i < SCENE_GRID; ++i)
        for (int j = 0; j < SCENE_GRID; ++j) {
            unsigned long long sad = 0;
            unsigned n = 0;
            for (int y = scene_cell_bound(i, H); y < scene_cell_bound(i + 1, H); ++y)
                for (int x = scene_cell_bound(j, W); x < scene_cell_bound(j + 1, W); ++x, ++n) {
                    unsigned l[2];
                    for (int q = 0; q < 2; ++q)
                        l[q] = C == 1 ? dedup_sample(gen(q, y, x, 0) & elem_mask, mask, shift)
                                      : scene_luma3(gen(q, y, x, 0) & 255u, gen(q, y, x, 1) & 255u, gen(q, y, x, 2) & 255u, rgb);
                    sad += dedup_absdiff(l[0], l[1]);
                }
            out[i * SCENE_GRID + j] = n ? dedup_cell_measure(sad, n) : 0u;
        }
}

int main()
{
    unsigned char *const ap = (unsigned char *)(uintptr_t)256, *const bp = (unsigned char *)(uintptr_t)65536;   // never dereferenced
    unsigned *const up = (unsigned *)(uintptr_t)8192, *const uq = (unsigned *)(uintptr_t)16384, *const ur = (unsigned *)(uintptr_t)32768;
    unsigned *const odd = (unsigned *)(uintptr_t)8194;
    const int MAXD = 16384;
    static_assert(EMAVFI_SCENE_SIG_WORDS == DEDUP_CELLS && EMAVFI_SCENE_GRID == SCENE_GRID, "header, scene_elem.h and dedup_elem.h disagree");

    // emavfi_frame_diff_cells(a, a_pitch, a_batch_stride, b, b_pitch, b_batch_stride, n, H, W, C, order, sample_bytes, depth, shift, cells, stream)
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 0, 8, 64, 3, 0, 1, 8, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 65536, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "65535");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 0, 64, 3, 0, 1, 8, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 8, -64, 3, 0, 1, 8, 0, up, nullptr), ">= 1");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, MAXD + 1, 64, 3, 0, 1, 8, 0, up, nullptr), "16384");
    REFUSED(emavfi_frame_diff_cells(ap, 1 << 20, 1 << 30, bp, 1 << 20, 1 << 30, 1, 8, 2147483647, 3, 0, 1, 8, 0, up, nullptr), "16384");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 2, 0, 1, 8, 0, up, nullptr), "1 or 3");
    REFUSED(emavfi_frame_diff_cells(ap, 256, 2048, bp, 256, 2048, 1, 8, 64, 4, 0, 1, 8, 0, up, nullptr), "1 or 3");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, 2, 1, 8, 0, up, nullptr), "order");
    REFUSED(emavfi_frame_diff_cells(ap, 64, 512, bp, 64, 512, 1, 8, 64, 1, -1, 1, 8, 0, up, nullptr), "order");
    REFUSED(emavfi_frame_diff_cells(ap, 64, 512, bp, 64, 512, 1, 8, 64, 1, 0, 0, 8, 0, up, nullptr), "sample_bytes");
    REFUSED(emavfi_frame_diff_cells(ap, 64, 512, bp, 64, 512, 1, 8, 64, 1, 0, 4, 8, 0, up, nullptr), "sample_bytes");
    REFUSED(emavfi_frame_diff_cells(ap, 64, 512, bp, 64, 512, 1, 8, 64, 1, 0, 1, 10, 0, up, nullptr), "depth");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 8, 0, up, nullptr), "depth");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 14, 0, up, nullptr), "depth");
    REFUSED(emavfi_frame_diff_cells(ap, 64, 512, bp, 64, 512, 1, 8, 64, 1, 0, 1, 8, 1, up, nullptr), "shift");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 10, 7, up, nullptr), "shift");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 12, 5, up, nullptr), "shift");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 16, 1, up, nullptr), "shift");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 10, -1, up, nullptr), "shift");
    REFUSED(emavfi_frame_diff_cells(ap, 384, 3072, bp, 384, 3072, 1, 8, 64, 3, 0, 2, 10, 0, up, nullptr), "C = 3 at sample_bytes 2");
    REFUSED(emavfi_frame_diff_cells(ap, 191, 1536, bp, 192, 1536, 1, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "a_pitch");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 63, 1536, 1, 8, 64, 1, 0, 1, 8, 0, up, nullptr), "b_pitch");
    REFUSED(emavfi_frame_diff_cells(ap, 127, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "a_pitch");
    REFUSED(emavfi_frame_diff_cells(ap, 129, 1040, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "odd");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 131, 1048, 1, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "odd");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1535, bp, 192, 1536, 2, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "a_batch_stride");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1535, 2, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "b_batch_stride");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1025, bp, 128, 1024, 2, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "odd");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp, 128, 1027, 2, 8, 64, 1, 0, 2, 16, 0, up, nullptr), "odd");
    REFUSED(emavfi_frame_diff_cells(nullptr, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "null");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, nullptr, 192, 1536, 1, 8, 64, 3, 0, 1, 8, 0, up, nullptr), "null");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, 0, 1, 8, 0, nullptr, nullptr), "null");
    REFUSED(emavfi_frame_diff_cells(ap + 1, 128, 1024, bp, 128, 1024, 1, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "2-byte");
    REFUSED(emavfi_frame_diff_cells(ap, 128, 1024, bp + 3, 128, 1024, 1, 8, 64, 1, 0, 2, 10, 6, up, nullptr), "2-byte");
    REFUSED(emavfi_frame_diff_cells(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, 0, 1, 8, 0, odd, nullptr), "4-byte");
    // an odd batch stride is unused, and not refused, at n = 1; an odd byte pointer is fine at sample_bytes 1: the next check is reached
    REFUSED(emavfi_frame_diff_cells(ap + 1, 128, 1025, bp, 128, 1027, 1, 8, 64, 1, 0, 2, 10, 0, up, nullptr), "2-byte");
    REFUSED(emavfi_frame_diff_cells(ap + 1, 64, 513, bp + 3, 64, 515, 1, 8, 64, 1, 0, 1, 8, 0, odd, nullptr), "4-byte");
    // the largest shapes and strides: the guards' size arithmetic must not overflow silently
    REFUSED(emavfi_frame_diff_cells(ap, SIZE_MAX, SIZE_MAX, bp, 192, 1536, 2, MAXD, MAXD, 1, 0, 1, 8, 0, up, nullptr), "overflows");
    REFUSED(emavfi_frame_diff_cells(ap, (size_t)MAXD * 2, (size_t)MAXD * MAXD * 2, bp, (size_t)MAXD * 2, SIZE_MAX - 1, 65535, MAXD, MAXD, 1, 0, 2, 16, 0, up,
                                    nullptr), "overflows");
    REFUSED(emavfi_frame_diff_cells(ap, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3 - 1, bp, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3, 65535, MAXD, MAXD, 3,
                                    0, 1, 8, 0, up, nullptr), "a_batch_stride");
    REFUSED(emavfi_frame_diff_cells(nullptr, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3, bp, (size_t)MAXD * 3, (size_t)MAXD * MAXD * 3, 65535, MAXD, MAXD, 3,
                                    0, 1, 8, 0, up, nullptr), "null");

    // emavfi_duplicate_flags(cells, stride_words, n, threshold, flags, scores, stream)
    REFUSED(emavfi_duplicate_flags(up, 1024, 0, 0, uq, ur, nullptr), ">= 1");
    REFUSED(emavfi_duplicate_flags(up, 1024, -3, 0, uq, ur, nullptr), ">= 1");
    REFUSED(emavfi_duplicate_flags(up, 1023, 2, 0, uq, ur, nullptr), "stride");
    REFUSED(emavfi_duplicate_flags(up, 0, 1, 0, uq, ur, nullptr), "stride");
    REFUSED(emavfi_duplicate_flags(up, SIZE_MAX, 3, 0, uq, ur, nullptr), "overflows");
    REFUSED(emavfi_duplicate_flags(up, SIZE_MAX / 4, 2147483647, 0, uq, ur, nullptr), "overflows");
    REFUSED(emavfi_duplicate_flags(nullptr, 1024, 2, 0, uq, ur, nullptr), "null");
    REFUSED(emavfi_duplicate_flags(up, 1024, 2, 0, nullptr, ur, nullptr), "null");
    REFUSED(emavfi_duplicate_flags(odd, 1024, 2, 0, uq, ur, nullptr), "4-byte");
    REFUSED(emavfi_duplicate_flags(up, 1024, 2, 0, odd, nullptr, nullptr), "4-byte");
    REFUSED(emavfi_duplicate_flags(up, 1024, 2, 0, uq, odd, nullptr), "4-byte");
    REFUSED(emavfi_duplicate_flags(nullptr, 1024, 2, 4294967295u, nullptr, nullptr, nullptr), "null");     // NULL scores alone is no refusal

    // the per-element functions against closed forms
    for (unsigned a = 0; a < 65536u; a += 257u)
        for (unsigned b = 0; b < 65536u; b += 4099u) {
            CHECK(dedup_absdiff(a, b) == dedup_absdiff(b, a) && dedup_absdiff(a, b) + (a < b ? a : b) == (a < b ? b : a) && dedup_absdiff(a, a) == 0u);
            CHECK(dedup_sample(a, 1023u, 6) == a / 64u && dedup_sample(a, 1023u, 0) == a % 1024u && dedup_sample(a, 4095u, 4) == a / 16u);
            CHECK(dedup_sample(a, 65535u, 0) == a && dedup_sample(a & 255u, 255u, 0) == (a & 255u) && dedup_sample(a, 4095u, 2) == (a / 4u) % 4096u);
        }
    for (unsigned n = 1; n <= 262144u; n = n < 70u ? n + 1u : n * 2u - 3u) {
        CHECK(dedup_cell_measure(0ull, n) == 0u);
        CHECK(dedup_cell_measure(1ull, n) == (16u + n - 1u) / n && dedup_cell_measure(1ull, n) >= 1u);                  // one count anywhere is seen
        for (unsigned d = 1; d <= 65535u; d = d * 3u + 1u)
            CHECK(dedup_cell_measure((unsigned long long)d * n, n) == 16u * d);                                              // a constant difference d: exactly 16 d
        CHECK(dedup_cell_measure(65535ull * n, n) == 1048560u);
        CHECK(dedup_cell_measure(65535ull * n - 1ull, n) == 1048560u - 16u / n);                                             // ceil(16 d - 16 / n)
    }
    CHECK(dedup_cell_measure(65535ull * 65792ull, 65792u) == 1048560u);     // a 256 x 257 cell of 16-bit samples: the sum passes 2^32
    CHECK(dedup_cell_measure(65535ull * 262144ull, 262144u) == 1048560u);   // the largest cell, 512 x 512
    CHECK(dedup_cell_measure(17ull, 16u) == 17u && dedup_cell_measure(17ull, 17u) == 16u && dedup_cell_measure(17ull, 18u) == 16u);

    // the generated pair in a plain loop: checksums for the oracle; identical images score 0 in every cell
    const struct { int H, W, C, rgb, sb, depth, shift; } cases[] = {
        {45, 100, 3, 0, 1, 8, 0}, {45, 100, 3, 1, 1, 8, 0}, {5, 7, 1, 0, 1, 8, 0}, {70, 130, 1, 0, 1, 8, 0}, {33, 47, 1, 0, 2, 10, 0},
        {33, 47, 1, 0, 2, 10, 6}, {40, 56, 1, 0, 2, 12, 2}, {31, 33, 1, 0, 2, 16, 0}};
    for (const auto &c : cases) {
        std::vector<unsigned> got;
        cells_of(c.H, c.W, c.C, c.rgb, (1u << c.depth) - 1u, c.shift, c.sb == 1 ? 255u : 65535u, got);
        unsigned ck = 0, best = 0;
        for (int k = 0; k < DEDUP_CELLS; ++k) {
            CHECK(got[k] <= 16u * ((1u << c.depth) - 1u));
            ck += got[k] * (unsigned)(k + 1);
            best = got[k] > best ? got[k] : best;
        }
        printf("host_check_dedup: %d x %d x %d order %d sample_bytes %d depth %d shift %d: cells %u score %u\n", c.H, c.W, c.C, c.rgb, c.sb, c.depth,
               c.shift, ck, best);
    }
    if (g_fail) { fprintf(stderr, "host_check_dedup: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_dedup: ok\n");
    return 0;
}
