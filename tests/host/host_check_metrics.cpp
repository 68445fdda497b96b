// Host-only exercise of the frame-metric entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_scene.cpp: every
// argument guard of emavfi_frame_metrics_workspace_bytes / emavfi_frame_metrics_u8 (include/emavfi.h, "FRAME METRIC DEFINITION") - no kernel
// is launched, every call here is refused on the host - and the per-element functions the kernel is made of (csrc/metrics_elem.h, the same
// text) in a plain loop over a generated image pair: the sums it prints are compared with the numpy oracle's by
// tests/test_metrics_cpu.py::test_metrics_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.  Built with -ffp-contract=off.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/metrics_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_metrics: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// the generated pair of the test: byte c of pixel (y, x) of image a, and of image b
static unsigned gen_a(int y, int x, int c) { return (unsigned)(y * 131 + x * 31 + c * 17 + (y * x) % 7) & 255u; }
static unsigned gen_b(int y, int x, int c) { return (gen_a(y, x, c) + (unsigned)((y * 5 + x * 3 + c) % 11)) & 255u; }

int main()
{
    unsigned char *const ap = (unsigned char *)(uintptr_t)256, *const bp = (unsigned char *)(uintptr_t)4096;   // never dereferenced
    long long *const out = (long long *)(uintptr_t)8192;
    void *const ws = (void *)(uintptr_t)16384;
    const int MAXD = 16384;
    const size_t WS = (size_t)1 << 40;
    static_assert(EMAVFI_METRICS_WINDOW == METRICS_WIN && METRICS_HALO == METRICS_WIN - 1, "header and metrics_elem.h disagree");

    // emavfi_frame_metrics_u8(a, a_pitch, a_batch_stride, b, b_pitch, b_batch_stride, B, H, W, C, out, workspace, workspace_bytes, stream)
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 0, 8, 64, 3, out, ws, WS, nullptr), ">= 1");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 2147483647, 8, 64, 3, out, ws, WS, nullptr), "65535");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 0, 64, 3, out, ws, WS, nullptr), ">= 1");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, -64, 3, out, ws, WS, nullptr), ">= 1");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, MAXD + 1, 64, 3, out, ws, WS, nullptr), "16384");
    REFUSED(emavfi_frame_metrics_u8(ap, 1 << 20, 1 << 30, bp, 1 << 20, 1 << 30, 1, 8, 2147483647, 3, out, ws, WS, nullptr), "16384");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 0, out, ws, WS, nullptr), "1..4");
    REFUSED(emavfi_frame_metrics_u8(ap, 512, 4096, bp, 512, 4096, 1, 8, 64, 5, out, ws, WS, nullptr), "1..4");
    REFUSED(emavfi_frame_metrics_u8(ap, 191, 1536, bp, 192, 1536, 1, 8, 64, 3, out, ws, WS, nullptr), "pitch of a");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 63, 1536, 1, 8, 64, 1, out, ws, WS, nullptr), "pitch of b");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1535, bp, 192, 1536, 2, 8, 64, 3, out, ws, WS, nullptr), "batch stride of a");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 0, 2, 8, 64, 3, out, ws, WS, nullptr), "batch stride of b");
    REFUSED(emavfi_frame_metrics_u8(nullptr, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, out, ws, WS, nullptr), "null");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, nullptr, 192, 1536, 1, 8, 64, 3, out, ws, WS, nullptr), "null");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, nullptr, ws, WS, nullptr), "null");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, out, nullptr, WS, nullptr), "null");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, (long long *)(uintptr_t)8196, ws, WS, nullptr), "8-byte");
    REFUSED(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, out, (void *)(uintptr_t)16385, WS, nullptr), "8-byte");
    // the largest shapes and strides: the guards' size arithmetic must not overflow silently
    REFUSED(emavfi_frame_metrics_u8(ap, SIZE_MAX, SIZE_MAX, bp, 192, 1536, 2, MAXD, 64, 3, out, ws, WS, nullptr), "overflows");
    REFUSED(emavfi_frame_metrics_u8(ap, (size_t)MAXD * 4, (size_t)MAXD * MAXD * 4, bp, (size_t)MAXD * 4, SIZE_MAX, 65535, MAXD, MAXD, 4, out, ws, WS, nullptr),
            "overflows");
    // a workspace that is too small is its own code; one tile of 32 x 32 windows per (b, c) and 16 bytes per tile
    CHECK(emavfi_frame_metrics_workspace_bytes(1, 8, 64, 3) == 3u * 2u * 16u);
    CHECK(emavfi_frame_metrics_workspace_bytes(2, 720, 1280, 3) == 2u * 3u * 23u * 40u * 16u);
    CHECK(emavfi_frame_metrics_workspace_bytes(1, 10, 10, 1) == 16u && emavfi_frame_metrics_workspace_bytes(1, 42, 43, 1) == 32u);
    CHECK(emavfi_frame_metrics_workspace_bytes(65535, MAXD, MAXD, 4) == (size_t)65535 * 4 * 512 * 512 * 16);
    CHECK(emavfi_frame_metrics_workspace_bytes(0, 8, 8, 1) == 0 && emavfi_frame_metrics_workspace_bytes(1, 8, 8, 5) == 0);
    CHECK(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, out, ws, 95, nullptr) == EMAVFI_E_WORKSPACE);
    CHECK(emavfi_frame_metrics_u8(ap, 192, 1536, bp, 192, 1536, 1, 8, 64, 3, out, ws, 0, nullptr) == EMAVFI_E_WORKSPACE);

    // the weight table
    unsigned gsum = 0;
    for (int j = 0; j < METRICS_WIN; ++j) {
        gsum += metrics_weight(j);
        CHECK(metrics_weight(j) == metrics_weight(METRICS_WIN - 1 - j));
    }
    CHECK(gsum == 65536u && metrics_weight(5) == 17434u);
    CHECK(metrics_sqdiff(0, 255) == 65025u && metrics_sqdiff(255, 0) == 65025u && metrics_sqdiff(7, 7) == 0u);

    // the per-element functions in a plain loop: row pass of every row, column pass and tail of every window, squared difference of every pixel
    const int shapes[][3] = {{45, 100, 3}, {11, 11, 1}, {10, 40, 1}, {23, 37, 4}};
    for (const auto &sh : shapes) {
        const int H = sh[0], W = sh[1], C = sh[2];
        std::vector<unsigned char> a((size_t)H * W * C), b((size_t)H * W * C);   // exact size: ASan sees any read past the image
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < C; ++c) {
                    a[((size_t)y * W + x) * C + c] = (unsigned char)gen_a(y, x, c);
                    b[((size_t)y * W + x) * C + c] = (unsigned char)gen_b(y, x, c);
                }
        const int nwx = W > METRICS_HALO ? W - METRICS_HALO : 0, nwy = H > METRICS_HALO ? H - METRICS_HALO : 0;
        for (int c = 0; c < C; ++c) {
            unsigned long long sse = 0;
            long long ssimq = 0;
            for (size_t i = c; i < a.size(); i += C) sse += metrics_sqdiff(a[i], b[i]);
            std::vector<unsigned> rows((size_t)5 * H * (nwx ? nwx : 1));
            for (int y = 0; y < H && nwx; ++y)
                for (int x = 0; x < nwx; ++x) {
                    unsigned m[5];
                    metrics_row5(&a[((size_t)y * W + x) * C + c], &b[((size_t)y * W + x) * C + c], C, m);
                    for (int k = 0; k < 5; ++k) {
                        CHECK(m[k] <= 65025ull * 65536ull);
                        rows[((size_t)k * H + y) * nwx + x] = m[k];
                    }
                }
            for (int y = 0; y < nwy; ++y)
                for (int x = 0; x < nwx; ++x) {
                    unsigned long long acc[5] = {0, 0, 0, 0, 0};
                    for (int j = 0; j < METRICS_WIN; ++j)
                        for (int k = 0; k < 5; ++k) acc[k] = metrics_col_tap(acc[k], j, rows[((size_t)k * H + y + j) * nwx + x]);
                    for (int k = 0; k < 5; ++k) CHECK(acc[k] <= 65025ull << 32);
                    ssimq += metrics_tail(acc[0], acc[1], acc[2], acc[3], acc[4]);
                }
            printf("host_check_metrics: %d x %d x %d channel %d: sse %llu ssimq %lld\n", H, W, C, c, sse, ssimq);
        }
    }
    // the extremes of the tail: identical windows give exactly 2^32, black against white the stated constant
    CHECK(metrics_tail(255ull << 32, 255ull << 32, 65025ull << 32, 65025ull << 32, 65025ull << 32) == 4294967296ll);
    CHECK(metrics_tail(0, 0, 0, 0, 0) == 4294967296ll);
    CHECK(metrics_tail(0, 255ull << 32, 0, 65025ull << 32, 0) == (long long)__builtin_floor(6.5025 / (65025.0 + 6.5025) * 4294967296.0));
    if (g_fail) { fprintf(stderr, "host_check_metrics: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_metrics: ok\n");
    return 0;
}
