// Host-only exercise of the active-area entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_static.cpp and the
// others: every argument guard of emavfi_active_bounds, emavfi_fill_outside_frames, emavfi_preprocess_u8_pitched and
// emavfi_postprocess_u8_pitched (include/emavfi.h, "ACTIVE AREA DEFINITION") - no kernel is launched, every call here is refused on the host -
// and the per-element functions the kernels are made of (csrc/active_elem.h, the same text) against literal expectations.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/active_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_active: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), "" word))

static bool same(const ActiveBounds &b, unsigned t, unsigned bo, unsigned l, unsigned r) { return b.top == t && b.bottom == bo && b.left == l && b.right == r; }

// the bounds of an image [H][W][C] of one unsigned per element, through the per-element functions in a plain loop
static ActiveBounds bounds_plain(const std::vector<unsigned> &img, int H, int W, int C, int depth, int shift, unsigned level)
{
    ActiveBounds b = active_none(H, W);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < C; ++c)
                if (active_content(active_sample(img[((size_t)y * W + x) * C + c], (1u << depth) - 1u, shift), level)) active_mark(b, y, x);
    return b;
}

int main()
{
    static_assert(EMAVFI_RESAMPLE_LAUNCH_CAP == ACTIVE_CAP, "header and active_elem.h disagree");
    // ---- the per-element functions
    CHECK(active_sample(0xABu, 255u, 0) == 0xABu && active_sample(0xFFC0u, 1023u, 6) == 1023u && active_sample(0xFC00u | 17u, 1023u, 0) == 17u);
    CHECK(!active_content(16u, 16u) && active_content(17u, 16u) && !active_content(0u, 0u) && active_content(1u, 0u));
    CHECK(same(active_none(5, 7), 5, 0, 7, 0) && active_is_empty(active_none(5, 7)));
    {
        ActiveBounds b = active_none(48, 96);
        active_mark(b, 10, 20);
        CHECK(same(b, 10, 11, 20, 21) && !active_is_empty(b));
        active_mark(b, 0, 95);
        active_mark(b, 47, 0);
        CHECK(same(b, 0, 48, 0, 96));
        ActiveBounds u = active_none(48, 96), e = active_none(48, 96);
        active_join(u, e);
        CHECK(active_is_empty(u) && same(active_rect(u, 48, 96), 0, 48, 0, 96));          // an empty union is the whole frame
        active_join(u, ActiveBounds{9, 39, 17, 79});
        active_join(u, e);
        CHECK(same(u, 9, 39, 17, 79) && same(active_rect(u, 48, 96), 8, 40, 16, 80));     // grown outward to 2 and 16
        CHECK(same(active_rect(ActiveBounds{8, 40, 16, 80}, 48, 96), 8, 40, 16, 80));     // aligned bounds stay
        CHECK(same(active_rect(ActiveBounds{1, 47, 3, 99}, 47, 100), 0, 47, 0, 100));     // clipped to an odd H and a W off the lattice
        CHECK(same(active_rect(ActiveBounds{2, 3, 90, 91}, 48, 100), 2, 4, 80, 96));
    }
    {
        // an image by hand: 5 x 7, one channel; (1, 2) = level + 1, (3, 5) = level, everything else 0
        std::vector<unsigned> img(35, 0u);
        img[1 * 7 + 2] = 17u;
        img[3 * 7 + 5] = 16u;
        CHECK(same(bounds_plain(img, 5, 7, 1, 8, 0, 16u), 1, 2, 2, 3));
        CHECK(same(bounds_plain(img, 5, 7, 1, 8, 0, 15u), 1, 4, 2, 6));
        CHECK(same(bounds_plain(img, 5, 7, 1, 8, 0, 17u), 5, 0, 7, 0));
        // three channels: only channel 2 of pixel (2, 1) is above the level
        std::vector<unsigned> bgr(4 * 3 * 3, 3u);
        bgr[(2 * 3 + 1) * 3 + 2] = 200u;
        CHECK(same(bounds_plain(bgr, 4, 3, 3, 8, 0, 3u), 2, 3, 1, 2));
        // words: junk in the ignored bits is not content
        std::vector<unsigned> w16(2 * 4, 0xFC00u);
        CHECK(same(bounds_plain(w16, 2, 4, 1, 10, 0, 0u), 2, 0, 4, 0));
        w16[5] = 0xFC00u | 65u;
        CHECK(same(bounds_plain(w16, 2, 4, 1, 10, 0, 64u), 1, 2, 1, 2) && same(bounds_plain(w16, 2, 4, 1, 10, 0, 65u), 2, 0, 4, 0));
        std::vector<unsigned> p010(2 * 4, 0x003Fu);                                      // P010: the sample in the top 10 bits, junk below
        CHECK(same(bounds_plain(p010, 2, 4, 1, 10, 6, 0u), 2, 0, 4, 0));
        p010[2] = (65u << 6) | 0x3Fu;
        CHECK(same(bounds_plain(p010, 2, 4, 1, 10, 6, 64u), 0, 1, 2, 3));
    }
    {
        // the span of a rectangle in every plane of a 32 x 48 frame: (8, 16, 16, 32)
        StaticPlane pl[3];
        size_t fb;
        CHECK(static_planes(STATIC_LAYOUT_INTERLEAVED, 3, 32, 48, 1, pl, &fb) == 1);
        ActiveSpan s = active_plane_span(pl[0], 1, 8, 16, 16, 32);
        CHECK(s.r0 == 8 && s.r1 == 24 && s.c0 == 48 && s.c1 == 144);
        CHECK(active_inside(s, 8, 48) && !active_inside(s, 7, 48) && !active_inside(s, 8, 47) && active_inside(s, 23, 143) && !active_inside(s, 24, 143)
              && !active_inside(s, 23, 144));
        CHECK(static_planes(STATIC_LAYOUT_NV12, 1, 32, 48, 2, pl, &fb) == 2 && fb == 32u * 48u * 3u);
        s = active_plane_span(pl[0], 2, 8, 16, 16, 32);
        CHECK(s.r0 == 8 && s.r1 == 24 && s.c0 == 32 && s.c1 == 96);
        s = active_plane_span(pl[1], 2, 8, 16, 16, 32);                                  // pairs {U, V} of words: 4 bytes per chroma position
        CHECK(s.r0 == 4 && s.r1 == 12 && s.c0 == 32 && s.c1 == 96);
        CHECK(static_planes(STATIC_LAYOUT_I420, 1, 32, 48, 1, pl, &fb) == 3);
        for (int q = 1; q < 3; ++q) {
            s = active_plane_span(pl[q], 1, 8, 16, 16, 32);
            CHECK(s.r0 == 4 && s.r1 == 12 && s.c0 == 8 && s.c1 == 24);
        }
        s = active_plane_span(pl[0], 1, 0, 0, 32, 48);                                   // the whole frame: nothing lies outside
        CHECK(s.r0 == 0 && s.r1 == 32 && s.c0 == 0 && s.c1 == 48);
    }

    // ---- the entries' guards: fake pointers, never dereferenced
    unsigned char *const ip = (unsigned char *)(uintptr_t)4096, *const dp = (unsigned char *)(uintptr_t)(1u << 20),
                  *const sp = (unsigned char *)(uintptr_t)(1u << 30);
    unsigned *const bp = (unsigned *)(uintptr_t)8192, *const bodd = (unsigned *)(uintptr_t)8194;
    float *const fp = (float *)(uintptr_t)(1u << 24), *const fodd = (float *)(uintptr_t)((1u << 24) + 2);
    const unsigned tab[3] = {0, 1, 2}, far[3] = {0, 3, 1};
    const float mean[4] = {0.5f, 0.5f, 0.5f, 0.5f}, stdv[4] = {0.25f, 0.25f, 0.25f, 0.25f}, std0[4] = {0.25f, 0.0f, 0.25f, 0.25f};
    const double meand[4] = {0.5, 0.5, 0.5, 0.5}, stdd[4] = {0.25, 0.25, 0.25, 0.25};
    const int IL = EMAVFI_LAYOUT_INTERLEAVED, NV = EMAVFI_LAYOUT_NV12, I4 = EMAVFI_LAYOUT_I420;

    // emavfi_active_bounds(img, pitch, batch_stride, n, H, W, C, sample_bytes, depth, shift, level, bounds, stream)
    REFUSED(emavfi_active_bounds(ip, 48, 384, 0, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "n must be");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 65536, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "65535");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 0, 16, 3, 1, 8, 0, 0, bp, nullptr), ">= 1");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16385, 3, 1, 8, 0, 0, bp, nullptr), "16384");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 2, 1, 8, 0, 0, bp, nullptr), "C = 2");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 4, 1, 8, 0, 0, bp, nullptr), "C = 4");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 3, 8, 0, 0, bp, nullptr), "sample_bytes");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 1, 10, 0, 0, bp, nullptr), "depth");
    REFUSED(emavfi_active_bounds(ip, 32, 256, 2, 8, 16, 1, 2, 8, 0, 0, bp, nullptr), "depth");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 1, 8, 1, 0, bp, nullptr), "shift");
    REFUSED(emavfi_active_bounds(ip, 32, 256, 2, 8, 16, 1, 2, 10, 7, 0, bp, nullptr), "shift");
    REFUSED(emavfi_active_bounds(ip, 96, 768, 2, 8, 16, 3, 2, 10, 0, 0, bp, nullptr), "C = 3 at sample_bytes 2");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 1, 8, 0, 256, bp, nullptr), "level");
    REFUSED(emavfi_active_bounds(ip, 32, 256, 2, 8, 16, 1, 2, 10, 6, 1024, bp, nullptr), "level");
    REFUSED(emavfi_active_bounds(ip, 47, 384, 2, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "pitch 47");
    REFUSED(emavfi_active_bounds(ip, 33, 264, 2, 8, 16, 1, 2, 10, 0, 0, bp, nullptr), "pitch 33 is odd");
    REFUSED(emavfi_active_bounds(ip, 48, 383, 2, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "batch_stride 383");
    REFUSED(emavfi_active_bounds(ip, 32, 257, 2, 8, 16, 1, 2, 10, 0, 0, bp, nullptr), "batch_stride 257 is odd");
    REFUSED(emavfi_active_bounds(ip, (size_t)-1, 384, 2, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "overflows");
    REFUSED(emavfi_active_bounds(ip, 48, (size_t)-1, 3, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "overflows");
    REFUSED(emavfi_active_bounds(nullptr, 48, 384, 2, 8, 16, 3, 1, 8, 0, 0, bp, nullptr), "null pointer img");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 1, 8, 0, 0, nullptr, nullptr), "null pointer bounds");
    REFUSED(emavfi_active_bounds(ip + 1, 32, 256, 2, 8, 16, 1, 2, 10, 0, 0, bp, nullptr), "2-byte");
    REFUSED(emavfi_active_bounds(ip, 48, 384, 2, 8, 16, 3, 1, 8, 0, 0, bodd, nullptr), "4-byte");
    REFUSED(emavfi_active_bounds(ip, 48, 0, 1, 8, 16, 3, 1, 8, 0, 255, nullptr, nullptr), "null pointer bounds");   // n = 1: the stride is not looked at

    // emavfi_fill_outside_frames(dst, dst_stride, n_dst, srcs, src_stride, n_srcs, table, H, W, layout, C, sample_bytes, top, left, height, width,
    //                            stream); an 8 x 16 x 3 byte frame has 384 bytes, an 8 x 16 4:2:0 frame 192 (words: 384)
    REFUSED(emavfi_fill_outside_frames(dp, 384, 0, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "n_dst");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 0, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "n_srcs");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 0, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), ">= 1");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16385, IL, 3, 1, 2, 0, 4, 16, nullptr), "16384");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, 3, 3, 1, 2, 0, 4, 16, nullptr), "layout");
    REFUSED(emavfi_fill_outside_frames(dp, 192, 3, sp, 192, 3, tab, 7, 16, NV, 1, 1, 2, 0, 4, 16, nullptr), "even");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 0, 1, 2, 0, 4, 16, nullptr), "C = 0");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 5, 1, 2, 0, 4, 16, nullptr), "C = 5");
    REFUSED(emavfi_fill_outside_frames(dp, 192, 3, sp, 192, 3, tab, 8, 16, I4, 3, 1, 2, 0, 4, 16, nullptr), "C = 3 at a 4:2:0");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 3, 2, 0, 4, 16, nullptr), "sample_bytes");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 0, 16, nullptr), "no area");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, -1, nullptr), "no area");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, -1, 0, 4, 16, nullptr), "leaves");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 5, 0, 4, 16, nullptr), "leaves");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 1, 4, 16, nullptr), "leaves");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2147483647, 0, 4, 16, nullptr), "leaves");
    REFUSED(emavfi_fill_outside_frames(dp, 192, 3, sp, 192, 3, tab, 8, 16, NV, 1, 1, 1, 0, 4, 16, nullptr), "odd at a 4:2:0");
    REFUSED(emavfi_fill_outside_frames(dp, 192, 3, sp, 192, 3, tab, 8, 16, I4, 1, 1, 2, 0, 4, 15, nullptr), "odd at a 4:2:0");
    REFUSED(emavfi_fill_outside_frames(dp, 383, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "dst_stride");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 191, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "src_stride");
    REFUSED(emavfi_fill_outside_frames(dp, 385, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 2, 0, 4, 16, nullptr), "dst_stride 385 is odd");
    REFUSED(emavfi_fill_outside_frames(dp, (size_t)-1, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "overflows");
    REFUSED(emavfi_fill_outside_frames(nullptr, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "null pointer dst");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, nullptr, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "null pointer srcs");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, nullptr, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "null pointer table");
    REFUSED(emavfi_fill_outside_frames(dp + 1, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 2, 0, 4, 16, nullptr), "2-byte");
    REFUSED(emavfi_fill_outside_frames(sp + 384, 384, 1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "dst overlaps srcs");
    REFUSED(emavfi_fill_outside_frames(sp - 383, 384, 1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "dst overlaps srcs");
    REFUSED(emavfi_fill_outside_frames(dp, 384, 3, sp, 384, 3, far, 8, 16, IL, 3, 1, 2, 0, 4, 16, nullptr), "table[1] = 3");
    REFUSED(emavfi_fill_outside_frames(sp - 384, 384, 1, sp, 384, 1, far + 1, 8, 16, IL, 3, 1, 0, 0, 8, 16, nullptr), "table[0] = 3");   // adjacent pools, the whole frame: the table is still read

    // emavfi_preprocess_u8_pitched(frames, pitch, batch_stride, out_nchw, B, H, W, C, mean, std, stream)
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 0, 8, 16, 3, mean, stdv, nullptr), "B must be");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 65536, 8, 16, 3, mean, stdv, nullptr), "65535");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 2, 8, 0, 3, mean, stdv, nullptr), ">= 1");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 2, 16385, 16, 3, mean, stdv, nullptr), "16384");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 2, 8, 16, 0, mean, stdv, nullptr), "C = 0");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 80, 640, fp, 2, 8, 16, 5, mean, stdv, nullptr), "C = 5");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 47, 384, fp, 2, 8, 16, 3, mean, stdv, nullptr), "pitch 47");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 383, fp, 2, 8, 16, 3, mean, stdv, nullptr), "batch_stride 383");
    REFUSED(emavfi_preprocess_u8_pitched(ip, (size_t)-1, 384, fp, 2, 8, 16, 3, mean, stdv, nullptr), "overflows");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 2, 8, 16, 3, nullptr, stdv, nullptr), "null mean / std");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fp, 2, 8, 16, 3, mean, std0, nullptr), "std[1]");
    REFUSED(emavfi_preprocess_u8_pitched(nullptr, 48, 384, fp, 2, 8, 16, 3, mean, stdv, nullptr), "null pointer frames");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, nullptr, 2, 8, 16, 3, mean, stdv, nullptr), "null pointer out_nchw");
    REFUSED(emavfi_preprocess_u8_pitched(ip, 48, 384, fodd, 2, 8, 16, 3, mean, stdv, nullptr), "4-byte");

    // emavfi_postprocess_u8_pitched(frames_nchw, out, pitch, batch_stride, B, H, W, C, mean, std, denormalize, stream)
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 48, 384, 0, 8, 16, 3, meand, stdd, 1, nullptr), "B must be");
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 48, 384, 2, 8, 16385, 3, meand, stdd, 1, nullptr), "16384");
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 48, 384, 2, 8, 16, 5, meand, stdd, 1, nullptr), "C = 5");
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 47, 384, 2, 8, 16, 3, meand, stdd, 1, nullptr), "pitch 47");
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 48, 383, 2, 8, 16, 3, meand, stdd, 1, nullptr), "batch_stride 383");
    REFUSED(emavfi_postprocess_u8_pitched(fp, dp, 48, 384, 2, 8, 16, 3, meand, nullptr, 1, nullptr), "null mean / std");
    REFUSED(emavfi_postprocess_u8_pitched(nullptr, dp, 48, 384, 2, 8, 16, 3, meand, stdd, 1, nullptr), "null pointer frames_nchw");
    REFUSED(emavfi_postprocess_u8_pitched(fp, nullptr, 48, 384, 2, 8, 16, 3, meand, stdd, 1, nullptr), "null pointer out");
    REFUSED(emavfi_postprocess_u8_pitched(fodd, dp, 48, 384, 2, 8, 16, 3, meand, stdd, 1, nullptr), "4-byte");

    if (g_fail) {
        fprintf(stderr, "host_check_active: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("host_check_active: ok\n");
    return 0;
}
