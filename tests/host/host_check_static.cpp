// Host-only exercise of the static-region entry for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_dedup.cpp and the
// others: every argument guard of emavfi_static_guard_frames (include/emavfi.h, "STATIC REGION DEFINITION") - no kernel is launched, every
// call here is refused on the host - and the per-element functions the kernel is made of (csrc/static_elem.h, the same text) against the
// definition's closed forms and in a plain loop over a generated frame pair; the checksums it prints are compared with the numpy oracle's by
// tests/test_static_cpu.py::test_static_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/static_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_static: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// the generated frames of the test, per flat sample index i: a, b (a with sparse differences of 1..3 counts) and d (unrelated)
static unsigned gen_a(unsigned i, unsigned elem_mask) { return ((i * 2654435761u) >> 9) & elem_mask; }
static unsigned gen_b(unsigned i, unsigned elem_mask)
{
    const unsigned a = gen_a(i, elem_mask);
    return (((i * 40503u + 12345u) >> 7) % 499u == 0u) ? (a + 1u + i % 3u) & elem_mask : a;
}
static unsigned gen_d(unsigned i, unsigned elem_mask) { return ((i * 2246822519u + 7u) >> 11) & elem_mask; }

// the definition through the per-element functions, on frames held as one unsigned per sample (static_planes with sample_bytes 1: offsets
// count samples); returns the number of core pixels
static unsigned guard_plain(int H, int W, int layout, int C, int depth, int shift, int r, unsigned tol, const std::vector<unsigned> &a,
                            const std::vector<unsigned> &b, std::vector<unsigned> &d)
{
    StaticPlane pl[3];
    size_t n_samples;
    const int np = static_planes(layout, C, H, W, 1, pl, &n_samples);
    CHECK(n_samples == a.size() && n_samples == b.size() && n_samples == d.size());
    const unsigned mask = (1u << depth) - 1u;
    std::vector<unsigned char> same((size_t)H * W, 1), core((size_t)H * W, 0);
    for (int q = 0; q < np; ++q)
        for (int i = 0; i < pl[q].rows; ++i)
            for (int s = 0; s < pl[q].samples; ++s) {
                const size_t at = pl[q].offset + (size_t)i * pl[q].samples + s;
                if (static_within(static_sample(a[at], mask, shift), static_sample(b[at], mask, shift), tol)) continue;
                const int px = s / pl[q].div;
                if (!pl[q].sub) same[(size_t)i * W + px] = 0;
                else
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx) same[(size_t)(2 * i + dy) * W + 2 * px + dx] = 0;
            }
    unsigned count = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool c = true;
            for (int yy = static_window_lo(y, r); yy <= static_window_hi(y, r, H); ++yy)
                for (int xx = static_window_lo(x, r); xx <= static_window_hi(x, r, W); ++xx) c = c && same[(size_t)yy * W + xx];
            core[(size_t)y * W + x] = c;
            count += c;
        }
    const auto at_core = [&](int y, int x) { return core[(size_t)y * W + x] != 0; };
    for (int q = 0; q < np; ++q)
        for (int i = 0; i < pl[q].rows; ++i)
            for (int s = 0; s < pl[q].samples; ++s) {
                const int px = s / pl[q].div;
                const bool rep = pl[q].sub ? static_chroma_core(at_core(2 * i, 2 * px), at_core(2 * i, 2 * px + 1), at_core(2 * i + 1, 2 * px),
                                                                at_core(2 * i + 1, 2 * px + 1))
                                           : at_core(i, px);
                const size_t at = pl[q].offset + (size_t)i * pl[q].samples + s;
                if (rep) d[at] = a[at];
            }
    return count;
}

int main()
{
    unsigned char *const dp = (unsigned char *)(uintptr_t)4096, *const sp = (unsigned char *)(uintptr_t)(1u << 30);   // never dereferenced
    unsigned *const cp = (unsigned *)(uintptr_t)8192, *const odd = (unsigned *)(uintptr_t)8194;
    const emavfi_static_entry tab[3] = {{0, 1}, {1, 2}, {2, 2}};
    const int IL = EMAVFI_LAYOUT_INTERLEAVED, NV = EMAVFI_LAYOUT_NV12, I4 = EMAVFI_LAYOUT_I420;
    const int MAXD = 16384;
    static_assert(EMAVFI_STATIC_MAX_RADIUS == STATIC_MAX_RADIUS && EMAVFI_RESAMPLE_LAUNCH_CAP == STATIC_CAP, "header and static_elem.h disagree");
    static_assert(EMAVFI_LAYOUT_INTERLEAVED == STATIC_LAYOUT_INTERLEAVED && EMAVFI_LAYOUT_NV12 == STATIC_LAYOUT_NV12 &&
                  EMAVFI_LAYOUT_I420 == STATIC_LAYOUT_I420, "header and static_elem.h disagree");

    // emavfi_static_guard_frames(dst, dst_stride, n_dst, srcs, src_stride, n_srcs, table, H, W, layout, C, sample_bytes, depth, shift, radius, tol,
    //                            counts, stream); an 8 x 16 x 3 byte frame has 384 bytes, an 8 x 16 4:2:0 frame 192 (words: 384)
    REFUSED(emavfi_static_guard_frames(dp, 384, 0, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "n_dst");
    REFUSED(emavfi_static_guard_frames(dp, 384, -1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "n_dst");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 0, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "n_srcs");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 0, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), ">= 1");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, -16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), ">= 1");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, MAXD + 1, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "16384");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 2147483647, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "16384");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, 3, 3, 1, 8, 0, 2, 0, cp, nullptr), "layout");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, -1, 3, 1, 8, 0, 2, 0, cp, nullptr), "layout");
    REFUSED(emavfi_static_guard_frames(dp, 192, 3, sp, 192, 3, tab, 7, 16, NV, 1, 1, 8, 0, 2, 0, cp, nullptr), "even");
    REFUSED(emavfi_static_guard_frames(dp, 192, 3, sp, 192, 3, tab, 8, 15, I4, 1, 1, 8, 0, 2, 0, cp, nullptr), "even");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 0, 1, 8, 0, 2, 0, cp, nullptr), "C = 0");
    REFUSED(emavfi_static_guard_frames(dp, 1024, 3, sp, 1024, 3, tab, 8, 16, IL, 5, 1, 8, 0, 2, 0, cp, nullptr), "C = 5");
    REFUSED(emavfi_static_guard_frames(dp, 192, 3, sp, 192, 3, tab, 8, 16, NV, 3, 1, 8, 0, 2, 0, cp, nullptr), "C = 3 at a 4:2:0");
    REFUSED(emavfi_static_guard_frames(dp, 192, 3, sp, 192, 3, tab, 8, 16, I4, 2, 1, 8, 0, 2, 0, cp, nullptr), "C = 2 at a 4:2:0");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 0, 8, 0, 2, 0, cp, nullptr), "sample_bytes");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 4, 8, 0, 2, 0, cp, nullptr), "sample_bytes");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 10, 0, 2, 0, cp, nullptr), "depth");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 8, 0, 2, 0, cp, nullptr), "depth");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 14, 0, 2, 0, cp, nullptr), "depth");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 1, 2, 0, cp, nullptr), "shift");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 10, 7, 2, 0, cp, nullptr), "shift");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 16, 1, 2, 0, cp, nullptr), "shift");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, I4, 1, 2, 12, -1, 2, 0, cp, nullptr), "shift");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, -1, 0, cp, nullptr), "radius");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 17, 0, cp, nullptr), "radius");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 256, cp, nullptr), "tol");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 10, 6, 2, 1024, cp, nullptr), "tol");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 16, 0, 2, 65536, cp, nullptr), "tol");
    REFUSED(emavfi_static_guard_frames(dp, 383, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "dst_stride");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 383, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "src_stride");
    REFUSED(emavfi_static_guard_frames(dp, 192, 3, sp, 191, 3, tab, 8, 16, NV, 1, 1, 8, 0, 2, 0, cp, nullptr), "src_stride");
    REFUSED(emavfi_static_guard_frames(dp, 383, 3, sp, 384, 3, tab, 8, 16, I4, 1, 2, 10, 0, 2, 0, cp, nullptr), "dst_stride");
    REFUSED(emavfi_static_guard_frames(dp, 385, 3, sp, 384, 3, tab, 8, 16, I4, 1, 2, 10, 0, 2, 0, cp, nullptr), "odd");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 387, 3, tab, 8, 16, NV, 1, 2, 10, 6, 2, 0, cp, nullptr), "odd");
    REFUSED(emavfi_static_guard_frames(nullptr, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "null pointer dst");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, nullptr, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "null pointer srcs");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, nullptr, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "null pointer table");
    REFUSED(emavfi_static_guard_frames(dp + 1, 384, 3, sp, 384, 3, tab, 8, 16, NV, 1, 2, 10, 6, 2, 0, cp, nullptr), "2-byte");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp + 3, 384, 3, tab, 8, 16, I4, 1, 2, 16, 0, 2, 0, cp, nullptr), "2-byte");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, odd, nullptr), "4-byte");
    // an odd byte pointer is fine at sample_bytes 1: the next check is reached
    REFUSED(emavfi_static_guard_frames(dp + 1, 384, 3, sp + 3, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, odd, nullptr), "4-byte");
    // size arithmetic
    REFUSED(emavfi_static_guard_frames(dp, SIZE_MAX, 3, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "overflows");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, SIZE_MAX / 2, 4, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "overflows");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, (unsigned char *)(uintptr_t)(SIZE_MAX - 4096), 2048, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr),
            "overflows");
    REFUSED(emavfi_static_guard_frames(dp, (size_t)MAXD * MAXD * 8 - 2, 3, sp, (size_t)MAXD * MAXD * 8, 3, tab, MAXD, MAXD, IL, 4, 2, 16, 0, 16, 65535, cp,
                                       nullptr), "dst_stride");
    // overlap: dst inside srcs, srcs inside dst, the last byte
    REFUSED(emavfi_static_guard_frames(sp + 384, 384, 1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "overlaps");
    REFUSED(emavfi_static_guard_frames(sp - 384, 384, 1, sp, 384, 1, tab + 2, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "table[0].a");   // adjacent is no overlap: the next check is reached
    REFUSED(emavfi_static_guard_frames(sp - 383, 384, 1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "overlaps");
    REFUSED(emavfi_static_guard_frames(sp + 3 * 384 - 1, 384, 1, sp, 384, 3, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "overlaps");
    // entry indices
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 2, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "table[1].b");
    REFUSED(emavfi_static_guard_frames(dp, 384, 3, sp, 384, 1, tab, 8, 16, IL, 3, 1, 8, 0, 2, 0, nullptr, nullptr), "table[0].b");
    {
        const emavfi_static_entry big[1] = {{4294967295u, 0}};
        REFUSED(emavfi_static_guard_frames(dp, 384, 1, sp, 384, 3, big, 8, 16, IL, 3, 1, 8, 0, 2, 0, cp, nullptr), "table[0].a");
    }

    // the per-element functions against the definition's closed forms
    for (unsigned a = 0; a < 65536u; a += 257u)
        for (unsigned b = 0; b < 65536u; b += 4099u) {
            const unsigned diff = a > b ? a - b : b - a;
            CHECK(static_within(a, b, diff) && static_within(b, a, diff) && (diff == 0u || !static_within(a, b, diff - 1u)) && static_within(a, a, 0u));
            CHECK(static_within(a, b, 65535u));
            CHECK(static_sample(a, 1023u, 6) == a / 64u && static_sample(a, 1023u, 0) == a % 1024u && static_sample(a, 4095u, 4) == a / 16u);
            CHECK(static_sample(a, 65535u, 0) == a && static_sample(a & 255u, 255u, 0) == (a & 255u));
        }
    for (int m = 0; m < 16; ++m)
        CHECK(static_chroma_core(m & 1, m & 2, m & 4, m & 8) == (m == 15));
    for (int n = 1; n <= 40; ++n)
        for (int r = 0; r <= STATIC_MAX_RADIUS; ++r)
            for (int p = 0; p < n; ++p) {
                const int lo = static_window_lo(p, r), hi = static_window_hi(p, r, n);
                CHECK(lo >= 0 && hi <= n - 1 && lo <= p && p <= hi && (lo == 0 || lo == p - r) && (hi == n - 1 || hi == p + r));
                CHECK(r > 0 || (lo == p && hi == p));
            }
    CHECK(static_window_lo(16383, 16) == 16367 && static_window_hi(16383, 16, 16384) == 16383 && static_window_hi(0, 16, 1) == 0);
    {
        StaticPlane pl[3];
        size_t fb;
        CHECK(static_planes(STATIC_LAYOUT_INTERLEAVED, 3, 8, 16, 1, pl, &fb) == 1 && fb == 384 && pl[0].samples == 48 && pl[0].div == 3 && !pl[0].sub);
        CHECK(static_planes(STATIC_LAYOUT_NV12, 1, 8, 16, 2, pl, &fb) == 2 && fb == 384 && pl[1].offset == 256 && pl[1].rows == 4 &&
              pl[1].samples == 16 && pl[1].div == 2 && pl[1].sub == 1);
        CHECK(static_planes(STATIC_LAYOUT_I420, 1, 8, 16, 1, pl, &fb) == 3 && fb == 192 && pl[1].offset == 128 && pl[2].offset == 160 &&
              pl[2].rows == 4 && pl[2].samples == 8 && pl[2].div == 1 && pl[2].sub == 1);
        CHECK(static_planes(STATIC_LAYOUT_INTERLEAVED, 4, 16384, 16384, 2, pl, &fb) == 1 && fb == ((size_t)1 << 31));
    }
    // closed forms of the whole definition in the plain loop: equal frames copy a; one differing sample leaves a clipped (2 r + 1)^2 hole
    for (int layout = 0; layout < 3; ++layout)
        for (int r = 0; r <= 5; r += 1 + (r > 1)) {
            const int H = 12, W = 14, C = layout ? 1 : 3;
            StaticPlane pl[3];
            size_t ns;
            static_planes(layout, C, H, W, 1, pl, &ns);
            std::vector<unsigned> a(ns), d(ns);
            for (size_t i = 0; i < ns; ++i) { a[i] = gen_a((unsigned)i, 255u); d[i] = gen_d((unsigned)i, 255u); }
            std::vector<unsigned> b = a, g = d;
            CHECK(guard_plain(H, W, layout, C, 8, 0, r, 0, a, b, g) == (unsigned)(H * W) && g == a);
            const int py[3] = {0, 5, H - 1}, px[3] = {0, 6, W - 1};
            for (int k = 0; k < 3; ++k) {
                b = a;
                b[(size_t)py[k] * pl[0].samples + (size_t)px[k] * pl[0].div] ^= 1u;      // one luma (or first-channel) sample
                g = d;
                const int hole = (static_window_hi(py[k], r, H) - static_window_lo(py[k], r) + 1) * (static_window_hi(px[k], r, W) - static_window_lo(px[k], r) + 1);
                CHECK(guard_plain(H, W, layout, C, 8, 0, r, 0, a, b, g) == (unsigned)(H * W - hole));
                CHECK(guard_plain(H, W, layout, C, 8, 0, r, 1, a, b, g) == (unsigned)(H * W));     // within a tolerance of 1
            }
        }

    // the generated pair in a plain loop: checksums for the oracle
    const struct { int H, W, layout, C, sb, depth, shift, r; unsigned tol; } cases[] = {
        {45, 100, 0, 3, 1, 8, 0, 2, 0},  {45, 100, 0, 3, 1, 8, 0, 0, 1},  {5, 7, 0, 1, 1, 8, 0, 1, 0},      {33, 47, 0, 4, 2, 10, 0, 3, 0},
        {70, 130, 1, 1, 1, 8, 0, 3, 0},  {70, 130, 1, 1, 2, 10, 6, 1, 2}, {40, 56, 2, 1, 1, 8, 0, 16, 0},   {40, 56, 2, 1, 2, 12, 0, 2, 1},
        {34, 66, 2, 1, 2, 16, 0, 1, 0},  {2, 2, 1, 1, 1, 8, 0, 16, 0},    {66, 130, 0, 2, 2, 12, 2, 4, 3}};
    for (const auto &c : cases) {
        const unsigned em = c.sb == 1 ? 255u : 65535u;
        StaticPlane pl[3];
        size_t ns;
        static_planes(c.layout, c.C, c.H, c.W, 1, pl, &ns);
        std::vector<unsigned> a(ns), b(ns), d(ns);
        for (size_t i = 0; i < ns; ++i) { a[i] = gen_a((unsigned)i, em); b[i] = gen_b((unsigned)i, em); d[i] = gen_d((unsigned)i, em); }
        const unsigned count = guard_plain(c.H, c.W, c.layout, c.C, c.depth, c.shift, c.r, c.tol, a, b, d);
        unsigned ck = 0;
        for (size_t i = 0; i < ns; ++i) ck += d[i] * (unsigned)(i + 1);
        printf("host_check_static: %d x %d layout %d C %d sample_bytes %d depth %d shift %d radius %d tol %u: count %u checksum %u\n", c.H, c.W,
               c.layout, c.C, c.sb, c.depth, c.shift, c.r, c.tol, count, ck);
    }
    if (g_fail) { fprintf(stderr, "host_check_static: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_static: ok\n");
    return 0;
}
