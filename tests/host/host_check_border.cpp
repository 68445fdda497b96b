// Host-only exercise of the two border entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_ensemble.cpp and its
// siblings: every argument guard of emavfi_border_pad_f32 and emavfi_border_crop_f32 (include/emavfi.h, "BORDER DEFINITION") - no kernel is
// launched, every call here is refused on the host - and the per-element functions the kernels are made of (csrc/border_elem.h, the same
// text) against closed forms and in a plain loop over a generated 2-plane 5 x 7 case, both modes and N = 1, 3, 9: the checksums it prints
// are compared with the numpy oracle's by tests/test_border_cpu.py::test_border_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/border_elem.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_border: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// element i of the generated tensor (tests/ensemble_oracle.py, generated(0, ...)): a signed 24-bit mantissa times 2^(e - 20), e in 0..7
static float gen(unsigned i)
{
    const unsigned h = (i * 2654435761u + 12345u) * 2246822519u;
    return std::ldexp((float)((int)(h >> 8) - (1 << 23)), (int)(h & 7u) - 20);
}
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

int main()
{
    static_assert(EMAVFI_BORDER_REPLICATE == BORDER_REPLICATE && EMAVFI_BORDER_REFLECT == BORDER_REFLECT && EMAVFI_BORDER_MAX == BORDER_MAX
                  && EMAVFI_RESIZE_MAX_DIM == BORDER_MAX_DIM, "header and border_elem.h disagree");
    float *const sp = (float *)(uintptr_t)(1u << 20), *const dp = (float *)(uintptr_t)(2u << 20);   // never dereferenced
    const size_t P = 3;
    const int H = 16, W = 32, N = 4;
    const size_t PIC = P * H * W * sizeof(float), PAD = P * (H + 2 * N) * (W + 2 * N) * sizeof(float);
    const size_t HUGE_PLANES = std::numeric_limits<size_t>::max() / 2;
    float *const top = (float *)(std::numeric_limits<uintptr_t>::max() - 1023);

    // emavfi_border_pad_f32(src, dst, planes, H, W, N, mode, stream): src is the picture, dst its extension
    REFUSED(emavfi_border_pad_f32(nullptr, dp, P, H, W, N, 0, nullptr), "src");
    REFUSED(emavfi_border_pad_f32(sp, nullptr, P, H, W, N, 0, nullptr), "dst");
    REFUSED(emavfi_border_pad_f32(sp, dp, 0, H, W, N, 0, nullptr), "planes");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, 0, W, N, 0, nullptr), "H, W");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, -1, N, 0, nullptr), "H, W");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, 16385, W, 0, 0, nullptr), "16384");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, 16385, 0, 0, nullptr), "16384");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, 16384, W, 1, 0, nullptr), "padded");       // the picture fits, its extension does not
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, 16384 - 7, 4, 1, nullptr), "padded");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, W, -1, 0, nullptr), "N =");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, W, 65, 0, nullptr), "N =");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, W, N, 2, nullptr), "mode");
    REFUSED(emavfi_border_pad_f32(sp, dp, P, H, W, N, -1, nullptr), "mode");
    REFUSED(emavfi_border_pad_f32((float *)((uintptr_t)sp + 2), dp, P, H, W, N, 1, nullptr), "4-byte");
    REFUSED(emavfi_border_pad_f32(sp, (float *)((uintptr_t)dp + 1), P, H, W, N, 1, nullptr), "4-byte");
    REFUSED(emavfi_border_pad_f32(sp, dp, HUGE_PLANES, 16384 - 128, 16384 - 128, 64, 0, nullptr), "overflows");
    REFUSED(emavfi_border_pad_f32(sp, dp, std::numeric_limits<size_t>::max() / (16 * 32 * 4), 16, 32, 64, 0, nullptr), "overflows");   // the picture's bytes fit, the extension's do not
    REFUSED(emavfi_border_pad_f32(sp, top, P, H, W, N, 0, nullptr), "overflows");
    REFUSED(emavfi_border_pad_f32(top, dp, P, H, W, N, 0, nullptr), "overflows");
    // dst (PAD bytes) against src (PIC bytes): its last word on src's first, its first on src's last, the same start
    REFUSED(emavfi_border_pad_f32(sp, (float *)((uintptr_t)sp - PAD + 4), P, H, W, N, 1, nullptr), "dst overlaps src");
    REFUSED(emavfi_border_pad_f32(sp, (float *)((uintptr_t)sp + PIC - 4), P, H, W, N, 1, nullptr), "dst overlaps src");
    REFUSED(emavfi_border_pad_f32(sp, sp, P, H, W, N, 0, nullptr), "dst overlaps src");
    REFUSED(emavfi_border_pad_f32(sp, sp, P, H, W, 0, 0, nullptr), "dst overlaps src");   // N = 0 is a copy, not an in-place no-op

    // emavfi_border_crop_f32(src, dst, planes, H, W, N, stream): src is the extension, dst the picture
    REFUSED(emavfi_border_crop_f32(nullptr, dp, P, H, W, N, nullptr), "src");
    REFUSED(emavfi_border_crop_f32(sp, nullptr, P, H, W, N, nullptr), "dst");
    REFUSED(emavfi_border_crop_f32(sp, dp, 0, H, W, N, nullptr), "planes");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, 0, W, N, nullptr), "H, W");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, H, 0, N, nullptr), "H, W");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, 20000, W, 0, nullptr), "16384");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, H, 16384, 64, nullptr), "padded");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, 16383, W, 1, nullptr), "padded");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, H, W, -1, nullptr), "N =");
    REFUSED(emavfi_border_crop_f32(sp, dp, P, H, W, 65, nullptr), "N =");
    REFUSED(emavfi_border_crop_f32((float *)((uintptr_t)sp + 3), dp, P, H, W, N, nullptr), "4-byte");
    REFUSED(emavfi_border_crop_f32(sp, (float *)((uintptr_t)dp + 2), P, H, W, N, nullptr), "4-byte");
    REFUSED(emavfi_border_crop_f32(sp, dp, HUGE_PLANES, 16384 - 128, 16384 - 128, 64, nullptr), "overflows");
    REFUSED(emavfi_border_crop_f32(sp, top, P, H, W, N, nullptr), "overflows");
    REFUSED(emavfi_border_crop_f32(sp, (float *)((uintptr_t)sp - PIC + 4), P, H, W, N, nullptr), "dst overlaps src");
    REFUSED(emavfi_border_crop_f32(sp, (float *)((uintptr_t)sp + PAD - 4), P, H, W, N, nullptr), "dst overlaps src");
    REFUSED(emavfi_border_crop_f32(sp, sp, P, H, W, N, nullptr), "dst overlaps src");

    // the index maps against closed forms
    {
        // reflect, n = 5: period 8, the edge sample not repeated
        const int want5[] = {1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1};   // i = -9 .. 17
        for (int i = -9; i <= 17; ++i) CHECK(border_reflect_index(i, 5) == want5[i + 9]);
        const int want2[] = {1, 0, 1, 0, 1, 0, 1};                                                               // n = 2, i = -3 .. 3
        for (int i = -3; i <= 3; ++i) CHECK(border_reflect_index(i, 2) == want2[i + 3]);
        for (int i = -64; i <= 64; ++i) CHECK(border_reflect_index(i, 1) == 0 && border_replicate_index(i, 1) == 0);
        for (const int n : {1, 2, 3, 5, 7, 16384})
            for (int i = -BORDER_MAX; i <= n - 1 + BORDER_MAX; i += (n > 100 && i >= 0 && i < n - 2 ? n - 2 : 1))
                for (int mode = 0; mode < 2; ++mode) {
                    const int j = border_index(i, n, mode);
                    CHECK(j >= 0 && j < n);
                    CHECK(border_index(n - 1 - i, n, mode) == n - 1 - j);            // symmetric under i -> n - 1 - i: padding commutes with a flip
                    if (i >= 0 && i < n) CHECK(j == i);
                    if (mode == BORDER_REPLICATE) CHECK(j == (i < 0 ? 0 : i >= n ? n - 1 : i));
                }
        CHECK(border_crop_index(0, 64) == 64 && border_crop_index(5, 0) == 5);
        CHECK(border_mode_ok(0) && border_mode_ok(1) && !border_mode_ok(2) && !border_mode_ok(-1));
        CHECK(border_n_ok(0) && border_n_ok(64) && !border_n_ok(65) && !border_n_ok(-1));
        CHECK(border_dim_ok(1) && border_dim_ok(16384) && !border_dim_ok(0) && !border_dim_ok(16385));
        int sx0;
        CHECK(border_unit_inside(4, 16, 4, false, &sx0) && sx0 == 0 && !border_unit_inside(0, 16, 4, false, &sx0) && sx0 == -4);
        CHECK(border_unit_inside(20, 18, 4, false, &sx0) == false && sx0 == 16);     // columns 16..19 of 18: straddles the edge
        CHECK(border_unit_inside(0, 24, 4, true, &sx0) && sx0 == 4 && border_unit_inside(12, 24, 4, true, &sx0) && sx0 == 16);
    }

    // the per-element functions in a plain loop: 2 planes of 5 x 7 into exactly-sized buffers, and back
    {
        const int gp = 2, gh = 5, gw = 7, ne = gp * gh * gw;
        std::vector<float> pic(ne);
        for (int i = 0; i < ne; ++i) pic[i] = gen((unsigned)i);
        pic[0] = -0.0f; pic[3] = std::numeric_limits<float>::infinity();             // moved, not computed with: the bits survive
        unsigned nanbits = 0x7FC12345u;
        memcpy(&pic[ne - 1], &nanbits, 4);
        for (int mode = 0; mode < 2; ++mode)
            for (const int n : {1, 3, 9}) {
                const int ph = border_padded_dim(gh, n), pw = border_padded_dim(gw, n);
                std::vector<float> pad((size_t)gp * ph * pw), back(ne);
                for (int pl = 0; pl < gp; ++pl)
                    for (int y = 0; y < ph; ++y)
                        for (int x = 0; x < pw; ++x) pad[((size_t)pl * ph + y) * pw + x] = pic[(size_t)pl * gh * gw + border_src_index(y, x, gh, gw, n, mode, false)];
                for (int pl = 0; pl < gp; ++pl)
                    for (int y = 0; y < gh; ++y)
                        for (int x = 0; x < gw; ++x) back[(pl * gh + y) * gw + x] = pad[(size_t)pl * ph * pw + border_src_index(y, x, ph, pw, n, mode, true)];
                unsigned ck = 0;
                for (size_t i = 0; i < pad.size(); ++i) ck += bits(pad[i]) * (unsigned)(i + 1);
                for (int i = 0; i < ne; ++i) CHECK(bits(back[i]) == bits(pic[i]));
                printf("host_check_border: mode %d N %d: %u\n", mode, n, ck);
            }
    }
    if (g_fail) { fprintf(stderr, "host_check_border: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_border: ok\n");
    return 0;
}
