// Host-only exercise of the coarse flow entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_border.cpp and its
// siblings: every argument guard of emavfi_downscale_f32 and emavfi_upsample_flow_f32, the host-side guards of emavfi_forward_flow and
// emavfi_forward_given_flow and their launch lists (include/emavfi.h, "COARSE FLOW DEFINITION") - no kernel is launched, every call here is
// refused or answered on the host - and the per-element functions the kernels are made of (csrc/coarse_elem.h, the same text; contraction
// off, as for the kernels) against closed forms and in a plain loop over a generated 2-plane 5 x 7 case at s = 2, 4, 8: the checksums it
// prints are compared with the numpy oracle's by tests/test_coarse_flow_cpu.py::test_coarse_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/coarse_elem.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_coarse: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// element i of the generated tensor (tests/ensemble_oracle.py, generated(0, ...)): a signed 24-bit mantissa times 2^(e - 20), e in 0..7
static float gen(unsigned i)
{
    const unsigned h = (i * 2654435761u + 12345u) * 2246822519u;
    return std::ldexp((float)((int)(h >> 8) - (1 << 23)), (int)(h & 7u) - 20);
}
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

static std::vector<float> down_loop(const std::vector<float> &x, int planes, int H, int W, int s)
{
    const int Hs = coarse_dim(H, s), Ws = coarse_dim(W, s);
    std::vector<float> out((size_t)planes * Hs * Ws);
    for (int pl = 0; pl < planes; ++pl)
        for (int i = 0; i < Hs; ++i)
            for (int j = 0; j < Ws; ++j) out[((size_t)pl * Hs + i) * Ws + j] = coarse_down_elem(x.data() + (size_t)pl * H * W, H, W, s, i, j);
    return out;
}
static std::vector<float> up_loop(const std::vector<float> &p, int planes, int H, int W, int s)
{
    const int Hs = coarse_dim(H, s), Ws = coarse_dim(W, s);
    std::vector<float> out((size_t)planes * H * W);
    for (int pl = 0; pl < planes; ++pl)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                out[((size_t)pl * H + y) * W + x] = coarse_up_elem(p.data() + (size_t)pl * Hs * Ws, Ws, coarse_up_tap(y, Hs, s), coarse_up_tap(x, Ws, s), s);
    return out;
}
static std::vector<std::string> launches(int kind, int mid, int dtype, unsigned gather)
{
    char names[8192];
    double fl[96], by[96];
    const int n = kind == 0   ? emavfi_forward_launches_routed(3, mid, 3, 1, 40, 56, dtype, gather, names, sizeof names, fl, by, 96)
                  : kind == 1 ? emavfi_forward_flow_launches(3, mid, 3, 1, 40, 56, dtype, names, sizeof names, fl, by, 96)
                              : emavfi_forward_given_flow_launches(3, mid, 3, 1, 40, 56, dtype, gather, names, sizeof names, fl, by, 96);
    std::vector<std::string> out;
    CHECK(n > 0);
    if (n <= 0) return out;
    const char *p = names;
    for (int i = 0; i < n; ++i) {
        const char *e = strchr(p, '\n');
        out.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    return out;
}

int main()
{
    static_assert(EMAVFI_RESIZE_MAX_DIM == COARSE_MAX_DIM, "header and coarse_elem.h disagree");
    float *const sp = (float *)(uintptr_t)(1u << 20), *const dp = (float *)(uintptr_t)(2u << 20);   // never dereferenced
    const size_t P = 3;
    const int H = 16, W = 32;
    const size_t FINE = P * H * W * sizeof(float), COARSE = P * (H / 2) * (W / 2) * sizeof(float);
    const size_t HUGE_PLANES = std::numeric_limits<size_t>::max() / 2;
    float *const top = (float *)(std::numeric_limits<uintptr_t>::max() - 1023);

    // emavfi_downscale_f32(src, dst, planes, H, W, s, stream)
    REFUSED(emavfi_downscale_f32(nullptr, dp, P, H, W, 2, nullptr), "src");
    REFUSED(emavfi_downscale_f32(sp, nullptr, P, H, W, 2, nullptr), "dst");
    REFUSED(emavfi_downscale_f32(sp, dp, 0, H, W, 2, nullptr), "planes");
    for (const int s : {0, 1, 3, 5, 6, 16, -2, std::numeric_limits<int>::max()}) REFUSED(emavfi_downscale_f32(sp, dp, P, H, W, s, nullptr), "s =");
    REFUSED(emavfi_downscale_f32(sp, dp, P, 0, W, 2, nullptr), "H, W");
    REFUSED(emavfi_downscale_f32(sp, dp, P, H, -1, 4, nullptr), "H, W");
    REFUSED(emavfi_downscale_f32(sp, dp, P, 16385, W, 8, nullptr), "16384");
    REFUSED(emavfi_downscale_f32(sp, dp, P, H, std::numeric_limits<int>::max(), 8, nullptr), "16384");   // (the ceiling is not computed from it)
    REFUSED(emavfi_downscale_f32((float *)((uintptr_t)sp + 2), dp, P, H, W, 2, nullptr), "4-byte");
    REFUSED(emavfi_downscale_f32(sp, (float *)((uintptr_t)dp + 1), P, H, W, 2, nullptr), "4-byte");
    REFUSED(emavfi_downscale_f32(sp, dp, HUGE_PLANES, 16384, 16384, 2, nullptr), "overflows");
    REFUSED(emavfi_downscale_f32(sp, dp, std::numeric_limits<size_t>::max() / (8 * 16 * 4), 16, 32, 2, nullptr), "overflows");   // the coarse bytes fit, the fine do not
    REFUSED(emavfi_downscale_f32(top, dp, P, H, W, 2, nullptr), "overflows");
    REFUSED(emavfi_downscale_f32(sp, top, P, H, W, 2, nullptr), "overflows");
    REFUSED(emavfi_downscale_f32(sp, sp, P, H, W, 2, nullptr), "dst overlaps src");
    REFUSED(emavfi_downscale_f32(sp, (float *)((uintptr_t)sp + FINE - 4), P, H, W, 2, nullptr), "dst overlaps src");
    REFUSED(emavfi_downscale_f32(sp, (float *)((uintptr_t)sp - COARSE + 4), P, H, W, 2, nullptr), "dst overlaps src");

    // emavfi_upsample_flow_f32(flow_s, flow, planes, Hs, Ws, H, W, s, stream)
    REFUSED(emavfi_upsample_flow_f32(nullptr, dp, P, 8, 16, H, W, 2, nullptr), "flow_s");
    REFUSED(emavfi_upsample_flow_f32(sp, nullptr, P, 8, 16, H, W, 2, nullptr), "flow");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, 0, 8, 16, H, W, 2, nullptr), "planes");
    for (const int s : {0, 1, 3, 7, 16, -4}) REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 16, H, W, s, nullptr), "s =");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 16, 0, W, 2, nullptr), "H, W");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 16, H, 16385, 2, nullptr), "16384");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 0, 16, H, W, 2, nullptr), "Hs, Ws");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 16385, H, W, 2, nullptr), "Hs, Ws");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 15, H, W, 2, nullptr), "ceil");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 9, 16, H, W, 2, nullptr), "ceil");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 8, 16, H, W, 4, nullptr), "ceil");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, P, 2, 4, 17, 33, 8, nullptr), "ceil");       // 17 x 33 at 8 is 3 x 5: the floor is refused
    REFUSED(emavfi_upsample_flow_f32((float *)((uintptr_t)sp + 3), dp, P, 8, 16, H, W, 2, nullptr), "4-byte");
    REFUSED(emavfi_upsample_flow_f32(sp, (float *)((uintptr_t)dp + 2), P, 8, 16, H, W, 2, nullptr), "4-byte");
    REFUSED(emavfi_upsample_flow_f32(sp, dp, HUGE_PLANES, 8192, 8192, 16384, 16384, 2, nullptr), "overflows");
    REFUSED(emavfi_upsample_flow_f32(sp, top, P, 8, 16, H, W, 2, nullptr), "overflows");
    REFUSED(emavfi_upsample_flow_f32(sp, sp, P, 8, 16, H, W, 2, nullptr), "flow overlaps flow_s");
    REFUSED(emavfi_upsample_flow_f32(sp, (float *)((uintptr_t)sp + COARSE - 4), P, 8, 16, H, W, 2, nullptr), "flow overlaps flow_s");
    REFUSED(emavfi_upsample_flow_f32(sp, (float *)((uintptr_t)sp - FINE + 4), P, 8, 16, H, W, 2, nullptr), "flow overlaps flow_s");

    // the two halves of the forward: what is refused before any device work (fake 16-byte aligned pointers, never dereferenced)
    {
        void *const pk = (void *)(uintptr_t)(16u << 20), *const ws = (void *)(uintptr_t)(32u << 20);
        float *const f1 = (float *)(uintptr_t)(3u << 20), *const f2 = (float *)(uintptr_t)(4u << 20), *const fl = (float *)(uintptr_t)(5u << 20),
                     *const out = (float *)(uintptr_t)(6u << 20);
        const size_t big = (size_t)1 << 40;
        REFUSED(emavfi_forward_flow(3, 8, 3, pk, big, f1, f2, nullptr, ws, big, 1, 24, 40, EMAVFI_F32, nullptr), "null pointer");
        REFUSED(emavfi_forward_flow(3, 8, 3, pk, big, nullptr, f2, fl, ws, big, 1, 24, 40, EMAVFI_F32, nullptr), "null pointer");
        REFUSED(emavfi_forward_flow(3, 8, 3, pk, big, f1, f2, (float *)((uintptr_t)fl + 4), ws, big, 1, 24, 40, EMAVFI_F32, nullptr), "16-byte");
        REFUSED(emavfi_forward_flow(3, 8, 3, pk, big, f1, f2, fl, ws, big, 0, 24, 40, EMAVFI_F32, nullptr), "B, H, W");
        CHECK(emavfi_forward_flow(3, 8, 3, pk, big, f1, f2, fl, ws, 16, 1, 24, 40, EMAVFI_F32, nullptr) == EMAVFI_E_WORKSPACE);
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, nullptr, out, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 0, nullptr), "null pointer");
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, nullptr, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 0, nullptr), "null pointer");
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, (float *)((uintptr_t)fl + 8), out, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 0, nullptr), "16-byte");
        float *taps[8] = {};
        taps[1] = out;
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, big, 1, 24, 40, EMAVFI_F32, taps, nullptr, nullptr, 0, 0, nullptr), "taps[1]");
        taps[1] = nullptr; taps[2] = out;
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, big, 1, 24, 40, EMAVFI_F32, taps, nullptr, nullptr, 0, 0, nullptr), "taps[2]");
        void *ev[2] = {};
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, ev, 1, 0, nullptr), "n_events");
        REFUSED(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 8u, nullptr), "gather_blocks");
        CHECK(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, big, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 1u, nullptr) == EMAVFI_E_UNSUPPORTED);
        CHECK(emavfi_forward_given_flow(3, 8, 3, pk, big, f1, f2, fl, out, ws, 16, 1, 24, 40, EMAVFI_F32, nullptr, nullptr, nullptr, 0, 0, nullptr) == EMAVFI_E_WORKSPACE);
    }
    // the launch lists: the flow's is the plain prefix through the flow's launch, the given-flow one the plain list without the context stage
    // (its convolutions, pool and linear) and motion estimation
    for (const int dtype : {EMAVFI_F32, EMAVFI_BF16, EMAVFI_F16, EMAVFI_AMP16, EMAVFI_F32X3})
        for (const int mid : {8, 64}) {
            const unsigned gather = (mid == 64 && (dtype == EMAVFI_BF16 || dtype == EMAVFI_F16)) ? 7u : 0u;
            for (const unsigned g : {0u, gather}) {
                const std::vector<std::string> plain = launches(0, mid, dtype, g), stop = launches(1, mid, dtype, 0u), given = launches(2, mid, dtype, g);
                size_t flow_at = plain.size();
                std::vector<std::string> want;
                for (size_t i = 0; i < plain.size(); ++i) {
                    const std::string &n = plain[i];
                    if (n.find("(flow)") != std::string::npos) flow_at = i;
                    if (n.find("context_encoding") == std::string::npos && n.find("motion_estimation") == std::string::npos && n != "avg_pool_partial"
                        && n != "context_linear_fold")
                        want.push_back(n);
                }
                CHECK(flow_at < plain.size() && stop.size() == flow_at + 1 && std::vector<std::string>(plain.begin(), plain.begin() + (long)stop.size()) == stop);
                CHECK(given == want && given.size() + 6 <= plain.size());
            }
        }

    // the per-element functions against closed forms
    {
        CHECK(coarse_scale_ok(2) && coarse_scale_ok(4) && coarse_scale_ok(8) && !coarse_scale_ok(0) && !coarse_scale_ok(1) && !coarse_scale_ok(3) && !coarse_scale_ok(16));
        CHECK(coarse_dim_ok(1) && coarse_dim_ok(16384) && !coarse_dim_ok(0) && !coarse_dim_ok(16385));
        CHECK(coarse_dim(1, 8) == 1 && coarse_dim(8, 8) == 1 && coarse_dim(9, 8) == 2 && coarse_dim(23, 2) == 12 && coarse_dim(16384, 2) == 8192 && coarse_dim(16384, 8) == 2048);
        // down_s of a constant is that constant, at every size, clamped edges included
        for (const int s : {2, 4, 8})
            for (const int h : {1, 3, 5, 8, 9})
                for (const int w : {1, 2, 7, 16, 17}) {
                    const float c = gen((unsigned)(s * 100 + h * 10 + w));
                    const std::vector<float> x((size_t)h * w, c), d = down_loop(x, 1, h, w, s);
                    CHECK((int)d.size() == coarse_dim(h, s) * coarse_dim(w, s));
                    for (const float v : d) CHECK(bits(v) == bits(c));
                }
        // a 2:1 box on a known 4 x 4: ((a + b) + (c + d)) / 4
        {
            const std::vector<float> x = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
            const std::vector<float> d = down_loop(x, 1, 4, 4, 2);
            CHECK(d.size() == 4 && d[0] == 3.5f && d[1] == 5.5f && d[2] == 11.5f && d[3] == 13.5f);
            CHECK(down_loop(x, 1, 4, 4, 4)[0] == 8.5f);
            // 8 over a 4 x 4: rows and columns 4..7 clamp to row and column 3
            // block sums by quadrant: (mean of all) , (mean of column 3), (mean of row 3), x[3][3], each weighted 1 / 4 by the top level
            const float q00 = 8.5f, q01 = (4 + 8 + 12 + 16) / 4.0f, q10 = (13 + 14 + 15 + 16) / 4.0f, q11 = 16.0f;
            CHECK(down_loop(x, 1, 4, 4, 8)[0] == ((q00 + q01) + (q10 + q11)) * 0.25f);
        }
        // the order is the tree's, not a running sum: leaves 1, 2^-24, 2^-24, 2^-24 (the tree keeps the small pair, a running sum loses each)
        {
            const float t = std::ldexp(1.0f, -24);
            const std::vector<float> x = {1.0f, t, t, t};
            const float tree = ((1.0f + t) + (t + t)) * 0.25f, running = (((1.0f + t) + t) + t) * 0.25f;
            CHECK(bits(down_loop(x, 1, 2, 2, 2)[0]) == bits(tree) && bits(tree) != bits(running));
        }
        // taps: num = 2 d + 1 - s; the first s / 2 positions clamp to coarse index 0 with both taps, the weights are dyadic
        for (const int s : {2, 4, 8})
            for (const int n : {1, 2, 5}) {
                for (int d = 0; d < s * n; ++d) {
                    const CoarseTap t = coarse_up_tap(d, n, s);
                    const int num = 2 * d + 1 - s, i0 = (int)std::floor((double)num / (2 * s));
                    CHECK(t.j0 == std::min(std::max(i0, 0), n - 1) && t.j1 == std::min(std::max(i0 + 1, 0), n - 1));
                    CHECK(t.w == (float)(num - 2 * s * i0) / (float)(2 * s) && t.w >= 0.0f && t.w < 1.0f);
                    if (d < s / 2) CHECK(t.j0 == 0 && t.j1 == 0);
                    if (n == 1) CHECK(t.j0 == 0 && t.j1 == 0);
                }
                // centre of block k (s even: between two destination samples): d = s k + s / 2 - 1 and the next one straddle it symmetrically
                const CoarseTap a = coarse_up_tap(s / 2 - 1, n, s), b = coarse_up_tap(s / 2, n, s);
                CHECK(a.w == 1.0f - 1.0f / (2 * s) && b.w == 1.0f / (2 * s));
            }
        // up of a constant flow c is exactly s c (c of few significant bits: both products exact), Hs = 1 and W < s included
        for (const int s : {2, 4, 8})
            for (const int h : {1, 3, 8, 9})
                for (const int w : {1, 5, 16, 17})
                    for (const float c : {1.5f, -2.25f, 0.0f, 96.0f}) {
                        const std::vector<float> p((size_t)coarse_dim(h, s) * coarse_dim(w, s), c), u = up_loop(p, 1, h, w, s);
                        for (const float v : u) CHECK(v == (float)s * c);
                    }
        // a ramp along x, coarse value k at column k: inside, flow_up = s ((2 d + 1 - s) / (2 s)), a straight line through the block centres
        {
            const int s = 4, n = 6, w = s * n;
            std::vector<float> p((size_t)n);
            for (int k = 0; k < n; ++k) p[(size_t)k] = (float)k;
            const std::vector<float> u = up_loop(p, 1, 1, w, s);
            for (int d = s / 2; d < w - s / 2; ++d) CHECK(u[(size_t)d] == (float)s * ((float)(2 * d + 1 - s) / (float)(2 * s)));
            for (int d = 0; d < s / 2; ++d) CHECK(u[(size_t)d] == 0.0f && u[(size_t)(w - 1 - d)] == (float)(s * (n - 1)));
        }
    }

    // the per-element functions in a plain loop: 2 planes of 5 x 7 into exactly-sized buffers, down then up again
    {
        const int gp = 2, gh = 5, gw = 7, ne = gp * gh * gw;
        std::vector<float> x((size_t)ne);
        for (int i = 0; i < ne; ++i) x[(size_t)i] = gen((unsigned)i);
        for (const int s : {2, 4, 8}) {
            const std::vector<float> d = down_loop(x, gp, gh, gw, s), u = up_loop(d, gp, gh, gw, s);
            unsigned ckd = 0, cku = 0;
            for (size_t i = 0; i < d.size(); ++i) ckd += bits(d[i]) * (unsigned)(i + 1);
            for (size_t i = 0; i < u.size(); ++i) cku += bits(u[i]) * (unsigned)(i + 1);
            printf("host_check_coarse: s %d: down %u up %u\n", s, ckd, cku);
        }
    }
    if (g_fail) { fprintf(stderr, "host_check_coarse: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_coarse: ok\n");
    return 0;
}
