// Host-only exercise of the two ensemble entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_static.cpp and its
// siblings: every argument guard of emavfi_flip_f32 and emavfi_ensemble_mean_f32 (include/emavfi.h, "ENSEMBLE DEFINITION") - no kernel is
// launched, every call here is refused on the host, and the member and flip lists are read from real host memory - and the per-element
// functions the kernels are made of (csrc/ensemble_elem.h, the same text) in a plain loop over a generated 2-plane 5 x 7 case, all four flips
// and n = 1, 2, 4, 8: the checksums it prints are compared with the numpy oracle's by
// tests/test_ensemble_cpu.py::test_ensemble_host_check_runs_clean_under_asan_ubsan_and_matches_the_oracle.  Built with contraction off, as
// the kernels are.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/ensemble_elem.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_ensemble: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// element i of generated member k (tests/ensemble_oracle.py, generated()): a signed 24-bit mantissa times 2^(e - 20), e in 0..7 - exact in
// fp32, and of mixed magnitude so that the additions round and the order of the tree shows
static float gen(unsigned k, unsigned i)
{
    const unsigned h = (i * 2654435761u + k * 40503u + 12345u) * 2246822519u;
    return std::ldexp((float)((int)(h >> 8) - (1 << 23)), (int)(h & 7u) - 20);
}
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

int main()
{
    static_assert(EMAVFI_FLIP_H == ENSEMBLE_FLIP_H && EMAVFI_FLIP_V == ENSEMBLE_FLIP_V && EMAVFI_ENSEMBLE_MAX_MEMBERS == ENSEMBLE_MAX_MEMBERS,
                  "header and ensemble_elem.h disagree");
    float *const sp = (float *)(uintptr_t)(1u << 20), *const dp = (float *)(uintptr_t)(2u << 20);   // never dereferenced
    const size_t P = 3, BYTES = P * 16 * 32 * sizeof(float);
    const int H = 16, W = 32;

    // emavfi_flip_f32(src, dst, planes, H, W, flip, stream)
    REFUSED(emavfi_flip_f32(nullptr, dp, P, H, W, 0, nullptr), "src");
    REFUSED(emavfi_flip_f32(sp, nullptr, P, H, W, 0, nullptr), "dst");
    REFUSED(emavfi_flip_f32(sp, dp, 0, H, W, 0, nullptr), "planes");
    REFUSED(emavfi_flip_f32(sp, dp, P, 0, W, 0, nullptr), "H, W");
    REFUSED(emavfi_flip_f32(sp, dp, P, H, -1, 0, nullptr), "H, W");
    REFUSED(emavfi_flip_f32(sp, dp, P, 16385, W, 0, nullptr), "16384");
    REFUSED(emavfi_flip_f32(sp, dp, P, H, 16385, 0, nullptr), "16384");
    REFUSED(emavfi_flip_f32(sp, dp, P, H, W, 4, nullptr), "flip");
    REFUSED(emavfi_flip_f32(sp, dp, P, H, W, -1, nullptr), "flip");
    REFUSED(emavfi_flip_f32((float *)((uintptr_t)sp + 2), dp, P, H, W, 1, nullptr), "4-byte");
    REFUSED(emavfi_flip_f32(sp, (float *)((uintptr_t)dp + 1), P, H, W, 1, nullptr), "4-byte");
    REFUSED(emavfi_flip_f32(sp, dp, std::numeric_limits<size_t>::max() / 2, 16384, 16384, 0, nullptr), "overflows");
    REFUSED(emavfi_flip_f32(sp, (float *)(std::numeric_limits<uintptr_t>::max() - 1023), P, H, W, 0, nullptr), "overflows");
    // dst against src: its last word on src's first, its first on src's last, the same tensor (a flip in place is refused too)
    REFUSED(emavfi_flip_f32(sp, (float *)((uintptr_t)sp - BYTES + 4), P, H, W, 3, nullptr), "dst overlaps src");
    REFUSED(emavfi_flip_f32(sp, (float *)((uintptr_t)sp + BYTES - 4), P, H, W, 3, nullptr), "dst overlaps src");
    REFUSED(emavfi_flip_f32(sp, sp, P, H, W, 0, nullptr), "dst overlaps src");

    // emavfi_ensemble_mean_f32(members, flips, n, out, planes, H, W, stream): the lists live in exactly-sized host arrays
    {
        std::vector<const float *> m(8);
        for (int k = 0; k < 8; ++k) m[k] = (const float *)((uintptr_t)(4 + k) << 20);
        std::vector<int> f = {0, 3, 1, 2, 0, 3, 1, 2};
        for (const int n : {0, 3, 5, 6, 7, 9, 16, -1}) REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), n, dp, P, H, W, nullptr), "n =");
        REFUSED(emavfi_ensemble_mean_f32(nullptr, f.data(), 8, dp, P, H, W, nullptr), "members");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), nullptr, 8, dp, P, H, W, nullptr), "flips");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, nullptr, P, H, W, nullptr), "out");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, dp, 0, H, W, nullptr), "planes");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, dp, P, 0, W, nullptr), "H, W");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, dp, P, H, 20000, nullptr), "16384");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, (float *)((uintptr_t)dp + 2), P, H, W, nullptr), "4-byte");
        REFUSED(emavfi_ensemble_mean_f32(m.data(), f.data(), 8, dp, std::numeric_limits<size_t>::max() / 4, 16384, 16384, nullptr), "overflows");
        for (const int n : {1, 2, 4, 8}) {                          // the LAST entry of each admitted length is looked at
            auto bm = m; auto bf = f;
            bm.resize(n); bf.resize(n);
            bf[n - 1] = 4;
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "flips[");
            bf[n - 1] = -2;
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "flips[");
            bf[n - 1] = 2;
            bm[n - 1] = nullptr;
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "members[");
            bm[n - 1] = (const float *)(((uintptr_t)9 << 20) + 3);
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "4-byte");
            bm[n - 1] = (const float *)((uintptr_t)dp + BYTES - 4);
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "out overlaps members[");
            bm[n - 1] = (const float *)((uintptr_t)dp - BYTES + 4);
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "out overlaps members[");
            bm[n - 1] = dp;
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "out overlaps members[");
            bm[n - 1] = (const float *)(std::numeric_limits<uintptr_t>::max() - 1023);
            REFUSED(emavfi_ensemble_mean_f32(bm.data(), bf.data(), n, dp, P, H, W, nullptr), "overflows");
        }
    }

    // the per-element functions in a plain loop: 2 planes of 5 x 7, 8 generated members
    {
        const int gp = 2, gh = 5, gw = 7, ne = gp * gh * gw;
        std::vector<std::vector<float>> mem(8, std::vector<float>(ne));
        for (unsigned k = 0; k < 8; ++k)
            for (int i = 0; i < ne; ++i) mem[k][i] = gen(k, (unsigned)i);
        for (int flip = 0; flip < 4; ++flip) {
            unsigned ck = 0;
            std::vector<float> once(ne), twice(ne);
            for (int pl = 0; pl < gp; ++pl)
                for (int y = 0; y < gh; ++y)
                    for (int x = 0; x < gw; ++x) once[(pl * gh + y) * gw + x] = mem[0][pl * gh * gw + ensemble_src_index(y, x, gh, gw, flip)];
            for (int pl = 0; pl < gp; ++pl)
                for (int y = 0; y < gh; ++y)
                    for (int x = 0; x < gw; ++x) twice[(pl * gh + y) * gw + x] = once[pl * gh * gw + ensemble_src_index(y, x, gh, gw, flip)];
            for (int i = 0; i < ne; ++i) { ck += bits(once[i]) * (unsigned)(i + 1); CHECK(bits(twice[i]) == bits(mem[0][i])); }
            printf("host_check_ensemble: flip %d: %u\n", flip, ck);
        }
        for (const int n : {1, 2, 4, 8}) {
            unsigned ck = 0;
            for (int pl = 0; pl < gp; ++pl)
                for (int y = 0; y < gh; ++y)
                    for (int x = 0; x < gw; ++x) {
                        float v[ENSEMBLE_MAX_MEMBERS];
                        for (int k = 0; k < n; ++k) v[k] = mem[k][pl * gh * gw + ensemble_src_index(y, x, gh, gw, (3 * k + n) & 3)];
                        ck += bits(ensemble_mean(v, n)) * (unsigned)((pl * gh + y) * gw + x + 1);
                    }
            printf("host_check_ensemble: mean n %d: %u\n", n, ck);
        }
    }
    // the unit form (four columns at once, lanes reversed under an H flip) against the element form: 3 x 8
    for (int flip = 0; flip < 4; ++flip)
        for (int y = 0; y < 3; ++y)
            for (int q = 0; q < 2; ++q) {
                const int u = ensemble_src_unit(y, q, 3, 2, flip);
                const EnsembleUnit e = ensemble_lanes(EnsembleUnit{4.f * u, 4.f * u + 1, 4.f * u + 2, 4.f * u + 3}, flip);   // lane values: element indices
                const float lanes[4] = {e.x, e.y, e.z, e.w};
                for (int j = 0; j < 4; ++j) CHECK((int)lanes[j] == ensemble_src_index(y, 4 * q + j, 3, 8, flip));
            }
    // closed forms: n = 1 is the value itself (NaN payload and -0 included), a NaN anywhere gives NaN, the tree is not the running sum
    {
        const float nan = std::numeric_limits<float>::quiet_NaN(), neg0 = -0.0f;
        CHECK(bits(ensemble_mean(&neg0, 1)) == 0x80000000u && bits(ensemble_mean(&nan, 1)) == bits(nan));
        for (int n : {2, 4, 8})
            for (int k = 0; k < n; ++k) {
                float v[8] = {1, 2, 3, 4, 5, 6, 7, 8};
                v[k] = nan;
                CHECK(std::isnan(ensemble_mean(v, n)));
            }
        const float v[4] = {16777216.f, 1.f, 1.f, 1.f};            // 2^24: (2^24 + 1) + (1 + 1) = 2^24 + 2, the running sum stays at 2^24
        CHECK(ensemble_mean(v, 4) == 4194304.5f);
        CHECK(ensemble_count_ok(1) && ensemble_count_ok(8) && !ensemble_count_ok(3) && !ensemble_count_ok(0) && !ensemble_count_ok(16));
        CHECK(ensemble_flip_ok(0) && ensemble_flip_ok(3) && !ensemble_flip_ok(4) && !ensemble_flip_ok(-1));
    }
    if (g_fail) { fprintf(stderr, "host_check_ensemble: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_ensemble: ok\n");
    return 0;
}
