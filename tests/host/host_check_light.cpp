// Host-only exercise of the linear-light entries for the sanitizer build (csrc/Makefile, target `asan`), beside host_check_shutter.cpp and its
// siblings: the per-element functions the kernel is made of (csrc/light_elem.h, the same text) in a plain loop against the definition
// (include/emavfi.h, "LINEAR LIGHT DEFINITION") written with `/` on unsigned long long and a linear scan; light_div, the schoolbook division in
// base 2^16 that stands in for the 64-bit division by the weight sum, against `/` for every sum; light_enc against a linear scan for the three
// built-in tables at depth 12; and every host-side refusal of emavfi_transfer_table, emavfi_transfer_table_check and
// emavfi_accumulate_frames_linear - no kernel is launched, every call of the last is refused on the host, its table read from real host memory.
#include "../../include/emavfi.h"
#include "../../video-frame-interpolation_amd/csrc/light_elem.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        if (!(cond)) { fprintf(stderr, "host_check_light: %s:%d: %s  [last error: %s]\n", __FILE__, __LINE__, #cond, emavfi_last_error()); ++g_fail; } \
    } while (0)
#define REFUSED(call, word) CHECK((call) == EMAVFI_E_ARG && strstr(emavfi_last_error(), word))

// sample i of generated frame t, before the depth mask
static unsigned gen(unsigned i, unsigned t)
{
    unsigned x = i * 2654435761u + (t * 40503u + 12345u);
    x ^= x >> 15;
    x *= 2246822519u;
    return x >> 9;
}

// the definition's encode, as a linear scan: the largest v with v == 0 or lin[v - 1] + lin[v] <= 2 L
static unsigned enc_scan(unsigned long long L, const std::vector<unsigned> &lin)
{
    unsigned v = 0;
    for (unsigned c = 1; c < lin.size(); ++c)
        if ((unsigned long long)lin[c - 1] + lin[c] <= 2ull * L) v = c;
    return v;
}

static emavfi_accumulate_entry entry(unsigned n, unsigned f, unsigned h)
{
    emavfi_accumulate_entry e{};
    e.n = n; e.f = f; e.h = h;
    for (unsigned t = 0; t < EMAVFI_ACCUMULATE_MAX_TAPS; ++t) { e.tap[t] = (t & 1u) ? (EMAVFI_RESAMPLE_NODES | 1u) : 0u; e.w[t] = 1u; }
    return e;
}

int main()
{
    static_assert(EMAVFI_LIGHT_ONE == LIGHT_ONE && EMAVFI_LIGHT_BIAS == LIGHT_BIAS && EMAVFI_LIGHT_LIMIT == LIGHT_LIMIT, "header and light_elem.h disagree");

    // ---- light_div against `/` on unsigned long long: every S; the ends of the range the definition reaches, the ends of what any table
    // reaches (x < 2^48), numerators around hashed multiples of S and around the digit boundaries 2^16 and 2^32
    const unsigned long long top = 65535ull * ((1ull << 30) - 1ull) + 32767ull, any = (1ull << 48) - 1ull;
    for (unsigned S = 1; S <= SHUTTER_MAX_SUM; ++S) {
        const unsigned M = shutter_magic(S);
        const unsigned long long h0 = ((unsigned long long)gen(S, 0u) << 23) ^ gen(S, 1u), h1 = ((unsigned long long)gen(S, 2u) << 7) ^ gen(S, 3u);
        const unsigned long long ks[] = {0ull, 1ull, (1ull << 30) - 1ull, h0 % (1ull << 30), h1 % (1ull << 30), any / S, (any / S) - 1ull,
                                         (1ull << 32) / S, (1ull << 16) / S};
        for (const unsigned long long k : ks) {
            const unsigned long long at = k * S;                      // k S <= 2^48 - 1: no wrap
            const unsigned long long xs[] = {at, at ? at - 1ull : 0ull, at + (S - 1u) <= any ? at + (S - 1u) : at, at + 1ull <= any ? at + 1ull : at};
            for (const unsigned long long x : xs)
                if (light_div(x, S, M) != x / S) { CHECK(light_div(x, S, M) == x / S); fprintf(stderr, "  x = %llu, S = %u\n", x, S); }
        }
        const unsigned long long ends[] = {0ull, S - 1ull, S, top, any, (unsigned long long)S * ((1ull << 30) - 1ull) + (S >> 1), 65535ull, 65536ull,
                                           (1ull << 32) - 1ull, 1ull << 32, (1ull << 32) + S, (unsigned long long)S << 32, ((unsigned long long)S << 32) - 1ull};
        for (const unsigned long long x : ends)
            if (light_div(x, S, M) != x / S) { CHECK(light_div(x, S, M) == x / S); fprintf(stderr, "  x = %llu, S = %u\n", x, S); }
    }

    // ---- the tables: every refusal, the properties the definition states, enc against the scan at depth 12
    {
        std::vector<unsigned> lin(4096);
        REFUSED(emavfi_transfer_table(3, 8, 1, lin.data()), "transfer");
        REFUSED(emavfi_transfer_table(-1, 8, 1, lin.data()), "transfer");
        REFUSED(emavfi_transfer_table(EMAVFI_TRANSFER_SRGB, 16, 1, lin.data()), "depth");
        REFUSED(emavfi_transfer_table(EMAVFI_TRANSFER_SRGB, 9, 1, lin.data()), "depth");
        REFUSED(emavfi_transfer_table(EMAVFI_TRANSFER_HLG, 8, 1, nullptr), "lin_host");
        REFUSED(emavfi_transfer_table_check(nullptr, 8), "lin_host");
        REFUSED(emavfi_transfer_table_check(lin.data(), 16), "depth");
        REFUSED(emavfi_transfer_table_check(lin.data(), 0), "depth");
        for (int transfer = 0; transfer < 3; ++transfer)
            for (const int depth : {8, 10, 12})
                for (int full = 0; full < 2; ++full) {
                    std::vector<unsigned> t(1u << depth);                // exactly 2^depth words: a write past them is ASan's to find
                    CHECK(emavfi_transfer_table(transfer, depth, full, t.data()) == EMAVFI_OK);
                    CHECK(emavfi_transfer_table_check(t.data(), depth) == EMAVFI_OK);
                    const unsigned lo = full ? 0u : 16u << (depth - 8), hi = full ? (1u << depth) - 1u : 235u << (depth - 8);
                    CHECK(t[lo] == LIGHT_BIAS && t[hi] + 8u >= LIGHT_BIAS + LIGHT_ONE && t[hi] <= LIGHT_BIAS + LIGHT_ONE + 8u);
                    for (unsigned v = 0; v < t.size(); ++v)
                        if (light_enc(t[v], t.data(), depth) != v) { CHECK(light_enc(t[v], t.data(), depth) == v); break; }
                    if (depth != 12) continue;
                    // enc against the linear scan: at every table value, one below and one above, at every midpoint (the tie), around it, and
                    // at the ends of the range of a mean
                    for (unsigned v = 0; v < t.size(); ++v) {
                        const unsigned mid = v ? (unsigned)(((unsigned long long)t[v - 1] + t[v]) / 2ull) : 0u;
                        const unsigned Ls[] = {t[v], t[v] - 1u, t[v] + 1u, mid, mid + 1u, mid ? mid - 1u : 0u};
                        for (const unsigned L : Ls)
                            if (light_enc(L, t.data(), depth) != enc_scan(L, t)) { CHECK(light_enc(L, t.data(), depth) == enc_scan(L, t)); fprintf(stderr, "  L = %u\n", L); }
                    }
                    CHECK(light_enc(0u, t.data(), depth) == 0u && light_enc(LIGHT_LIMIT - 1u, t.data(), depth) == (1u << depth) - 1u);
                }
        std::vector<unsigned> t(256);
        CHECK(emavfi_transfer_table(EMAVFI_TRANSFER_SRGB, 8, 1, t.data()) == EMAVFI_OK);
        auto bad = t;
        bad[77] = bad[76];                                            // a flat step
        REFUSED(emavfi_transfer_table_check(bad.data(), 8), "lin[77]");
        bad = t; bad[200] = bad[199] - 1u;                            // a decreasing step
        REFUSED(emavfi_transfer_table_check(bad.data(), 8), "lin[200]");
        bad = t; bad[255] = 1u << 30;
        REFUSED(emavfi_transfer_table_check(bad.data(), 8), "lin[255]");
        bad = t; bad[0] = 0xffffffffu;
        REFUSED(emavfi_transfer_table_check(bad.data(), 8), "lin[0]");
    }

    // ---- the per-element functions in a plain loop against the definition: byte frames and every (depth, shift) of the word frames, the
    // dword form against the scalar one; the tables bt709 limited and hlg full, and the affine table, which must give the coded mean
    const int formats[][3] = {{1, 8, 0}, {2, 10, 0}, {2, 10, 6}, {2, 12, 0}, {2, 12, 4}};
    std::vector<std::vector<unsigned>> cases = {{1u, 1u}, {1u, 2u, 1u}, {5u, 6u, 1u}, {65534u, 1u}, {192u, 64u}, std::vector<unsigned>(33, 1985u)};
    cases[5][32] = 2015u;                                         // 32 * 1985 + 2015 = 65535
    const unsigned n = 1032;                                      // samples per frame
    for (const auto &f : formats) {
        const int sb = f[0], depth = f[1], shift = f[2];
        const unsigned mask = (1u << depth) - 1u, full = sb == 1 ? 255u : 65535u;
        for (int which = 0; which < 3; ++which) {
            std::vector<unsigned> lin(1u << depth);
            if (which == 0) CHECK(emavfi_transfer_table(EMAVFI_TRANSFER_BT709, depth, 0, lin.data()) == EMAVFI_OK);
            else if (which == 1) CHECK(emavfi_transfer_table(EMAVFI_TRANSFER_HLG, depth, 1, lin.data()) == EMAVFI_OK);
            else for (unsigned v = 0; v < lin.size(); ++v) lin[v] = LIGHT_BIAS + 65536u * v;
            CHECK(emavfi_transfer_table_check(lin.data(), depth) == EMAVFI_OK);
            for (size_t c = 0; c < cases.size(); ++c) {
                const std::vector<unsigned> &w = cases[c];
                unsigned S = 0;
                for (const unsigned v : w) S += v;
                const unsigned M = shutter_magic(S);
                std::vector<unsigned> out(n);
                for (unsigned i = 0; i < n; ++i) {
                    unsigned long long sum = 0;
                    unsigned coded = 0, lo = 0xffffffffu, hi = 0;
                    for (unsigned t = 0; t < w.size(); ++t) {         // whole words: the bits outside the sample must not leak
                        // the first samples of every frame all ones, the next all zeros: the largest intermediate occurs
                        const unsigned word = i < 32 ? full : i < 64 ? 0u : gen(i, t) & full;
                        const unsigned s = shutter_sample(word, mask, shift);
                        sum += (unsigned long long)w[t] * lin[s];
                        coded += w[t] * s;
                        lo = s < lo ? s : lo; hi = s > hi ? s : hi;
                    }
                    const unsigned v = light_enc(light_mean(sum, S, M), lin.data(), depth);
                    CHECK(v == enc_scan((sum + S / 2) / S, lin) && v >= lo && v <= hi);
                    if (which == 2) CHECK(v == (coded + S / 2) / S);      // the affine table is the coded mean, ties included
                    out[i] = v << shift;
                }
                CHECK((out[0] >> shift) == mask && out[40] == 0u);
                for (unsigned i = 0; i + 4 / sb <= n; i += 4 / sb) {
                    LightSums acc{};
                    unsigned want = 0;
                    for (unsigned t = 0; t < w.size(); ++t) {
                        unsigned d = 0;
                        for (unsigned q = 0; q < 4u / sb; ++q) d |= ((i + q) < 32 ? full : (i + q) < 64 ? 0u : gen(i + q, t) & full) << (8 * sb * q);
                        light_add_dword(acc, d, w[t], lin.data(), sb, mask, shift);
                    }
                    for (unsigned q = 0; q < 4u / sb; ++q) want |= out[i + q] << (8 * sb * q);
                    CHECK(light_mean_dword(acc, S, M, lin.data(), sb, depth, shift) == want);
                }
            }
        }
    }
    // a table that is not valid: the search stays inside it (ASan watches the exact-size vector) and returns a code
    for (const int depth : {8, 10, 12}) {
        std::vector<unsigned> junk(1u << depth);
        for (unsigned v = 0; v < junk.size(); ++v) junk[v] = gen(v, 7u) * 2654435761u;
        for (unsigned i = 0; i < 4096; ++i) CHECK(light_enc(gen(i, 9u) * 40503u, junk.data(), depth) < junk.size());
        std::vector<unsigned> zero(1u << depth, 0u);
        CHECK(light_enc(0u, zero.data(), depth) == junk.size() - 1u && light_enc(0xffffffffu, zero.data(), depth) < zero.size());
    }

    // ---- emavfi_accumulate_frames_linear: what it adds to the refusals of emavfi_accumulate_frames, and that those are reached under its name
    unsigned char *const dp = (unsigned char *)(uintptr_t)(1u << 20), *const sp = (unsigned char *)(uintptr_t)(2u << 20);   // never dereferenced
    unsigned char *const np = (unsigned char *)(uintptr_t)(3u << 20);
    unsigned *const fp = (unsigned *)(uintptr_t)(4u << 20), *const lp = (unsigned *)(uintptr_t)(5u << 20);
    std::vector<emavfi_accumulate_entry> t(19, entry(3u, 0u, 0u));
    const emavfi_accumulate_entry *tp = t.data();
    const size_t FB = 4096;
#define CALL(dst, n, tab, fb, sb, dep, sh, lin, lb) \
    emavfi_accumulate_frames_linear(dst, FB, n, sp, FB, 2, np, FB, 2, tab, fp, 2, fb, sb, dep, sh, lin, lb, nullptr)
    REFUSED(CALL(dp, 2, tp, FB, 1, 8, 0, nullptr, FB), "lin");
    REFUSED(CALL(dp, 2, tp, FB, 1, 8, 0, (unsigned *)((uintptr_t)lp + 2), FB), "4-byte");
    REFUSED(CALL(dp, 2, tp, FB, 2, 16, 0, lp, FB), "depth = 16");
    REFUSED(CALL(dp, 2, tp, FB, 1, 8, 0, lp, FB + 1), "linear_bytes");
    REFUSED(CALL(dp, 2, tp, FB, 2, 10, 6, lp, FB + 2), "linear_bytes");
    REFUSED(CALL(dp, 2, tp, FB, 2, 10, 6, lp, 99), "linear_bytes");
    REFUSED(CALL(dp, 2, tp, FB, 2, 12, 0, lp, SIZE_MAX), "linear_bytes");
    REFUSED(CALL(dp, 0, tp, FB, 1, 8, 0, lp, FB), "n_out");
    REFUSED(CALL(nullptr, 2, tp, FB, 1, 8, 0, lp, FB), "dst");
    REFUSED(CALL(dp, 2, nullptr, FB, 1, 8, 0, lp, FB), "table");
    REFUSED(CALL(dp, 2, tp, 0, 1, 8, 0, lp, 0), "frame_bytes");
    REFUSED(CALL(dp, 2, tp, FB, 1, 10, 0, lp, FB), "depth");
    REFUSED(CALL(dp, 2, tp, FB, 2, 14, 0, lp, FB), "depth");
    REFUSED(CALL(dp, 2, tp, FB, 2, 12, 5, lp, FB), "shift");
    REFUSED(CALL(sp + FB, 2, tp, FB, 1, 8, 0, lp, FB), "overlaps srcs");
    {
        auto bad = t;
        bad[18].n = 0u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[18].n");
        bad = t; bad[9].tap[2] = 2u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[9].tap[2]");
        bad = t; bad[3].w[1] = 0u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[3].w[1] is zero");
        bad = t; bad[4].w[0] = 65534u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[4].w sums to more than 65535");
        bad = t; bad[5].f = 3u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[5].f");
        bad = t; bad[7].f = 1u; bad[7].h = 2u;
        REFUSED(CALL(dp, 19, bad.data(), FB, 1, 8, 0, lp, FB), "table[7].h");
    }
    CHECK(strstr(emavfi_last_error(), "accumulate_frames_linear"));

    if (g_fail) { fprintf(stderr, "host_check_light: %d check(s) failed\n", g_fail); return 1; }
    printf("host_check_light: ok\n");
    return 0;
}
