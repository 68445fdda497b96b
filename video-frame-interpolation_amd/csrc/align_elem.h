// The per-element functions of the align definition (include/emavfi.h, "ALIGN DEFINITION"): the quantised luma of a pixel, the mean absolute
// difference m(d) of a candidate, the order in which candidates are preferred, the acceptance test, the half-shift a record stands for and
// the clamped source index of a shifted position, with the validity predicates of every argument.  One text for the kernels
// (misc_kernels.hip), for the entries' guards (emavfi_api.hip) and for the host check (tests/host/host_check_align.cpp, a plain C++
// program).  Every decision is an integer one; the only floating point is the pixel's sum and its product with 64, in the order written.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIP__
#define ALIGN_HD __host__ __device__
#else
#define ALIGN_HD
#endif

constexpr int ALIGN_CELL = 4;            // EMAVFI_ALIGN_CELL: a cell is 4 x 4 pixels
constexpr int ALIGN_MAX_RADIUS = 32;     // EMAVFI_ALIGN_MAX_RADIUS, in cells
constexpr int ALIGN_MAX_RATIO = 1024;    // EMAVFI_ALIGN_MAX_RATIO: the acceptance ratio is a count of 1024ths
constexpr int ALIGN_MIN_DIM = 8;         // the signature wants at least 2 x 2 cells
constexpr int ALIGN_MAX_DIM = 16384;     // every dimension of a frame lies in 1..16384 (the signature: 8..16384)
constexpr int ALIGN_MAX_HALF = 16384;    // a half-shift is clamped to +-16384 before any index arithmetic
constexpr int ALIGN_Q_MAX = 1023;        // a pixel's quantised luma lies in 0..1023, a cell's sum in 0..16368
constexpr unsigned ALIGN_G_MAX = 16u * ALIGN_Q_MAX;

ALIGN_HD inline bool align_sig_dim_ok(int d) { return d >= ALIGN_MIN_DIM && d <= ALIGN_MAX_DIM; }
ALIGN_HD inline bool align_dim_ok(int d) { return d >= 1 && d <= ALIGN_MAX_DIM; }
ALIGN_HD inline bool align_grid_dim_ok(int d) { return d >= ALIGN_MIN_DIM / ALIGN_CELL && d <= ALIGN_MAX_DIM / ALIGN_CELL; }
ALIGN_HD inline bool align_radius_ok(int R) { return R >= 1 && R <= ALIGN_MAX_RADIUS; }
// every candidate keeps at least half of each axis
ALIGN_HD inline bool align_radius_fits(int R, int Hc, int Wc) { return 2 * R <= (Hc < Wc ? Hc : Wc); }
ALIGN_HD inline bool align_ratio_ok(int ratio) { return ratio >= 0 && ratio <= ALIGN_MAX_RATIO; }
ALIGN_HD inline bool align_sign_ok(int sign) { return sign == 1 || sign == -1; }
ALIGN_HD inline int align_cells(int n) { return n / ALIGN_CELL; }
ALIGN_HD inline int align_candidates(int R) { return (2 * R + 1) * (2 * R + 1); }

// step 1: l = (x0 + x1) + x2, t = l * 64; 0 where !(t >= -512) (NaN included), 1023 where t >= 512, floor(t) + 512 between
ALIGN_HD inline int align_q(float x0, float x1, float x2)
{
    const float l = (x0 + x1) + x2;
    const float t = l * 64.0f;
    if (!(t >= -512.0f)) return 0;
    if (t >= 512.0f) return ALIGN_Q_MAX;
    return (int)floorf(t) + 512;
}

ALIGN_HD inline unsigned align_abs_diff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }
ALIGN_HD inline int align_abs(int v) { return v < 0 ? -v : v; }

// step 2: N(d) = (Hc - |dy|)(Wc - |dx|), m(d) = floor(SAD(d) * 256 / N(d)) in unsigned 64-bit (SAD <= 16368 * 2^24)
ALIGN_HD inline uint64_t align_overlap(int Hc, int Wc, int dy, int dx) { return (uint64_t)(Hc - align_abs(dy)) * (uint64_t)(Wc - align_abs(dx)); }
ALIGN_HD inline uint64_t align_m(uint64_t sad, int Hc, int Wc, int dy, int dx) { return sad * 256u / align_overlap(Hc, Wc, dy, dx); }

// step 3: candidates are preferred by the least m, then the least |dy| + |dx|, then the least |dy|: one 64-bit key, the least wins
// (m <= 4 190 208 < 2^22, |dy| + |dx| <= 64, |dy| <= 32).  Candidates of one key differ only in signs; more than one of them: d* = 0.
ALIGN_HD inline uint64_t align_key(uint64_t m, int dy, int dx)
{
    return (m << 14) | (uint64_t)((align_abs(dy) + align_abs(dx)) << 7) | (uint64_t)align_abs(dy);
}
// a non-zero d* is kept only where m(d*) * 1024 <= m(0) * ratio
ALIGN_HD inline bool align_accepts(uint64_t m_best, uint64_t m_zero, int ratio) { return m_best * 1024u <= m_zero * (uint64_t)ratio; }

// the record of a sample from the winner of the order above and how many candidates share its key
ALIGN_HD inline void align_record(int dy, int dx, unsigned winners, uint64_t m_best, uint64_t m_zero, int ratio, int *rec)
{
    const bool keep = winners == 1 && (dy != 0 || dx != 0) && align_accepts(m_best, m_zero, ratio);
    rec[0] = keep ? ALIGN_CELL * dy : 0;
    rec[1] = keep ? ALIGN_CELL * dx : 0;
    rec[2] = (int)(keep ? m_best : m_zero);
    rec[3] = (int)m_zero;
}

// step 4: the half-shift of a recorded shift in pixels, whatever the word holds: an arithmetic shift, clamped to +-16384
ALIGN_HD inline int align_half(int d_px)
{
    const int h = d_px >> 1;
    return h < -ALIGN_MAX_HALF ? -ALIGN_MAX_HALF : (h > ALIGN_MAX_HALF ? ALIGN_MAX_HALF : h);
}
// the sample of an axis of n that destination position i reads under a move by `move` (= sign * half-shift): clamp(i - move)
ALIGN_HD inline int align_src_index(int i, int move, int n)
{
    const int s = i - move;
    return s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
}
// whether the four destination columns x .. x + 3 read four CONSECUTIVE source columns starting at *sx0 (nothing clamps)
ALIGN_HD inline bool align_unit_inside(int x, int move, int W, int *sx0)
{
    *sx0 = x - move;
    return *sx0 >= 0 && *sx0 + 3 <= W - 1;
}
