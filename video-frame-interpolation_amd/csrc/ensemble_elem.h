// The per-element functions of the ensemble definition (include/emavfi.h, "ENSEMBLE DEFINITION"): where a flipped member is read, the same for a
// 16-byte unit of four columns with its lanes put back in output order, and the balanced summation tree.  One text for the kernels
// (misc_kernels.hip), for the entries' guards (emavfi_api.hip) and for the host check (tests/host/host_check_ensemble.cpp, a plain C++
// program).  The tree is plain fp32 `+` and one `*`: every user is compiled with contraction off and without fast-math, and there is no
// multiply-add to contract in it anyway.
#pragma once

#ifdef __HIP__
#define ENSEMBLE_HD __host__ __device__
#else
#define ENSEMBLE_HD
#endif

constexpr int ENSEMBLE_FLIP_H = 1;        // EMAVFI_FLIP_H: column x reads column W - 1 - x
constexpr int ENSEMBLE_FLIP_V = 2;        // EMAVFI_FLIP_V: row y reads row H - 1 - y
constexpr int ENSEMBLE_MAX_MEMBERS = 8;   // EMAVFI_ENSEMBLE_MAX_MEMBERS

ENSEMBLE_HD inline bool ensemble_flip_ok(int flip) { return flip >= 0 && flip <= (ENSEMBLE_FLIP_H | ENSEMBLE_FLIP_V); }
ENSEMBLE_HD inline bool ensemble_count_ok(int n) { return n == 1 || n == 2 || n == 4 || n == 8; }

// the element of a [H][W] plane (H * W <= 2^28) that output position (y, x) reads through `flip`
ENSEMBLE_HD inline int ensemble_src_index(int y, int x, int H, int W, int flip)
{
    const int sy = (flip & ENSEMBLE_FLIP_V) ? H - 1 - y : y, sx = (flip & ENSEMBLE_FLIP_H) ? W - 1 - x : x;
    return sy * W + sx;
}
// the same for the unit of output columns 4 q .. 4 q + 3 of a plane of Wq = W / 4 units per row: under an H flip that is the mirrored unit,
// whose four lanes ensemble_lanes() puts back in output order
ENSEMBLE_HD inline int ensemble_src_unit(int y, int q, int H, int Wq, int flip) { return ensemble_src_index(y, q, H, Wq, flip); }
struct EnsembleUnit { float x, y, z, w; };
ENSEMBLE_HD inline EnsembleUnit ensemble_lanes(EnsembleUnit v, int flip) { return (flip & ENSEMBLE_FLIP_H) ? EnsembleUnit{v.w, v.z, v.y, v.x} : v; }

// the mean of n in {1, 2, 4, 8} member values, in the order given: a balanced pairwise tree of fp32 additions, then ONE multiplication by the
// exact constant 1 / n (n = 1: the value itself).  Do not reassociate: the pairing is what the definition's symmetry arguments rest on.
ENSEMBLE_HD inline float ensemble_mean(const float *m, int n)
{
    if (n == 1) return m[0];
    if (n == 2) return (m[0] + m[1]) * 0.5f;
    if (n == 4) return ((m[0] + m[1]) + (m[2] + m[3])) * 0.25f;
    return (((m[0] + m[1]) + (m[2] + m[3])) + ((m[4] + m[5]) + (m[6] + m[7]))) * 0.125f;
}
