// The per-element functions of the agreement guard definition (include/emavfi.h, "AGREEMENT GUARD DEFINITION"): whether a sample of the two
// time directions is flagged, the value of a pixel that is kept and the value of a pixel that is held.  The clipped window and its largest
// radius are the static guard's (static_elem.h: static_window_lo / static_window_hi, STATIC_MAX_RADIUS).  One text
// for the kernel (misc_kernels.hip), for the entry's guards (emavfi_api.hip) and for the host check (tests/host/host_check_agreement.cpp, a
// plain C++ program).  Plain fp32 `-`, `+`, `*` and comparisons: every user is compiled with contraction off and without fast-math, and the
// one place a multiply-add could be contracted (agreement_fallback) switches contraction off itself as well.
#pragma once

#include "static_elem.h"

#ifdef __HIP__
#define AGREEMENT_HD __host__ __device__
#else
#define AGREEMENT_HD
#endif

constexpr int AGREEMENT_MAX_BATCH = 65535;  // EMAVFI_AGREEMENT_MAX_BATCH: a sample is one slice of the grid

// 0 <= tol <= 1; false for a NaN
AGREEMENT_HD inline bool agreement_tol_ok(float tol) { return tol >= 0.0f && tol <= 1.0f; }
// a divisor of the de-normalisation that is neither zero nor non-finite (a NaN fails the first comparison)
AGREEMENT_HD inline bool agreement_std_ok(float s) { return (s > 0.0f || s < 0.0f) && s - s == 0.0f; }

// d = |u - v|: one IEEE subtraction, then the sign bit cleared
AGREEMENT_HD inline float agreement_disagreement(float u, float v) { return __builtin_fabsf(u - v); }
// NOT (d <= tol): a NaN in u or v flags the sample
AGREEMENT_HD inline bool agreement_flagged(float u, float v, float tol) { return !(agreement_disagreement(u, v) <= tol); }
// a pixel that is not held: the mean of the two time directions, one addition and one exact multiplication
AGREEMENT_HD inline float agreement_kept(float u, float v) { return (u + v) * 0.5f; }
// a held pixel: the blend of the two normalised sources, de-normalised and clamped to [0, 1]; a NaN stays a NaN (both comparisons fail)
AGREEMENT_HD inline float agreement_fallback(float a, float b, float mean, float std)
{
#pragma clang fp contract(off)
    const float h = (a + b) * 0.5f;
    float t = h * std;
    t = t + mean;
    return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
}
