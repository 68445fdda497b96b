// The per-element functions of the static region definition (include/emavfi.h, "STATIC REGION DEFINITION"): the sample of a word, the
// within-tolerance test, the chroma-core rule, the clipped window bounds and the planes of a dense frame.  One text for the kernel
// (misc_kernels.hip), for the entry's guards (emavfi_api.hip) and for the host check (tests/host/host_check_static.cpp, a plain C++
// program): all integer.
#pragma once

#include <stddef.h>

#ifdef __HIP__
#define STATIC_HD __host__ __device__
#else
#define STATIC_HD
#endif

constexpr int STATIC_MAX_RADIUS = 16;           // EMAVFI_STATIC_MAX_RADIUS
constexpr int STATIC_CAP = 64;                  // table entries per launch (EMAVFI_RESAMPLE_LAUNCH_CAP)
constexpr int STATIC_LAYOUT_INTERLEAVED = 0;    // EMAVFI_LAYOUT_INTERLEAVED: [H][W][C]
constexpr int STATIC_LAYOUT_NV12 = 1;           // EMAVFI_LAYOUT_NV12: [H][W] Y, then [H/2][W/2] pairs {U, V}
constexpr int STATIC_LAYOUT_I420 = 2;           // EMAVFI_LAYOUT_I420: [H][W] Y, then [H/2][W/2] U, then [H/2][W/2] V

// the sample of one element: a byte (mask 255, shift 0) or the depth-bit value of a 16-bit little-endian word
STATIC_HD inline unsigned static_sample(unsigned word, unsigned mask, int shift) { return (word >> shift) & mask; }
// |sa - sb| <= tol for two samples <= 65535
STATIC_HD inline bool static_within(unsigned sa, unsigned sb, unsigned tol) { return (sa > sb ? sa - sb : sb - sa) <= tol; }
// a chroma sample of a 4:2:0 frame is replaced exactly when all four luma pixels it covers are core
STATIC_HD inline bool static_chroma_core(bool c00, bool c01, bool c10, bool c11) { return c00 && c01 && c10 && c11; }
// the window of radius r around position p of an axis of n positions, clipped to the frame: [lo, hi], both inclusive
STATIC_HD inline int static_window_lo(int p, int r) { return p - r > 0 ? p - r : 0; }
STATIC_HD inline int static_window_hi(int p, int r, int n) { return p + r < n - 1 ? p + r : n - 1; }

// One plane of a dense frame: `rows` rows of `samples` samples, `offset` BYTES into the frame.  Sample s of row i belongs to plane pixel
// (i, s / div); sub = 0: that IS luma pixel (i, s / div); sub = 1 (4:2:0 chroma): it covers the luma pixels (2 i + {0, 1}, 2 (s / div) + {0, 1}).
struct StaticPlane { size_t offset; int rows, samples, div, sub; };

// the planes of a frame (validated arguments: a known layout, even H and W at 4:2:0); returns their number, *frame_bytes = the dense frame
STATIC_HD inline int static_planes(int layout, int C, int H, int W, int sample_bytes, StaticPlane (&pl)[3], size_t *frame_bytes)
{
    const size_t sb = (size_t)sample_bytes, luma = (size_t)H * W * sb;
    if (layout == STATIC_LAYOUT_INTERLEAVED) {
        pl[0] = StaticPlane{0, H, W * C, C, 0};
        *frame_bytes = luma * C;
        return 1;
    }
    pl[0] = StaticPlane{0, H, W, 1, 0};
    *frame_bytes = luma + luma / 2;
    if (layout == STATIC_LAYOUT_NV12) {
        pl[1] = StaticPlane{luma, H / 2, W, 2, 1};
        return 2;
    }
    pl[1] = StaticPlane{luma, H / 2, W / 2, 1, 1};
    pl[2] = StaticPlane{luma + luma / 4, H / 2, W / 2, 1, 1};
    return 3;
}
