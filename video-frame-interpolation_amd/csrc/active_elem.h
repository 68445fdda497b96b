// The per-element functions of the active area definition (include/emavfi.h, "ACTIVE AREA DEFINITION"): the sample of a word, the content
// test, the bounds of a frame and how a pixel widens them, the rectangle of a set of bounds, and the part of a plane of a dense frame that
// a rectangle covers.  One text for the kernels (misc_kernels.hip), for the entries' guards (emavfi_api.hip) and for the host check
// (tests/host/host_check_active.cpp, a plain C++ program): all integer.  The planes of a frame are static_elem.h's.
#pragma once

#include "static_elem.h"

#ifdef __HIP__
#define ACTIVE_HD __host__ __device__
#else
#define ACTIVE_HD
#endif

constexpr int ACTIVE_CAP = 64;          // table entries per launch (EMAVFI_RESAMPLE_LAUNCH_CAP)
constexpr int ACTIVE_ALIGN_Y = 2;       // a rectangle's top and bottom: whole 4:2:0 chroma rows
constexpr int ACTIVE_ALIGN_X = 16;      // its left and right: whole 16-byte units at every sample size

// the sample of one element: a byte (mask 255, shift 0) or the depth-bit value of a 16-bit little-endian word
ACTIVE_HD inline unsigned active_sample(unsigned word, unsigned mask, int shift) { return (word >> shift) & mask; }
// a sample is content when it is GREATER than the level
ACTIVE_HD inline bool active_content(unsigned sample, unsigned level) { return sample > level; }

// {top, bottom, left, right} of a frame: rows [top, bottom) and columns [left, right) hold its content; no content: {H, 0, W, 0}
struct ActiveBounds { unsigned top, bottom, left, right; };
ACTIVE_HD inline ActiveBounds active_none(int H, int W) { return ActiveBounds{(unsigned)H, 0u, (unsigned)W, 0u}; }
ACTIVE_HD inline void active_mark(ActiveBounds &b, int y, int x)
{
    const unsigned uy = (unsigned)y, ux = (unsigned)x;
    if (uy < b.top) b.top = uy;
    if (uy + 1u > b.bottom) b.bottom = uy + 1u;
    if (ux < b.left) b.left = ux;
    if (ux + 1u > b.right) b.right = ux + 1u;
}
ACTIVE_HD inline void active_join(ActiveBounds &b, const ActiveBounds &o)
{
    if (o.top < b.top) b.top = o.top;
    if (o.bottom > b.bottom) b.bottom = o.bottom;
    if (o.left < b.left) b.left = o.left;
    if (o.right > b.right) b.right = o.right;
}
ACTIVE_HD inline bool active_is_empty(const ActiveBounds &b) { return b.bottom <= b.top || b.right <= b.left; }

// the rectangle of a union of bounds: grown outward to multiples of 2 (rows) and 16 (columns), clipped to the frame; an empty union or a
// rectangle that covers the frame is the whole frame.  Returns {top, bottom, left, right}.
ACTIVE_HD inline ActiveBounds active_rect(const ActiveBounds &u, int H, int W)
{
    const ActiveBounds whole{0u, (unsigned)H, 0u, (unsigned)W};
    if (active_is_empty(u)) return whole;
    ActiveBounds r;
    r.top = u.top / ACTIVE_ALIGN_Y * ACTIVE_ALIGN_Y;
    r.left = u.left / ACTIVE_ALIGN_X * ACTIVE_ALIGN_X;
    r.bottom = (u.bottom + ACTIVE_ALIGN_Y - 1) / ACTIVE_ALIGN_Y * ACTIVE_ALIGN_Y;
    r.right = (u.right + ACTIVE_ALIGN_X - 1) / ACTIVE_ALIGN_X * ACTIVE_ALIGN_X;
    if (r.bottom > (unsigned)H) r.bottom = (unsigned)H;
    if (r.right > (unsigned)W) r.right = (unsigned)W;
    return r;
}

// what a rectangle (top, left, height, width) of luma pixels covers of one plane: rows [r0, r1), BYTES [c0, c1) of each of those rows.  A
// 4:2:0 chroma sample belongs to the rectangle exactly when its 2 x 2 luma block does: the rectangle's edges are even there.
struct ActiveSpan { int r0, r1, c0, c1; };
ACTIVE_HD inline ActiveSpan active_plane_span(const StaticPlane &pl, int sample_bytes, int top, int left, int height, int width)
{
    return ActiveSpan{top >> pl.sub, (top + height) >> pl.sub, (left >> pl.sub) * pl.div * sample_bytes,
                      ((left + width) >> pl.sub) * pl.div * sample_bytes};
}
// byte `c` of row `r` of the plane lies inside the rectangle
ACTIVE_HD inline bool active_inside(const ActiveSpan &s, int r, int c) { return r >= s.r0 && r < s.r1 && c >= s.c0 && c < s.c1; }
