// The per-element functions of the coarse flow definition (include/emavfi.h, "COARSE FLOW DEFINITION"): the balanced quadtree mean of an
// s x s block of clamped leaves (step 1, down_s), the per-axis bilinear tap at half-pixel centres and the scaled sample (step 3), and the
// validity predicates of s and of a dimension.  One text for the kernels (misc_kernels.hip), for the entries' guards (emavfi_api.hip)
// and for the host check (tests/host/host_check_coarse.cpp, a plain C++ program).  IEEE fp32, no contraction: the translation units that
// include this for arithmetic are built with -ffp-contract=off.
#pragma once

#ifdef __HIP__
#define COARSE_HD __host__ __device__
#else
#define COARSE_HD
#endif

constexpr int COARSE_MAX_DIM = 16384;   // every dimension of the fine and of the coarse tensor lies in 1..16384

COARSE_HD inline bool coarse_scale_ok(int s) { return s == 2 || s == 4 || s == 8; }
COARSE_HD inline bool coarse_dim_ok(int d) { return d >= 1 && d <= COARSE_MAX_DIM; }
// Hs = ceil(H / s)
COARSE_HD inline int coarse_dim(int n, int s) { return (n + s - 1) / s; }

// ---- step 1.  T_M(r, c) over leaves leaf(r, c), r and c counted in leaves of the block:
//   T_1 = L,  T_2m(r, c) = ((T_m(2r, 2c) + T_m(2r, 2c+1)) + (T_m(2r+1, 2c) + T_m(2r+1, 2c+1))) * 0.25f.
// `leaf` is any callable (row, column) -> float: the clamped global load of the scalar path, a register tile of the wide one.
template <int M, class Leaf>
COARSE_HD inline float coarse_tree(const Leaf &leaf, int r, int c)
{
    if constexpr (M == 1) {
        return leaf(r, c);
    } else {
        constexpr int h = M / 2;
        const float top = coarse_tree<h>(leaf, 2 * r, 2 * c) + coarse_tree<h>(leaf, 2 * r, 2 * c + 1);
        const float bot = coarse_tree<h>(leaf, 2 * r + 1, 2 * c) + coarse_tree<h>(leaf, 2 * r + 1, 2 * c + 1);
        return (top + bot) * 0.25f;
    }
}
// (coarse_tree<M>(leaf, r, c) addresses leaves r M .. r M + M - 1: T_m's indices count blocks of m leaves, the recursion turns them into
// leaf indices by doubling on the way down)

// the leaves of block (i, j) of a [H][W] plane, clamped once, at the leaves: an edge block still has s^2 of them
struct CoarseClampedLeaf {
    const float *plane;
    int H, W, y0, x0;   // y0 = s i, x0 = s j
    COARSE_HD float operator()(int r, int c) const
    {
        const int y = y0 + r < H - 1 ? y0 + r : H - 1, x = x0 + c < W - 1 ? x0 + c : W - 1;
        return plane[(size_t)y * W + x];
    }
};
template <int S>
COARSE_HD inline float coarse_down_elem_s(const float *plane, int H, int W, int i, int j)
{
    return coarse_tree<S>(CoarseClampedLeaf{plane, H, W, S * i, S * j}, 0, 0);
}
// down_s at coarse position (i, j) (s already valid)
COARSE_HD inline float coarse_down_elem(const float *plane, int H, int W, int s, int i, int j)
{
    return s == 2 ? coarse_down_elem_s<2>(plane, H, W, i, j) : s == 4 ? coarse_down_elem_s<4>(plane, H, W, i, j) : coarse_down_elem_s<8>(plane, H, W, i, j);
}

// ---- step 3.  One axis: destination index d, coarse length n.  num = 2 d + 1 - s >= 1 - s, i0 = floor(num / (2 s)) >= -1,
// w = (num - 2 s i0) / (2 s): a quotient of an integer below 2 s by a power of two, so the multiplication by the exact reciprocal IS
// the division; j0 = clamp(i0), j1 = clamp(i0 + 1).
struct CoarseTap { int j0, j1; float w; };
COARSE_HD inline float coarse_inv2s(int s) { return s == 2 ? 0.25f : s == 4 ? 0.125f : 0.0625f; }
COARSE_HD inline CoarseTap coarse_up_tap(int d, int n, int s)
{
    const int num = 2 * d + 1 - s, i0 = num >= 0 ? num / (2 * s) : -1;
    CoarseTap t;
    t.w = (float)(num - 2 * s * i0) * coarse_inv2s(s);
    t.j0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
    t.j1 = i0 + 1 > n - 1 ? n - 1 : i0 + 1;
    return t;
}
// flow_up at (y, x) of one coarse [Hs][Ws] plane: top, bot, v in the definition's order, then (float)s * v
COARSE_HD inline float coarse_up_elem(const float *p, int Ws, const CoarseTap &ty, const CoarseTap &tx, int s)
{
    const float *r0 = p + (size_t)ty.j0 * Ws, *r1 = p + (size_t)ty.j1 * Ws;
    const float top = (1.0f - tx.w) * r0[tx.j0] + tx.w * r0[tx.j1];
    const float bot = (1.0f - tx.w) * r1[tx.j0] + tx.w * r1[tx.j1];
    const float v = (1.0f - ty.w) * top + ty.w * bot;
    return (float)s * v;
}
