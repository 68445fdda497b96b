// The per-element functions of the border definition (include/emavfi.h, "BORDER DEFINITION"): which sample of an axis of n samples position i
// of the extended axis reads (i in -N .. n - 1 + N), for both modes, where a cropped position reads, and the validity predicates of N, mode
// and a dimension.  One text for the kernels (misc_kernels.hip), for the entries' guards (emavfi_api.hip) and for the host check
// (tests/host/host_check_border.cpp, a plain C++ program).  Integer arithmetic only: pad and crop move words, they compute nothing.
#pragma once

#ifdef __HIP__
#define BORDER_HD __host__ __device__
#else
#define BORDER_HD
#endif

constexpr int BORDER_REPLICATE = 0;   // EMAVFI_BORDER_REPLICATE: i -> min(max(i, 0), n - 1)
constexpr int BORDER_REFLECT = 1;     // EMAVFI_BORDER_REFLECT: mirrored about the edge sample, which is not repeated; periodic in 2 (n - 1)
constexpr int BORDER_MAX = 64;        // EMAVFI_BORDER_MAX
constexpr int BORDER_MAX_DIM = 16384; // every dimension of the picture and of the extended picture lies in 1..16384

BORDER_HD inline bool border_mode_ok(int mode) { return mode == BORDER_REPLICATE || mode == BORDER_REFLECT; }
BORDER_HD inline bool border_n_ok(int N) { return N >= 0 && N <= BORDER_MAX; }
BORDER_HD inline bool border_dim_ok(int d) { return d >= 1 && d <= BORDER_MAX_DIM; }
// the extended length of an axis of n samples (n, N already valid: at most 16384 + 128)
BORDER_HD inline int border_padded_dim(int n, int N) { return n + 2 * N; }

BORDER_HD inline int border_replicate_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
// p = 2 (n - 1), m = ((i mod p) + p) mod p, the sample is m where m <= n - 1 and p - m beyond: defined for any i, so for N > n - 1 too
// (several reflections); n = 1 has one sample.  Inside the picture m = i: the test in front only spares the two divisions.
BORDER_HD inline int border_reflect_index(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1), m = ((i % p) + p) % p;
    return m <= n - 1 ? m : p - m;
}
BORDER_HD inline int border_index(int i, int n, int mode) { return mode == BORDER_REFLECT ? border_reflect_index(i, n) : border_replicate_index(i, n); }
// crop_N: position i of the picture's axis reads position i + N of the extended axis
BORDER_HD inline int border_crop_index(int i, int N) { return i + N; }

// the element of a source [Hs][Ws] plane that destination position (y, x) reads.  Pad (crop = false): the source is the picture, the
// destination its extension by N.  Crop: the source is the extended picture (Hs = H + 2 N, Ws = W + 2 N), `mode` is not looked at.
BORDER_HD inline int border_src_index(int y, int x, int Hs, int Ws, int N, int mode, bool crop)
{
    const int sy = crop ? border_crop_index(y, N) : border_index(y - N, Hs, mode);
    const int sx = crop ? border_crop_index(x, N) : border_index(x - N, Ws, mode);
    return sy * Ws + sx;
}
// whether the four destination columns x .. x + 3 read four CONSECUTIVE source columns starting at *sx0 (the unit lies wholly inside the
// picture; always so for a crop): what a 16-byte load needs besides an aligned address
BORDER_HD inline bool border_unit_inside(int x, int Ws, int N, bool crop, int *sx0)
{
    *sx0 = crop ? border_crop_index(x, N) : x - N;
    return *sx0 >= 0 && *sx0 + 3 <= Ws - 1;
}
