// The per-element functions of the scene-cut definition (include/emavfi.h, "SCENE CUT DEFINITION"): cell bound, luma, cell mean.
// One text for the kernels (misc_kernels.hip) and for the host check (tests/host/host_check_scene.cpp, a plain C++ program): all integer.
#pragma once

#ifdef __HIP__
#define SCENE_HD __host__ __device__
#else
#define SCENE_HD
#endif

constexpr int SCENE_GRID = 32;   // EMAVFI_SCENE_GRID

// first row / column of cell i along an axis of n pixels: floor(i n / 32); cell i covers [bound(i), bound(i + 1)); i n <= 32 * 16384
SCENE_HD inline int scene_cell_bound(int i, int n) { return (i * n) / SCENE_GRID; }
// luma of one 3-byte pixel: the BT.601 full-range encode row {313524, 615514, 119538} (sum 2^20: 0..255, no clip); rgb: byte 0 is R
SCENE_HD inline unsigned scene_luma3(unsigned c0, unsigned c1, unsigned c2, int rgb)
{
    const unsigned r = rgb ? c0 : c2, b = rgb ? c2 : c0;
    return (313524u * r + 615514u * c1 + 119538u * b + (1u << 19)) >> 20;
}
// mean of a cell of n >= 1 pixels in sixteenths of a count, rounded: 0..4080 (16 sum + n / 2 < 2^31 for the largest cell, 512 x 512)
SCENE_HD inline unsigned scene_cell_mean(unsigned sum, unsigned n) { return (16u * sum + n / 2u) / n; }
