// The per-element functions of the duplicate-frame definition (include/emavfi.h, "DUPLICATE FRAME DEFINITION"): the sample of a word, the
// absolute difference of two lumas, a cell's measure.  One text for the kernels (misc_kernels.hip) and for the host check
// (tests/host/host_check_dedup.cpp, a plain C++ program): all integer.  The cells and the 3-byte luma are scene_elem.h's.
#pragma once

#ifdef __HIP__
#define DEDUP_HD __host__ __device__
#else
#define DEDUP_HD
#endif

constexpr int DEDUP_CELLS = 1024;   // EMAVFI_SCENE_SIG_WORDS: the 32 x 32 cells of the scene grid

// the sample of one element: a byte (mask 255, shift 0) or the depth-bit value of a 16-bit little-endian word
DEDUP_HD inline unsigned dedup_sample(unsigned word, unsigned mask, int shift) { return (word >> shift) & mask; }
// |a - b| of two lumas <= 65535
DEDUP_HD inline unsigned dedup_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }
// m of a cell of n >= 1 pixels: the ceiling of its mean absolute difference in sixteenths of a count; sad <= 65535 * 2^18, so 16 sad + n - 1
// < 2^39 needs 64 bits and the quotient, at most 16 * 65535 = 1 048 560, fits u32.  m = 0 exactly when sad = 0.
DEDUP_HD inline unsigned dedup_cell_measure(unsigned long long sad, unsigned n) { return (unsigned)((16ull * sad + (n - 1u)) / n); }
