// What the planar 4:2:0 formats (include/emavfi.h, "PLANAR 4:2:0") add to the per-element functions of NV12 / P010: where a sample sits.
// One text for the kernels (misc_kernels.hip: preprocess_yuv420_kernel / postprocess_yuv420_kernel, whose four formats - planar and interleaved,
// bytes and words - all read and write a row piece through yuv420p_get / yuv420p_put) and for the host check
// (tests/host/host_check_yuv420p.cpp, a plain C++ program).  The colour arithmetic itself is not here: the kernels call nv12_* (depth 8) and
// p010_elem.h (above) on the samples these functions hand them.
#pragma once
#include "p010_elem.h"

// the sample of a planar word: its LOW `depth` bits (P = 2^depth - 1 is the mask); a byte at depth 8
P010_HD inline int yuv420p_sample(unsigned word, int P) { return (int)(word & (unsigned)P); }
// sample `idx` of a row piece held as little-endian dwords, BITS = 8 or 16 per sample: read whole, written into zeroed dwords
template <int BITS> P010_HD inline unsigned yuv420p_get(const unsigned *w, int idx)
{
    constexpr int PER = 32 / BITS;
    return (w[idx / PER] >> (BITS * (idx % PER))) & (0xffffffffu >> (32 - BITS));
}
template <int BITS> P010_HD inline void yuv420p_put(unsigned *w, int idx, unsigned v)
{
    constexpr int PER = 32 / BITS;
    w[idx / PER] |= v << (BITS * (idx % PER));
}
