// HBM-bound helper kernels of libemavfi: weight packing, layout conversion at the NCHW
// boundary, global-average-pool + context folding, and the backward bilinear warp.
#include "common.h"
#include "misc_kernels.h"
#include "scene_elem.h"
#include "resample_elem.h"
#include "shutter_elem.h"
#include "light_elem.h"
#include "dedup_elem.h"
#include "static_elem.h"
#include "active_elem.h"
#include "ensemble_elem.h"
#include "border_elem.h"
#include "align_elem.h"
#include "coarse_elem.h"
#include "agreement_elem.h"
#include "metrics_elem.h"
#include "p010_elem.h"
#include "yuv420p_elem.h"
#include <atomic>
#include <type_traits>
#include <cstddef>
#include <cstdlib>

int device_cu_count()
{
    static std::atomic<int> cache[64];  // zero-initialised; a racing first call just queries twice
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -1;
    if (dev < 64) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return -1;
    if (dev < 64) cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// ------------------------------------------------------------------------------------------
// Weight packing: OIHW fp32 -> [pass][chunk][tap][kg][nf][lane][16 B] in MFMA operand order.
// Lane (r, h) of fragment nf holds output channel pass*NF*32 + nf*32 + r and input channels
// chunk*CK + kg*CHKG + h*EPV + e (e < EPV).  Everything outside the real tensor packs as 0,
// which is what keeps the pad channels of every activation exactly zero.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int route_cout(int pos, int perm)
{
    // perm 1 = ModulatedDeformConvPack routing (ema_vfi.py:57-59): the 27 raw channels are
    // chunked (static offsets | mask | dynamic offsets); packed channel order is
    // [18 offsets = cat(first, third)] [9 mask].
    if (perm == 0) return pos;
    if (pos < 9) return pos;
    if (pos < 18) return pos + 9;
    if (pos < 27) return pos - 9;
    return 1 << 30;
}

template <typename T>
__global__ void pack_conv_kernel(const float *__restrict__ w, const float *__restrict__ bias, T *__restrict__ wp,
                                 float *__restrict__ bp, PackDesc d)
{
    constexpr int CHKG = DT<T>::CHKG, EPV = DT<T>::EPV;
    // the layouts beside the regular one (ConvRoute, common.h): fragments for v_mfma_f32_16x16x32, [tap][k32][cout16 block][lane (i, kb)][8 elements];
    const bool k32 = d.route == CONV_PERSIST16 || d.route == CONV_LIGHT, tail3 = d.route == CONV_RING_TAIL3;
    if (tail3) d.ck = 64;   // the main fragments take input channels 0..63, channels 64.. go to the tail below
    const int KG = d.ck / CHKG;
    const size_t total = (size_t)d.npass * d.nchunk * 9 * KG * d.nf * 64 * EPV;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t t = idx;
        const int e = t % EPV; t /= EPV;
        const int lane = t % 64; t /= 64;
        const int n = t % d.nf; t /= d.nf;
        const int kg = t % KG; t /= KG;
        const int tap = t % 9; t /= 9;
        const int chunk = t % d.nchunk; t /= d.nchunk;
        const int pass = (int)t;
        int co = route_cout(pass * d.nf * 32 + n * 32 + (lane & 31), d.perm);
        int ci = chunk * d.ck + kg * CHKG + (lane >> 5) * EPV + e;
        if (k32) {   // same number of elements, regrouped: (kg, n) enumerates (k32, cout16 block) = KG * nf = (KG / 2) * (2 nf)
            const int flat = kg * d.nf + n, nb16 = 2 * d.nf, k32 = flat / nb16, blk = flat - k32 * nb16;
            co = route_cout(pass * d.nf * 32 + blk * 16 + (lane & 15), d.perm);
            ci = chunk * d.ck + k32 * 32 + (lane >> 4) * 8 + e;
        }
        int term = 0;
        if (d.x3) {   // virtual chunk 3 c + t -> real chunk c
            const int rc = chunk / 3;
            term = chunk - 3 * rc;
            ci = rc * d.ck + kg * CHKG + (lane >> 5) * EPV + e;
        }
        float v = 0.0f;
        if (co < d.cout && ci < d.cin_take && ci < d.ck * (d.x3 ? d.nchunk / 3 : d.nchunk)) v = w[((size_t)co * d.cin_raw + d.cin_off + ci) * 9 + tap];
        if (d.via_bf16) v = (float)(bf16_t)v;
        if (term == 1) v = v - (float)(T)v;   // the lo part of the weight
        wp[idx] = (T)v;
    }
    if (tail3 && EPV == 8) {
        for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)3 * 2 * 64 * 8; idx += (size_t)gridDim.x * blockDim.x) {
            size_t t = idx;
            const int e = t % 8; t /= 8;
            const int lane = t % 64; t /= 64;
            const int n = t % 2; t /= 2;
            const int j = (int)t;
            const int ts = 4 * j + 2 * (lane >> 5) + (e >> 2), ci = 64 + (e & 3), co = n * 32 + (lane & 31);
            float v = 0.0f;
            if (ts < 9 && ci < d.cin_take && co < d.cout) v = w[((size_t)co * d.cin_raw + d.cin_off + ci) * 9 + ts];
            wp[total + idx] = (T)v;
        }
    }
    if (d.first6 && EPV == 8) {   // a second copy behind the regular fragments: conv_first.inl's ten tap slots of 8
        for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)5 * 2 * 64 * 8; idx += (size_t)gridDim.x * blockDim.x) {
            size_t t = idx;
            const int e = t % 8; t /= 8;
            const int lane = t % 64; t /= 64;
            const int n = t % 2; t /= 2;
            const int kg = (int)t;
            const int tap = 2 * kg + (lane >> 5), co = n * 32 + (lane & 31);
            float v = 0.0f;
            if (tap < 9 && e < d.cin_take && co < d.cout) v = w[((size_t)co * d.cin_raw + d.cin_off + e) * 9 + tap];
            wp[total + idx] = (T)v;
        }
    }
    const int coutpad = d.npass * d.nf * 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < coutpad; i += gridDim.x * blockDim.x) {
        const int co = route_cout(i, d.perm);
        float bv = (co < d.cout && bias) ? bias[co] : 0.0f;
        if (d.bias_f16) bv = (float)(half_t)bv;
        bp[i] = bv;
    }
}

// deform_pack3.inl layouts (always f16 elements; via_bf16 rounds to bf16 first).  Input channels 0..63 are four k-groups per
// tap; channels 64..66 of all nine taps form three im2col k-groups: K = 16 j + 8 h + e <-> tap slot 4 j + 2 h + (e >> 2),
// channel 64 + (e & 3) (slots 9..11 and channel 67 are zero).
//   pack3 = 1 (DCN):          [tap][kg 4][nf 2][lane][8] | third fragment as a table [tap][kg 4][row 0..3][h][8] (row 3 = zeros)
//                             | tail [j 3][nf 3][lane][8]
//   pack3 = 2 (offset_conv):  [tap][kg 4][lane][8] | tail [j 3][lane][8]
__global__ void pack_deform3_kernel(const float *__restrict__ w, const float *__restrict__ bias, half_t *__restrict__ wp,
                                    float *__restrict__ bp, PackDesc d)
{
    const int nA = d.pack3 == 1 ? 9 * 4 * 2 * 64 * 8 : 9 * 4 * 64 * 8;
    const int nB = d.pack3 == 1 ? 9 * 4 * 4 * 2 * 8 : 0;
    const int nC = d.pack3 == 1 ? 3 * 3 * 64 * 8 : 3 * 64 * 8;
    const int nfm = d.pack3 == 1 ? 2 : 1, nft = d.pack3 == 1 ? 3 : 1;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nA + nB + nC; idx += gridDim.x * blockDim.x) {
        int co, ci, tap;
        bool real = true;
        if (idx < nA) {
            int t = idx;
            const int e = t % 8; t /= 8;
            const int lane = t % 64; t /= 64;
            const int n = t % nfm; t /= nfm;
            const int kg = t % 4; t /= 4;
            tap = t;
            co = n * 32 + (lane & 31);
            ci = kg * 16 + (lane >> 5) * 8 + e;
        } else if (idx < nA + nB) {
            int t = idx - nA;
            const int e = t % 8; t /= 8;
            const int hh = t % 2; t /= 2;
            const int row = t % 4; t /= 4;
            const int kg = t % 4; t /= 4;
            tap = t;
            co = 64 + row;
            real = row < 3;
            ci = kg * 16 + hh * 8 + e;
        } else {
            int t = idx - nA - nB;
            const int e = t % 8; t /= 8;
            const int lane = t % 64; t /= 64;
            const int n = t % nft; t /= nft;
            const int j = t;
            tap = 4 * j + 2 * (lane >> 5) + (e >> 2);
            co = n * 32 + (lane & 31);
            ci = 64 + (e & 3);
            real = tap < 9 && (e & 3) < 3;
            if (!real) tap = 0;
        }
        co = route_cout(co, d.perm);
        float v = 0.0f;
        if (real && co < d.cout && ci < d.cin_take) v = w[((size_t)co * d.cin_raw + d.cin_off + ci) * 9 + tap];
        if (d.via_bf16) v = (float)(bf16_t)v;
        wp[idx] = (half_t)v;
    }
    const int coutpad = d.npass * d.nf * 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < coutpad; i += gridDim.x * blockDim.x) {
        const int co = route_cout(i, d.perm);
        float bv = (co < d.cout && bias) ? bias[co] : 0.0f;
        if (d.bias_f16) bv = (float)(half_t)bv;
        bp[i] = bv;
    }
}

// deform_f32w.inl layout (fp32, 67 -> <= 80 channels): [tap][half 2][cout block 5]{ group 0: [lane][4] | group 1: [lane][4] |
// leftover: [lane][1] }; lane (i = lane & 15, kb = lane >> 4) of a group holds W[16 c + i][36 half + 16 G + 4 kb + t] for the
// group's four MFMA steps t = 0..3 (step t contracts the channel set {16 G + 4 kb' + t}: the order in which a lane's 16-byte
// gather piece feeds the steps), the leftover step W[16 c + i][36 half + 32 + kb].
__global__ void pack_deform_f32w_kernel(const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ wp,
                                        float *__restrict__ bp, PackDesc d)
{
    constexpr int CB = 64 * 4 * 2 + 64, HALF = 5 * CB, TAP = 2 * HALF;   // floats
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < 9 * TAP; idx += gridDim.x * blockDim.x) {
        int t = idx;
        const int tap = t / TAP; t -= tap * TAP;
        const int half = t / HALF; t -= half * HALF;
        const int c = t / CB; t -= c * CB;
        int lane, ci;
        if (t < 512) { const int G = t / 256, r = t - G * 256; lane = r >> 2; ci = 36 * half + 16 * G + 4 * (lane >> 4) + (r & 3); }
        else { lane = t - 512; ci = 36 * half + 32 + (lane >> 4); }
        const int co = 16 * c + (lane & 15);
        if (!d.x3) {
            wp[idx] = (co < d.cout && ci < d.cin_take) ? w[((size_t)co * d.cin_raw + d.cin_off + ci) * 9 + tap] : 0.0f;
            continue;
        }
        // EMAVFI_F32X3: the same bytes hold f16 (hi, lo) pairs - a lane's four floats become {hi[4], lo[4]}, the leftover float {hi, lo}:
        // float slot r of the lane's quad (r = 0..3) holds half elements (2 r, 2 r + 1) of that 8-half vector
        half_t *hp = reinterpret_cast<half_t *>(wp + idx);
        auto wval = [&](int cin) { return (co < d.cout && cin < d.cin_take) ? w[((size_t)co * d.cin_raw + d.cin_off + cin) * 9 + tap] : 0.0f; };
        if (t < 512) {
            const int r = t & 3, cbase = ci - r;   // the quad's first channel
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = 2 * r + q;           // element of {hi0..hi3, lo0..lo3}
                const float v = wval(cbase + (e & 3));
                const half_t hi = (half_t)v;
                hp[q] = e < 4 ? hi : (half_t)(v - (float)hi);
            }
        } else {
            const float v = wval(ci);
            const half_t hi = (half_t)v;
            hp[0] = hi;
            hp[1] = (half_t)(v - (float)hi);
        }
    }
    const int coutpad = d.npass * d.nf * 32;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < coutpad; i += gridDim.x * blockDim.x) bp[i] = (i < d.cout && bias) ? bias[i] : 0.0f;
}

int launch_pack_conv(const float *w, const float *bias, void *wp, float *bp, const PackDesc &d, int dtype, hipStream_t s)
{
    if (d.pack3 == 3) {
        pack_deform_f32w_kernel<<<64, 256, 0, s>>>(w, bias, (float *)wp, bp, d);
        return (int)hipGetLastError();
    }
    if (d.pack3) {
        pack_deform3_kernel<<<64, 256, 0, s>>>(w, bias, (half_t *)wp, bp, d);
        return (int)hipGetLastError();
    }
    if (dtype == 0)
        pack_conv_kernel<float><<<256, 256, 0, s>>>(w, bias, (float *)wp, bp, d);
    else if (dtype == 2)
        pack_conv_kernel<half_t><<<256, 256, 0, s>>>(w, bias, (half_t *)wp, bp, d);
    else
        pack_conv_kernel<bf16_t><<<256, 256, 0, s>>>(w, bias, (bf16_t *)wp, bp, d);
    return (int)hipGetLastError();
}

// raw fp32 copies the context kernels need: Linear weight/bias, the context half of
// motion_estimation.0.0.weight as [o][c][tap], its bias.
__global__ void pack_ctx_kernel(const float *__restrict__ lin_w, const float *__restrict__ lin_b,
                                const float *__restrict__ w9, const float *__restrict__ b9, float *__restrict__ dst, int m, int round16)
{
    // round16: autocast casts Linear's and the convolution's weight and bias to fp16 (EMAVFI_AMP16)
    const auto rq = [round16](float v) { return round16 ? (float)(half_t)v : v; };
    float *o_lw = dst, *o_lb = o_lw + (size_t)m * 4 * m, *o_w9 = o_lb + m, *o_b9 = o_w9 + (size_t)m * m * 9;
    const int n_lw = m * 4 * m, n_w9 = m * m * 9;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lw + n_w9 + 2 * m; i += gridDim.x * blockDim.x) {
        if (i < n_lw) {   // Linear weight transposed to [c][o]: the threads of ctx_finish_kernel (one per o) read consecutive addresses
            const int c = i / m, o = i - c * m;
            o_lw[i] = rq(lin_w[(size_t)o * 4 * m + c]);
        } else if (i < n_lw + m) o_lb[i - n_lw] = rq(lin_b[i - n_lw]);
        else if (i < n_lw + m + n_w9) {   // context half of motion_estimation.0's weight as [c][o * 9 + tap]
            const int k = i - n_lw - m, c = k / (m * 9), rem = k - c * m * 9, o = rem / 9, tap = rem - o * 9;
            o_w9[k] = rq(w9[((size_t)o * 2 * m + m + c) * 9 + tap]);
        } else o_b9[i - n_lw - m - n_w9] = rq(b9[i - n_lw - m - n_w9]);
    }
}
int launch_pack_ctx(const float *lin_w, const float *lin_b, const float *w9, const float *b9, float *dst, int m, int round16,
                    hipStream_t s)
{
    pack_ctx_kernel<<<64, 256, 0, s>>>(lin_w, lin_b, w9, b9, dst, m, round16);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Layout conversion at the boundary.
// ------------------------------------------------------------------------------------------
// torch.cat([frame1, frame2], dim=1) (ema_vfi.py:112) fused with the NCHW -> channels-last pack.
template <typename T>
__global__ void pack_input_kernel(const float *__restrict__ f1, const float *__restrict__ f2, T *__restrict__ dst,
                                  int B, int C, int H, int W, int cpad)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        T *o = dst + i * cpad;
        if (cpad == 16) {  // the model's case (2*in_channels <= 16): one pixel = 16 channels, 16-byte stores
            float v[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                v[c] = 0.0f;
                if (c < C) v[c] = f1[(b * C + c) * plane + pix];
                else if (c < 2 * C) v[c] = f2[(b * C + (c - C)) * plane + pix];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) store4(o + 4 * q, v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            continue;
        }
        for (int c = 0; c < cpad; ++c) {
            float v = 0.0f;
            if (c < C) v = f1[(b * C + c) * plane + pix];
            else if (c < 2 * C) v = f2[(b * C + (c - C)) * plane + pix];
            o[c] = (T)v;
        }
    }
}
int launch_pack_input(const float *f1, const float *f2, void *dst, int B, int C, int H, int W, int cpad, int dtype, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    if (dtype == 0) pack_input_kernel<float><<<grid, 256, 0, s>>>(f1, f2, (float *)dst, B, C, H, W, cpad);
    else if (dtype == 2) pack_input_kernel<half_t><<<grid, 256, 0, s>>>(f1, f2, (half_t *)dst, B, C, H, W, cpad);
    else pack_input_kernel<bf16_t><<<grid, 256, 0, s>>>(f1, f2, (bf16_t *)dst, B, C, H, W, cpad);
    return (int)hipGetLastError();
}

template <typename T>
__global__ void nchw_to_cl_kernel(const float *__restrict__ src, T *__restrict__ dst, int B, int C, int c0, int ctake, int H, int W, int ps)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        T *o = dst + i * ps;
        for (int c = 0; c < ps; ++c) o[c] = (T)(c < ctake ? src[(b * C + c0 + c) * plane + pix] : 0.0f);
    }
}
template <typename T>
__global__ void cl_to_nchw_kernel(const T *__restrict__ src, float *__restrict__ dst, int B, int C, int H, int W, int ps, int coff)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        const T *o = src + i * ps + coff;
        for (int c = 0; c < C; ++c) dst[(b * C + c) * plane + pix] = (float)o[c];
    }
}
// EMAVFI_F32X3: fp32 <-> two f16 halves per pixel
__global__ void nchw_to_cl_x3_kernel(const float *__restrict__ src, half_t *__restrict__ dst, int B, int C, int H, int W, int psh)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        half_t *o = dst + i * 2 * psh;
        for (int c = 0; c < psh; ++c) {
            const float v = c < C ? src[(b * C + c) * plane + pix] : 0.0f;
            const half_t hi = (half_t)v;
            o[c] = hi;
            o[psh + c] = (half_t)(v - (float)hi);
        }
    }
}
__global__ void cl_to_nchw_x3_kernel(const half_t *__restrict__ src, float *__restrict__ dst, int B, int C, int H, int W, int psh, int coff)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        const half_t *o = src + i * 2 * psh + coff;
        for (int c = 0; c < C; ++c) dst[(b * C + c) * plane + pix] = (float)o[c] + (float)o[psh + c];
    }
}
int launch_nchw_to_cl_x3(const float *src, void *dst, int B, int C, int H, int W, int ps_half, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    nchw_to_cl_x3_kernel<<<grid, 256, 0, s>>>(src, (half_t *)dst, B, C, H, W, ps_half);
    return (int)hipGetLastError();
}
int launch_cl_to_nchw_x3(const void *src, float *dst, int B, int C, int H, int W, int ps_half, int coff, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    cl_to_nchw_x3_kernel<<<grid, 256, 0, s>>>((const half_t *)src, dst, B, C, H, W, ps_half, coff);
    return (int)hipGetLastError();
}
__global__ void pack_input_x3_kernel(const float *__restrict__ f1, const float *__restrict__ f2, half_t *__restrict__ dst, int B, int C, int H, int W, int cpad)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        half_t *o = dst + i * 2 * cpad;
        if (cpad == 16) {   // the model's case: 16-byte stores (the scalar loop below cost 1.1 ms at B = 8 x 720p)
            float v[16], l[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                v[c] = 0.0f;
                if (c < C) v[c] = f1[(b * C + c) * plane + pix];
                else if (c < 2 * C) v[c] = f2[(b * C + (c - C)) * plane + pix];
                l[c] = v[c] - (float)(half_t)v[c];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                store4(o + 4 * q, v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
                store4(o + 16 + 4 * q, l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]);
            }
            continue;
        }
        for (int c = 0; c < cpad; ++c) {
            float v = 0.0f;
            if (c < C) v = f1[(b * C + c) * plane + pix];
            else if (c < 2 * C) v = f2[(b * C + (c - C)) * plane + pix];
            const half_t hi = (half_t)v;
            o[c] = hi;
            o[cpad + c] = (half_t)(v - (float)hi);
        }
    }
}
int launch_pack_input_x3(const float *f1, const float *f2, void *dst, int B, int C, int H, int W, int cpad, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    pack_input_x3_kernel<<<grid, 256, 0, s>>>(f1, f2, (half_t *)dst, B, C, H, W, cpad);
    return (int)hipGetLastError();
}

int launch_nchw_to_cl_sub(const float *src, void *dst, int B, int C, int c0, int ctake, int H, int W, int ps, int dtype, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    if (dtype == 0) nchw_to_cl_kernel<float><<<grid, 256, 0, s>>>(src, (float *)dst, B, C, c0, ctake, H, W, ps);
    else if (dtype == 2) nchw_to_cl_kernel<half_t><<<grid, 256, 0, s>>>(src, (half_t *)dst, B, C, c0, ctake, H, W, ps);
    else nchw_to_cl_kernel<bf16_t><<<grid, 256, 0, s>>>(src, (bf16_t *)dst, B, C, c0, ctake, H, W, ps);
    return (int)hipGetLastError();
}
int launch_nchw_to_cl(const float *src, void *dst, int B, int C, int H, int W, int ps, int dtype, hipStream_t s)
{
    return launch_nchw_to_cl_sub(src, dst, B, C, 0, C, H, W, ps, dtype, s);
}
int launch_cl_to_nchw(const void *src, float *dst, int B, int C, int H, int W, int ps, int coff, int dtype, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    if (dtype == 0) cl_to_nchw_kernel<float><<<grid, 256, 0, s>>>((const float *)src, dst, B, C, H, W, ps, coff);
    else if (dtype == 2) cl_to_nchw_kernel<half_t><<<grid, 256, 0, s>>>((const half_t *)src, dst, B, C, H, W, ps, coff);
    else cl_to_nchw_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t *)src, dst, B, C, H, W, ps, coff);
    return (int)hipGetLastError();
}

// EMAVFI_AMP16 keeps the fusion tensor twice: fp32 (what the fp32 DCN reads and writes) and fp16 (what the fp16
// convolutions read).  One thread = 4 channels of one pixel.
template <bool WIDEN>
__global__ void convert_cl_kernel(const void *__restrict__ src, void *__restrict__ dst, size_t npx, int ps_src, int ps_dst, int c0, int nc, int lo_off)
{
    const int groups = nc / 4;
    const size_t total = npx * groups;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t px = i / groups;
        const int c = c0 + 4 * (int)(i - px * groups);
        if (WIDEN) {
            const f16x4 v = *reinterpret_cast<const f16x4 *>((const half_t *)src + px * ps_src + c);
            f32x4 o = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
            if (lo_off > 0) {
                const f16x4 l = *reinterpret_cast<const f16x4 *>((const half_t *)src + px * ps_src + lo_off + c);
                o = f32x4{o[0] + (float)l[0], o[1] + (float)l[1], o[2] + (float)l[2], o[3] + (float)l[3]};
            }
            *reinterpret_cast<f32x4 *>((float *)dst + px * ps_dst + c) = o;
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4 *>((const float *)src + px * ps_src + c);
            const f16x4 hi = f16x4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *reinterpret_cast<f16x4 *>((half_t *)dst + px * ps_dst + c) = hi;
            if (lo_off > 0)
                *reinterpret_cast<f16x4 *>((half_t *)dst + px * ps_dst + lo_off + c) =
                    f16x4{(half_t)(v[0] - (float)hi[0]), (half_t)(v[1] - (float)hi[1]), (half_t)(v[2] - (float)hi[2]), (half_t)(v[3] - (float)hi[3])};
        }
    }
}
// EMAVFI_F32X3, the model's case of the narrow conversion: 16 fp32 channels of every pixel -> their f16 (hi, lo) halves, one thread per
// pixel, whole 16-byte stores (the generic kernel above ran four threads per pixel on 8-byte stores: 0.8 ms at B = 8 x 720p for 16 channels)
__global__ void split16_cl_kernel(const float *__restrict__ src, half_t *__restrict__ dst, size_t npx, int ps_src, int ps_dst, int c0, int lo_off)
{
    for (size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x; px < npx; px += (size_t)gridDim.x * blockDim.x) {
        const float *i = src + px * ps_src + c0;
        half_t *o = dst + px * ps_dst + c0;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(i + 4 * q);
            v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
        }
        unsigned hi[8], lo[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const half_t h0 = (half_t)v[2 * q], h1 = (half_t)v[2 * q + 1];
            const half_t l0 = (half_t)(v[2 * q] - (float)h0), l1 = (half_t)(v[2 * q + 1] - (float)h1);
            hi[q] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
            lo[q] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<uint4 *>(o + 8 * q) = make_uint4(hi[4 * q], hi[4 * q + 1], hi[4 * q + 2], hi[4 * q + 3]);
            *reinterpret_cast<uint4 *>(o + lo_off + 8 * q) = make_uint4(lo[4 * q], lo[4 * q + 1], lo[4 * q + 2], lo[4 * q + 3]);
        }
    }
}
int launch_convert_cl(const void *src, void *dst, size_t npx, int ps_src, int ps_dst, int c0, int nc, int widen, hipStream_t s, int lo_off)
{
    if (!widen && lo_off > 0 && nc == 16 && (c0 & 7) == 0 && (lo_off & 7) == 0 && (ps_dst & 7) == 0 && (ps_src & 3) == 0) {
        const int grid16 = (int)std::min<size_t>((npx + 255) / 256, 65535 * 4);
        split16_cl_kernel<<<grid16, 256, 0, s>>>((const float *)src, (half_t *)dst, npx, ps_src, ps_dst, c0, lo_off);
        return (int)hipGetLastError();
    }
    const int grid = (int)std::min<size_t>((npx * (nc / 4) + 255) / 256, 65535 * 4);
    if (widen) convert_cl_kernel<true><<<grid, 256, 0, s>>>(src, dst, npx, ps_src, ps_dst, c0, nc, lo_off);
    else convert_cl_kernel<false><<<grid, 256, 0, s>>>(src, dst, npx, ps_src, ps_dst, c0, nc, lo_off);
    return (int)hipGetLastError();
}

// offset [B,18,H,W] + mask [B,9,H,W] (torchvision argument layout) -> om [px][32]
__global__ void om_from_nchw_kernel(const float *__restrict__ off, const float *__restrict__ msk, float *__restrict__ om,
                                    int B, int H, int W)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        float *o = om + i * 32;
        for (int c = 0; c < 18; ++c) o[c] = off[(b * 18 + c) * plane + pix];
        for (int c = 0; c < 9; ++c) o[18 + c] = msk[(b * 9 + c) * plane + pix];
        for (int c = 27; c < 32; ++c) o[c] = 0.0f;
    }
}
int launch_om_from_nchw(const float *off, const float *msk, float *om, int B, int H, int W, hipStream_t s)
{
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    om_from_nchw_kernel<<<grid, 256, 0, s>>>(off, msk, om, B, H, W);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// AdaptiveAvgPool2d(1) -> Flatten -> Linear (ema_vfi.py:83-85) and the folding of the
// broadcast context into motion_estimation.0's bias (ema_vfi.py:124 concat eliminated).
// Deterministic: fixed partition, fixed summation order, no atomics - shards of a batch give
// bit-identical results on any GPU.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pool_partial_kernel(const T *__restrict__ src, float *__restrict__ part, int npix,
                                                           int cp, int ps, int nparts)
{
    const int b = blockIdx.y, part_i = blockIdx.x;
    const int per = (npix + nparts - 1) / nparts;
    const int p0 = part_i * per, p1 = min(npix, p0 + per);
    // 16-byte path (the model's case: cp = 256 channels): a thread sums VEC consecutive channels, cp / VEC threads cover a pixel,
    // 256 * VEC / cp pixels are in flight per iteration (the scalar path below issued one 2-byte load per thread and iteration:
    // 112 us for 236 MB); the pixel lanes are then combined through the LDS in a fixed order
    constexpr int VEC = 16 / (int)sizeof(T);
    if (cp % VEC == 0 && ps % VEC == 0 && 256 % (cp / VEC) == 0 && cp / VEC <= 256) {
        __shared__ float redv[256 * VEC];
        typedef __attribute__((ext_vector_type(VEC))) T vecT;
        const int tpp = cp / VEC, nlv = 256 / tpp;
        const int cv = threadIdx.x % tpp, plv = threadIdx.x / tpp;
        float a[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = 0.0f;
        for (int px = p0 + plv; px < p1; px += nlv) {
            const vecT v = *reinterpret_cast<const vecT *>(src + ((size_t)b * npix + px) * ps + cv * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[e] += (float)v[e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) redv[(plv * tpp + cv) * VEC + e] = a[e];
        __syncthreads();
        for (int c = threadIdx.x; c < cp; c += 256) {
            float t = 0.0f;
            for (int l = 0; l < nlv; ++l) t += redv[l * cp + c];
            part[((size_t)b * nparts + part_i) * cp + c] = t;
        }
        return;
    }
    __shared__ float red[256];
    const int nl = 256 / cp;  // pixel lanes
    const int c = threadIdx.x % cp, pl = threadIdx.x / cp;
    float s = 0.0f;
    for (int px = p0 + pl; px < p1; px += nl) s += (float)src[((size_t)b * npix + px) * ps + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (pl == 0) {
        for (int l = 1; l < nl; ++l) s += red[l * cp + c];
        part[((size_t)b * nparts + part_i) * cp + c] = s;
    }
}
int launch_pool_partial(const void *src, float *part, int B, int npix, int cp, int ps, int nparts, int dtype, hipStream_t s)
{
    dim3 grid(nparts, B);
    if (dtype == 0) pool_partial_kernel<float><<<grid, 256, 0, s>>>((const float *)src, part, npix, cp, ps, nparts);
    else if (dtype == 2) pool_partial_kernel<half_t><<<grid, 256, 0, s>>>((const half_t *)src, part, npix, cp, ps, nparts);
    else pool_partial_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t *)src, part, npix, cp, ps, nparts);
    return (int)hipGetLastError();
}

// One block of 1024 threads per sample (m <= 64: 4m divides 256).  ctxw = [lin_w TRANSPOSED 4m x m][lin_b m][w9c as [c][o * 9 + tap]][b9 m]
// (pack_ctx_kernel): every loop below reads consecutive addresses from consecutive threads.
// Writes ctx[b][m] and the border-class bias table R[b][16][coutpad]:
//   R[cls][o] = b9[o] + sum over taps (ky,kx) inside the image for that class of
//               sum_c W9[o, m + c, ky, kx] * ctx[c]
// cls = ym*4 + xm; bit0 of ym: row y-1 exists, bit1: row y+1 exists (same for xm / columns).
// The kernel is a chain of four dependent phases of a few hundred KB each - latency, not bandwidth: round 4 spreads every phase's
// sum over all 1024 threads (partial sums meet in LDS, added in a fixed order: deterministic), which cut the loads a thread issues
// one after another from 192 to 44 in the longest phase (37 -> ~15 us at B = 8).
constexpr int kCtxThreads = 1024;
__global__ __launch_bounds__(kCtxThreads) void ctx_finish_kernel(const float *__restrict__ part, const float *__restrict__ ctxw,
                                                                 float *__restrict__ ctx_out, float *__restrict__ table,
                                                                 int m, int cp, int nparts, int npix, int coutpad, int round16, int lo_off)
{
    // round16 (EMAVFI_AMP16): the pooled mean and the Linear output are fp16 tensors under autocast
    const auto rq = [round16](float v) { return round16 ? (float)(half_t)v : v; };
    constexpr int NT = kCtxThreads;
    extern __shared__ float sm[];
    float *mean = sm, *ctx = sm + 4 * m, *tsum = ctx + m, *red = tsum + 9 * m;  // tsum [m][9]; red: max(NT, 3 * 9 m) floats
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *lw = ctxw, *lb = lw + (size_t)m * 4 * m, *w9 = lb + m, *b9 = w9 + (size_t)m * m * 9;
    {   // ---- mean over the partial sums: thread (c, g) adds parts g, g + G, ...
        const int C4 = 4 * m, G = NT / C4, c = tid % C4, g = tid / C4;
        float a = 0.0f;
        if (g < G)
            for (int q = g; q < nparts; q += G) {
                a += part[((size_t)b * nparts + q) * cp + c];
                if (lo_off > 0) a += part[((size_t)b * nparts + q) * cp + lo_off + c];   // EMAVFI_F32X3: the lo halves' sums
            }
        if (g < G) red[g * C4 + c] = a;
        __syncthreads();
        if (tid < C4) {
            float s = 0.0f;
            for (int q = 0; q < G; ++q) s += red[q * C4 + tid];
            mean[tid] = rq(s / (float)npix);
        }
        __syncthreads();
    }
    {   // ---- Linear (ema_vfi.py:91, 121): thread (o, g) sums a slice of the 4m inputs from the [c][o] copy (coalesced), four chains
        const int G = NT / m, o = tid % m, g = tid / m, per = (4 * m + G - 1) / G;
        if (g < G) {
            float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int c1 = (g + 1) * per < 4 * m ? (g + 1) * per : 4 * m;
            int c = g * per;
            for (; c + 4 <= c1; c += 4)
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = fmaf(lw[(size_t)(c + u) * m + o], mean[c + u], a[u]);
            for (; c < c1; ++c) a[0] = fmaf(lw[(size_t)c * m + o], mean[c], a[0]);
            red[g * m + o] = (a[0] + a[1]) + (a[2] + a[3]);
        }
        __syncthreads();
        if (tid < m) {
            float t = lb[tid];
            for (int q = 0; q < G; ++q) t += red[q * m + tid];
            t = rq(t);
            ctx[tid] = t;
            ctx_out[(size_t)b * m + tid] = t;
        }
        __syncthreads();
    }
    {   // ---- tsum[k = o * 9 + tap] = sum_c w9[c][k] ctx[c]: blocks of KB outputs, thread (k, cg) sums a third (or less) of the channels
        const int K9 = 9 * m, KB = K9 < 288 ? K9 : 288;
        int CG = NT / KB; CG = CG > m ? m : CG; CG = CG > 3 ? 3 : CG;
        const int per = (m + CG - 1) / CG, kk = tid % KB, cg = tid / KB;
        for (int k0 = 0; k0 < K9; k0 += KB) {
            const int k = k0 + kk;
            if (cg < CG && k < K9) {
                float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                const int c1 = (cg + 1) * per < m ? (cg + 1) * per : m;
                int c = cg * per;
                for (; c + 4 <= c1; c += 4)
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = fmaf(w9[(size_t)(c + u) * K9 + k], ctx[c + u], a[u]);
                for (; c < c1; ++c) a[0] = fmaf(w9[(size_t)c * K9 + k], ctx[c], a[0]);
                red[cg * K9 + k] = (a[0] + a[1]) + (a[2] + a[3]);
            }
        }
        __syncthreads();
        for (int k = tid; k < K9; k += NT) {
            float t = 0.0f;
            for (int q = 0; q < CG; ++q) t += red[q * K9 + k];
            tsum[k] = t;
        }
        __syncthreads();
    }
    for (int k = tid; k < 16 * coutpad; k += NT) {
        const int cls = k / coutpad, o = k - cls * coutpad;
        float s = 0.0f;
        if (o < m) {
            const int ym = cls >> 2, xm = cls & 3;
            s = b9[o];
            for (int ky = 0; ky < 3; ++ky) {
                if ((ky == 0 && !(ym & 1)) || (ky == 2 && !(ym & 2))) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    if ((kx == 0 && !(xm & 1)) || (kx == 2 && !(xm & 2))) continue;
                    s += tsum[o * 9 + ky * 3 + kx];
                }
            }
        }
        table[((size_t)b * 16 + cls) * coutpad + o] = s;
    }
}
int launch_ctx_finish(const float *part, const float *ctxw, float *ctx_out, float *table, int B, int m, int cp, int nparts,
                      int npix, int coutpad, int round16, hipStream_t s, int lo_off)
{
    const int nred = kCtxThreads > 27 * m ? kCtxThreads : 27 * m;
    const size_t sh = (size_t)(4 * m + m + 9 * m + nred) * sizeof(float);
    ctx_finish_kernel<<<B, kCtxThreads, sh, s>>>(part, ctxw, ctx_out, table, m, cp, nparts, npix, coutpad, round16, lo_off);
    return (int)hipGetLastError();
}

// The forward's LAST launch: the blob's header against what the call expects (misc_kernels.h, BlobGuard).  A match costs one
// 36-byte compare per thread of a 64-workgroup grid; a foreign blob (another library version / model / dtype / layout-switch
// setting, or no header at all) overwrites the frame with NaN - the forward cannot return a code for device-resident bytes
// without synchronising, but it must not hand back plausible garbage either.  (Not through the arithmetic: ReLU - v_max_f32 -
// turns a poisoned activation into 0.)
__global__ __launch_bounds__(256) void blob_guard_kernel(const BlobGuard guard, float *__restrict__ out, size_t n)
{
    const uint32_t *got = (const uint32_t *)guard.hdr, *want = (const uint32_t *)&guard.expect;
    bool foreign = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) foreign |= got[i] != want[i];   // magic, version, header_bytes, in, mid, nb, dtype, layout_tag
    if (!foreign) return;
    const float poison = __builtin_nanf("");
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = poison;
}
int launch_blob_guard(const BlobGuard &guard, float *out, size_t n, hipStream_t s)
{
    blob_guard_kernel<<<64, 256, 0, s>>>(guard, out, n);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Bytes set to zero by a launch (misc_kernels.h, launch_clear_bytes): what the entries clear on the caller's stream - the census, the
// zero page, a per-call blob and its padding - is cleared by a kernel of that stream and not by a memset, so that a captured graph
// replays the clear in order like any other launch (a memset node took effect on the first replay only: profiles/r29_graph_replay.md).
// Whole 16-byte units by vector stores; the bytes in front of the first aligned unit and behind the last whole one by block 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clear_bytes_kernel(unsigned char *__restrict__ p, size_t head, size_t units, size_t tail)
{
    uint4 *const q = reinterpret_cast<uint4 *>(p + head);
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < units; i += (size_t)gridDim.x * 256u) q[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) p[threadIdx.x] = 0;
        if (threadIdx.x < tail) p[head + units * 16u + threadIdx.x] = 0;
    }
}
int launch_clear_bytes(void *ptr, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return 0;
    size_t head = (size_t)(-(intptr_t)ptr & 15);
    if (head > bytes) head = bytes;
    const size_t units = (bytes - head) / 16, tail = bytes - head - units * 16, blocks = (units + 255) / 256;
    clear_bytes_kernel<<<(unsigned)(blocks < 1 ? 1 : blocks < 1024 ? blocks : 1024), 256, 0, s>>>((unsigned char *)ptr, head, units, tail);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Blob header (misc_kernels.h, BlobHeader): written behind the pack kernels on the same stream, then the payload's checksum is
// added into it.  Integer addition commutes, so the atomics leave a deterministic value.
// ------------------------------------------------------------------------------------------
__global__ void blob_header_kernel(BlobHeader *dst, const BlobHeader h)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = h;
    // (the rest of the 256 header bytes is zeroed by the clearing launch in front of this one)
}
__global__ __launch_bounds__(256) void blob_checksum_kernel(const uint32_t *__restrict__ payload, size_t nwords, unsigned long long *sum)
{
    unsigned long long a = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x)
        a += ((unsigned long long)payload[i] + 0x9E3779B9ull) * (2ull * i + 1ull);
    __shared__ unsigned long long part[256];
    part[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(sum, part[0]);
}
int launch_blob_seal(void *blob, const BlobHeader &h, hipStream_t s)
{
    if (const int e = launch_clear_bytes(blob, kBlobHeaderBytes, s); e != 0) return e;
    BlobHeader w = h;
    w.checksum = 0;
    blob_header_kernel<<<1, 64, 0, s>>>((BlobHeader *)blob, w);
    const size_t nwords = (size_t)(h.total_bytes - kBlobHeaderBytes) / 4;
    blob_checksum_kernel<<<64, 256, 0, s>>>((const uint32_t *)((const char *)blob + kBlobHeaderBytes), nwords,
                                            (unsigned long long *)((char *)blob + offsetof(BlobHeader, checksum)));
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Backward bilinear warp = EMA_VFI.warp (ema_vfi.py:149-171).  The grid the reference builds on
// the host (:153-160), the add (:162), the normalisation (:165-166, true fp32 division) and
// ATen's grid_sampler_2d (un-normalise, floor, four masked taps) are one kernel; the operation
// order of the coordinate math is kept exactly, because sampling directly at x+flow differs from
// the reference by up to 5e-4 at 720p.  Compiled without fast-math.
// ------------------------------------------------------------------------------------------
struct WarpTap { int o00, o01, o10, o11; float nw, ne, sw, se; int xa, xb, ya, yb; bool v00, v01, v10, v11; };

__device__ __forceinline__ WarpTap warp_tap(int x, int y, float fx, float fy, int H, int W, float wden, float hden)
{
    const float vx = (float)x + fx, vy = (float)y + fy;
    const float gx = 2.0f * vx / wden - 1.0f;
    const float gy = 2.0f * vy / hden - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float xw = floorf(ix), yn = floorf(iy);
    const float w = ix - xw, e = 1.0f - w, n = iy - yn, s = 1.0f - n;
    // range tests in float: a finite coordinate far outside fails all of them -> 0.  A NaN / infinite coordinate (NaN or
    // infinite flow, or a flow so large that 2 * v overflows: same operation order as the reference, so the same cases)
    // yields NaN in every channel, as ATen's CPU grid_sample does (its corner weights are NaN - NaN / inf - inf there and
    // 0 * NaN = NaN): ema_vfi.py:169 on the CPU forward, which is the oracle this path is held to.
    const bool bad = !(fabsf(ix) <= 3.402823466e38f) || !(fabsf(iy) <= 3.402823466e38f);
    const bool x0 = xw >= 0.0f && xw <= (float)(W - 1), x1 = xw + 1.0f >= 0.0f && xw + 1.0f <= (float)(W - 1);
    const bool y0 = yn >= 0.0f && yn <= (float)(H - 1), y1 = yn + 1.0f >= 0.0f && yn + 1.0f <= (float)(H - 1);
    const int xi = x0 ? (int)xw : (x1 ? (int)xw : 0), yi = y0 ? (int)yn : (y1 ? (int)yn : 0);
    const int xa = max(xi, 0), xb = min(xi + 1, W - 1), ya = max(yi, 0), yb = min(yi + 1, H - 1);
    WarpTap t;
    t.o00 = ya * W + xa; t.o01 = ya * W + xb; t.o10 = yb * W + xa; t.o11 = yb * W + xb;
    t.xa = xa; t.xb = xb; t.ya = ya; t.yb = yb;
    const float qnan = __builtin_nanf("");
    t.nw = bad ? qnan : ((y0 && x0) ? s * e : 0.0f);
    t.ne = bad ? qnan : ((y0 && x1) ? s * w : 0.0f);
    t.sw = bad ? qnan : ((y1 && x0) ? n * e : 0.0f);
    t.se = bad ? qnan : ((y1 && x1) ? n * w : 0.0f);
    t.v00 = y0 && x0; t.v01 = y0 && x1; t.v10 = y1 && x0; t.v11 = y1 && x1;
    return t;
}
// The blend of the four corner values (read at the clamped addresses o00.. / their window images).  An out-of-range corner contributes
// exactly nothing: ATen's CPU grid_sample skips it, so what frame2 holds at its clamped address - pixel (0, 0) of the plane for a sample
// far outside, row 0 / column 0 just past an edge - never reaches the result, not even a NaN or an infinity (selected on the corner's
// validity; a zero weight alone would turn them into NaN).  An in-range corner multiplies in IEEE, zero weight included, as ATen does.
// A bad coordinate has no valid corner and NaN weights: 0 * NaN = NaN in every channel.  Accumulation order nw, ne, sw, se as ATen's.
__device__ __forceinline__ float warp_blend(float p00, float p01, float p10, float p11, const WarpTap &t)
{
    float a = (t.v00 ? p00 : 0.0f) * t.nw;
    a += (t.v01 ? p01 : 0.0f) * t.ne;
    a += (t.v10 ? p10 : 0.0f) * t.sw;
    a += (t.v11 ? p11 : 0.0f) * t.se;
    return a;
}
__device__ __forceinline__ float warp_sample(const float *__restrict__ p, const WarpTap &t)
{
    return warp_blend(p[t.o00], p[t.o01], p[t.o10], p[t.o11], t);
}

// NCHW -> NCHW (the C-ABI emavfi_warp; 32 algorithmic bytes per pixel at C = 3).
// One thread = 4 consecutive pixels of a row: 16-byte flow loads and output stores.
template <bool VEC4>
__global__ __launch_bounds__(256) void warp_nchw_kernel(const float *__restrict__ frame2, const float *__restrict__ flow,
                                                        float *__restrict__ out, int B, int C, int H, int W)
{
    const size_t plane = (size_t)H * W;
    const float wden = (float)max(W - 1, 1), hden = (float)max(H - 1, 1);
    constexpr int V = VEC4 ? 4 : 1;
    const size_t nitem = (size_t)B * plane / V;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < nitem; it += (size_t)gridDim.x * blockDim.x) {
        const size_t i = it * V;
        const size_t b = i / plane, pix = i - b * plane;
        const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
        float fx[V], fy[V];
        if (VEC4) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(flow + (b * 2) * plane + pix);
            const f32x4 c = *reinterpret_cast<const f32x4 *>(flow + (b * 2 + 1) * plane + pix);
#pragma unroll
            for (int k = 0; k < V; ++k) { fx[k] = a[k]; fy[k] = c[k]; }
        } else {
            fx[0] = flow[(b * 2) * plane + pix];
            fy[0] = flow[(b * 2 + 1) * plane + pix];
        }
        WarpTap t[V];
#pragma unroll
        for (int k = 0; k < V; ++k) t[k] = warp_tap(x + k, y, fx[k], fy[k], H, W, wden, hden);
        for (int c = 0; c < C; ++c) {
            const float *p = frame2 + (b * C + c) * plane;
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = warp_sample(p, t[k]);
            float *o = out + (b * C + c) * plane + pix;
            if (VEC4) *reinterpret_cast<f32x4 *>(o) = f32x4{v[0], v[1], v[2], v[3]};
            else o[0] = v[0];
        }
    }
}
// Tiled variant (the one emavfi_warp launches when W % 4 == 0 and C == 3): a 256-thread block
// owns a 32x64 pixel tile.  The frame2 window the tile can reach with |flow| <= R = 8 px
// (tile + R each side + 1 for the bilinear neighbour: 49 rows x 84 columns x 3 planes = 48 KiB)
// is brought into LDS by global->LDS DMA in 16-byte pieces (rows outside the image read a zero
// page), so HBM/L2 traffic is coalesced full lines instead of 12 scattered 4-byte gathers per
// pixel; the four taps are then read from LDS.  A pixel whose taps leave the window (|flow| > R)
// gathers from global memory as the simple kernel does - same arithmetic, same result.
__device__ const float g_zero_page[64] = {0};

// T = void: NCHW fp32 planes (emavfi_warp).  T = float / bf16_t: the forward's fused variant, which
// writes channels [coff, ps) of the channels-last fusion buffer (warped RGB, then zero padding).
// TH = tile rows (32: a 49-row window, 48 KiB, three workgroups per CU).  Round 6 measured TH = 16 (33 KiB, four per CU) for the forward's
// variant: 66.4 against 64.0 us - the kernel is bound by the LDS-DMA ingest of its window (46 KB per 2 048 pixels = 1.87 x the tile,
// 169 MB per launch through a path that takes ~ 6.4 TB/s chip-wide) and by ~ 100 issued instructions per pixel, not by occupancy;
// smaller tiles only raise the halo share (profiles/r06_experiments_that_lost.txt)
template <int C, typename T, int TH = 32>
__global__ __launch_bounds__(256) void warp_tiled_kernel(const float *__restrict__ frame2, const float *__restrict__ flow,
                                                         float *__restrict__ out, int B, int H, int W, void *cl_dst, int ps,
                                                         int coff, void *cl_dst16 = nullptr, int ps16 = 0)
{
    constexpr int TW = 64, R = 8, WR = TH + 2 * R + 1, WC = 84, PCS = WC / 4;
    constexpr int NPIECE = C * WR * PCS, NINST = (NPIECE + 63) / 64;
    typedef __attribute__((address_space(1))) const void gptr_t;
    typedef __attribute__((address_space(3))) void lptr_t;
    __shared__ __attribute__((aligned(16))) float win[NINST * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (id % 8 labels the
    // XCD group); give each group a contiguous run of tiles so x-neighbours, which share halo
    // columns, hit the same XCD's L2.  Bijective for any grid size; placement only affects speed.
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH, nwg = gridDim.x;
    const int grp = blockIdx.x & 7, kk = blockIdx.x >> 3, qq = nwg >> 3, rr = nwg & 7;
    const int wg = (grp < rr ? grp * (qq + 1) : rr * (qq + 1) + (grp - rr) * qq) + kk;
    const int b = wg / (ntx * nty), trem = wg - b * (ntx * nty);
    const int ty = (trem / ntx) * TH, tx = (trem - (trem / ntx) * ntx) * TW;
    const int wy0 = ty - R, wx0 = tx - R;  // tx is a multiple of 64, so wx0 is 16-byte aligned when W % 4 == 0
    const size_t plane = (size_t)H * W;
    const float *src_b = frame2 + (size_t)b * C * plane;
#pragma unroll
    for (int i = 0; i < (NINST + 3) / 4; ++i) {
        const int j = i * 4 + wave;
        if (j < NINST) {
            const int idx = j * 64 + lane;
            const int ch = idx / (WR * PCS), rem = idx - ch * (WR * PCS);
            const int row = rem / PCS, pc = rem - row * PCS;
            const int gy = wy0 + row, gx = wx0 + 4 * pc;
            const bool ok = idx < NPIECE && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float *src = ok ? src_b + (size_t)ch * plane + (size_t)gy * W + gx : g_zero_page;
            __builtin_amdgcn_global_load_lds((gptr_t *)src, (lptr_t *)(win + j * 256), 16, 0, 0);
        }
    }
    const float wden = (float)max(W - 1, 1), hden = (float)max(H - 1, 1);
    if constexpr (std::is_same<T, bf16_t>::value || std::is_same<T, half_t>::value) {
        if ((ps == 8 || ps == 4) && coff == 0) {
            // The forward's 16-bit variant (compact tail of the fusion input: 8 channels = 16 bytes per pixel, or - round 6 - 4 channels =
            // 8 bytes, which is what the forward passes: 22 % fewer bytes moved): a wave takes whole ROWS of the
            // tile, lane = column.  A store instruction then writes 1 KiB of consecutive addresses (the 4-pixels-per-thread mapping
            // below wrote 16 bytes of every 64: four partial passes over each line), the corner reads of a wave are consecutive dwords
            // of the window (conflict-free for a smooth flow; lanes four pixels apart were a four-way bank conflict) and the flow loads
            // are 256 contiguous bytes per instruction.  Same warp_tap / warp_sample arithmetic per pixel: identical results.
            constexpr int NR = TH / 4;
            float gx[NR], gy[NR];
            const int x = tx + lane;
#pragma unroll
            for (int k = 0; k < NR; ++k) {   // while the DMA is in flight
                const int y = ty + wave + 4 * k;
                const bool ok = y < H && x < W;
                const size_t pix = (size_t)(ok ? y : 0) * W + (ok ? x : 0);
                gx[k] = flow[((size_t)b * 2) * plane + pix];
                gy[k] = flow[((size_t)b * 2 + 1) * plane + pix];
            }
            // the window is filled by LDS-DMA, which hipcc drains (vmcnt(0)) ahead of the barrier today; pinned here so that a compiler
            // that moves its wait behind the barrier cannot let a wave read another wave's unlanded window.  Free: the
            // flow loads were issued after the DMA and return in order.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            typedef __attribute__((ext_vector_type(8))) T vec8;
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int y = ty + wave + 4 * k;
                if (y >= H || x >= W) continue;
                const WarpTap t = warp_tap(x, y, gx[k], gy[k], H, W, wden, hden);
                const bool inside = t.ya >= wy0 && t.yb <= wy0 + WR - 1 && t.xa >= wx0 && t.xb <= wx0 + WC - 1;
                float v[C];
                if (inside) {
                    const int l00 = (t.ya - wy0) * WC + (t.xa - wx0), l01 = (t.ya - wy0) * WC + (t.xb - wx0);
                    const int l10 = (t.yb - wy0) * WC + (t.xa - wx0), l11 = (t.yb - wy0) * WC + (t.xb - wx0);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float *p = win + c * (WR * WC);
                        v[c] = warp_blend(p[l00], p[l01], p[l10], p[l11], t);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = warp_sample(src_b + (size_t)c * plane, t);
                }
                const T z = (T)0.0f;
                T *o = reinterpret_cast<T *>(cl_dst) + ((size_t)b * plane + (size_t)y * W + x) * ps;
                if (ps == 4) {
                    typedef __attribute__((ext_vector_type(4))) T vec4;
                    *reinterpret_cast<vec4 *>(o) = vec4{(T)v[0], C > 1 ? (T)v[C > 1 ? 1 : 0] : z, C > 2 ? (T)v[C > 2 ? 2 : 0] : z, z};
                } else {
                    *reinterpret_cast<vec8 *>(o) = vec8{(T)v[0], C > 1 ? (T)v[C > 1 ? 1 : 0] : z, C > 2 ? (T)v[C > 2 ? 2 : 0] : z, z, z, z, z, z};
                }
            }
            return;
        }
    }
    // flow for this thread's items (4 pixels each; two per thread for the 32-row tile) while the DMA is in flight
    constexpr int NI = TH * TW / 4 / 256;
    f32x4 fx[NI], fy[NI];
    int iy[NI], ix[NI];
    bool live[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int item = tid + 256 * k;
        iy[k] = ty + item / (TW / 4);
        ix[k] = tx + 4 * (item % (TW / 4));
        live[k] = iy[k] < H && ix[k] < W;
        const size_t pix = (size_t)(live[k] ? iy[k] : 0) * W + (live[k] ? ix[k] : 0);
        fx[k] = *reinterpret_cast<const f32x4 *>(flow + ((size_t)b * 2) * plane + pix);
        fy[k] = *reinterpret_cast<const f32x4 *>(flow + ((size_t)b * 2 + 1) * plane + pix);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA has landed before the barrier, whatever hipcc does with its own wait
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        if (!live[k]) continue;
        float v[C][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const WarpTap t = warp_tap(ix[k] + q, iy[k], fx[k][q], fy[k][q], H, W, wden, hden);
            const bool inside = t.ya >= wy0 && t.yb <= wy0 + WR - 1 && t.xa >= wx0 && t.xb <= wx0 + WC - 1;
            if (inside) {
                const int l00 = (t.ya - wy0) * WC + (t.xa - wx0), l01 = (t.ya - wy0) * WC + (t.xb - wx0);
                const int l10 = (t.yb - wy0) * WC + (t.xa - wx0), l11 = (t.yb - wy0) * WC + (t.xb - wx0);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float *p = win + c * (WR * WC);
                    v[c][q] = warp_blend(p[l00], p[l01], p[l10], p[l11], t);
                }
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) v[c][q] = warp_sample(src_b + (size_t)c * plane, t);
            }
        }
        const size_t pix = (size_t)iy[k] * W + ix[k];
        if constexpr (std::is_void<T>::value) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                *reinterpret_cast<f32x4 *>(out + ((size_t)b * C + c) * plane + pix) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                T *o = reinterpret_cast<T *>(cl_dst) + ((size_t)b * plane + pix + q) * ps + coff;
                if constexpr (std::is_same<T, float>::value) {
                    // EMAVFI_AMP16: the fp16 rounding of the same values into channels [coff, ps16) of a second (fp16) fusion tensor, in the
                    // same launch (was a conversion pass of its own: fusion_round_warped)
                    if (cl_dst16) {
                        half_t *o16 = reinterpret_cast<half_t *>(cl_dst16) + ((size_t)b * plane + pix + q) * ps16 + coff;
                        if (ps16 - coff == 16 && (coff & 7) == 0 && (ps16 & 7) == 0) {   // mid_channels 64: channels 64..79 as two 16-byte stores
                            typedef __attribute__((ext_vector_type(8))) half_t h8;
                            const half_t z = (half_t)0.0f;
                            *reinterpret_cast<h8 *>(o16) = h8{(half_t)v[0][q], C > 1 ? (half_t)v[C > 1 ? 1 : 0][q] : z, C > 2 ? (half_t)v[C > 2 ? 2 : 0][q] : z, z, z, z, z, z};
                            *reinterpret_cast<h8 *>(o16 + 8) = h8{z, z, z, z, z, z, z, z};
                        } else {
#pragma unroll
                            for (int c = 0; c < C; ++c) o16[c] = (half_t)v[c][q];
                            for (int c = C; c < ps16 - coff; ++c) o16[c] = (half_t)0.0f;
                        }
                    }
                }
                if (ps - coff == 16 && (coff & 7) == 0) {  // mid_channels 64: channels 64..79, aligned
                    store4(o, v[0][q], C > 1 ? v[C > 1 ? 1 : 0][q] : 0.0f, C > 2 ? v[C > 2 ? 2 : 0][q] : 0.0f, 0.0f);
                    store4(o + 4, 0.0f, 0.0f, 0.0f, 0.0f);
                    store4(o + 8, 0.0f, 0.0f, 0.0f, 0.0f);
                    store4(o + 12, 0.0f, 0.0f, 0.0f, 0.0f);
                    continue;
                }
                if constexpr (sizeof(T) == 2) {
                    if (ps == 8 && coff == 0) {  // compact 8-channel tail of the fusion input: one 16-byte store per pixel
                        typedef __attribute__((ext_vector_type(8))) T vec8;
                        const T z = (T)0.0f;
                        *reinterpret_cast<vec8 *>(o) = vec8{(T)v[0][q], C > 1 ? (T)v[C > 1 ? 1 : 0][q] : z, C > 2 ? (T)v[C > 2 ? 2 : 0][q] : z, z, z, z, z, z};
                        continue;
                    }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = (T)v[c][q];
                for (int c = C; c < ps - coff; ++c) o[c] = (T)0.0f;
            }
        }
    }
}

int launch_warp_nchw(const float *frame2, const float *flow, float *out, int B, int C, int H, int W, hipStream_t s)
{
    const size_t n = (size_t)B * H * W;
    if ((W & 3) == 0 && C == 3) {
        const int nwg = ((W + 63) / 64) * ((H + 31) / 32) * B;
        warp_tiled_kernel<3, void><<<nwg, 256, 0, s>>>(frame2, flow, out, B, H, W, nullptr, 0, 0);
        return (int)hipGetLastError();
    }
    if ((W & 3) == 0) {
        const int grid = (int)std::min<size_t>((n / 4 + 255) / 256, 256 * 32);
        warp_nchw_kernel<true><<<grid, 256, 0, s>>>(frame2, flow, out, B, C, H, W);
    } else {
        const int grid = (int)std::min<size_t>((n + 255) / 256, 256 * 32);
        warp_nchw_kernel<false><<<grid, 256, 0, s>>>(frame2, flow, out, B, C, H, W);
    }
    return (int)hipGetLastError();
}

// Forward-path variant: writes the warped RGB straight into channels [coff, ps) of the
// channels-last fusion buffer (the torch.cat of ema_vfi.py:134 never materialises); channels
// past coff + C are the zero padding.
template <typename T>
__global__ __launch_bounds__(256) void warp_fused_kernel(const float *__restrict__ frame2, const float *__restrict__ flow,
                                                         T *__restrict__ dst, int B, int C, int H, int W, int ps, int coff,
                                                         half_t *__restrict__ dst16 = nullptr, int ps16 = 0)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    const float wden = (float)max(W - 1, 1), hden = (float)max(H - 1, 1);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
        const WarpTap t = warp_tap(x, y, flow[(b * 2) * plane + pix], flow[(b * 2 + 1) * plane + pix], H, W, wden, hden);
        T *o = dst + i * ps + coff;
        for (int c = 0; c < ps - coff; ++c) {
            const float v = c < C ? warp_sample(frame2 + (b * C + c) * plane, t) : 0.0f;
            o[c] = (T)v;
            if (dst16 && c < ps16 - coff) dst16[i * ps16 + coff + c] = (half_t)v;
        }
    }
}
int launch_warp_fused(const float *frame2, const float *flow, void *dst, int B, int C, int H, int W, int ps, int coff, int dtype,
                      hipStream_t s, void *dst16, int ps16)
{
    if (dst16 && (dtype != 0 || ps16 - coff > ps - coff)) return (int)hipErrorInvalidValue;   // the second (fp16) destination belongs to the fp32 variant
    if ((W & 3) == 0 && C == 3) {
        const int nwg = ((W + 63) / 64) * ((H + 31) / 32) * B;
        if (dtype == 0) warp_tiled_kernel<3, float><<<nwg, 256, 0, s>>>(frame2, flow, nullptr, B, H, W, dst, ps, coff, dst16, ps16);
        else if (dtype == 2) warp_tiled_kernel<3, half_t><<<nwg, 256, 0, s>>>(frame2, flow, nullptr, B, H, W, dst, ps, coff);
        else warp_tiled_kernel<3, bf16_t><<<nwg, 256, 0, s>>>(frame2, flow, nullptr, B, H, W, dst, ps, coff);
        return (int)hipGetLastError();
    }
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 256 * 64);
    if (dtype == 0) warp_fused_kernel<float><<<grid, 256, 0, s>>>(frame2, flow, (float *)dst, B, C, H, W, ps, coff, (half_t *)dst16, ps16);
    else if (dtype == 2) warp_fused_kernel<half_t><<<grid, 256, 0, s>>>(frame2, flow, (half_t *)dst, B, C, H, W, ps, coff);
    else warp_fused_kernel<bf16_t><<<grid, 256, 0, s>>>(frame2, flow, (bf16_t *)dst, B, C, H, W, ps, coff);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Frame pre/post-processing on the GPU: what the reference does on the
// host around every forward.
//   preprocess:  transforms.ToTensor() + Normalize(mean, std)  (inference.py:38-41, 44-48):
//                uint8 HWC -> float32 /255 -> (x - mean) / std, NCHW.  True fp32 divisions, same order.
//   postprocess: denormalize_frame (inference.py:51-58): NCHW fp32 -> HWC, x * std + mean (the
//                reference applies this to an output that is already in [0,1] - kept behind `denorm`),
//                clip to [0,1], * 255, astype(uint8) (truncation).  numpy promotes to float64 there
//                (np.array([...]) is float64), so the arithmetic here is double: bit-exact bytes.
// ------------------------------------------------------------------------------------------
struct Stats4 { float mean[4], stdv[4]; };
struct Stats4d { double mean[4], stdv[4]; };  // numpy's float64 constants in denormalize_frame

__global__ void preprocess_u8_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst, int B, int H, int W, int C,
                                     Stats4 st)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        const unsigned char *p = src + i * C;
        for (int c = 0; c < C; ++c) {
            const float v = (float)p[c] / 255.0f;
            dst[(b * C + c) * plane + pix] = (v - st.mean[c]) / st.stdv[c];
        }
    }
}
__global__ void postprocess_u8_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, int B, int H, int W, int C,
                                      Stats4d st, int denorm)
{
    const size_t plane = (size_t)H * W, total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / plane, pix = i - b * plane;
        unsigned char *p = dst + i * C;
        for (int c = 0; c < C; ++c) {
            double v = (double)src[(b * C + c) * plane + pix];
            if (denorm) v = v * st.stdv[c] + st.mean[c];
            v = fmin(fmax(v, 0.0), 1.0) * 255.0;   // NaN -> 0 (fmax), as np.clip then astype would not define
            p[c] = (unsigned char)v;
        }
    }
}
// C = 3, H*W % 4 == 0: one thread = 4 consecutive pixels = 12 contiguous bytes (three dword accesses on the uint8 side,
// three 16-byte accesses on the fp32 planes).  Same per-element arithmetic as the scalar kernels; what changes is the
// access width - the uint8 side may be pinned host memory reached over PCIe, where single-byte accesses crawl.
__global__ void preprocess_u8x4_kernel(const unsigned *__restrict__ src, float *__restrict__ dst, int B, size_t plane, Stats4 st)
{
    const size_t groups = plane / 4, total = (size_t)B * groups;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t b = g / groups, pix = (g - b * groups) * 4;
        const unsigned w0 = src[g * 3], w1 = src[g * 3 + 1], w2 = src[g * 3 + 2];
        const unsigned char by[12] = {(unsigned char)w0, (unsigned char)(w0 >> 8), (unsigned char)(w0 >> 16), (unsigned char)(w0 >> 24),
                                      (unsigned char)w1, (unsigned char)(w1 >> 8), (unsigned char)(w1 >> 16), (unsigned char)(w1 >> 24),
                                      (unsigned char)w2, (unsigned char)(w2 >> 8), (unsigned char)(w2 >> 16), (unsigned char)(w2 >> 24)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = (float)by[q * 3 + c] / 255.0f;
                o[q] = (v - st.mean[c]) / st.stdv[c];
            }
            *reinterpret_cast<f32x4 *>(dst + (b * 3 + c) * plane + pix) = o;
        }
    }
}
__global__ void postprocess_u8x4_kernel(const float *__restrict__ src, unsigned *__restrict__ dst, int B, size_t plane, Stats4d st,
                                        int denorm)
{
    const size_t groups = plane / 4, total = (size_t)B * groups;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t b = g / groups, pix = (g - b * groups) * 4;
        unsigned char by[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 x = *reinterpret_cast<const f32x4 *>(src + (b * 3 + c) * plane + pix);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double v = (double)x[q];
                if (denorm) v = v * st.stdv[c] + st.mean[c];
                v = fmin(fmax(v, 0.0), 1.0) * 255.0;
                by[q * 3 + c] = (unsigned char)v;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dst[g * 3 + k] = (unsigned)by[4 * k] | ((unsigned)by[4 * k + 1] << 8) | ((unsigned)by[4 * k + 2] << 16) | ((unsigned)by[4 * k + 3] << 24);
    }
}
// C = 3, the whole batch a multiple of 16 bytes on the uint8 side: one thread = ONE 16-byte quad of the interleaved byte stream
// (5 1/3 pixels), so that a wave's access to the uint8 side is 1 KiB of consecutive addresses per instruction.  That side is pinned
// host memory in the streaming harness (emavfi/stream.py): fine-grained, not cached by the GPU, every instruction its own PCIe
// transactions - the dword kernels above touch every 64-byte line three times (three 12-byte-strided instructions per thread).  The
// fp32 planes (HBM) are read / written as scalars at a lane stride of 5 1/3 floats: cached, cheap.  Byte g of the batch is channel
// g % 3 of global pixel g / 3; same per-element arithmetic as the scalar kernels (round 5).
__global__ __launch_bounds__(256) void preprocess_u8q_kernel(const uint4 *__restrict__ src, float *__restrict__ dst, size_t nquads, size_t plane,
                                                             Stats4 st)
{
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquads; q += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = src[q];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        const size_t g0 = q * 16;
        size_t px = g0 / 3;
        int c = (int)(g0 - px * 3);
        size_t b = px / plane, pix = px - b * plane;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float u = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu) / 255.0f;
            dst[(b * 3 + c) * plane + pix] = (u - st.mean[c]) / st.stdv[c];
            if (++c == 3) { c = 0; if (++pix == plane) { pix = 0; ++b; } }
        }
    }
}
__global__ __launch_bounds__(256) void postprocess_u8q_kernel(const float *__restrict__ src, uint4 *__restrict__ dst, size_t nquads, size_t plane,
                                                              Stats4d st, int denorm)
{
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquads; q += (size_t)gridDim.x * blockDim.x) {
        const size_t g0 = q * 16;
        size_t px = g0 / 3;
        int c = (int)(g0 - px * 3);
        size_t b = px / plane, pix = px - b * plane;
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            double v = (double)src[(b * 3 + c) * plane + pix];
            if (denorm) v = v * st.stdv[c] + st.mean[c];
            v = fmin(fmax(v, 0.0), 1.0) * 255.0;
            w[j >> 2] |= (unsigned)(unsigned char)v << (8 * (j & 3));
            if (++c == 3) { c = 0; if (++pix == plane) { pix = 0; ++b; } }
        }
        dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}
// measurement knob (round 5): cap the grid of the quad kernels (EMAVFI_PREPOST_WGS=n; 0 / unset: one thread per quad up to 262 140 blocks)
static int prepost_grid(size_t nq)
{
    static const int cap = [] { const char *e = getenv("EMAVFI_PREPOST_WGS"); return e ? atoi(e) : 0; }();
    const size_t want = (nq + 255) / 256;
    return (int)std::min<size_t>(want, cap > 0 ? (size_t)cap : (size_t)65535 * 4);
}
static bool u8q_ok(const void *u8, int B, int H, int W, int C)
{
    return C == 3 && ((size_t)B * H * W * 3) % 16 == 0 && ((uintptr_t)u8 & 15) == 0;
}
static bool u8x4_ok(const void *u8, const void *f32, int H, int W, int C)
{
    return C == 3 && ((size_t)H * W) % 4 == 0 && ((uintptr_t)u8 & 3) == 0 && ((uintptr_t)f32 & 15) == 0;
}
int launch_preprocess_u8(const unsigned char *src, float *dst, int B, int H, int W, int C, const float *mean, const float *stdv,
                         hipStream_t s)
{
    Stats4 st{};
    for (int c = 0; c < C && c < 4; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    if (u8q_ok(src, B, H, W, C)) {
        const size_t nq = (size_t)B * H * W * 3 / 16;
        const int grid = prepost_grid(nq);
        preprocess_u8q_kernel<<<grid, 256, 0, s>>>((const uint4 *)src, dst, nq, (size_t)H * W, st);
        return (int)hipGetLastError();
    }
    if (u8x4_ok(src, dst, H, W, C)) {
        const int grid = (int)std::min<size_t>(((size_t)B * H * W / 4 + 255) / 256, 65535 * 4);
        preprocess_u8x4_kernel<<<grid, 256, 0, s>>>((const unsigned *)src, dst, B, (size_t)H * W, st);
        return (int)hipGetLastError();
    }
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    preprocess_u8_kernel<<<grid, 256, 0, s>>>(src, dst, B, H, W, C, st);
    return (int)hipGetLastError();
}
int launch_postprocess_u8(const float *src, unsigned char *dst, int B, int H, int W, int C, const double *mean, const double *stdv,
                          int denorm, hipStream_t s)
{
    Stats4d st{};
    for (int c = 0; c < C && c < 4; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    if (u8q_ok(dst, B, H, W, C)) {
        const size_t nq = (size_t)B * H * W * 3 / 16;
        const int grid = prepost_grid(nq);
        postprocess_u8q_kernel<<<grid, 256, 0, s>>>(src, (uint4 *)dst, nq, (size_t)H * W, st, denorm);
        return (int)hipGetLastError();
    }
    if (u8x4_ok(dst, src, H, W, C)) {
        const int grid4 = (int)std::min<size_t>(((size_t)B * H * W / 4 + 255) / 256, 65535 * 4);
        postprocess_u8x4_kernel<<<grid4, 256, 0, s>>>(src, (unsigned *)dst, B, (size_t)H * W, st, denorm);
        return (int)hipGetLastError();
    }
    const int grid = (int)std::min<size_t>(((size_t)B * H * W + 255) / 256, 65535 * 4);
    postprocess_u8_kernel<<<grid, 256, 0, s>>>(src, dst, B, H, W, C, st, denorm);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// 4:2:0 frames (include/emavfi.h, "NV12", "HIGH BIT DEPTH", "PLANAR 4:2:0"): a pitched full-resolution Y plane and half-resolution chroma, decoded
// to / encoded from what the u8 kernels above read / write.  One kernel pair, preprocess_yuv420_kernel<F> / postprocess_yuv420_kernel<F>, and
// four formats F that differ in where a sample sits, never in what is computed from it:
//   NV12                 Yuv8<true>    bytes; U and V interleaved in one plane
//   P010 / P012 / P016   Yuv16<true>   little-endian 16-bit words, the sample in the word's top `depth` bits; U and V interleaved
//   planar, depth 8      Yuv8<false>   bytes; a U plane and a V plane
//   planar, depth > 8    Yuv16<false>  16-bit words, the sample in the word's low `depth` bits; a U plane and a V plane
// Bytes go through nv12_decode / _norm / _byte / _luma / _chroma below (signed 32-bit fixed point, 20 fractional bits), words through
// p010_elem.h's functions (signed 64-bit; the same text the host check runs), so that
//   preprocess  == preprocess_u8 of the decoded bytes (same fp32 / 255, - mean, / std; 255 -> P = 2^depth - 1 above depth 8);
//   postprocess == the encode of what postprocess_u8 would write (same float64 arithmetic, truncation, NaN -> 0).
// One lane owns a block of 2 rows x 16 BYTES of Y = NX columns (16 of bytes, 8 of words) and the NX / 2 chroma pairs under it: 16 bytes of an
// interleaved UV row, or 8 bytes of a U and 8 of a V row.  A planar chroma row is half as wide as an interleaved one, so the planar layouts take
// the narrower chroma access and keep the block: chroma is 0.5 - 1 of the 13.5 - 15 bytes per pixel, 12 are fp32, and the fp32 pattern stays the
// same for all four (profiles/r15_yuv420p_y4m.md measured the other choice, a block of 2 rows x 32 bytes).  A block takes either of two forms with
// the same per-element arithmetic:
//   FAST   two 16-byte Y accesses, one 16-byte UV access or an 8-byte U and an 8-byte V access, 16-byte accesses on the three fp32 planes; a
//          wave's access to a row is consecutive addresses, every chroma pair is fetched / written once for its four pixels.  Conditions:
//          yuv420_fast_ok below - and the block lies inside the frame (NX columns, 2 rows).
//   SCALAR sample and dword accesses with the encode's edge clamp: every block when a FAST condition fails, otherwise the right (W % NX)
//          and bottom (odd H) remainders only.
// No LDS, no waiting, one block per lane and a grid-stride loop: the launches are short-lived beside the persistent convolutions.  The sample
// side may be pinned host memory reached over PCIe, as for the u8 kernels.
// ------------------------------------------------------------------------------------------
struct YuvCoef { int dec[5], enc[9], limited, rgb; };   // tables of include/emavfi.h; limited: Y - 16 floor / + 16 offset; rgb: channel 0 is R

void yuv_coefficients(int standard, int dec[5], int enc[9])
{
    const bool full = (standard & 1) != 0, bt709 = (standard >> 1) != 0;
    const double kr = bt709 ? 0.2126 : 0.299, kb = bt709 ? 0.0722 : 0.114, kg = 1 - kr - kb;
    const double cy = full ? 1.0 : 255.0 / 219, s = full ? 1.0 : 255.0 / 224, t = full ? 1.0 : 219.0 / 255, sp = full ? 1.0 : 224.0 / 255;
    const double kd[5] = {cy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s};
    const double ke[9] = {kr * t, kg * t, kb * t,
                          -kr / (2 * (1 - kb)) * sp, -kg / (2 * (1 - kb)) * sp, 0.5 * sp,
                          0.5 * sp, -kg / (2 * (1 - kr)) * sp, -kb / (2 * (1 - kr)) * sp};
    for (int i = 0; i < 5; ++i) dec[i] = (int)floor(kd[i] * 1048576.0 + 0.5);
    for (int i = 0; i < 9; ++i) enc[i] = (int)floor(ke[i] * 1048576.0 + 0.5);
}
static YuvCoef yuv_coef(int standard, int order)
{
    YuvCoef k{};
    yuv_coefficients(standard, k.dec, k.enc);
    k.limited = (standard & 1) == 0;
    k.rgb = order == 1;
    return k;
}

__device__ __forceinline__ int nv12_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// one pixel: (Y, U, V) -> the three bytes of the u8 layout, ch[0] = channel 0 of `order`
__device__ __forceinline__ void nv12_decode(int Y, int U, int V, const YuvCoef &k, int ch[3])
{
    const int u = U - 128, v = V - 128, l = k.limited ? max(Y - 16, 0) : Y, yl = k.dec[0] * l + (1 << 19);
    const int r = nv12_clip((yl + k.dec[1] * v) >> 20);
    const int g = nv12_clip((yl + k.dec[2] * u + k.dec[3] * v) >> 20);
    const int b = nv12_clip((yl + k.dec[4] * u) >> 20);
    ch[0] = k.rgb ? r : b; ch[1] = g; ch[2] = k.rgb ? b : r;
}
__device__ __forceinline__ float nv12_norm(int byte, float mean, float stdv)
{
    const float v = (float)byte / 255.0f;   // preprocess_u8_kernel's two true divisions, same order
    return (v - mean) / stdv;
}
// postprocess_u8_kernel's byte of one element
__device__ __forceinline__ int nv12_byte(float x, double mean, double stdv, int denorm)
{
    double v = (double)x;
    if (denorm) v = v * stdv + mean;
    v = fmin(fmax(v, 0.0), 1.0) * 255.0;
    return (int)(unsigned char)v;
}
__device__ __forceinline__ int nv12_luma(const int ch[3], const YuvCoef &k)
{
    const int r = k.rgb ? ch[0] : ch[2], g = ch[1], b = k.rgb ? ch[2] : ch[0];
    return nv12_clip(((k.enc[0] * r + k.enc[1] * g + k.enc[2] * b + (1 << 19)) >> 20) + (k.limited ? 16 : 0));
}
// sum[c]: the 2x2 block's four bytes of channel c added up
__device__ __forceinline__ void nv12_chroma(const int sum[3], const YuvCoef &k, int &U, int &V)
{
    const int m0 = (sum[0] + 2) >> 2, m1 = (sum[1] + 2) >> 2, m2 = (sum[2] + 2) >> 2;
    const int r = k.rgb ? m0 : m2, g = m1, b = k.rgb ? m2 : m0;
    U = nv12_clip(((k.enc[3] * r + k.enc[4] * g + k.enc[5] * b + (1 << 19)) >> 20) + 128);
    V = nv12_clip(((k.enc[6] * r + k.enc[7] * g + k.enc[8] * b + (1 << 19)) >> 20) + 128);
}

// yuv_coefficients with the depth as a parameter (it returns yuv_coefficients' tables at depth 8) and BT.2020
void yuv_coefficients_depth(int standard, int depth, int dec[5], int enc[9])
{
    const bool full = (standard & 1) != 0;
    const int matrix = standard >> 1;   // 0 BT.601, 1 BT.709, 2 BT.2020 (non-constant luminance)
    const double kr = matrix == 2 ? 0.2627 : matrix == 1 ? 0.2126 : 0.299, kb = matrix == 2 ? 0.0593 : matrix == 1 ? 0.0722 : 0.114, kg = 1 - kr - kb;
    const double P = (double)((1 << depth) - 1), Yr = full ? P : (double)(219 << (depth - 8)), Cr = full ? P : (double)(224 << (depth - 8));
    const double cy = P / Yr, s = P / Cr, t = Yr / P, sp = Cr / P;
    const double kd[5] = {cy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s};
    const double ke[9] = {kr * t, kg * t, kb * t,
                          -kr / (2 * (1 - kb)) * sp, -kg / (2 * (1 - kb)) * sp, 0.5 * sp,
                          0.5 * sp, -kg / (2 * (1 - kr)) * sp, -kb / (2 * (1 - kr)) * sp};
    for (int i = 0; i < 5; ++i) dec[i] = (int)floor(kd[i] * 1048576.0 + 0.5);
    for (int i = 0; i < 9; ++i) enc[i] = (int)floor(ke[i] * 1048576.0 + 0.5);
}
static P010Coef p010_coef(int standard, int depth, int order)
{
    P010Coef k{};
    yuv_coefficients_depth(standard, depth, k.dec, k.enc);
    p010_constants(depth, (standard & 1) == 0, k);
    k.rgb = order == 1;
    return k;
}

// 2 or 4 consecutive dwords at an 8- / 16-byte aligned address, moved in one access
template <int N> __device__ __forceinline__ void load_dwords(const unsigned char *p, unsigned (&w)[N])
{
    static_assert(N == 2 || N == 4, "an 8- or a 16-byte access");
    if constexpr (N == 2) {
        const uint2 q = *reinterpret_cast<const uint2 *>(p);
        w[0] = q.x; w[1] = q.y;
    } else {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    }
}
template <int N> __device__ __forceinline__ void store_dwords(unsigned char *p, const unsigned (&w)[N])
{
    static_assert(N == 2 || N == 4, "an 8- or a 16-byte access");
    if constexpr (N == 2) *reinterpret_cast<uint2 *>(p) = make_uint2(w[0], w[1]);
    else *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// The four formats.  A format names the type in memory, whether U and V share a plane (SEMI), how a sample is read from its word and written
// back, and the per-element functions the samples go through.
// bytes, NV12 (SEMI) and planar depth 8: 32-bit fixed point
template <bool SEMI> struct Yuv8 {
    typedef unsigned char T;
    static constexpr bool semi = SEMI;
    YuvCoef k;
    __device__ __forceinline__ int sample(unsigned w) const { return (int)w; }
    __device__ __forceinline__ unsigned word(int v) const { return (unsigned)v; }
    __device__ __forceinline__ void decode(int Y, int U, int V, int ch[3]) const { nv12_decode(Y, U, V, k, ch); }
    __device__ __forceinline__ float norm(int v, float mean, float stdv) const { return nv12_norm(v, mean, stdv); }
    __device__ __forceinline__ int quant(float x, double mean, double stdv, int denorm) const { return nv12_byte(x, mean, stdv, denorm); }
    __device__ __forceinline__ int luma(const int ch[3]) const { return nv12_luma(ch, k); }
    __device__ __forceinline__ void chroma(const int sum[3], int &U, int &V) const { nv12_chroma(sum, k, U, V); }
};
// 16-bit words, P010 / P012 / P016 (SEMI: the sample in the word's TOP `depth` bits, the low bits written as zero) and planar depth 10 / 12 / 16
// (the sample in the LOW `depth` bits, the high bits written as zero): p010_elem.h's 64-bit fixed point
template <bool SEMI> struct Yuv16 {
    typedef unsigned short T;
    static constexpr bool semi = SEMI;
    P010Coef k;
    __device__ __forceinline__ int sample(unsigned w) const { return SEMI ? p010_sample(w, k) : yuv420p_sample(w, k.P); }
    __device__ __forceinline__ unsigned word(int v) const { return SEMI ? (unsigned)v << k.shift : (unsigned)v; }
    __device__ __forceinline__ void decode(int Y, int U, int V, int ch[3]) const { p010_decode(Y, U, V, k, ch); }
    __device__ __forceinline__ float norm(int v, float mean, float stdv) const { return p010_norm(v, (float)k.P, mean, stdv); }
    __device__ __forceinline__ int quant(float x, double mean, double stdv, int denorm) const { return p010_quant(x, mean, stdv, denorm, (double)k.P); }
    __device__ __forceinline__ int luma(const int ch[3]) const { return p010_luma(ch, k); }
    __device__ __forceinline__ void chroma(const int sum[3], int &U, int &V) const { p010_chroma(sum, k, U, V); }
};
// What the kernels below derive from a format.  Chroma sample c of a lane's row piece is sample CS c of the U piece and sample CS c + VO of the
// V piece (yuv420p_get / yuv420p_put); with SEMI the V piece is the U piece, one sample further on.
template <class F> struct Yuv420Block {
    static constexpr int ES = (int)sizeof(typename F::T), BITS = 8 * ES;
    static constexpr int NX = 16 / ES, NW = 4;              // columns and dwords of a lane's 16 bytes of a Y row
    static constexpr int CS = F::semi ? 2 : 1, VO = F::semi ? 1 : 0;
    static constexpr int NC = NW * CS / 2;                  // dwords of a lane's piece of a chroma row: 16 bytes of UV, or 8 of U and 8 of V
};

template <class F>
__global__ __launch_bounds__(256) void preprocess_yuv420_kernel(const unsigned char *__restrict__ ysrc, const unsigned char *__restrict__ usrc,
                                                                const unsigned char *__restrict__ vsrc, float *__restrict__ dst, int B, int H,
                                                                int W, Yuv420Strides pl, Stats4 st, F f, int fast)
{
    typedef typename F::T T;
    typedef Yuv420Block<F> K;
    constexpr int ES = K::ES, BITS = K::BITS, NX = K::NX, CS = K::CS;
    const size_t nbx = ((size_t)W + NX - 1) / NX, nby = ((size_t)H + 1) / 2, plane = (size_t)H * W, total = (size_t)B * nby * nbx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / (nby * nbx), rem = i - b * nby * nbx, by = rem / nbx;
        const int y0 = (int)by * 2, x0 = (int)(rem - by * nbx) * NX;
        const unsigned char *yp = ysrc + b * pl.bstride[0] + (size_t)y0 * pl.pitch[0] + (size_t)x0 * ES;
        const unsigned char *up = usrc + b * pl.bstride[1] + by * pl.pitch[1] + (size_t)(x0 / 2) * CS * ES;   // chroma sample x0 / 2 of row y0 / 2
        const unsigned char *vp = F::semi ? up + ES : vsrc + b * pl.bstride[2] + by * pl.pitch[2] + (size_t)(x0 / 2) * ES;
        float *o = dst + b * 3 * plane + (size_t)y0 * W + x0;
        if (fast && x0 + NX <= W && y0 + 2 <= H) {
            unsigned uw[K::NC], vw[K::NC];
            load_dwords(up, uw);
            if constexpr (!F::semi) load_dwords(vp, vw);
            const unsigned *vq = F::semi ? uw : vw;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                unsigned yw[K::NW];
                load_dwords(yp + (size_t)r * pl.pitch[0], yw);
#pragma unroll
                for (int q = 0; q < NX / 4; ++q) {   // 4 pixels = 2 chroma samples of each kind = one 16-byte access of each fp32 plane
                    f32x4 out[3];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int p = q * 4 + j, c = CS * (p >> 1);
                        int ch[3];
                        f.decode(f.sample(yuv420p_get<BITS>(yw, p)), f.sample(yuv420p_get<BITS>(uw, c)), f.sample(yuv420p_get<BITS>(vq, c + K::VO)), ch);
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) out[cc][j] = f.norm(ch[cc], st.mean[cc], st.stdv[cc]);
                    }
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) *reinterpret_cast<f32x4 *>(o + cc * plane + (size_t)r * W + q * 4) = out[cc];
                }
            }
            continue;
        }
        const int nx = min(NX, W - x0), ny = min(2, H - y0);
        for (int x = 0; x < nx; ++x) {
            const int c = CS * (x >> 1);
            const int U = f.sample(reinterpret_cast<const T *>(up)[c]), V = f.sample(reinterpret_cast<const T *>(vp)[c]);
            for (int r = 0; r < ny; ++r) {
                int ch[3];
                f.decode(f.sample(reinterpret_cast<const T *>(yp + (size_t)r * pl.pitch[0])[x]), U, V, ch);
                for (int cc = 0; cc < 3; ++cc) o[cc * plane + (size_t)r * W + x] = f.norm(ch[cc], st.mean[cc], st.stdv[cc]);
            }
        }
    }
}

template <class F>
__global__ __launch_bounds__(256) void postprocess_yuv420_kernel(const float *__restrict__ src, unsigned char *__restrict__ ydst,
                                                                 unsigned char *__restrict__ udst, unsigned char *__restrict__ vdst, int B, int H,
                                                                 int W, Yuv420Strides pl, Stats4d st, F f, int denorm, int fast)
{
    typedef typename F::T T;
    typedef Yuv420Block<F> K;
    constexpr int ES = K::ES, BITS = K::BITS, NX = K::NX, CS = K::CS;
    const size_t nbx = ((size_t)W + NX - 1) / NX, nby = ((size_t)H + 1) / 2, plane = (size_t)H * W, total = (size_t)B * nby * nbx;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / (nby * nbx), rem = i - b * nby * nbx, by = rem / nbx;
        const int y0 = (int)by * 2, x0 = (int)(rem - by * nbx) * NX;
        unsigned char *yp = ydst + b * pl.bstride[0] + (size_t)y0 * pl.pitch[0] + (size_t)x0 * ES;
        unsigned char *up = udst + b * pl.bstride[1] + by * pl.pitch[1] + (size_t)(x0 / 2) * CS * ES;
        unsigned char *vp = F::semi ? up + ES : vdst + b * pl.bstride[2] + by * pl.pitch[2] + (size_t)(x0 / 2) * ES;
        const float *s = src + b * 3 * plane;
        if (fast && x0 + NX <= W && y0 + 2 <= H) {
            unsigned yw[2][K::NW] = {}, uw[K::NC] = {}, vw[K::NC] = {};   // the bits of a word that f.word() leaves out stay zero
            unsigned *vq = F::semi ? uw : vw;
#pragma unroll
            for (int q = 0; q < NX / 4; ++q) {
                int v[2][4][3];   // [row][pixel][channel]
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const f32x4 x = *reinterpret_cast<const f32x4 *>(s + c * plane + (size_t)(y0 + r) * W + x0 + q * 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[r][j][c] = f.quant(x[j], st.mean[c], st.stdv[c], denorm);
                    }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) yuv420p_put<BITS>(yw[r], q * 4 + j, f.word(f.luma(v[r][j])));
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    int sum[3], U, V;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[c] = v[0][2 * p][c] + v[0][2 * p + 1][c] + v[1][2 * p][c] + v[1][2 * p + 1][c];
                    f.chroma(sum, U, V);
                    yuv420p_put<BITS>(uw, CS * (q * 2 + p), f.word(U));
                    yuv420p_put<BITS>(vq, CS * (q * 2 + p) + K::VO, f.word(V));
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) store_dwords(yp + (size_t)r * pl.pitch[0], yw[r]);
            store_dwords(up, uw);
            if constexpr (!F::semi) store_dwords(vp, vw);
            continue;
        }
        const int nx = min(NX, W - x0);
        for (int x = 0; x < nx; x += 2) {
            int sum[3] = {0, 0, 0}, U, V;
            for (int r = 0; r < 2; ++r)
                for (int dx = 0; dx < 2; ++dx) {
                    const int yy = min(y0 + r, H - 1), xx = min(x0 + x + dx, W - 1);   // past the last row / column: clamped
                    int ch[3];
                    for (int c = 0; c < 3; ++c) {
                        ch[c] = f.quant(s[c * plane + (size_t)yy * W + xx], st.mean[c], st.stdv[c], denorm);
                        sum[c] += ch[c];
                    }
                    if (yy == y0 + r && xx == x0 + x + dx) reinterpret_cast<T *>(yp + (size_t)r * pl.pitch[0])[x + dx] = (T)f.word(f.luma(ch));
                }
            f.chroma(sum, U, V);
            reinterpret_cast<T *>(up)[CS * (x >> 1)] = (T)f.word(U);
            reinterpret_cast<T *>(vp)[CS * (x >> 1)] = (T)f.word(V);
        }
    }
}

// FAST needs, of every plane, the pointer, the pitch and (B > 1) the batch stride to be multiples of the plane's access width - 16 bytes of Y and
// of interleaved UV, 8 of planar U and V -, a 16-byte aligned fp32 pointer and W % 4 == 0 (every fp32 row then starts on a 16-byte boundary).
// A batch stride is never used at b == 0, so at B == 1 it is not looked at.  (NV12 and P010 looked at it until the formats got one predicate: a
// B == 1 call with an unaligned batch stride took SCALAR then and takes FAST now.  Both paths write the same bytes.)
static bool yuv420_fast_ok(const Yuv420Frame &fr, const void *f32, int B, int W)
{
    const bool semi = fr.layout == YUV420_SEMIPLANAR;
    size_t bad = (uintptr_t)f32 & 15;
    for (int p = 0; p < (semi ? 2 : 3); ++p)
        bad |= ((uintptr_t)fr.plane[p] | fr.strides.pitch[p] | (B > 1 ? fr.strides.bstride[p] : 0)) & ((p == 0 || semi) ? 15 : 7);
    return bad == 0 && W % 4 == 0;
}
static int yuv420_grid(int B, int H, int W, int depth)
{
    const size_t nx = depth == 8 ? 16 : 8, lanes = (size_t)B * (((size_t)H + 1) / 2) * (((size_t)W + nx - 1) / nx);
    return (int)std::min<size_t>((lanes + 255) / 256, (size_t)65535 * 4);
}
int launch_preprocess_yuv420(const Yuv420Frame &src, float *dst, int B, int H, int W, int standard, int order, const float *mean, const float *stdv,
                             hipStream_t s)
{
    Stats4 st{};
    for (int c = 0; c < 3; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    const unsigned char *y = (const unsigned char *)src.plane[0], *u = (const unsigned char *)src.plane[1], *v = (const unsigned char *)src.plane[2];
    const int grid = yuv420_grid(B, H, W, src.depth), fast = yuv420_fast_ok(src, dst, B, W) ? 1 : 0;
    const bool semi = src.layout == YUV420_SEMIPLANAR;
    if (src.depth == 8) {
        const YuvCoef k = yuv_coef(standard, order);
        if (semi) preprocess_yuv420_kernel<<<grid, 256, 0, s>>>(y, u, v, dst, B, H, W, src.strides, st, Yuv8<true>{k}, fast);
        else preprocess_yuv420_kernel<<<grid, 256, 0, s>>>(y, u, v, dst, B, H, W, src.strides, st, Yuv8<false>{k}, fast);
    } else {
        const P010Coef k = p010_coef(standard, src.depth, order);
        if (semi) preprocess_yuv420_kernel<<<grid, 256, 0, s>>>(y, u, v, dst, B, H, W, src.strides, st, Yuv16<true>{k}, fast);
        else preprocess_yuv420_kernel<<<grid, 256, 0, s>>>(y, u, v, dst, B, H, W, src.strides, st, Yuv16<false>{k}, fast);
    }
    return (int)hipGetLastError();
}
int launch_postprocess_yuv420(const float *src, const Yuv420Frame &dst, int B, int H, int W, int standard, int order, const double *mean,
                              const double *stdv, int denorm, hipStream_t s)
{
    Stats4d st{};
    for (int c = 0; c < 3; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    unsigned char *y = (unsigned char *)dst.plane[0], *u = (unsigned char *)dst.plane[1], *v = (unsigned char *)dst.plane[2];
    const int grid = yuv420_grid(B, H, W, dst.depth), fast = yuv420_fast_ok(dst, src, B, W) ? 1 : 0;
    const bool semi = dst.layout == YUV420_SEMIPLANAR;
    if (dst.depth == 8) {
        const YuvCoef k = yuv_coef(standard, order);
        if (semi) postprocess_yuv420_kernel<<<grid, 256, 0, s>>>(src, y, u, v, B, H, W, dst.strides, st, Yuv8<true>{k}, denorm, fast);
        else postprocess_yuv420_kernel<<<grid, 256, 0, s>>>(src, y, u, v, B, H, W, dst.strides, st, Yuv8<false>{k}, denorm, fast);
    } else {
        const P010Coef k = p010_coef(standard, dst.depth, order);
        if (semi) postprocess_yuv420_kernel<<<grid, 256, 0, s>>>(src, y, u, v, B, H, W, dst.strides, st, Yuv16<true>{k}, denorm, fast);
        else postprocess_yuv420_kernel<<<grid, 256, 0, s>>>(src, y, u, v, B, H, W, dst.strides, st, Yuv16<false>{k}, denorm, fast);
    }
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Frames resized on the device (include/emavfi.h, "RESIZE DEFINITION"): the reference's cv2.resize(frame, (int(w * scale), int(h * scale)))
// (inference.py:46), bilinear with half-pixel centres, 11-bit weights, signed 32-bit integer arithmetic.
//   resize_u8_kernel<C>             interleaved bytes [B][Hs][Ws][C] -> bytes [B][Hd][Wd][C] and / or normalised fp32 [B][C][Hd][Wd]
//                                   (= preprocess_u8 of the resized bytes) in one launch;
//   preprocess_nv12_resized_kernel  Y resized as a 1-channel image, UV as a 2-channel image, then nv12_decode / nv12_norm per pixel
//                                   (= preprocess_nv12 of the resized planes) in one launch.
// A workgroup owns a tile of the DESTINATION.  It computes the tile's column table (x0, wx) and row table (y0, wy) once into LDS - the
// integer divisions run per tile edge, not per pixel -, stages the source span the tile needs in LDS (every source byte is fetched once per
// tile; neighbouring tiles share at most one row / column) and blends from there.  A lane owns 4 consecutive destination columns (x 2 rows
// for NV12: two chroma pairs), so that an fp32 plane row is written 16 bytes per lane.  Two access forms, the same per-element arithmetic
// (resize_axis / resize_blend / nv12_decode / nv12_norm):
//   WIDE    16-byte source loads into LDS (source pointer, pitch and batch stride multiples of 16; only chunks that end inside the row -
//           the rest of a row moves byte by byte, pitch padding is never read), 16-byte fp32 stores (Wd % 4 == 0, 16-byte aligned
//           pointer), dword stores of the optional byte outputs (their pointers, pitches and batch strides multiples of 4);
//   SCALAR  byte loads / dword fp32 stores / byte stores: whenever a condition above fails, and for the right remainder of a row.
// A tile whose span does not fit RS_SPAN_BYTES (reductions beyond about 3:1) reads its four taps from global memory instead.
// ------------------------------------------------------------------------------------------
constexpr int RS_SPAN_BYTES = 40 * 1024;
struct Nv12Planes { size_t y_pitch, y_bstride, uv_pitch, uv_bstride; };

// one axis: destination index d of nd <- source indices i0, min(i0 + 1, ns - 1) with weight w / 2048 on the second
__device__ __forceinline__ void resize_axis(int d, int nd, int ns, int &i0, int &w)
{
    const int hi = 2 * nd * (ns - 1);
    int num = (2 * d + 1) * ns - nd;
    num = num < 0 ? 0 : num > hi ? hi : num;
    i0 = num / (2 * nd);
    const int fr = num - i0 * 2 * nd;
    w = (fr * 2048 + nd) / (2 * nd);
}
__device__ __forceinline__ int resize_blend(int p00, int p01, int p10, int p11, int wx, int wy)
{
    const int top = (2048 - wx) * p00 + wx * p01, bot = (2048 - wx) * p10 + wx * p11;
    return ((2048 - wy) * top + wy * bot + (1 << 21)) >> 22;
}
// C interleaved channels of one destination pixel; row0 / row1 point at byte `sub` of the two source rows (LDS or global)
template <int C>
__device__ __forceinline__ void resize_pixel(const unsigned char *row0, const unsigned char *row1, int sub, int x0, int ns, int wx, int wy, int out[C])
{
    const int b0 = x0 * C - sub, b1 = min(x0 + 1, ns - 1) * C - sub;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = resize_blend(row0[b0 + c], row0[b1 + c], row1[b0 + c], row1[b1 + c], wx, wy);
}
// Copies bytes [a0, hi) of rows r0 .. r0 + nrows - 1 of a pitched plane into LDS (row stride ls = (hi - a0) rounded up to 16).  hi <= rowbytes.
// wide: a0, the plane's address and its pitch are multiples of 16, and a chunk that ends inside the row moves as one 16-byte access.
__device__ __forceinline__ void resize_stage(unsigned char *lds, int ls, const unsigned char *plane, size_t pitch, int rowbytes, int r0, int nrows,
                                             int a0, int hi, int wide)
{
    const int chunks = ls >> 4;
    for (int i = threadIdx.x; i < nrows * chunks; i += blockDim.x) {
        const int r = i / chunks, q = i - r * chunks, b0 = a0 + 16 * q;
        const unsigned char *p = plane + (size_t)(r0 + r) * pitch + b0;
        unsigned char *o = lds + r * ls + 16 * q;
        if (wide && b0 + 16 <= rowbytes) {
            *reinterpret_cast<uint4 *>(o) = *reinterpret_cast<const uint4 *>(p);
        } else {
            const int n = min(16, hi - b0);
            for (int j = 0; j < n; ++j) o[j] = p[j];
        }
    }
}
// the span of one axis of a tile: source indices [lo, hi] the n destination entries of the table need
__device__ __forceinline__ void resize_span(const int *i0, int n, int ns, int &lo, int &hi)
{
    lo = i0[0];
    hi = min(i0[n - 1] + 1, ns - 1);
}

struct ResizeArgs {
    const unsigned char *src; size_t src_pitch, src_bstride;
    unsigned char *dst; size_t dst_pitch, dst_bstride;   // dst may be null
    float *f32;                                          // may be null
    int Hs, Ws, Hd, Wd, wide_src, wide_f32, wide_u8;
};

template <int C>
__global__ __launch_bounds__(256) void resize_u8_kernel(ResizeArgs a, Stats4 st)
{
    constexpr int TW = 64, TH = 16;   // 16 x 16 lanes of 1 row x 4 columns
    __shared__ __attribute__((aligned(16))) unsigned char span[RS_SPAN_BYTES];
    __shared__ int cx0[TW], cwx[TW], ry0[TH], rwy[TH];
    const int tid = threadIdx.x, X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    const size_t b = blockIdx.z;
    if (tid < TW) resize_axis(min(X0 + tid, a.Wd - 1), a.Wd, a.Ws, cx0[tid], cwx[tid]);
    else if (tid < TW + TH) resize_axis(min(Y0 + tid - TW, a.Hd - 1), a.Hd, a.Hs, ry0[tid - TW], rwy[tid - TW]);
    __syncthreads();
    const int nx = min(TW, a.Wd - X0), ny = min(TH, a.Hd - Y0);
    int ys_lo, ys_hi, xs_lo, xs_hi;
    resize_span(ry0, ny, a.Hs, ys_lo, ys_hi);
    resize_span(cx0, nx, a.Ws, xs_lo, xs_hi);
    const int lo = xs_lo * C, hi = (xs_hi + 1) * C, a0 = a.wide_src ? (lo & ~15) : lo, ls = (hi - a0 + 15) & ~15, nrows = ys_hi - ys_lo + 1;
    const unsigned char *plane = a.src + b * a.src_bstride;
    const bool staged = (long long)nrows * ls <= RS_SPAN_BYTES;   // uniform over the workgroup
    if (staged) {
        resize_stage(span, ls, plane, a.src_pitch, a.Ws * C, ys_lo, nrows, a0, hi, a.wide_src);
        __syncthreads();
    }
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    if (r >= ny || c4 >= nx) return;
    const int n = min(4, nx - c4), y = Y0 + r, y0 = ry0[r], y1 = min(y0 + 1, a.Hs - 1), wy = rwy[r];
    int v[4][C];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < n) {
            if (staged) resize_pixel<C>(span + (y0 - ys_lo) * ls, span + (y1 - ys_lo) * ls, a0, cx0[c4 + j], a.Ws, cwx[c4 + j], wy, v[j]);
            else resize_pixel<C>(plane + (size_t)y0 * a.src_pitch, plane + (size_t)y1 * a.src_pitch, 0, cx0[c4 + j], a.Ws, cwx[c4 + j], wy, v[j]);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) v[j][c] = 0;
        }
    }
    if (a.dst) {
        unsigned char *o = a.dst + b * a.dst_bstride + (size_t)y * a.dst_pitch + (size_t)(X0 + c4) * C;
        if (a.wide_u8 && n == 4) {
            unsigned w[C];
#pragma unroll
            for (int q = 0; q < C; ++q) w[q] = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) w[(j * C + c) >> 2] |= (unsigned)v[j][c] << (8 * ((j * C + c) & 3));
#pragma unroll
            for (int q = 0; q < C; ++q) reinterpret_cast<unsigned *>(o)[q] = w[q];
        } else {
            for (int j = 0; j < n; ++j)
                for (int c = 0; c < C; ++c) o[j * C + c] = (unsigned char)v[j][c];
        }
    }
    if (a.f32) {
        const size_t dplane = (size_t)a.Hd * a.Wd;
        float *o = a.f32 + b * C * dplane + (size_t)y * a.Wd + X0 + c4;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (a.wide_f32 && n == 4) {
                *reinterpret_cast<f32x4 *>(o + c * dplane) = f32x4{nv12_norm(v[0][c], st.mean[c], st.stdv[c]), nv12_norm(v[1][c], st.mean[c], st.stdv[c]),
                                                                   nv12_norm(v[2][c], st.mean[c], st.stdv[c]), nv12_norm(v[3][c], st.mean[c], st.stdv[c])};
            } else {
                for (int j = 0; j < n; ++j) o[c * dplane + j] = nv12_norm(v[j][c], st.mean[c], st.stdv[c]);
            }
        }
    }
}

struct ResizeNv12Args {
    const unsigned char *y, *uv; Nv12Planes in;
    float *f32;
    unsigned char *yo, *uvo; Nv12Planes out;             // yo / uvo may be null
    int Hs, Ws, Hd, Wd, wide_src, wide_f32, wide_out;
};

__global__ __launch_bounds__(256) void preprocess_nv12_resized_kernel(ResizeNv12Args a, Stats4 st, YuvCoef k)
{
    constexpr int TW = 64, TH = 32;   // luma tile: 16 x 16 lanes of 2 rows x 4 columns = 2 chroma pairs each
    __shared__ __attribute__((aligned(16))) unsigned char span[RS_SPAN_BYTES];
    __shared__ int yx0[TW], ywx[TW], yy0[TH], ywy[TH], ux0[TW / 2], uwx[TW / 2], uy0[TH / 2], uwy[TH / 2];
    const int tid = threadIdx.x, X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    const size_t b = blockIdx.z;
    const int Hs2 = (a.Hs + 1) / 2, Ws2 = (a.Ws + 1) / 2, Hd2 = (a.Hd + 1) / 2, Wd2 = (a.Wd + 1) / 2;
    if (tid < 64) resize_axis(min(X0 + tid, a.Wd - 1), a.Wd, a.Ws, yx0[tid], ywx[tid]);
    else if (tid < 96) resize_axis(min(Y0 + tid - 64, a.Hd - 1), a.Hd, a.Hs, yy0[tid - 64], ywy[tid - 64]);
    else if (tid < 128) resize_axis(min(X0 / 2 + tid - 96, Wd2 - 1), Wd2, Ws2, ux0[tid - 96], uwx[tid - 96]);
    else if (tid < 144) resize_axis(min(Y0 / 2 + tid - 128, Hd2 - 1), Hd2, Hs2, uy0[tid - 128], uwy[tid - 128]);
    __syncthreads();
    const int nx = min(TW, a.Wd - X0), ny = min(TH, a.Hd - Y0), nxc = (nx + 1) / 2, nyc = (ny + 1) / 2;
    int ys_lo, ys_hi, xs_lo, xs_hi, us_lo, us_hi, ucs_lo, ucs_hi;
    resize_span(yy0, ny, a.Hs, ys_lo, ys_hi);
    resize_span(yx0, nx, a.Ws, xs_lo, xs_hi);
    resize_span(uy0, nyc, Hs2, us_lo, us_hi);
    resize_span(ux0, nxc, Ws2, ucs_lo, ucs_hi);
    const int yhi = xs_hi + 1, ya0 = a.wide_src ? (xs_lo & ~15) : xs_lo, yls = (yhi - ya0 + 15) & ~15, yrows = ys_hi - ys_lo + 1;
    const int uhi = (ucs_hi + 1) * 2, ua0 = a.wide_src ? ((ucs_lo * 2) & ~15) : ucs_lo * 2, uls = (uhi - ua0 + 15) & ~15, urows = us_hi - us_lo + 1;
    const unsigned char *yplane = a.y + b * a.in.y_bstride, *uvplane = a.uv + b * a.in.uv_bstride;
    unsigned char *const uspan = span + yrows * yls;
    const bool staged = (long long)yrows * yls + (long long)urows * uls <= RS_SPAN_BYTES;   // uniform over the workgroup
    if (staged) {
        resize_stage(span, yls, yplane, a.in.y_pitch, a.Ws, ys_lo, yrows, ya0, yhi, a.wide_src);
        resize_stage(uspan, uls, uvplane, a.in.uv_pitch, 2 * Ws2, us_lo, urows, ua0, uhi, a.wide_src);
        __syncthreads();
    }
    const int r2 = tid >> 4, c4 = (tid & 15) * 4;
    if (2 * r2 >= ny || c4 >= nx) return;
    const int n = min(4, nx - c4), np = (n + 1) / 2, nr = min(2, ny - 2 * r2), cc = c4 / 2;
    int UV[2][2] = {{128, 128}, {128, 128}};
    {
        const int y0 = uy0[r2], y1 = min(y0 + 1, Hs2 - 1), wy = uwy[r2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (p < np) {
                if (staged) resize_pixel<2>(uspan + (y0 - us_lo) * uls, uspan + (y1 - us_lo) * uls, ua0, ux0[cc + p], Ws2, uwx[cc + p], wy, UV[p]);
                else resize_pixel<2>(uvplane + (size_t)y0 * a.in.uv_pitch, uvplane + (size_t)y1 * a.in.uv_pitch, 0, ux0[cc + p], Ws2, uwx[cc + p], wy, UV[p]);
            }
    }
    if (a.uvo) {
        unsigned char *o = a.uvo + b * a.out.uv_bstride + (size_t)(Y0 / 2 + r2) * a.out.uv_pitch + X0 + c4;   // pair (X0 + c4) / 2 starts at byte X0 + c4
        if (a.wide_out && np == 2) {
            *reinterpret_cast<unsigned *>(o) = (unsigned)UV[0][0] | ((unsigned)UV[0][1] << 8) | ((unsigned)UV[1][0] << 16) | ((unsigned)UV[1][1] << 24);
        } else {
            for (int p = 0; p < np; ++p) { o[2 * p] = (unsigned char)UV[p][0]; o[2 * p + 1] = (unsigned char)UV[p][1]; }
        }
    }
    const size_t dplane = (size_t)a.Hd * a.Wd;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        if (rr >= nr) break;
        const int r = 2 * r2 + rr, y = Y0 + r, y0 = yy0[r], y1 = min(y0 + 1, a.Hs - 1), wy = ywy[r];
        int Y[4] = {0, 0, 0, 0};
        float out[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                if (staged) resize_pixel<1>(span + (y0 - ys_lo) * yls, span + (y1 - ys_lo) * yls, ya0, yx0[c4 + j], a.Ws, ywx[c4 + j], wy, &Y[j]);
                else resize_pixel<1>(yplane + (size_t)y0 * a.in.y_pitch, yplane + (size_t)y1 * a.in.y_pitch, 0, yx0[c4 + j], a.Ws, ywx[c4 + j], wy, &Y[j]);
            }
            int ch[3];
            nv12_decode(Y[j], UV[j >> 1][0], UV[j >> 1][1], k, ch);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c][j] = nv12_norm(ch[c], st.mean[c], st.stdv[c]);
        }
        if (a.yo) {
            unsigned char *o = a.yo + b * a.out.y_bstride + (size_t)y * a.out.y_pitch + X0 + c4;
            if (a.wide_out && n == 4) {
                *reinterpret_cast<unsigned *>(o) = (unsigned)Y[0] | ((unsigned)Y[1] << 8) | ((unsigned)Y[2] << 16) | ((unsigned)Y[3] << 24);
            } else {
                for (int j = 0; j < n; ++j) o[j] = (unsigned char)Y[j];
            }
        }
        float *o = a.f32 + b * 3 * dplane + (size_t)y * a.Wd + X0 + c4;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.wide_f32 && n == 4) {
                *reinterpret_cast<f32x4 *>(o + c * dplane) = f32x4{out[c][0], out[c][1], out[c][2], out[c][3]};
            } else {
                for (int j = 0; j < n; ++j) o[c * dplane + j] = out[c][j];
            }
        }
    }
}

static bool mult_of(unsigned m, std::initializer_list<size_t> v)
{
    size_t acc = 0;
    for (size_t x : v) acc |= x;
    return (acc & (m - 1)) == 0;
}
int launch_resize_u8(const unsigned char *src, size_t src_pitch, size_t src_bstride, unsigned char *dst_u8, size_t dst_pitch, size_t dst_bstride,
                     float *dst_f32, int B, int Hs, int Ws, int Hd, int Wd, int C, const float *mean, const float *stdv, hipStream_t s)
{
    Stats4 st{};
    for (int c = 0; c < C && c < 4; ++c) { st.mean[c] = mean ? mean[c] : 0.0f; st.stdv[c] = stdv ? stdv[c] : 1.0f; }
    ResizeArgs a{src, src_pitch, src_bstride, dst_u8, dst_pitch, dst_bstride, dst_f32, Hs, Ws, Hd, Wd, 0, 0, 0};
    a.wide_src = mult_of(16, {(size_t)(uintptr_t)src, src_pitch, B > 1 ? src_bstride : 0});
    a.wide_f32 = dst_f32 && mult_of(16, {(size_t)(uintptr_t)dst_f32}) && Wd % 4 == 0;
    a.wide_u8 = dst_u8 && mult_of(4, {(size_t)(uintptr_t)dst_u8, dst_pitch, B > 1 ? dst_bstride : 0});
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)((Hd + 15) / 16), (unsigned)B);
    switch (C) {
    case 1: resize_u8_kernel<1><<<grid, 256, 0, s>>>(a, st); break;
    case 2: resize_u8_kernel<2><<<grid, 256, 0, s>>>(a, st); break;
    case 3: resize_u8_kernel<3><<<grid, 256, 0, s>>>(a, st); break;
    default: resize_u8_kernel<4><<<grid, 256, 0, s>>>(a, st); break;
    }
    return (int)hipGetLastError();
}
int launch_preprocess_nv12_resized(const unsigned char *y, size_t y_pitch, size_t y_bstride, const unsigned char *uv, size_t uv_pitch,
                                   size_t uv_bstride, float *dst, unsigned char *y_out, size_t yo_pitch, size_t yo_bstride, unsigned char *uv_out,
                                   size_t uvo_pitch, size_t uvo_bstride, int B, int Hs, int Ws, int Hd, int Wd, int standard, int order,
                                   const float *mean, const float *stdv, hipStream_t s)
{
    Stats4 st{};
    for (int c = 0; c < 3; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    ResizeNv12Args a{y, uv, Nv12Planes{y_pitch, y_bstride, uv_pitch, uv_bstride}, dst, y_out, uv_out, Nv12Planes{yo_pitch, yo_bstride, uvo_pitch, uvo_bstride},
                     Hs, Ws, Hd, Wd, 0, 0, 0};
    a.wide_src = mult_of(16, {(size_t)(uintptr_t)y, (size_t)(uintptr_t)uv, y_pitch, uv_pitch, B > 1 ? y_bstride : 0, B > 1 ? uv_bstride : 0});
    a.wide_f32 = mult_of(16, {(size_t)(uintptr_t)dst}) && Wd % 4 == 0;
    a.wide_out = mult_of(4, {y_out ? (size_t)(uintptr_t)y_out | yo_pitch | (B > 1 ? yo_bstride : 0) : 0,
                             uv_out ? (size_t)(uintptr_t)uv_out | uvo_pitch | (B > 1 ? uvo_bstride : 0) : 0});
    const dim3 grid((unsigned)((Wd + 63) / 64), (unsigned)((Hd + 31) / 32), (unsigned)B);
    preprocess_nv12_resized_kernel<<<grid, 256, 0, s>>>(a, st, yuv_coef(standard, order));
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Scene cuts decided and applied on the device (include/emavfi.h, "SCENE CUT DEFINITION"; per-element functions: scene_elem.h).
//   luma_signature_kernel<C>  bytes [B][H][W][C] (C = 1: a Y plane, C = 3: interleaved colour) -> sig [B][32][32] u32, the luma sum of each cell.
//                             The one pass that touches every byte.  Grid (32 cell rows, 4 groups of 8 cell columns, B): 1152 workgroups for
//                             nine frames.  A workgroup OWNS the 8 cells it stores - no global atomics, no zeroing beforehand.  A lane takes
//                             units of 16 pixels on the frame's 16-pixel lattice (so a unit starts on a 16-byte boundary of an aligned row) and
//                             adds each cell's part of a unit into its own LDS slot [cell][lane] (plain LDS adds, nothing shared); at the end
//                             32 lanes per cell sum the 256 slots and finish with a wave reduction.  A unit on the edge of the group is read by
//                             both neighbours, each keeping its own columns.  Two access forms, the same per-element arithmetic:
//                               WIDE    C 16-byte loads per unit (pointer, pitch and batch stride multiples of 16; only units that end inside the
//                                       row - pitch padding is never read);
//                               SCALAR  byte loads: whenever a condition above fails, and for the right remainder of a row.
//   scene_flags_kernel        one workgroup per pair: sum over the cells of |mean_a - mean_b| -> scores[k], flags[k] = score >= threshold
//   hold_frames_kernel        grid (32 KiB pieces of a frame, rep, n): a workgroup of an unflagged pair leaves at once; the others copy their
//                             piece of alt[k] over frame k rep + r, 16 bytes per lane where both frame addresses allow, bytes elsewhere
// ------------------------------------------------------------------------------------------
constexpr int SG_CELLS = 8, SG_GROUPS = SCENE_GRID / SG_CELLS;
struct SigArgs { const unsigned char *src; size_t pitch, bstride; unsigned *sig; int H, W, rgb, wide; };

template <int C>
__global__ __launch_bounds__(256) void luma_signature_kernel(SigArgs a)
{
    __shared__ unsigned slot[SG_CELLS * 256];
    __shared__ int cb[SG_CELLS + 1];
    const int tid = threadIdx.x, ci = blockIdx.x, g = blockIdx.y;
    const size_t b = blockIdx.z;
    const int y0 = scene_cell_bound(ci, a.H), y1 = scene_cell_bound(ci + 1, a.H);
    if (tid <= SG_CELLS) cb[tid] = scene_cell_bound(g * SG_CELLS + tid, a.W);
#pragma unroll
    for (int k = 0; k < SG_CELLS; ++k) slot[k * 256 + tid] = 0u;
    __syncthreads();
    const int xlo = cb[0], xhi = cb[SG_CELLS];   // xhi <= W
    if (y1 > y0 && xhi > xlo) {                  // uniform over the workgroup
        const int u0 = xlo >> 4, nu = ((xhi + 15) >> 4) - u0, items = (y1 - y0) * nu;
        const unsigned char *plane = a.src + b * a.bstride;
        for (int t = tid; t < items; t += 256) {
            const int r = t / nu, x0 = (u0 + (t - r * nu)) << 4;
            const unsigned char *p = plane + (size_t)(y0 + r) * a.pitch + (size_t)x0 * C;
            unsigned w[4 * C];
            if (a.wide && x0 + 16 <= a.W) {
#pragma unroll
                for (int q = 0; q < C; ++q) {
                    const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
                    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
                }
            } else {
                const int nb = min(16, a.W - x0) * C;
#pragma unroll
                for (int q = 0; q < 4 * C; ++q) w[q] = 0u;
#pragma unroll
                for (int k = 0; k < 16 * C; ++k)
                    if (k < nb) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
            }
            int j = 0, hi = cb[1];
            unsigned acc = 0u;
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const int x = x0 + px;
                if (x >= xlo && x < xhi) {
                    while (x >= hi) {            // ends at j <= 7: x < xhi = cb[8]
                        slot[j * 256 + tid] += acc;
                        acc = 0u;
                        ++j;
                        hi = cb[j + 1];
                    }
                    if constexpr (C == 1) {
                        acc += (w[px >> 2] >> (8 * (px & 3))) & 0xffu;
                    } else {
                        const int k = 3 * px;
                        acc += scene_luma3((w[k >> 2] >> (8 * (k & 3))) & 0xffu, (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu,
                                           (w[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 0xffu, a.rgb);
                    }
                }
            }
            slot[j * 256 + tid] += acc;
        }
    }
    __syncthreads();
    const int c = tid >> 5, l = tid & 31;
    unsigned s = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += slot[c * 256 + l + 32 * k];
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 32);
    if (l == 0) a.sig[b * (SCENE_GRID * SCENE_GRID) + ci * SCENE_GRID + g * SG_CELLS + c] = s;
}

__global__ __launch_bounds__(256) void scene_flags_kernel(const unsigned *__restrict__ sig_a, size_t stride_a, const unsigned *__restrict__ sig_b,
                                                          size_t stride_b, int H, int W, unsigned threshold, unsigned *__restrict__ flags,
                                                          unsigned *__restrict__ scores)
{
    __shared__ unsigned part[4];
    const int tid = threadIdx.x;
    const size_t k = blockIdx.x;
    const unsigned *sa = sig_a + k * stride_a, *sb = sig_b + k * stride_b;
    unsigned s = 0u;
    for (int c = tid; c < SCENE_GRID * SCENE_GRID; c += 256) {
        const int i = c >> 5, j = c & 31;
        const unsigned n = (unsigned)(scene_cell_bound(i + 1, H) - scene_cell_bound(i, H)) * (unsigned)(scene_cell_bound(j + 1, W) - scene_cell_bound(j, W));
        if (n) {
            const unsigned ma = scene_cell_mean(sa[c], n), mb = scene_cell_mean(sb[c], n);
            s += ma > mb ? ma - mb : mb - ma;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const unsigned score = part[0] + part[1] + part[2] + part[3];
        flags[k] = score >= threshold ? 1u : 0u;
        if (scores) scores[k] = score;
    }
}

constexpr size_t HOLD_PIECE = 32768;   // bytes of a frame per workgroup, a multiple of 16
__global__ __launch_bounds__(256) void hold_frames_kernel(unsigned char *dst, size_t dst_stride, int rep, const unsigned char *alt, size_t alt_stride,
                                                          const unsigned *__restrict__ flags, size_t frame_bytes)
{
    const size_t k = blockIdx.z;
    if (!flags[k]) return;
    unsigned char *d = dst + (k * (size_t)rep + blockIdx.y) * dst_stride;
    const unsigned char *s = alt + k * alt_stride;
    const size_t lo = (size_t)blockIdx.x * HOLD_PIECE, hi = lo + HOLD_PIECE < frame_bytes ? lo + HOLD_PIECE : frame_bytes;
    size_t x = lo + threadIdx.x;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        const size_t nv = (hi - lo) >> 4;
        for (size_t q = threadIdx.x; q < nv; q += 256) reinterpret_cast<uint4 *>(d + lo)[q] = reinterpret_cast<const uint4 *>(s + lo)[q];
        x += nv << 4;
    }
    for (; x < hi; x += 256) d[x] = s[x];
}

int launch_luma_signature_u8(const unsigned char *src, size_t pitch, size_t bstride, int B, int H, int W, int C, int order, unsigned *sig, hipStream_t s)
{
    SigArgs a{src, pitch, bstride, sig, H, W, order == 1, 0};
    a.wide = mult_of(16, {(size_t)(uintptr_t)src, pitch, B > 1 ? bstride : 0});
    const dim3 grid(SCENE_GRID, SG_GROUPS, (unsigned)B);
    if (C == 1) luma_signature_kernel<1><<<grid, 256, 0, s>>>(a);
    else luma_signature_kernel<3><<<grid, 256, 0, s>>>(a);
    return (int)hipGetLastError();
}
int launch_scene_flags(const unsigned *sig_a, size_t stride_a, const unsigned *sig_b, size_t stride_b, int n, int H, int W, unsigned threshold,
                       unsigned *flags, unsigned *scores, hipStream_t s)
{
    scene_flags_kernel<<<dim3((unsigned)n), 256, 0, s>>>(sig_a, stride_a, sig_b, stride_b, H, W, threshold, flags, scores);
    return (int)hipGetLastError();
}
int launch_hold_frames_u8(unsigned char *dst, size_t dst_stride, int rep, const unsigned char *alt, size_t alt_stride, const unsigned *flags, int n,
                          size_t frame_bytes, hipStream_t s)
{
    const dim3 grid((unsigned)((frame_bytes + HOLD_PIECE - 1) / HOLD_PIECE), (unsigned)rep, (unsigned)n);
    hold_frames_kernel<<<grid, 256, 0, s>>>(dst, dst_stride, rep, alt, alt_stride, flags, frame_bytes);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Duplicate frames found on the device (include/emavfi.h, "DUPLICATE FRAME DEFINITION"; per-element functions: dedup_elem.h and, for the
// cells and the 3-byte luma, scene_elem.h).
//   frame_diff_cells_kernel<BPP>  two images of BPP bytes per pixel (1: C = 1 bytes, 2: C = 1 words, 3: C = 3 bytes) -> cells [n][32][32] u32, per
//                                 cell the ceiling of the mean absolute luma difference in sixteenths of a count.  The structure is the
//                                 signature kernel's: grid (32 cell rows, 4 groups of 8 cell columns, n), a workgroup OWNS the 8 cells it
//                                 stores - no global atomics, no zeroing -, a lane takes units of 16 pixels on the frame's 16-pixel lattice
//                                 and adds each cell's part of a unit into its own LDS slot [cell][lane].  Per image, two access forms with
//                                 the same per-element arithmetic:
//                                   WIDE    BPP 16-byte loads per unit (pointer, pitch and batch stride multiples of 16; only units that end
//                                           inside the row - pitch padding is never read);
//                                   SCALAR  byte loads: whenever a condition above fails, and for the right remainder of a row.
//                                 A slot is u32: a workgroup has at most 512 rows x 257 units (a group spans at most 4096 columns and may
//                                 start inside a unit), so a lane takes at most ceil(512 * 257 / 256) = 515 units = 8240 pixels, and
//                                 8240 * 65535 < 2^30 even when every one of them falls into one cell.  The cell total over the 256 slots
//                                 is 64-bit (a 257 x 256 cell of 16-bit samples already passes 2^32).  Reads both images once, waits on nothing.
//   duplicate_flags_kernel        one workgroup per pair: the maximum over the 1024 cells -> scores[k], flags[k] = score <= threshold
// ------------------------------------------------------------------------------------------
struct DiffArgs { const unsigned char *img[2]; size_t pitch[2], bstride[2]; unsigned *cells; int H, W, rgb, wide[2], shift; unsigned mask; };

// the 16 pixels of one unit as they lie in memory, little-endian in w; nb: the bytes of the unit that lie inside the row (the rest reads as 0)
template <int BPP>
__device__ inline void diff_load_unit(const unsigned char *p, bool wide, int nb, unsigned (&w)[4 * BPP])
{
    if (wide) {
#pragma unroll
        for (int q = 0; q < BPP; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4 * BPP; ++q) w[q] = 0u;
#pragma unroll
        for (int k = 0; k < 16 * BPP; ++k)
            if (k < nb) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    }
}

template <int BPP>
__device__ inline unsigned diff_luma(const unsigned (&w)[4 * BPP], int px, unsigned mask, int shift, int rgb)
{
    if constexpr (BPP == 1) {
        return dedup_sample((w[px >> 2] >> (8 * (px & 3))) & 0xffu, mask, shift);
    } else if constexpr (BPP == 2) {
        return dedup_sample((w[px >> 1] >> (16 * (px & 1))) & 0xffffu, mask, shift);
    } else {
        const int k = 3 * px;
        return scene_luma3((w[k >> 2] >> (8 * (k & 3))) & 0xffu, (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu,
                           (w[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 0xffu, rgb);
    }
}

template <int BPP>
__global__ __launch_bounds__(256) void frame_diff_cells_kernel(DiffArgs a)
{
    __shared__ unsigned slot[SG_CELLS * 256];
    __shared__ int cb[SG_CELLS + 1];
    const int tid = threadIdx.x, ci = blockIdx.x, g = blockIdx.y;
    const size_t b = blockIdx.z;
    const int y0 = scene_cell_bound(ci, a.H), y1 = scene_cell_bound(ci + 1, a.H);
    if (tid <= SG_CELLS) cb[tid] = scene_cell_bound(g * SG_CELLS + tid, a.W);
#pragma unroll
    for (int k = 0; k < SG_CELLS; ++k) slot[k * 256 + tid] = 0u;
    __syncthreads();
    const int xlo = cb[0], xhi = cb[SG_CELLS];   // xhi <= W
    if (y1 > y0 && xhi > xlo) {                  // uniform over the workgroup
        const int u0 = xlo >> 4, nu = ((xhi + 15) >> 4) - u0, items = (y1 - y0) * nu;
        const unsigned char *pa = a.img[0] + b * a.bstride[0], *pb = a.img[1] + b * a.bstride[1];
        for (int t = tid; t < items; t += 256) {
            const int r = t / nu, x0 = (u0 + (t - r * nu)) << 4;      // x0 < xhi <= W
            const bool inside = x0 + 16 <= a.W;
            const int nb = min(16, a.W - x0) * BPP;
            unsigned wa[4 * BPP], wb[4 * BPP];
            diff_load_unit<BPP>(pa + (size_t)(y0 + r) * a.pitch[0] + (size_t)x0 * BPP, a.wide[0] && inside, nb, wa);
            diff_load_unit<BPP>(pb + (size_t)(y0 + r) * a.pitch[1] + (size_t)x0 * BPP, a.wide[1] && inside, nb, wb);
            int j = 0, hi = cb[1];
            unsigned acc = 0u;
#pragma unroll
            for (int px = 0; px < 16; ++px) {
                const int x = x0 + px;
                if (x >= xlo && x < xhi) {
                    while (x >= hi) {            // ends at j <= 7: x < xhi = cb[8]
                        slot[j * 256 + tid] += acc;
                        acc = 0u;
                        ++j;
                        hi = cb[j + 1];
                    }
                    acc += dedup_absdiff(diff_luma<BPP>(wa, px, a.mask, a.shift, a.rgb), diff_luma<BPP>(wb, px, a.mask, a.shift, a.rgb));
                }
            }
            slot[j * 256 + tid] += acc;
        }
    }
    __syncthreads();
    const int c = tid >> 5, l = tid & 31;
    unsigned long long s = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += slot[c * 256 + l + 32 * k];
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) s += __shfl_xor(s, off, 32);
    if (l == 0) {
        const unsigned n = (unsigned)(y1 - y0) * (unsigned)(cb[c + 1] - cb[c]);
        a.cells[b * DEDUP_CELLS + ci * SCENE_GRID + g * SG_CELLS + c] = n ? dedup_cell_measure(s, n) : 0u;
    }
}

__global__ __launch_bounds__(256) void duplicate_flags_kernel(const unsigned *__restrict__ cells, size_t stride, unsigned threshold,
                                                              unsigned *__restrict__ flags, unsigned *__restrict__ scores)
{
    __shared__ unsigned part[4];
    const int tid = threadIdx.x;
    const size_t k = blockIdx.x;
    const unsigned *c = cells + k * stride;
    unsigned m = 0u;
    for (int i = tid; i < DEDUP_CELLS; i += 256) m = max(m, c[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor(m, off, 64));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        const unsigned score = max(max(part[0], part[1]), max(part[2], part[3]));
        flags[k] = score <= threshold ? 1u : 0u;
        if (scores) scores[k] = score;
    }
}

int launch_frame_diff_cells(const unsigned char *a, size_t a_pitch, size_t a_bstride, const unsigned char *b, size_t b_pitch, size_t b_bstride, int n,
                            int H, int W, int C, int order, int sample_bytes, int depth, int shift, unsigned *cells, hipStream_t s)
{
    DiffArgs p{{a, b}, {a_pitch, b_pitch}, {a_bstride, b_bstride}, cells, H, W, order == 1, {0, 0}, shift, (1u << depth) - 1u};
    p.wide[0] = mult_of(16, {(size_t)(uintptr_t)a, a_pitch, n > 1 ? a_bstride : 0});
    p.wide[1] = mult_of(16, {(size_t)(uintptr_t)b, b_pitch, n > 1 ? b_bstride : 0});
    const dim3 grid(SCENE_GRID, SG_GROUPS, (unsigned)n);
    if (C == 3) frame_diff_cells_kernel<3><<<grid, 256, 0, s>>>(p);
    else if (sample_bytes == 2) frame_diff_cells_kernel<2><<<grid, 256, 0, s>>>(p);
    else frame_diff_cells_kernel<1><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}
int launch_duplicate_flags(const unsigned *cells, size_t stride, int n, unsigned threshold, unsigned *flags, unsigned *scores, hipStream_t s)
{
    duplicate_flags_kernel<<<dim3((unsigned)n), 256, 0, s>>>(cells, stride, threshold, flags, scores);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Temporal resampling: the output frames of a batch assembled from its source and node frames (include/emavfi.h, "TEMPORAL RESAMPLE
// DEFINITION"; per-element functions: resample_elem.h).
//   resample_frames_kernel   grid (32 KiB pieces of a frame, entries of this launch).  The table travels as kernel arguments, at most
//                            RESAMPLE_CAP entries per launch; a workgroup reads its entry (and, for an entry with a flag index, that one
//                            flag word), and then either copies its piece of ONE frame - a held, w = 0 or w = 256 entry never forms the
//                            address of the frame it does not use - or blends its piece of two.  16 bytes per lane where every frame
//                            address the entry uses is 16-byte aligned (the last frame_bytes % 16 bytes: bytes / words), else bytes / words
//                            throughout, through the same per-element functions.  Nothing waits on anything: no LDS, no atomics.
// ------------------------------------------------------------------------------------------
struct ResampleArgs {
    unsigned char *dst;              // the first output frame of THIS launch
    size_t dst_stride;
    const unsigned char *srcs;
    size_t src_stride;
    const unsigned char *nodes;
    size_t node_stride;
    const unsigned *flags;
    size_t frame_bytes;
    int sample_bytes, shift;
    unsigned mask;
    ResampleEntry e[RESAMPLE_CAP];
};
static_assert(sizeof(ResampleArgs) <= 2048, "the table must fit the kernel argument segment");

__global__ __launch_bounds__(256) void resample_frames_kernel(ResampleArgs p)
{
    const ResampleEntry e = p.e[blockIdx.y];
    unsigned ia = e.a, w = e.w;
    if (p.flags && e.f && p.flags[e.f - 1]) { ia = e.h; w = 0u; }     // held: source frame h (pool bit clear)
    else if (w == 256u) { ia = e.b; w = 0u; }                         // b alone
    const auto frame = [&](unsigned i) {
        return (i & RESAMPLE_POOL_NODES) ? p.nodes + (size_t)(i & ~RESAMPLE_POOL_NODES) * p.node_stride : p.srcs + (size_t)i * p.src_stride;
    };
    unsigned char *d = p.dst + (size_t)blockIdx.y * p.dst_stride;
    const unsigned char *a = frame(ia);
    const size_t lo = (size_t)blockIdx.x * HOLD_PIECE, hi = lo + HOLD_PIECE < p.frame_bytes ? lo + HOLD_PIECE : p.frame_bytes;
    size_t x = lo;
    if (w == 0u) {
        if ((((uintptr_t)d | (uintptr_t)a) & 15) == 0) {
            const size_t nv = (hi - lo) >> 4;
            for (size_t q = threadIdx.x; q < nv; q += 256) reinterpret_cast<uint4 *>(d + lo)[q] = reinterpret_cast<const uint4 *>(a + lo)[q];
            x += nv << 4;
        }
        for (x += threadIdx.x; x < hi; x += 256) d[x] = a[x];
        return;
    }
    const unsigned char *b = frame(e.b);
    if ((((uintptr_t)d | (uintptr_t)a | (uintptr_t)b) & 15) == 0) {
        const size_t nv = (hi - lo) >> 4;
        for (size_t q = threadIdx.x; q < nv; q += 256) {
            const uint4 va = reinterpret_cast<const uint4 *>(a + lo)[q], vb = reinterpret_cast<const uint4 *>(b + lo)[q];
            uint4 r;
            r.x = resample_blend_dword(va.x, vb.x, w, p.sample_bytes, p.mask, p.shift);
            r.y = resample_blend_dword(va.y, vb.y, w, p.sample_bytes, p.mask, p.shift);
            r.z = resample_blend_dword(va.z, vb.z, w, p.sample_bytes, p.mask, p.shift);
            r.w = resample_blend_dword(va.w, vb.w, w, p.sample_bytes, p.mask, p.shift);
            reinterpret_cast<uint4 *>(d + lo)[q] = r;
        }
        x += nv << 4;
    }
    if (p.sample_bytes == 1) {
        for (x += threadIdx.x; x < hi; x += 256) d[x] = (unsigned char)resample_blend(a[x], b[x], w);
    } else {                                                          // frame_bytes, lo and every frame address are even
        for (x += 2 * (size_t)threadIdx.x; x < hi; x += 512)
            *reinterpret_cast<unsigned short *>(d + x) = (unsigned short)resample_blend_word(
                *reinterpret_cast<const unsigned short *>(a + x), *reinterpret_cast<const unsigned short *>(b + x), w, p.mask, p.shift);
    }
}

int launch_resample_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                           const unsigned char *nodes, size_t node_stride, const ResampleEntry *table, const unsigned *flags, size_t frame_bytes,
                           int sample_bytes, int depth, int shift, hipStream_t s)
{
    ResampleArgs p{};
    p.dst_stride = dst_stride; p.srcs = srcs; p.src_stride = src_stride; p.nodes = nodes; p.node_stride = node_stride;
    p.flags = flags; p.frame_bytes = frame_bytes; p.sample_bytes = sample_bytes; p.shift = shift; p.mask = (1u << depth) - 1u;
    const unsigned pieces = (unsigned)((frame_bytes + HOLD_PIECE - 1) / HOLD_PIECE);
    for (int first = 0; first < n_out; first += RESAMPLE_CAP) {
        const int n = n_out - first < RESAMPLE_CAP ? n_out - first : RESAMPLE_CAP;
        p.dst = dst + (size_t)first * dst_stride;
        for (int k = 0; k < n; ++k) p.e[k] = table[first + k];
        resample_frames_kernel<<<dim3(pieces, (unsigned)n), 256, 0, s>>>(p);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Shutter accumulation: every output frame the weighted integer mean of up to 33 source and node frames (include/emavfi.h, "SHUTTER
// DEFINITION"; per-element functions: shutter_elem.h).
//   accumulate_frames_kernel   grid (32 KiB pieces of a frame, entries of this launch): one workgroup row per entry.  The table travels as
//                              kernel arguments, SHUTTER_CAP entries per launch, with each entry's weight sum S and its reciprocal word
//                              (S is uniform per entry, so the division is shutter_div's multiply and correct); a workgroup reads its
//                              entry through scalar loads.  A held or single-tap entry copies its piece of ONE frame and forms no other
//                              address.  Else 16 bytes per lane and tap where dst and every tap of the entry are 16-byte aligned (the last
//                              frame_bytes % 16 bytes: bytes / words), the 16 (or 8) sums of a lane in 32-bit registers and the loads of
//                              SHUTTER_FLIGHT taps issued before the first is used: the kernel reads n frames and writes one, and what
//                              limits it is how many bytes it keeps in flight.  Unaligned entries go by bytes / words throughout,
//                              through the same per-element functions.  Nothing waits on anything: no LDS, no atomics.
// ------------------------------------------------------------------------------------------
constexpr int SHUTTER_FLIGHT = 4;
struct AccumulateArgs {
    unsigned char *dst;              // the first output frame of THIS launch
    size_t dst_stride;
    const unsigned char *srcs;
    size_t src_stride;
    const unsigned char *nodes;
    size_t node_stride;
    const unsigned *flags;
    size_t frame_bytes;
    int shift;
    unsigned mask;
    unsigned sum[SHUTTER_CAP], magic[SHUTTER_CAP];   // per entry: S = the sum of its weights, shutter_magic(S)
    AccumulateEntry e[SHUTTER_CAP];
};
static_assert(sizeof(AccumulateArgs) <= 4096, "the table must fit the kernel argument segment");

__device__ __forceinline__ const unsigned char *accumulate_frame(const AccumulateArgs &p, unsigned i)
{
    return (i & RESAMPLE_POOL_NODES) ? p.nodes + (size_t)(i & ~RESAMPLE_POOL_NODES) * p.node_stride : p.srcs + (size_t)i * p.src_stride;
}

// taps t0 .. t0 + K - 1 of an entry into the sums of the 16 bytes at `at`: K loads issued, then used
template <int SB, int K>
__device__ __forceinline__ void accumulate_taps(const AccumulateArgs &p, const AccumulateEntry &e, unsigned t0, size_t at, ShutterSums &ax,
                                                ShutterSums &ay, ShutterSums &az, ShutterSums &aw)
{
    uint4 v[K];
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = *reinterpret_cast<const uint4 *>(accumulate_frame(p, e.tap[t0 + i]) + at);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const unsigned w = e.w[t0 + i];
        shutter_add_dword(ax, v[i].x, w, SB, p.mask, p.shift);
        shutter_add_dword(ay, v[i].y, w, SB, p.mask, p.shift);
        shutter_add_dword(az, v[i].z, w, SB, p.mask, p.shift);
        shutter_add_dword(aw, v[i].w, w, SB, p.mask, p.shift);
    }
}

template <int SB>   // sample_bytes
__global__ __launch_bounds__(256) void accumulate_frames_kernel(AccumulateArgs p)
{
    const AccumulateEntry &e = p.e[blockIdx.y];                       // uniform: read where it lies, among the kernel arguments
    unsigned char *d = p.dst + (size_t)blockIdx.y * p.dst_stride;
    const size_t lo = (size_t)blockIdx.x * HOLD_PIECE, hi = lo + HOLD_PIECE < p.frame_bytes ? lo + HOLD_PIECE : p.frame_bytes;
    size_t x = lo;
    const bool held = p.flags && e.f && p.flags[e.f - 1];
    const unsigned n = e.n;
    if (held || n == 1u) {                                            // one frame, byte for byte: source frame h, or the only tap
        const unsigned char *a = accumulate_frame(p, held ? e.h : e.tap[0]);
        if ((((uintptr_t)d | (uintptr_t)a) & 15) == 0) {
            const size_t nv = (hi - lo) >> 4;
            for (size_t q = threadIdx.x; q < nv; q += 256) reinterpret_cast<uint4 *>(d + lo)[q] = reinterpret_cast<const uint4 *>(a + lo)[q];
            x += nv << 4;
        }
        for (x += threadIdx.x; x < hi; x += 256) d[x] = a[x];
        return;
    }
    const unsigned S = p.sum[blockIdx.y], M = p.magic[blockIdx.y];
    uintptr_t bits = (uintptr_t)d;
    for (unsigned t = 0; t < n; ++t) bits |= (uintptr_t)accumulate_frame(p, e.tap[t]);
    if ((bits & 15) == 0) {
        const size_t nv = (hi - lo) >> 4;
        for (size_t q = threadIdx.x; q < nv; q += 256) {
            const size_t at = lo + (q << 4);
            ShutterSums ax{}, ay{}, az{}, aw{};                       // one per dword of the lane's 16 bytes
            unsigned t = 0;
            for (; t + SHUTTER_FLIGHT <= n; t += SHUTTER_FLIGHT) accumulate_taps<SB, SHUTTER_FLIGHT>(p, e, t, at, ax, ay, az, aw);
            if (n - t == 3u) accumulate_taps<SB, 3>(p, e, t, at, ax, ay, az, aw);
            else if (n - t == 2u) accumulate_taps<SB, 2>(p, e, t, at, ax, ay, az, aw);
            else if (n - t == 1u) accumulate_taps<SB, 1>(p, e, t, at, ax, ay, az, aw);
            uint4 r;
            r.x = shutter_mean_dword(ax, S, M, SB, p.shift);
            r.y = shutter_mean_dword(ay, S, M, SB, p.shift);
            r.z = shutter_mean_dword(az, S, M, SB, p.shift);
            r.w = shutter_mean_dword(aw, S, M, SB, p.shift);
            *reinterpret_cast<uint4 *>(d + at) = r;
        }
        x += nv << 4;
    }
    if (SB == 1) {
        for (x += threadIdx.x; x < hi; x += 256) {
            unsigned sum = 0u;
            for (unsigned t = 0; t < n; ++t) sum += e.w[t] * accumulate_frame(p, e.tap[t])[x];
            d[x] = (unsigned char)shutter_mean(sum, S, M);
        }
    } else {                                                          // frame_bytes, lo and every frame address are even
        for (x += 2 * (size_t)threadIdx.x; x < hi; x += 512) {
            unsigned sum = 0u;
            for (unsigned t = 0; t < n; ++t)
                sum += e.w[t] * shutter_sample(*reinterpret_cast<const unsigned short *>(accumulate_frame(p, e.tap[t]) + x), p.mask, p.shift);
            *reinterpret_cast<unsigned short *>(d + x) = (unsigned short)(shutter_mean(sum, S, M) << p.shift);
        }
    }
}

int launch_accumulate_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                             const unsigned char *nodes, size_t node_stride, const AccumulateEntry *table, const unsigned *flags,
                             size_t frame_bytes, int sample_bytes, int depth, int shift, hipStream_t s)
{
    AccumulateArgs p{};
    p.dst_stride = dst_stride; p.srcs = srcs; p.src_stride = src_stride; p.nodes = nodes; p.node_stride = node_stride;
    p.flags = flags; p.frame_bytes = frame_bytes; p.shift = shift; p.mask = (1u << depth) - 1u;
    const unsigned pieces = (unsigned)((frame_bytes + HOLD_PIECE - 1) / HOLD_PIECE);
    for (int first = 0; first < n_out; first += SHUTTER_CAP) {
        const int n = n_out - first < SHUTTER_CAP ? n_out - first : SHUTTER_CAP;
        p.dst = dst + (size_t)first * dst_stride;
        for (int k = 0; k < n; ++k) {
            p.e[k] = table[first + k];
            p.sum[k] = 0u;
            for (unsigned t = 0; t < p.e[k].n; ++t) p.sum[k] += p.e[k].w[t];
            p.magic[k] = shutter_magic(p.sum[k]);
        }
        if (sample_bytes == 1) accumulate_frames_kernel<1><<<dim3(pieces, (unsigned)n), 256, 0, s>>>(p);
        else accumulate_frames_kernel<2><<<dim3(pieces, (unsigned)n), 256, 0, s>>>(p);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Shutter accumulation in linear light: the first linear_bytes bytes of every output frame are averaged in light, the rest as above
// (include/emavfi.h, "LINEAR LIGHT DEFINITION"; per-element functions: light_elem.h, and shutter_elem.h for the coded rest).
//   accumulate_linear_kernel   the grid, the table as kernel arguments, the copy of a held or single-tap entry and the choice of 16-byte or
//                              byte / word accesses are accumulate_frames_kernel's.  A workgroup that mixes first copies the table `lin`
//                              (2^depth words: 1, 4 or 16 KiB of the CU's 160 KiB) into LDS, 256 threads striding over it; one barrier.
//                              Decode is one LDS gather per sample and tap, its index masked to the table; the 16 (or 8) sums of a lane
//                              are 64-bit; the division by S is light_div's three multiplies; encode is a `depth`-step search, two
//                              neighbouring LDS words per step.  A 16-byte piece lies below linear_bytes (light), at or above it (the
//                              coded mean, through accumulate_taps) or across it: then, and in the byte / word forms, every sample
//                              goes alone by the rule of its own offset.  No address depends on what the table holds.
// ------------------------------------------------------------------------------------------
struct AccumulateLinearArgs {
    AccumulateArgs a;
    const unsigned *lin;             // device: 2^depth words
    size_t linear_bytes;
    int depth;
};
static_assert(sizeof(AccumulateLinearArgs) <= 4096, "the table must fit the kernel argument segment");

// the sample at byte offset x of the entry's output: in light below linear_bytes, else the coded mean
template <int SB>
__device__ __forceinline__ unsigned accumulate_linear_sample(const AccumulateLinearArgs &p, const AccumulateEntry &e, const unsigned *lin,
                                                             size_t x, unsigned S, unsigned M)
{
    const AccumulateArgs &a = p.a;
    const unsigned n = e.n;
    if (x < p.linear_bytes) {
        unsigned long long sum = 0ull;
        for (unsigned t = 0; t < n; ++t) {
            const unsigned char *f = accumulate_frame(a, e.tap[t]) + x;
            const unsigned v = SB == 1 ? (unsigned)*f : shutter_sample(*reinterpret_cast<const unsigned short *>(f), a.mask, a.shift);
            sum += (unsigned long long)(e.w[t] & 65535u) * lin[v & a.mask];
        }
        return light_enc(light_mean(sum, S, M), lin, p.depth) << a.shift;
    }
    unsigned sum = 0u;
    for (unsigned t = 0; t < n; ++t) {
        const unsigned char *f = accumulate_frame(a, e.tap[t]) + x;
        sum += e.w[t] * (SB == 1 ? (unsigned)*f : shutter_sample(*reinterpret_cast<const unsigned short *>(f), a.mask, a.shift));
    }
    return shutter_mean(sum, S, M) << a.shift;
}

// taps t0 .. t0 + K - 1 of an entry into the light sums of the 16 bytes at `at`: K loads issued, then used
template <int SB, int K>
__device__ __forceinline__ void accumulate_linear_taps(const AccumulateArgs &p, const AccumulateEntry &e, const unsigned *lin, unsigned t0,
                                                       size_t at, LightSums &ax, LightSums &ay, LightSums &az, LightSums &aw)
{
    uint4 v[K];
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = *reinterpret_cast<const uint4 *>(accumulate_frame(p, e.tap[t0 + i]) + at);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const unsigned w = e.w[t0 + i];
        light_add_dword(ax, v[i].x, w, lin, SB, p.mask, p.shift);
        light_add_dword(ay, v[i].y, w, lin, SB, p.mask, p.shift);
        light_add_dword(az, v[i].z, w, lin, SB, p.mask, p.shift);
        light_add_dword(aw, v[i].w, w, lin, SB, p.mask, p.shift);
    }
}

template <int SB>   // sample_bytes
__global__ __launch_bounds__(256) void accumulate_linear_kernel(AccumulateLinearArgs pl)
{
    __shared__ unsigned lin[SB == 1 ? 256 : 4096];                    // 2^depth words: depth 8 at bytes, 10 or 12 at words
    const AccumulateArgs &p = pl.a;
    const AccumulateEntry &e = p.e[blockIdx.y];                       // uniform: read where it lies, among the kernel arguments
    unsigned char *d = p.dst + (size_t)blockIdx.y * p.dst_stride;
    const size_t lo = (size_t)blockIdx.x * HOLD_PIECE, hi = lo + HOLD_PIECE < p.frame_bytes ? lo + HOLD_PIECE : p.frame_bytes;
    size_t x = lo;
    const bool held = p.flags && e.f && p.flags[e.f - 1];
    const unsigned n = e.n;
    if (held || n == 1u) {                                            // one frame, byte for byte: source frame h, or the only tap
        const unsigned char *a = accumulate_frame(p, held ? e.h : e.tap[0]);
        if ((((uintptr_t)d | (uintptr_t)a) & 15) == 0) {
            const size_t nv = (hi - lo) >> 4;
            for (size_t q = threadIdx.x; q < nv; q += 256) reinterpret_cast<uint4 *>(d + lo)[q] = reinterpret_cast<const uint4 *>(a + lo)[q];
            x += nv << 4;
        }
        for (x += threadIdx.x; x < hi; x += 256) d[x] = a[x];
        return;
    }
    if (lo < pl.linear_bytes) {                                       // uniform: a piece wholly in the coded rest needs no table
        const unsigned words = 1u << pl.depth, cap = SB == 1 ? 256u : 4096u;
        for (unsigned i = threadIdx.x; i < words && i < cap; i += 256) lin[i] = pl.lin[i];
        __syncthreads();
    }
    const unsigned S = p.sum[blockIdx.y], M = p.magic[blockIdx.y];
    uintptr_t bits = (uintptr_t)d;
    for (unsigned t = 0; t < n; ++t) bits |= (uintptr_t)accumulate_frame(p, e.tap[t]);
    if ((bits & 15) == 0) {
        const size_t nv = (hi - lo) >> 4;
        for (size_t q = threadIdx.x; q < nv; q += 256) {
            const size_t at = lo + (q << 4);
            uint4 r;
            unsigned t = 0;
            if (at + 16 <= pl.linear_bytes) {
                LightSums ax{}, ay{}, az{}, aw{};                     // one per dword of the lane's 16 bytes
                for (; t + SHUTTER_FLIGHT <= n; t += SHUTTER_FLIGHT) accumulate_linear_taps<SB, SHUTTER_FLIGHT>(p, e, lin, t, at, ax, ay, az, aw);
                if (n - t == 3u) accumulate_linear_taps<SB, 3>(p, e, lin, t, at, ax, ay, az, aw);
                else if (n - t == 2u) accumulate_linear_taps<SB, 2>(p, e, lin, t, at, ax, ay, az, aw);
                else if (n - t == 1u) accumulate_linear_taps<SB, 1>(p, e, lin, t, at, ax, ay, az, aw);
                r.x = light_mean_dword(ax, S, M, lin, SB, pl.depth, p.shift);
                r.y = light_mean_dword(ay, S, M, lin, SB, pl.depth, p.shift);
                r.z = light_mean_dword(az, S, M, lin, SB, pl.depth, p.shift);
                r.w = light_mean_dword(aw, S, M, lin, SB, pl.depth, p.shift);
            } else if (at >= pl.linear_bytes) {
                ShutterSums ax{}, ay{}, az{}, aw{};
                for (; t + SHUTTER_FLIGHT <= n; t += SHUTTER_FLIGHT) accumulate_taps<SB, SHUTTER_FLIGHT>(p, e, t, at, ax, ay, az, aw);
                if (n - t == 3u) accumulate_taps<SB, 3>(p, e, t, at, ax, ay, az, aw);
                else if (n - t == 2u) accumulate_taps<SB, 2>(p, e, t, at, ax, ay, az, aw);
                else if (n - t == 1u) accumulate_taps<SB, 1>(p, e, t, at, ax, ay, az, aw);
                r.x = shutter_mean_dword(ax, S, M, SB, p.shift);
                r.y = shutter_mean_dword(ay, S, M, SB, p.shift);
                r.z = shutter_mean_dword(az, S, M, SB, p.shift);
                r.w = shutter_mean_dword(aw, S, M, SB, p.shift);
            } else {                                                  // the one piece of a frame that lies across linear_bytes
                unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 16; k += SB) o[k >> 2] |= accumulate_linear_sample<SB>(pl, e, lin, at + k, S, M) << (8 * (k & 3));
                r.x = o[0]; r.y = o[1]; r.z = o[2]; r.w = o[3];
            }
            *reinterpret_cast<uint4 *>(d + at) = r;
        }
        x += nv << 4;
    }
    if (SB == 1) {
        for (x += threadIdx.x; x < hi; x += 256) d[x] = (unsigned char)accumulate_linear_sample<1>(pl, e, lin, x, S, M);
    } else {                                                          // frame_bytes, lo and every frame address are even
        for (x += 2 * (size_t)threadIdx.x; x < hi; x += 512)
            *reinterpret_cast<unsigned short *>(d + x) = (unsigned short)accumulate_linear_sample<2>(pl, e, lin, x, S, M);
    }
}

int launch_accumulate_frames_linear(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                                    const unsigned char *nodes, size_t node_stride, const AccumulateEntry *table, const unsigned *flags,
                                    size_t frame_bytes, int sample_bytes, int depth, int shift, const unsigned *lin, size_t linear_bytes,
                                    hipStream_t s)
{
    AccumulateLinearArgs pl{};
    AccumulateArgs &p = pl.a;
    pl.lin = lin; pl.linear_bytes = linear_bytes; pl.depth = depth;
    p.dst_stride = dst_stride; p.srcs = srcs; p.src_stride = src_stride; p.nodes = nodes; p.node_stride = node_stride;
    p.flags = flags; p.frame_bytes = frame_bytes; p.shift = shift; p.mask = (1u << depth) - 1u;
    const unsigned pieces = (unsigned)((frame_bytes + HOLD_PIECE - 1) / HOLD_PIECE);
    for (int first = 0; first < n_out; first += SHUTTER_CAP) {
        const int n = n_out - first < SHUTTER_CAP ? n_out - first : SHUTTER_CAP;
        p.dst = dst + (size_t)first * dst_stride;
        for (int k = 0; k < n; ++k) {
            p.e[k] = table[first + k];
            p.sum[k] = 0u;
            for (unsigned t = 0; t < p.e[k].n; ++t) p.sum[k] += p.e[k].w[t];
            p.magic[k] = shutter_magic(p.sum[k]);
        }
        if (sample_bytes == 1) accumulate_linear_kernel<1><<<dim3(pieces, (unsigned)n), 256, 0, s>>>(pl);
        else accumulate_linear_kernel<2><<<dim3(pieces, (unsigned)n), 256, 0, s>>>(pl);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// Static regions held on the device (include/emavfi.h, "STATIC REGION DEFINITION"; per-element functions: static_elem.h).
//   static_guard_kernel   grid (tiles along x, tiles along y, entries of this launch), 256 threads.  The table travels as kernel arguments,
//                         at most STATIC_CAP entries per launch.  A workgroup owns a tile of ST_TH x ST_TW = 64 x 128 luma pixels of ONE
//                         destination frame.  Chosen against 160 KiB of LDS per CU and wave64: the `bad` map of the tile plus its halo is
//                         one byte per pixel, (64 + 32) rows x (128 + 32 + 4) bytes = 15.4 KiB (the row stride of 41 dwords lets the 64 lanes
//                         of a wave, one row each, hit 64 different banks), the row-eroded map (64 + 32) x (128 + 4) = 12.4 KiB: 27.8 KiB,
//                         5 workgroups = 20 waves per CU.  At r = 16 the tile plus halo is 96 x 160 pixels, 1.875 x the tile, so with d's
//                         stores the traffic is at most (2 * 1.875 + 1) / 3 = 1.58 x what the definition obliges; at r = 4 1.13 x.
//                         Stages: (1) `bad` = 0; (2) every plane's samples of a and b inside the tile plus halo, CLIPPED to the frame, are
//                         compared and a differing sample marks its pixel - a 4:2:0 chroma sample the (up to four) luma pixels it covers, so
//                         the chroma comparison is folded in at luma resolution; positions outside the frame stay 0, which is the clipped
//                         window; (3) erosion along rows, then along columns, each by a running count over the 2 r + 1 window (a lane walks 32
//                         outputs: 2 r + 1 + 64 LDS reads, not 32 (2 r + 1)); the column pass leaves the `core` map of the tile in the `bad`
//                         buffer and counts the tile's core pixels, one atomic add per wave into counts[k] (cleared by a launch of its own
//                         ahead: an integer sum, the order does not matter); (4) a's samples are stored at the replaced positions of d.
//                         a's tile is read a second time here, right after stage (2) read it (keeping it in LDS would cost up to 64 KiB);
//                         d is never read, so a 16-byte unit is stored whole only when every sample of it is replaced, else sample by sample.
//                         Access width: 16-byte loads and stores when the three frame addresses of the entry, every plane's offset and
//                         every plane's row bytes are multiples of 16 (a tile's samples are then whole units; a halo unit may reach past
//                         the halo but never past its row); else bytes / words throughout.  Both forms run the same per-element functions.
//                         No byte beyond a frame is read.  Short-lived, waits on nothing.
// ------------------------------------------------------------------------------------------
constexpr int ST_TH = 64, ST_TW = 128;
constexpr int ST_RH = ST_TH + 2 * STATIC_MAX_RADIUS;            // rows of the tile plus halo
constexpr int ST_BS = ST_TW + 2 * STATIC_MAX_RADIUS + 4;        // row stride of `bad`: 164 bytes = 41 dwords
constexpr int ST_ES = ST_TW + 4;                                // row stride of the row-eroded map: 33 dwords
static_assert(ST_TH % 32 == 0 && ST_TW == 128 && (ST_TH & 1) == 0, "the passes below walk 32 outputs per lane, 128 columns per 2 x 128 threads");

struct StaticArgs {
    unsigned char *dst;              // the first destination frame of THIS launch
    size_t dst_stride;
    const unsigned char *srcs;
    size_t src_stride;
    unsigned *counts;                // the first count of THIS launch, or null
    StaticPlane plane[3];
    int n_planes, H, W, sb, shift, radius, wide;
    unsigned mask, tol;
    unsigned a[STATIC_CAP], b[STATIC_CAP];
};
static_assert(sizeof(StaticArgs) <= 2048, "the table must fit the kernel argument segment");

__global__ __launch_bounds__(256) void static_counts_clear_kernel(unsigned *__restrict__ counts, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) counts[i] = 0u;
}

// sample k of a 16-byte unit held as four little-endian dwords
template <int SB>
__device__ __forceinline__ unsigned static_unit_sample(const uint4 &v, int k)
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (SB == 1) return (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    else return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
}

// The window passes the static guard and the agreement guard share.  On entry `map` [ST_RH][ST_BS] holds one byte per pixel of the tile plus
// its r-wide halo, 1 = marked (positions outside the frame 0: the clipped window); the caller has synchronised.  Rows: lane = (row, 32
// columns), a running count over the 2 r + 1 window; then columns: lane = (column, 32 rows).  On return `map` [ST_TH][ST_TW] holds per tile
// pixel whether SOME marked pixel lies in its window (ANY: a dilation) or NONE does (!ANY: the erosion of the unmarked), and the result is
// this lane's number of 1s inside the clipped tile [ty0, ty1) x [tx0, tx1); the caller synchronises before it reads the map.
template <bool ANY>
__device__ __forceinline__ unsigned tile_window_passes(unsigned char *map, unsigned char *rowmap, int r, int tid, int tx0, int tx1, int ty0, int ty1)
{
    const int RH = ST_TH + 2 * r;
    for (int t = tid; t < 4 * RH; t += 256) {
        const int row = t % RH, seg = t / RH;
        const unsigned char *br = map + row * ST_BS + seg * 32;
        unsigned char *er = rowmap + row * ST_ES + seg * 32;
        int cnt = 0;
        for (int k = 0; k <= 2 * r; ++k) cnt += br[k];
        for (int x = 0; x < 32; ++x) {
            er[x] = cnt ? 1 : 0;
            if (x < 31) cnt += (int)br[x + 2 * r + 1] - (int)br[x];      // at most column 96 + 30 + 33 = 159 of RW = 128 + 2 r
        }
    }
    __syncthreads();
    // the result replaces `map`, which the row pass has finished reading
    const int x = tid & (ST_TW - 1);
    unsigned n = 0u;
    for (int seg = tid >> 7; seg < ST_TH / 32; seg += 2) {
        const unsigned char *cr = rowmap + seg * 32 * ST_ES + x;
        int cnt = 0;
        for (int k = 0; k <= 2 * r; ++k) cnt += cr[k * ST_ES];
        for (int y = 0; y < 32; ++y) {
            const int yy = seg * 32 + y;
            const bool c = ANY ? cnt != 0 : cnt == 0;
            map[yy * ST_TW + x] = c ? 1 : 0;
            n += (c && tx0 + x < tx1 && ty0 + yy < ty1) ? 1u : 0u;
            if (y < 31) cnt += (int)cr[(y + 2 * r + 1) * ST_ES] - (int)cr[y * ST_ES];   // at most row 32 + 30 + 33 = 95 of RH = 64 + 2 r
        }
    }
    return n;
}

template <int SB>
__global__ __launch_bounds__(256) void static_guard_kernel(StaticArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char bad[ST_RH * ST_BS];      // stage (3) on: core [ST_TH][ST_TW]
    __shared__ __attribute__((aligned(16))) unsigned char rowbad[ST_RH * ST_ES];
    constexpr int NS = 16 / SB;                                  // samples of a 16-byte unit
    const int tid = threadIdx.x, r = p.radius;
    const unsigned e = blockIdx.z;
    const int tx0 = blockIdx.x * ST_TW, ty0 = blockIdx.y * ST_TH;
    const int tx1 = min(tx0 + ST_TW, p.W), ty1 = min(ty0 + ST_TH, p.H);           // the tile, clipped: [ty0, ty1) x [tx0, tx1)
    const int X0 = static_window_lo(tx0, r), X1 = static_window_hi(tx1 - 1, r, p.W) + 1;
    const int Y0 = static_window_lo(ty0, r), Y1 = static_window_hi(ty1 - 1, r, p.H) + 1;   // the tile plus halo, clipped to the frame
    const int ox = tx0 - r, oy = ty0 - r, RW = ST_TW + 2 * r, RH = ST_TH + 2 * r;  // the LDS map: RH x RW pixels from (oy, ox)
    const unsigned char *fa = p.srcs + (size_t)p.a[e] * p.src_stride, *fb = p.srcs + (size_t)p.b[e] * p.src_stride;
    unsigned char *fd = p.dst + (size_t)e * p.dst_stride;
    const bool wide = p.wide && ((((uintptr_t)fa | (uintptr_t)fb | (uintptr_t)fd) & 15) == 0);

    for (int i = tid; i < ST_RH * ST_BS / 4; i += 256) reinterpret_cast<unsigned *>(bad)[i] = 0u;
    __syncthreads();

    // (2) a differing sample marks the luma pixel(s) it belongs to
    const auto mark1 = [&](int y, int x) {
        const int ly = y - oy, lx = x - ox;
        if (ly >= 0 && ly < RH && lx >= 0 && lx < RW) bad[ly * ST_BS + lx] = 1;
    };
    const auto mark = [&](int row, int px, int sub) {
        if (!sub) mark1(row, px);
        else { mark1(2 * row, 2 * px); mark1(2 * row, 2 * px + 1); mark1(2 * row + 1, 2 * px); mark1(2 * row + 1, 2 * px + 1); }
    };
    const auto differ = [&](unsigned wa, unsigned wb) {
        return !static_within(static_sample(wa, p.mask, p.shift), static_sample(wb, p.mask, p.shift), p.tol);
    };
    for (int q = 0; q < p.n_planes; ++q) {
        const StaticPlane pl = p.plane[q];
        const int row0 = Y0 >> pl.sub, nrows = ((Y1 - 1) >> pl.sub) + 1 - row0;
        const int s0 = (X0 >> pl.sub) * pl.div, s1 = (((X1 - 1) >> pl.sub) + 1) * pl.div;   // the samples of a row: s1 <= pl.samples
        const size_t rb = (size_t)pl.samples * SB;
        if (wide) {
            const int b0 = (s0 * SB) & ~15, b1 = (s1 * SB + 15) & ~15;                      // rb is a multiple of 16: b1 <= rb
            const int nu = (b1 - b0) >> 4, items = nrows * nu;
            for (int t = tid; t < items; t += 256) {
                const int rr = t / nu, u = t - rr * nu, row = row0 + rr;
                const size_t off = pl.offset + (size_t)row * rb + (size_t)(b0 + 16 * u);
                const uint4 va = *reinterpret_cast<const uint4 *>(fa + off), vb = *reinterpret_cast<const uint4 *>(fb + off);
                const int s = (b0 + 16 * u) / SB;
                int px = s / pl.div, rem = s - px * pl.div;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    if (differ(static_unit_sample<SB>(va, k), static_unit_sample<SB>(vb, k))) mark(row, px, pl.sub);
                    if (++rem == pl.div) { rem = 0; ++px; }
                }
            }
        } else {
            const int ns = s1 - s0, items = nrows * ns;
            for (int t = tid; t < items; t += 256) {
                const int rr = t / ns, s = s0 + (t - rr * ns), row = row0 + rr;
                const size_t off = pl.offset + (size_t)row * rb + (size_t)s * SB;
                unsigned wa, wb;
                if constexpr (SB == 1) { wa = fa[off]; wb = fb[off]; }
                else { wa = *reinterpret_cast<const unsigned short *>(fa + off); wb = *reinterpret_cast<const unsigned short *>(fb + off); }
                if (differ(wa, wb)) mark(row, s / pl.div, pl.sub);
            }
        }
    }
    __syncthreads();

    // (3) erosion, rows then columns: the core map replaces `bad`
    unsigned char *const core = bad;
    {
        unsigned n = tile_window_passes<false>(bad, rowbad, r, tid, tx0, tx1, ty0, ty1);
        if (p.counts) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
            if ((tid & 63) == 0 && n) atomicAdd(p.counts + e, n);
        }
    }
    __syncthreads();

    // (4) a's samples at the replaced positions of d
    const auto core_at = [&](int y, int x) { return core[(y - ty0) * ST_TW + (x - tx0)] != 0; };
    const auto replaced = [&](int row, int px, int sub) {
        if (!sub) return core_at(row, px);
        return static_chroma_core(core_at(2 * row, 2 * px), core_at(2 * row, 2 * px + 1), core_at(2 * row + 1, 2 * px), core_at(2 * row + 1, 2 * px + 1));
    };
    for (int q = 0; q < p.n_planes; ++q) {
        const StaticPlane pl = p.plane[q];
        const int row0 = ty0 >> pl.sub, nrows = (ty1 >> pl.sub) - row0;                     // 4:2:0: ty0, ty1 even
        const int s0 = (tx0 >> pl.sub) * pl.div, s1 = (tx1 >> pl.sub) * pl.div;
        const size_t rb = (size_t)pl.samples * SB;
        if (wide) {
            const int nu = ((s1 - s0) * SB) >> 4, items = nrows * nu;                       // whole units: s0 SB and s1 SB are multiples of 16
            for (int t = tid; t < items; t += 256) {
                const int rr = t / nu, u = t - rr * nu, row = row0 + rr;
                const int s = s0 + u * NS;
                int px = s / pl.div, rem = s - px * pl.div;
                unsigned flags = 0u;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    flags |= (replaced(row, px, pl.sub) ? 1u : 0u) << k;
                    if (++rem == pl.div) { rem = 0; ++px; }
                }
                if (!flags) continue;
                const size_t off = pl.offset + (size_t)row * rb + (size_t)s * SB;
                const uint4 va = *reinterpret_cast<const uint4 *>(fa + off);
                if (flags == (1u << NS) - 1u) {
                    *reinterpret_cast<uint4 *>(fd + off) = va;
                } else {
#pragma unroll
                    for (int k = 0; k < NS; ++k)
                        if (flags >> k & 1u) {
                            if constexpr (SB == 1) fd[off + k] = (unsigned char)static_unit_sample<SB>(va, k);
                            else *reinterpret_cast<unsigned short *>(fd + off + 2 * k) = (unsigned short)static_unit_sample<SB>(va, k);
                        }
                }
            }
        } else {
            const int ns = s1 - s0, items = nrows * ns;
            for (int t = tid; t < items; t += 256) {
                const int rr = t / ns, s = s0 + (t - rr * ns), row = row0 + rr;
                if (!replaced(row, s / pl.div, pl.sub)) continue;
                const size_t off = pl.offset + (size_t)row * rb + (size_t)s * SB;
                if constexpr (SB == 1) fd[off] = fa[off];
                else *reinterpret_cast<unsigned short *>(fd + off) = *reinterpret_cast<const unsigned short *>(fa + off);
            }
        }
    }
}

int launch_static_guard_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride,
                               const StaticEntry *table, int H, int W, int layout, int C, int sample_bytes, int depth, int shift, int radius,
                               unsigned tol, unsigned *counts, hipStream_t s)
{
    StaticArgs p{};
    size_t frame_bytes;
    p.n_planes = static_planes(layout, C, H, W, sample_bytes, p.plane, &frame_bytes);
    p.dst_stride = dst_stride; p.srcs = srcs; p.src_stride = src_stride;
    p.H = H; p.W = W; p.sb = sample_bytes; p.shift = shift; p.radius = radius; p.mask = (1u << depth) - 1u; p.tol = tol;
    p.wide = 1;
    for (int q = 0; q < p.n_planes; ++q) p.wide = p.wide && mult_of(16, {p.plane[q].offset, (size_t)p.plane[q].samples * sample_bytes});
    if (counts) {
        static_counts_clear_kernel<<<dim3((unsigned)((n_dst + 255) / 256)), 256, 0, s>>>(counts, n_dst);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    const dim3 tiles((unsigned)((W + ST_TW - 1) / ST_TW), (unsigned)((H + ST_TH - 1) / ST_TH));
    for (int first = 0; first < n_dst; first += STATIC_CAP) {
        const int n = n_dst - first < STATIC_CAP ? n_dst - first : STATIC_CAP;
        p.dst = dst + (size_t)first * dst_stride;
        p.counts = counts ? counts + first : nullptr;
        for (int k = 0; k < n; ++k) { p.a[k] = table[first + k].a; p.b[k] = table[first + k].b; }
        if (sample_bytes == 1) static_guard_kernel<1><<<dim3(tiles.x, tiles.y, (unsigned)n), 256, 0, s>>>(p);
        else static_guard_kernel<2><<<dim3(tiles.x, tiles.y, (unsigned)n), 256, 0, s>>>(p);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// The active picture found and its bars restored on the device (include/emavfi.h, "ACTIVE AREA DEFINITION"; per-element functions:
// active_elem.h).
//   active_bounds_init_kernel     every frame's four words = {H, 0, W, 0}: a launch of its own ahead of the scan, as the static guard's counts.
//   active_bounds_kernel<BPP>     grid (pieces of a frame, n), 256 threads; BPP 1: bytes, C = 1; 2: 16-bit words; 3: bytes, C = 3.  A lane
//                                 walks 16-byte units of the rows and keeps its four extremes in registers; a unit is ONE 16-byte load where
//                                 pointer, pitch and batch stride are multiples of 16 and the unit ends inside the row (pitch padding is never
//                                 read), byte loads otherwise and for the row's remainder (diff_load_unit: bytes beyond the row read as 0, which
//                                 is never above a level), four units in flight.  A wave folds its lanes' extremes by shuffles, the workgroup its
//                                 four waves' through 16 words of LDS, and one lane issues atomicMin / atomicMax on the frame's four words - those
//                                 that beat the word as it reads then; min and max are order-free, the result is exact.  No staging in LDS.
//   fill_outside_kernel<SB>       grid (pieces of a frame, entries of this launch), 256 threads.  Per plane the outside of the rectangle is four
//                                 bands - above, below, left, right - walked in 16-byte units of the plane's rows: a unit that lies wholly in
//                                 its band moves as one 16-byte load and store where the two frame addresses, the plane's offset and its row
//                                 bytes are multiples of 16, everything else sample by sample.  Bytes inside the rectangle are not touched.
//   preprocess_u8_pitched_kernel / postprocess_u8_pitched_kernel   the u8 kernels' per-element arithmetic (nv12_norm / nv12_byte: the same two
//                                 functions the 4:2:0 kernels share with them) over rows of `pitch` bytes: a lane takes one 16-byte unit of a
//                                 row, wide where pointer, pitch and batch stride allow and the unit ends inside the row.
// All are short-lived and wait on nothing.
// ------------------------------------------------------------------------------------------
struct BoundsArgs { const unsigned char *img; size_t pitch, bstride; unsigned *bounds; int H, W, rowbytes, nu, wide, shift; unsigned mask, level; };

__global__ __launch_bounds__(256) void active_bounds_init_kernel(unsigned *__restrict__ bounds, int n, int H, int W)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const ActiveBounds e = active_none(H, W);
        bounds[4 * i] = e.top; bounds[4 * i + 1] = e.bottom; bounds[4 * i + 2] = e.left; bounds[4 * i + 3] = e.right;
    }
}

template <int BPP>
__global__ __launch_bounds__(256) void active_bounds_kernel(BoundsArgs a)
{
    constexpr int SB = BPP == 2 ? 2 : 1, NS = 16 / SB, PX = BPP == 3 ? 3 : 1;    // bytes per sample, samples per unit, samples per pixel
    constexpr int UN = 4;                                                        // units a lane has in flight
    __shared__ unsigned part[4][4];
    const size_t b = blockIdx.y;
    const unsigned char *img = a.img + b * a.bstride;
    ActiveBounds mine = active_none(a.H, a.W);
    const int items = a.H * a.nu, stride = gridDim.x * 256;                      // at most 16384 rows x 3072 units
    for (int t0 = blockIdx.x * 256 + threadIdx.x; t0 < items; t0 += UN * stride) {
        unsigned w[UN][4];
        int y[UN], b0[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int t = t0 + u * stride < items ? t0 + u * stride : t0;        // past the end: unit t0 once more, which marks nothing new
            y[u] = t / a.nu;
            b0[u] = (t - y[u] * a.nu) << 4;
            const int nb = min(16, a.rowbytes - b0[u]);
            diff_load_unit<1>(img + (size_t)y[u] * a.pitch + (size_t)b0[u], a.wide && nb == 16, nb, w[u]);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int first = -1, last = -1;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const unsigned word = SB == 2 ? (w[u][k >> 1] >> (16 * (k & 1))) & 0xffffu : (w[u][k >> 2] >> (8 * (k & 3))) & 0xffu;
                if (active_content(active_sample(word, a.mask, a.shift), a.level)) {
                    if (first < 0) first = k;
                    last = k;
                }
            }
            if (first >= 0) {
                const int s0 = b0[u] / SB;
                active_mark(mine, y[u], (s0 + first) / PX);
                active_mark(mine, y[u], (s0 + last) / PX);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mine.top = min(mine.top, (unsigned)__shfl_xor(mine.top, off, 64));
        mine.bottom = max(mine.bottom, (unsigned)__shfl_xor(mine.bottom, off, 64));
        mine.left = min(mine.left, (unsigned)__shfl_xor(mine.left, off, 64));
        mine.right = max(mine.right, (unsigned)__shfl_xor(mine.right, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned *mp = part[threadIdx.x >> 6];
        mp[0] = mine.top; mp[1] = mine.bottom; mp[2] = mine.left; mp[3] = mine.right;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) active_join(mine, ActiveBounds{part[k][0], part[k][1], part[k][2], part[k][3]});
        if (!active_is_empty(mine)) {
            // a word only ever moves one way, so what is read here is no nearer the result than the word is now: an extreme that does not
            // beat it cannot change it and its atomic is skipped.  The words of all frames share a cache line or two: few, cheap visits.
            unsigned *o = a.bounds + 4 * b;
            if (mine.top < __atomic_load_n(o, __ATOMIC_RELAXED)) atomicMin(o, mine.top);
            if (mine.bottom > __atomic_load_n(o + 1, __ATOMIC_RELAXED)) atomicMax(o + 1, mine.bottom);
            if (mine.left < __atomic_load_n(o + 2, __ATOMIC_RELAXED)) atomicMin(o + 2, mine.left);
            if (mine.right > __atomic_load_n(o + 3, __ATOMIC_RELAXED)) atomicMax(o + 3, mine.right);
        }
    }
}

int launch_active_bounds(const unsigned char *img, size_t pitch, size_t bstride, int n, int H, int W, int C, int sample_bytes, int depth, int shift,
                         unsigned level, unsigned *bounds, hipStream_t s)
{
    active_bounds_init_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(bounds, n, H, W);
    if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    BoundsArgs p{img, pitch, bstride, bounds, H, W, W * C * sample_bytes, 0, 0, shift, (1u << depth) - 1u, level};
    p.nu = (p.rowbytes + 15) >> 4;
    p.wide = mult_of(16, {(size_t)(uintptr_t)img, pitch, n > 1 ? bstride : 0});
    // at most 64 workgroups a frame, four units in flight per lane: the frames' words share a cache line or two, and every visit to them
    // queues there (measured: one visit per wave of a fine grid cost more than the whole scan, profiles/r27_active_area.md)
    const size_t want = ((size_t)H * p.nu + 1023) / 1024;
    const dim3 grid((unsigned)std::min<size_t>(std::max<size_t>(want, 1), 64), (unsigned)n);
    if (C == 3) active_bounds_kernel<3><<<grid, 256, 0, s>>>(p);
    else if (sample_bytes == 2) active_bounds_kernel<2><<<grid, 256, 0, s>>>(p);
    else active_bounds_kernel<1><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

struct FillArgs {
    unsigned char *dst;              // the first destination frame of THIS launch
    size_t dst_stride;
    const unsigned char *srcs;
    size_t src_stride;
    StaticPlane plane[3];
    int n_planes, top, left, height, width, wide;
    unsigned idx[ACTIVE_CAP];
};
static_assert(sizeof(FillArgs) <= 2048, "the table must fit the kernel argument segment");

template <int SB>
__global__ __launch_bounds__(256) void fill_outside_kernel(FillArgs p)
{
    const unsigned e = blockIdx.y;
    const unsigned char *fa = p.srcs + (size_t)p.idx[e] * p.src_stride;
    unsigned char *fd = p.dst + (size_t)e * p.dst_stride;
    const bool wide = p.wide && ((((uintptr_t)fa | (uintptr_t)fd) & 15) == 0);
    const int tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (int q = 0; q < p.n_planes; ++q) {
        const StaticPlane pl = p.plane[q];
        const int rb = pl.samples * SB;                                           // at most 16384 * 4 * 2 bytes
        const ActiveSpan sp = active_plane_span(pl, SB, p.top, p.left, p.height, p.width);
        // the outside of the span: rows [y0, y1) x bytes [c0, c1) above, below, left and right of it
        const int band[4][4] = {{0, sp.r0, 0, rb}, {sp.r1, pl.rows, 0, rb}, {sp.r0, sp.r1, 0, sp.c0}, {sp.r0, sp.r1, sp.c1, rb}};
        for (int k = 0; k < 4; ++k) {
            const int y0 = band[k][0], y1 = band[k][1], c0 = band[k][2], c1 = band[k][3];
            if (y1 <= y0 || c1 <= c0) continue;
            const int u0 = c0 >> 4, nu = ((c1 + 15) >> 4) - u0, items = (y1 - y0) * nu;   // at most 16384 rows x 8192 units
            for (int t = tid; t < items; t += step) {
                const int rr = t / nu, ub = (u0 + (t - rr * nu)) << 4;            // the unit's first byte in its row
                const size_t off = pl.offset + (size_t)(y0 + rr) * rb + (size_t)ub;
                if (wide && ub >= c0 && ub + 16 <= c1) {                          // c1 <= rb: the unit ends inside the row
                    *reinterpret_cast<uint4 *>(fd + off) = *reinterpret_cast<const uint4 *>(fa + off);
                } else {
#pragma unroll
                    for (int j = 0; j < 16; j += SB) {
                        if (ub + j < c0 || ub + j >= c1) continue;
                        if constexpr (SB == 1) fd[off + j] = fa[off + j];
                        else *reinterpret_cast<unsigned short *>(fd + off + j) = *reinterpret_cast<const unsigned short *>(fa + off + j);
                    }
                }
            }
        }
    }
}

int launch_fill_outside_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, const unsigned *table,
                               int H, int W, int layout, int C, int sample_bytes, int top, int left, int height, int width, hipStream_t s)
{
    if (height == H && width == W) return 0;                                       // the rectangle is the frame: nothing lies outside
    FillArgs p{};
    size_t frame_bytes;
    p.n_planes = static_planes(layout, C, H, W, sample_bytes, p.plane, &frame_bytes);
    p.dst_stride = dst_stride; p.srcs = srcs; p.src_stride = src_stride;
    p.top = top; p.left = left; p.height = height; p.width = width;
    p.wide = 1;
    size_t inside = 0;
    for (int q = 0; q < p.n_planes; ++q) {
        p.wide = p.wide && mult_of(16, {p.plane[q].offset, (size_t)p.plane[q].samples * sample_bytes});
        const ActiveSpan sp = active_plane_span(p.plane[q], sample_bytes, top, left, height, width);
        inside += (size_t)(sp.r1 - sp.r0) * (size_t)(sp.c1 - sp.c0);
    }
    const size_t want = ((frame_bytes - inside) / 16 + 1023) / 1024;               // four units per lane
    const unsigned gx = (unsigned)std::min<size_t>(std::max<size_t>(want, 1), 1024);
    for (int first = 0; first < n_dst; first += ACTIVE_CAP) {
        const int n = n_dst - first < ACTIVE_CAP ? n_dst - first : ACTIVE_CAP;
        p.dst = dst + (size_t)first * dst_stride;
        for (int k = 0; k < n; ++k) p.idx[k] = table[first + k];
        if (sample_bytes == 1) fill_outside_kernel<1><<<dim3(gx, (unsigned)n), 256, 0, s>>>(p);
        else fill_outside_kernel<2><<<dim3(gx, (unsigned)n), 256, 0, s>>>(p);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    return 0;
}

__global__ __launch_bounds__(256) void preprocess_u8_pitched_kernel(const unsigned char *__restrict__ src, size_t pitch, size_t bstride,
                                                                    float *__restrict__ dst, int B, int H, int W, int C, int wide, Stats4 st)
{
    const int rowbytes = W * C, nu = (rowbytes + 15) >> 4;
    const size_t plane = (size_t)H * W, total = (size_t)B * H * nu;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t row = t / nu, b = row / H;
        const int y = (int)(row - b * H), b0 = (int)(t - row * nu) << 4, nb = min(16, rowbytes - b0);
        unsigned w[4];
        diff_load_unit<1>(src + b * bstride + (size_t)y * pitch + (size_t)b0, wide && nb == 16, nb, w);
        int x = b0 / C, c = b0 - x * C;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < nb) {
                dst[(b * C + c) * plane + (size_t)y * W + x] = nv12_norm((int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu), st.mean[c], st.stdv[c]);
                if (++c == C) { c = 0; ++x; }
            }
        }
    }
}
__global__ __launch_bounds__(256) void postprocess_u8_pitched_kernel(const float *__restrict__ src, unsigned char *__restrict__ dst, size_t pitch,
                                                                     size_t bstride, int B, int H, int W, int C, int wide, Stats4d st, int denorm)
{
    const int rowbytes = W * C, nu = (rowbytes + 15) >> 4;
    const size_t plane = (size_t)H * W, total = (size_t)B * H * nu;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t row = t / nu, b = row / H;
        const int y = (int)(row - b * H), b0 = (int)(t - row * nu) << 4, nb = min(16, rowbytes - b0);
        int x = b0 / C, c = b0 - x * C;
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < nb) {
                w[k >> 2] |= (unsigned)nv12_byte(src[(b * C + c) * plane + (size_t)y * W + x], st.mean[c], st.stdv[c], denorm) << (8 * (k & 3));
                if (++c == C) { c = 0; ++x; }
            }
        }
        unsigned char *o = dst + b * bstride + (size_t)y * pitch + (size_t)b0;
        if (wide && nb == 16) {
            *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < nb) o[k] = (unsigned char)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        }
    }
}

int launch_preprocess_u8_pitched(const unsigned char *src, size_t pitch, size_t bstride, float *dst, int B, int H, int W, int C, const float *mean,
                                 const float *stdv, hipStream_t s)
{
    Stats4 st{};
    for (int c = 0; c < C && c < 4; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    const int wide = mult_of(16, {(size_t)(uintptr_t)src, pitch, B > 1 ? bstride : 0});
    const size_t total = (size_t)B * H * (((size_t)W * C + 15) / 16);
    preprocess_u8_pitched_kernel<<<prepost_grid(total), 256, 0, s>>>(src, pitch, bstride, dst, B, H, W, C, wide, st);
    return (int)hipGetLastError();
}
int launch_postprocess_u8_pitched(const float *src, unsigned char *dst, size_t pitch, size_t bstride, int B, int H, int W, int C, const double *mean,
                                  const double *stdv, int denorm, hipStream_t s)
{
    Stats4d st{};
    for (int c = 0; c < C && c < 4; ++c) { st.mean[c] = mean[c]; st.stdv[c] = stdv[c]; }
    const int wide = mult_of(16, {(size_t)(uintptr_t)dst, pitch, B > 1 ? bstride : 0});
    const size_t total = (size_t)B * H * (((size_t)W * C + 15) / 16);
    postprocess_u8_pitched_kernel<<<prepost_grid(total), 256, 0, s>>>(src, dst, pitch, bstride, B, H, W, C, wide, st, denorm);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Test-time ensembling (include/emavfi.h, "ENSEMBLE DEFINITION"; per-element functions: ensemble_elem.h).
//   flip_f32_kernel        dst = the flipped src: the body below with one member and no arithmetic.
//   ensemble_mean_kernel   out = the tree mean of N members, each read through its own flip.
//                          Both: grid (pieces of a plane, planes - at most 65535 rows of the grid, a workgroup walks the planes beyond), 256
//                          threads, pure streaming: no LDS, no atomics, nothing waits on anything, the grid follows the element count.  A lane
//                          owns U units of one plane, 256 units apart, and issues the loads of all of them before the first use: 4 loads in
//                          flight per lane (8 at N = 8).  Wide form (W % 4 == 0 and every pointer 16-byte aligned, so every plane and every
//                          row starts on a unit): a unit is 4 output columns, one 16-byte store; a member flipped along H is read as the
//                          MIRRORED unit of its row and its four lanes are reversed in registers, so loads stay 16 bytes wide and a wave
//                          still covers one contiguous 1 KiB run, walked downwards.  Scalar form: a unit is one element.  The members and
//                          flips travel as kernel arguments (scalar registers after unrolling).  Plane offsets are 64-bit, indices inside a
//                          plane (at most 2^28 elements) 32-bit.
// ------------------------------------------------------------------------------------------
struct EnsembleArgs {
    const float *m[ENSEMBLE_MAX_MEMBERS];
    int flip[ENSEMBLE_MAX_MEMBERS];
    float *out;
    size_t planes, plane_elems;
    int H, W;
};

template <int N, int U, bool WIDE>
__device__ __forceinline__ void ensemble_body(const EnsembleArgs &p)
{
    using T = std::conditional_t<WIDE, float4, float>;
    const unsigned Wu = (unsigned)(WIDE ? p.W >> 2 : p.W), units = (unsigned)p.H * Wu;
    const unsigned u0 = blockIdx.x * (256u * U) + threadIdx.x;
    for (size_t pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
        const size_t base = pl * p.plane_elems;
        T v[U][N];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            const int y = (int)(u / Wu), q = (int)(u - (unsigned)y * Wu);
#pragma unroll
            for (int i = 0; i < N; ++i)
                v[k][i] = reinterpret_cast<const T *>(p.m[i] + base)[ensemble_src_unit(y, q, p.H, (int)Wu, p.flip[i])];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            if constexpr (WIDE) {
                float a[N], b[N], c[N], d[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const EnsembleUnit e = ensemble_lanes(EnsembleUnit{v[k][i].x, v[k][i].y, v[k][i].z, v[k][i].w}, p.flip[i]);
                    a[i] = e.x; b[i] = e.y; c[i] = e.z; d[i] = e.w;
                }
                reinterpret_cast<float4 *>(p.out + base)[u] = make_float4(ensemble_mean(a, N), ensemble_mean(b, N), ensemble_mean(c, N), ensemble_mean(d, N));
            } else {
                (p.out + base)[u] = ensemble_mean(v[k], N);
            }
        }
    }
}

template <bool WIDE> __global__ __launch_bounds__(256) void flip_f32_kernel(EnsembleArgs p) { ensemble_body<1, 4, WIDE>(p); }
constexpr int ensemble_units(int n) { return n >= 4 ? 1 : 4 / n; }
template <int N, bool WIDE> __global__ __launch_bounds__(256) void ensemble_mean_kernel(EnsembleArgs p) { ensemble_body<N, ensemble_units(N), WIDE>(p); }

static bool ensemble_wide(const EnsembleArgs &p, int n)
{
    uintptr_t bits = (uintptr_t)p.out | (uintptr_t)(p.W & 3);
    for (int i = 0; i < n; ++i) bits |= (uintptr_t)p.m[i];
    return (bits & 15) == 0;
}

static dim3 ensemble_grid(const EnsembleArgs &p, bool wide, int per_lane)
{
    const size_t units = (size_t)p.H * (size_t)(wide ? p.W >> 2 : p.W), per_wg = 256u * (size_t)per_lane;   // units <= 2^28
    return dim3((unsigned)((units + per_wg - 1) / per_wg), (unsigned)(p.planes < 65535 ? p.planes : 65535));
}

int launch_flip_f32(const float *src, float *dst, size_t planes, int H, int W, int flip, hipStream_t s)
{
    EnsembleArgs p{};
    p.m[0] = src; p.flip[0] = flip; p.out = dst; p.planes = planes; p.plane_elems = (size_t)H * W; p.H = H; p.W = W;
    const bool wide = ensemble_wide(p, 1);
    if (wide) flip_f32_kernel<true><<<ensemble_grid(p, true, 4), 256, 0, s>>>(p);
    else flip_f32_kernel<false><<<ensemble_grid(p, false, 4), 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

template <int N> static void launch_ensemble_mean_n(const EnsembleArgs &p, hipStream_t s)
{
    if (ensemble_wide(p, N)) ensemble_mean_kernel<N, true><<<ensemble_grid(p, true, ensemble_units(N)), 256, 0, s>>>(p);
    else ensemble_mean_kernel<N, false><<<ensemble_grid(p, false, ensemble_units(N)), 256, 0, s>>>(p);
}

int launch_ensemble_mean_f32(const float *const *members, const int *flips, int n, float *out, size_t planes, int H, int W, hipStream_t s)
{
    EnsembleArgs p{};
    for (int i = 0; i < n; ++i) { p.m[i] = members[i]; p.flip[i] = flips[i]; }
    p.out = out; p.planes = planes; p.plane_elems = (size_t)H * W; p.H = H; p.W = W;
    switch (n) {
    case 1: launch_ensemble_mean_n<1>(p, s); break;
    case 2: launch_ensemble_mean_n<2>(p, s); break;
    case 4: launch_ensemble_mean_n<4>(p, s); break;
    case 8: launch_ensemble_mean_n<8>(p, s); break;
    default: return -2;
    }
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Frame borders (include/emavfi.h, "BORDER DEFINITION"; per-element functions: border_elem.h).
//   border_pad_f32_kernel    dst [planes][H + 2N][W + 2N] = the picture extended by replication or reflection.
//   border_crop_f32_kernel   dst [planes][H][W] = the middle of the extended picture.
//                          One body, two directions: every destination word is one source word, found by border_src_index().  Both in
//                          the mould of flip_f32_kernel: grid (pieces of a DESTINATION plane, planes - at most 65535 rows of the grid, a
//                          workgroup walks the planes beyond), 256 threads, pure streaming: no LDS, no atomics, nothing waits on anything.
//                          A lane owns 4 units of one plane, 256 units apart, and issues the loads of all of them before the first
//                          store.  Wide form (the destination's row length % 4 == 0 and dst 16-byte aligned, so every plane and row of it
//                          starts on a unit): a unit is 4 destination columns, one 16-byte store.  Its four values come as ONE 16-byte
//                          load where they are four consecutive source columns (the unit lies wholly inside the picture; always for a
//                          crop) and `vec` holds: src 16-byte aligned, the source's row length % 4 == 0 and N % 4 == 0, which together
//                          put every such unit on a 16-byte boundary of the source.  Otherwise - the border columns, the units that
//                          straddle the picture's edge, a misaligned interior - four scalar loads through the index map.  Scalar form:
//                          a unit is one element.  Plane offsets are 64-bit, indices inside a plane (at most 2^28 elements) 32-bit.
// ------------------------------------------------------------------------------------------
struct BorderArgs {
    const float *src;
    float *dst;
    size_t planes, src_plane, dst_plane;   // elements per plane
    int Hs, Ws, Hd, Wd, N, mode, vec;
};

template <bool CROP, bool WIDE>
__device__ __forceinline__ void border_body(const BorderArgs &p)
{
    constexpr int U = 4;
    using T = std::conditional_t<WIDE, float4, float>;
    const unsigned Wu = (unsigned)(WIDE ? p.Wd >> 2 : p.Wd), units = (unsigned)p.Hd * Wu;
    const unsigned u0 = blockIdx.x * (256u * U) + threadIdx.x;
    for (size_t pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
        const float *const s = p.src + pl * p.src_plane;
        T v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            const int y = (int)(u / Wu), q = (int)(u - (unsigned)y * Wu);
            if constexpr (WIDE) {
                const int x = 4 * q;
                int sx0;
                if (border_unit_inside(x, p.Ws, p.N, CROP, &sx0) && p.vec) {
                    v[k] = *reinterpret_cast<const float4 *>(s + border_src_index(y, x, p.Hs, p.Ws, p.N, p.mode, CROP));
                } else {
                    v[k] = make_float4(s[border_src_index(y, x, p.Hs, p.Ws, p.N, p.mode, CROP)], s[border_src_index(y, x + 1, p.Hs, p.Ws, p.N, p.mode, CROP)],
                                       s[border_src_index(y, x + 2, p.Hs, p.Ws, p.N, p.mode, CROP)], s[border_src_index(y, x + 3, p.Hs, p.Ws, p.N, p.mode, CROP)]);
                }
            } else {
                v[k] = s[border_src_index(y, q, p.Hs, p.Ws, p.N, p.mode, CROP)];
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            reinterpret_cast<T *>(p.dst + pl * p.dst_plane)[u] = v[k];
        }
    }
}

template <bool WIDE> __global__ __launch_bounds__(256) void border_pad_f32_kernel(BorderArgs p) { border_body<false, WIDE>(p); }
template <bool WIDE> __global__ __launch_bounds__(256) void border_crop_f32_kernel(BorderArgs p) { border_body<true, WIDE>(p); }

// the access widths of a call and its grid: the wide form needs dst alone aligned, the 16-byte loads src as well
static dim3 border_plan(BorderArgs &p, bool *wide)
{
    *wide = (((uintptr_t)p.dst | (uintptr_t)(p.Wd & 3)) & 15) == 0;
    p.vec = *wide && (((uintptr_t)p.src | (uintptr_t)(p.Ws & 3) | (uintptr_t)(p.N & 3)) & 15) == 0;
    const size_t units = (size_t)p.Hd * (size_t)(*wide ? p.Wd >> 2 : p.Wd), per_wg = 256u * 4u;   // units <= 2^28
    return dim3((unsigned)((units + per_wg - 1) / per_wg), (unsigned)(p.planes < 65535 ? p.planes : 65535));
}

int launch_border_pad_f32(const float *src, float *dst, size_t planes, int H, int W, int N, int mode, hipStream_t s)
{
    BorderArgs p{};
    p.src = src; p.dst = dst; p.planes = planes; p.Hs = H; p.Ws = W; p.Hd = border_padded_dim(H, N); p.Wd = border_padded_dim(W, N);
    p.src_plane = (size_t)p.Hs * p.Ws; p.dst_plane = (size_t)p.Hd * p.Wd; p.N = N; p.mode = mode;
    bool wide;
    const dim3 grid = border_plan(p, &wide);
    if (wide) border_pad_f32_kernel<true><<<grid, 256, 0, s>>>(p);
    else border_pad_f32_kernel<false><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

int launch_border_crop_f32(const float *src, float *dst, size_t planes, int H, int W, int N, hipStream_t s)
{
    BorderArgs p{};
    p.src = src; p.dst = dst; p.planes = planes; p.Hs = border_padded_dim(H, N); p.Ws = border_padded_dim(W, N); p.Hd = H; p.Wd = W;
    p.src_plane = (size_t)p.Hs * p.Ws; p.dst_plane = (size_t)p.Hd * p.Wd; p.N = N; p.mode = BORDER_REPLICATE;
    bool wide;
    const dim3 grid = border_plan(p, &wide);
    if (wide) border_crop_f32_kernel<true><<<grid, 256, 0, s>>>(p);
    else border_crop_f32_kernel<false><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Coarse flow (include/emavfi.h, "COARSE FLOW DEFINITION"; per-element functions: coarse_elem.h).
//   coarse_down_f32_kernel   dst [planes][Hs][Ws] = down_s of src [planes][H][W]: the quadtree mean of s x s clamped leaves.
//   coarse_up_f32_kernel     dst [planes][H][W] = s times the bilinear sample of src [planes][Hs][Ws] at half-pixel centres.
//                          Both in the mould of border_body: grid (pieces of a DESTINATION plane, planes - at most 65535 rows of the
//                          grid, a workgroup walks the planes beyond), 256 threads, pure streaming: no LDS, no atomics, nothing waits on
//                          anything.  A lane owns one unit of a plane.
//                          Down, wide form (src 16-byte aligned and W % 4 == 0, so every leaf row starts on a 16-byte boundary): a unit
//                          is K destination columns of one row - K = 4 for s = 2 and 4, K = 1 for s = 8 -, its s K leaf columns are
//                          s K / 4 16-byte loads per leaf row (rows clamped one by one), all issued before the first addition; a unit
//                          whose leaves reach past column W - 1 (the clamped edge, a short last unit) runs the scalar per-element
//                          function instead.  The K results leave as one 16-byte store where dst is 16-byte aligned and Ws % 4 == 0.
//                          Up, wide form (dst 16-byte aligned and W % 4 == 0): a unit is 4 destination columns, one 16-byte store; the
//                          coarse samples are scalar loads (1 / s^2 of the traffic, and neighbours share them in the cache).
//                          Scalar forms: a unit is one element.  Plane offsets are 64-bit, indices inside a plane (at most 2^28
//                          elements) 32-bit.  Every load's row and column index is clamped into its plane by the per-element functions.
// ------------------------------------------------------------------------------------------
struct CoarseArgs {
    const float *src;
    float *dst;
    size_t planes, src_plane, dst_plane;   // elements per plane
    int H, W, Hs, Ws, s, svec;             // H, W: the fine tensor; Hs, Ws: the coarse one; svec: 16-byte stores (down)
};

// the leaves of a wide unit, in registers: row r, column c of the unit's s x s K tile (every index is a constant after inlining)
template <int S, int K> struct CoarseTileLeaf {
    const float (&v)[S][S * K];
    int k;
    __device__ __forceinline__ float operator()(int r, int c) const { return v[r][S * k + c]; }
};

template <int S, bool WIDE>
__global__ __launch_bounds__(256) void coarse_down_f32_kernel(CoarseArgs p)
{
    constexpr int K = WIDE ? (S == 8 ? 1 : 4) : 1, Q = WIDE ? S * K / 4 : 1;
    const unsigned Wu = (unsigned)(p.Ws + K - 1) / K, units = (unsigned)p.Hs * Wu;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const int i = (int)(u / Wu), j0 = (int)(u - (unsigned)i * Wu) * K;
    const bool inside = WIDE && S * (j0 + K) <= p.W;   // every leaf column of the unit exists: no clamp along x, K valid results
    for (size_t pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
        const float *const s = p.src + pl * p.src_plane;
        float *const d = p.dst + pl * p.dst_plane + (size_t)i * p.Ws + j0;
        float o[K];
        if constexpr (WIDE) {
            if (inside) {
                float v[S][S * K];
#pragma unroll
                for (int r = 0; r < S; ++r) {
                    const int y = S * i + r < p.H - 1 ? S * i + r : p.H - 1;
                    const float4 *row = reinterpret_cast<const float4 *>(s + (size_t)y * p.W + S * j0);
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const float4 t = row[q];
                        v[r][4 * q] = t.x; v[r][4 * q + 1] = t.y; v[r][4 * q + 2] = t.z; v[r][4 * q + 3] = t.w;
                    }
                }
#pragma unroll
                for (int k = 0; k < K; ++k) o[k] = coarse_tree<S>(CoarseTileLeaf<S, K>{v, k}, 0, 0);
                if (K == 4 && p.svec) {
                    *reinterpret_cast<float4 *>(d) = make_float4(o[0], o[K > 1 ? 1 : 0], o[K > 2 ? 2 : 0], o[K > 3 ? 3 : 0]);
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) d[k] = o[k];
                }
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (j0 + k < p.Ws) d[k] = coarse_down_elem_s<S>(s, p.H, p.W, i, j0 + k);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void coarse_up_f32_kernel(CoarseArgs p)
{
    constexpr int K = WIDE ? 4 : 1;
    const unsigned Wu = (unsigned)(WIDE ? p.W >> 2 : p.W), units = (unsigned)p.H * Wu;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const int y = (int)(u / Wu), x0 = (int)(u - (unsigned)y * Wu) * K;
    const CoarseTap ty = coarse_up_tap(y, p.Hs, p.s);
    CoarseTap tx[K];
#pragma unroll
    for (int k = 0; k < K; ++k) tx[k] = coarse_up_tap(x0 + k, p.Ws, p.s);
    for (size_t pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
        const float *const s = p.src + pl * p.src_plane;
        float *const d = p.dst + pl * p.dst_plane + (size_t)y * p.W + x0;
        float o[K];
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = coarse_up_elem(s, p.Ws, ty, tx[k], p.s);
        if constexpr (WIDE) *reinterpret_cast<float4 *>(d) = make_float4(o[0], o[K > 1 ? 1 : 0], o[K > 2 ? 2 : 0], o[K > 3 ? 3 : 0]);
        else d[0] = o[0];
    }
}

static CoarseArgs coarse_args(const float *src, float *dst, size_t planes, int H, int W, int s, bool down)
{
    CoarseArgs p{};
    p.src = src; p.dst = dst; p.planes = planes; p.H = H; p.W = W; p.Hs = coarse_dim(H, s); p.Ws = coarse_dim(W, s); p.s = s;
    const size_t fine = (size_t)H * W, coarse = (size_t)p.Hs * p.Ws;
    p.src_plane = down ? fine : coarse; p.dst_plane = down ? coarse : fine;
    return p;
}
static dim3 coarse_grid(size_t units, size_t planes) { return dim3((unsigned)((units + 255) / 256), (unsigned)(planes < 65535 ? planes : 65535)); }

template <int S> static void launch_coarse_down_s(const CoarseArgs &p, bool wide, hipStream_t s)
{
    constexpr int K = S == 8 ? 1 : 4;
    if (wide) coarse_down_f32_kernel<S, true><<<coarse_grid((size_t)p.Hs * (size_t)((p.Ws + K - 1) / K), p.planes), 256, 0, s>>>(p);
    else coarse_down_f32_kernel<S, false><<<coarse_grid((size_t)p.Hs * (size_t)p.Ws, p.planes), 256, 0, s>>>(p);
}

int launch_coarse_down_f32(const float *src, float *dst, size_t planes, int H, int W, int s, hipStream_t st)
{
    CoarseArgs p = coarse_args(src, dst, planes, H, W, s, true);
    const bool wide = (((uintptr_t)src | (uintptr_t)(W & 3)) & 15) == 0;
    p.svec = (((uintptr_t)dst | (uintptr_t)(p.Ws & 3)) & 15) == 0;
    if (s == 2) launch_coarse_down_s<2>(p, wide, st);
    else if (s == 4) launch_coarse_down_s<4>(p, wide, st);
    else launch_coarse_down_s<8>(p, wide, st);
    return (int)hipGetLastError();
}

int launch_coarse_up_f32(const float *flow_s, float *flow, size_t planes, int H, int W, int s, hipStream_t st)
{
    const CoarseArgs p = coarse_args(flow_s, flow, planes, H, W, s, false);
    const bool wide = (((uintptr_t)flow | (uintptr_t)(W & 3)) & 15) == 0;
    if (wide) coarse_up_f32_kernel<true><<<coarse_grid((size_t)H * (size_t)(W >> 2), planes), 256, 0, st>>>(p);
    else coarse_up_f32_kernel<false><<<coarse_grid((size_t)H * (size_t)W, planes), 256, 0, st>>>(p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Agreement guard (include/emavfi.h, "AGREEMENT GUARD DEFINITION"; per-element functions: agreement_elem.h).
//   agreement_guard_kernel   grid (tiles along x, tiles along y, B), 256 threads, in the mould of static_guard_kernel: a workgroup owns a
//                         tile of ST_TH x ST_TW = 64 x 128 pixels of ONE sample, and the two LDS maps, their strides and the budget
//                         (27.8 KiB, 5 workgroups = 20 waves per CU) are that kernel's.  Here the map is `flagged` and the window passes
//                         DILATE it (held = some flagged pixel in the window), which is the static guard's erosion of `same` read the
//                         other way round.  Stages: (1) the map = 0; (2) every channel's u and v inside the tile plus halo, CLIPPED to
//                         the frame, are compared and a flagged sample marks its pixel - the reduction over channels is the marking
//                         itself; positions outside the frame stay 0, which is the clipped window.  The elements of the tile proper
//                         get out = (u + v) * 0.5f stored right here, so u and v are read once (plus the halo: at r = 16 the tile plus
//                         halo is 1.875 x the tile, at r = 4 1.2 x) and never again; (3) dilation along rows, then along columns, each
//                         by a running count over the 2 r + 1 window; the column pass leaves the `held` map of the tile in the first
//                         buffer and counts the tile's held pixels, one atomic add per wave into counts[b] (cleared by a launch of its
//                         own ahead: an integer sum, the order does not matter); (4) a and b are read ONLY where held and the blend
//                         overwrites what stage (2) stored there - the same workgroup, after a barrier, so the second store lands last.
//                         With nothing held the traffic is what the definition obliges - u, v in, out out - plus the halo.  In the two
//                         streaming stages (2) and (4) a lane issues the loads of AG_U = 4 units, 256 units apart, before the first use.
//                         Access width: 16-byte loads and stores, 4 columns per lane, when W % 4 == 0 and u, v, a, b, out are 16-byte
//                         aligned (every sample, plane and row then starts on a unit, and a tile's columns are whole units; a halo unit
//                         may reach past the halo but never past its row); else one element per lane.  Both forms run the same
//                         per-element functions.  Nothing outside a tensor is read.  Short-lived, waits on nothing.
// ------------------------------------------------------------------------------------------
struct AgreementArgs {
    const float *u, *v, *a, *b;
    float *out;
    unsigned *counts;
    int C, H, W, radius;
    float tol, mean[4], std[4];
};

constexpr int AG_U = 4;                                          // units a lane has in flight in the two streaming stages

template <bool WIDE>
__global__ __launch_bounds__(256) void agreement_guard_kernel(AgreementArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char flag[ST_RH * ST_BS];      // stage (3) on: held [ST_TH][ST_TW]
    __shared__ __attribute__((aligned(16))) unsigned char rowflag[ST_RH * ST_ES];
    using T = std::conditional_t<WIDE, float4, float>;
    constexpr int E = WIDE ? 4 : 1;                              // elements of a unit
    const int tid = threadIdx.x, r = p.radius;
    const int tx0 = blockIdx.x * ST_TW, ty0 = blockIdx.y * ST_TH;
    const int tx1 = min(tx0 + ST_TW, p.W), ty1 = min(ty0 + ST_TH, p.H);           // the tile, clipped: [ty0, ty1) x [tx0, tx1)
    const int X0 = static_window_lo(tx0, r), X1 = static_window_hi(tx1 - 1, r, p.W) + 1;
    const int Y0 = static_window_lo(ty0, r), Y1 = static_window_hi(ty1 - 1, r, p.H) + 1;   // the tile plus halo, clipped to the frame
    const int ox = tx0 - r, oy = ty0 - r, RW = ST_TW + 2 * r, RH = ST_TH + 2 * r;  // the LDS map: RH x RW pixels from (oy, ox)
    const size_t plane = (size_t)p.H * p.W, sample = (size_t)blockIdx.z * p.C * plane;
    const float *const u = p.u + sample, *const v = p.v + sample, *const a = p.a + sample, *const b = p.b + sample;
    float *const out = p.out + sample;

    for (int i = tid; i < ST_RH * ST_BS / 4; i += 256) reinterpret_cast<unsigned *>(flag)[i] = 0u;
    __syncthreads();

    // (2) a flagged sample marks its pixel; the tile's own elements are stored as kept.  A lane issues the loads of AG_U units, 256 units
    // apart, before the first use: 2 AG_U loads in flight per lane.
    {
        const int x0 = WIDE ? X0 & ~3 : X0, x1 = WIDE ? (X1 + 3) & ~3 : X1;      // wide: W % 4 == 0, so x1 <= W
        const int nu = (x1 - x0) / E, per = (Y1 - Y0) * nu, items = p.C * per;
        for (int t0 = tid; t0 < items; t0 += 256 * AG_U) {
            T uu[AG_U], vv[AG_U];
            size_t off[AG_U];
            int y[AG_U], x[AG_U];
#pragma unroll
            for (int k = 0; k < AG_U; ++k) {
                const int t = t0 + 256 * k;
                if (t >= items) continue;
                const int c = t / per, rem = t - c * per, rr = rem / nu;
                y[k] = Y0 + rr; x[k] = x0 + (rem - rr * nu) * E;
                off[k] = (size_t)c * plane + (size_t)y[k] * p.W + x[k];
                uu[k] = *reinterpret_cast<const T *>(u + off[k]);
                vv[k] = *reinterpret_cast<const T *>(v + off[k]);
            }
#pragma unroll
            for (int k = 0; k < AG_U; ++k) {
                if (t0 + 256 * k >= items) continue;
                const float *const ue = reinterpret_cast<const float *>(&uu[k]), *const ve = reinterpret_cast<const float *>(&vv[k]);
                const int ly = y[k] - oy;                                         // 0 <= ly < RH: Y0 >= oy and Y1 <= ty1 + r
                T kept;
                float *const ke = reinterpret_cast<float *>(&kept);
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const int lx = x[k] + j - ox;
                    if (agreement_flagged(ue[j], ve[j], p.tol) && lx >= 0 && lx < RW) flag[ly * ST_BS + lx] = 1;
                    ke[j] = agreement_kept(ue[j], ve[j]);
                }
                // a unit lies inside the tile or outside it
                if (y[k] >= ty0 && y[k] < ty1 && x[k] >= tx0 && x[k] < tx1) *reinterpret_cast<T *>(out + off[k]) = kept;
            }
        }
    }
    __syncthreads();

    // (3) dilation, rows then columns: the held map replaces `flag`
    unsigned char *const held = flag;
    {
        unsigned n = tile_window_passes<true>(flag, rowflag, r, tid, tx0, tx1, ty0, ty1);
        if (p.counts) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
            if ((tid & 63) == 0 && n) atomicAdd(p.counts + blockIdx.z, n);
        }
    }
    __syncthreads();

    // (4) the blend of the sources at the held positions, over what stage (2) stored there; again AG_U units' loads ahead of their use
    {
        const int nu = (tx1 - tx0) / E, per = (ty1 - ty0) * nu, items = p.C * per;   // wide: tx0 and tx1 are multiples of 4
        for (int t0 = tid; t0 < items; t0 += 256 * AG_U) {
            T aa[AG_U], bb[AG_U];
            size_t off[AG_U];
            unsigned hm[AG_U];
            int ch[AG_U];
#pragma unroll
            for (int k = 0; k < AG_U; ++k) {
                const int t = t0 + 256 * k;
                hm[k] = 0u;
                if (t >= items) continue;
                const int c = t / per, rem = t - c * per, rr = rem / nu, x = tx0 + (rem - rr * nu) * E;
                const unsigned char *const hp = held + rr * ST_TW + (x - tx0);
#pragma unroll
                for (int j = 0; j < E; ++j) hm[k] |= (hp[j] ? 1u : 0u) << j;
                if (!hm[k]) continue;
                ch[k] = c;
                off[k] = (size_t)c * plane + (size_t)(ty0 + rr) * p.W + x;
                aa[k] = *reinterpret_cast<const T *>(a + off[k]);
                bb[k] = *reinterpret_cast<const T *>(b + off[k]);
            }
#pragma unroll
            for (int k = 0; k < AG_U; ++k) {
                if (!hm[k]) continue;
                const float *const ae = reinterpret_cast<const float *>(&aa[k]), *const be = reinterpret_cast<const float *>(&bb[k]);
                T blend;
                float *const le = reinterpret_cast<float *>(&blend);
#pragma unroll
                for (int j = 0; j < E; ++j) le[j] = agreement_fallback(ae[j], be[j], p.mean[ch[k]], p.std[ch[k]]);
                if (hm[k] == (1u << E) - 1u) {
                    *reinterpret_cast<T *>(out + off[k]) = blend;
                } else {
#pragma unroll
                    for (int j = 0; j < E; ++j)
                        if (hm[k] >> j & 1u) out[off[k] + j] = le[j];
                }
            }
        }
    }
}

int launch_agreement_guard_f32(const float *u, const float *v, const float *a, const float *b, float *out, int B, int C, int H, int W,
                               int radius, float tol, const float *mean, const float *std, unsigned *counts, hipStream_t s)
{
    AgreementArgs p{};
    p.u = u; p.v = v; p.a = a; p.b = b; p.out = out; p.counts = counts; p.C = C; p.H = H; p.W = W; p.radius = radius; p.tol = tol;
    for (int c = 0; c < C; ++c) { p.mean[c] = mean[c]; p.std[c] = std[c]; }
    if (counts) {
        static_counts_clear_kernel<<<dim3((unsigned)((B + 255) / 256)), 256, 0, s>>>(counts, B);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess) return (int)err;
    }
    const dim3 grid((unsigned)((W + ST_TW - 1) / ST_TW), (unsigned)((H + ST_TH - 1) / ST_TH), (unsigned)B);   // B <= 65535
    const bool wide = W % 4 == 0 && mult_of(16, {(size_t)(uintptr_t)u, (size_t)(uintptr_t)v, (size_t)(uintptr_t)a, (size_t)(uintptr_t)b,
                                                  (size_t)(uintptr_t)out});
    if (wide) agreement_guard_kernel<true><<<grid, 256, 0, s>>>(p);
    else agreement_guard_kernel<false><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Frame metrics on the device (include/emavfi.h, "FRAME METRIC DEFINITION"; per-element functions: metrics_elem.h): per image pair and
// channel the sum of squared differences and the sum of the windows' quantised SSIM.
//   frame_metrics_kernel   grid (tiles of 32 windows along x, along y, B), 256 threads.  A workgroup OWNS the 32 x 32 windows of its tile and
//                          the 32 x 32 pixels at the tile's origin (the last tile of an axis: every pixel up to the edge), so each window and
//                          each SSE pixel is counted exactly once; an image with no window (H or W below 11) is one tile that only sums
//                          squared differences.  Stages: (1) the tile's 42 x 42 pixels of BOTH images go to LDS as they lie in memory
//                          (channels interleaved; 192 bytes per row: 42 pixels of 4 channels and up to 15 bytes of alignment slack), with
//                          16-byte loads where pointer, pitch and batch stride allow and the unit ends inside the row, else byte by byte - pitch
//                          padding is never read; then per channel (2) the squared differences of the owned pixels and the row pass: a lane
//                          per (row, window column) writes the five 11-tap sums as u32 words [moment][row][32 columns]; (3) the column pass:
//                          lane = window column, 8 groups of 4 window rows; a lane walks 14 rows of its column and feeds each word to the (up
//                          to 4) windows it belongs to, in u64.  The 32 lanes of a half-wave read 32 consecutive words of one row: no bank
//                          conflict, whatever the row stride; (4) the double-precision tail per window, q summed as int64; (5) integer
//                          reduction over the workgroup -> part[b][c][tile] = {sse, ssimq}.  Integer sums: the grouping does not matter.
//   frame_metrics_finish   one workgroup per (b, c) adds the tiles' partial sums -> out[b][c] = {sse, ssimq}: every word of `out` is written
// ------------------------------------------------------------------------------------------
constexpr int MT = 32, MROWS = MT + METRICS_HALO, MLROW = 192;
static_assert(MROWS * 4 + 15 <= MLROW && MLROW % 16 == 0, "a staged row: 42 pixels of 4 channels behind at most 15 bytes of alignment slack");
struct MetricArgs {
    const unsigned char *img[2];
    size_t pitch[2], bstride[2];
    unsigned long long *part;
    int H, W, C, wide[2];
};

template <typename T> __device__ inline T metrics_block_sum(T v, T *red, int tid)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const T s = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(256) void frame_metrics_kernel(MetricArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char px[2][MROWS * MLROW];
    __shared__ unsigned rw[5 * MROWS * MT];
    __shared__ unsigned long long red_u[4];
    __shared__ long long red_q[4];
    const int tid = threadIdx.x, C = p.C;
    const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
    const int nwx = max(p.W - METRICS_HALO, 0), nwy = max(p.H - METRICS_HALO, 0);
    const int wx = min(max(nwx - x0, 0), MT), wy = min(max(nwy - y0, 0), MT);       // windows of this tile
    const int ncols = min(MROWS, p.W - x0), nrows = min(MROWS, p.H - y0);          // staged pixels: >= 1 each
    const int ow = blockIdx.x + 1 == gridDim.x ? p.W - x0 : MT, oh = blockIdx.y + 1 == gridDim.y ? p.H - y0 : MT;   // owned pixels: <= staged
    const int rowbytes = p.W * C, bx0 = x0 * C, bx1 = (x0 + ncols) * C;
    int off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const unsigned char *base = p.img[i] + (size_t)blockIdx.z * p.bstride[i] + (size_t)y0 * p.pitch[i];
        if (p.wide[i]) {
            const int ax0 = bx0 & ~15, nu = (bx1 - ax0 + 15) >> 4;   // <= 12 units
            off[i] = bx0 - ax0;
            for (int t = tid; t < nrows * nu; t += 256) {
                const int r = t / nu, u = t - r * nu, g0 = ax0 + 16 * u;
                const unsigned char *src = base + (size_t)r * p.pitch[i] + g0;
                unsigned char *dst = &px[i][r * MLROW + 16 * u];
                if (g0 + 16 <= rowbytes) {
                    *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
                } else {
                    for (int k = 0; k < rowbytes - g0; ++k) dst[k] = src[k];
                }
            }
        } else {
            const int nb = bx1 - bx0;   // <= 168
            off[i] = 0;
            for (int t = tid; t < nrows * nb; t += 256) {
                const int r = t / nb, k = t - r * nb;
                px[i][r * MLROW + k] = base[(size_t)r * p.pitch[i] + bx0 + k];
            }
        }
    }
    __syncthreads();
    const int tile = blockIdx.y * gridDim.x + blockIdx.x, ntiles = gridDim.x * gridDim.y;
    const bool windows = wx > 0 && wy > 0;
    for (int c = 0; c < C; ++c) {
        const unsigned char *la = &px[0][off[0] + c], *lb = &px[1][off[1] + c];
        unsigned long long sse = 0ull;
        for (int t = tid; t < oh * ow; t += 256) {
            const int r = t / ow, x = t - r * ow;
            sse += metrics_sqdiff(la[r * MLROW + x * C], lb[r * MLROW + x * C]);
        }
        if (windows) {
            for (int t = tid; t < (wy + METRICS_HALO) * MT; t += 256) {
                const int r = t >> 5, x = t & (MT - 1);
                if (x < wx) {
                    unsigned m[5];
                    metrics_row5(la + r * MLROW + x * C, lb + r * MLROW + x * C, C, m);
#pragma unroll
                    for (int k = 0; k < 5; ++k) rw[(k * MROWS + r) * MT + x] = m[k];
                }
            }
        }
        __syncthreads();
        long long q = 0;
        const int x = tid & (MT - 1), yb = (tid >> 5) * 4;
        if (windows && x < wx && yb < wy) {
            unsigned long long acc[4][5];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[k][m] = 0ull;
#pragma unroll
            for (int r = 0; r < 4 + METRICS_HALO; ++r) {       // rows yb + r <= 41: inside rw; rows past wy + 9 feed discarded windows only
                unsigned v[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) v[m] = rw[(m * MROWS + yb + r) * MT + x];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (r - k >= 0 && r - k < METRICS_WIN) {
#pragma unroll
                        for (int m = 0; m < 5; ++m) acc[k][m] = metrics_col_tap(acc[k][m], r - k, v[m]);
                    }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (yb + k < wy) q += metrics_tail(acc[k][0], acc[k][1], acc[k][2], acc[k][3], acc[k][4]);
        }
        const unsigned long long sse_all = metrics_block_sum(sse, red_u, tid);
        const long long q_all = metrics_block_sum(q, red_q, tid);
        if (tid == 0) {
            unsigned long long *o = p.part + (((size_t)blockIdx.z * C + c) * ntiles + tile) * 2;
            o[0] = sse_all;
            o[1] = (unsigned long long)q_all;
        }
    }
}

__global__ __launch_bounds__(256) void frame_metrics_finish(const unsigned long long *__restrict__ part, int ntiles, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long red_u[4];
    __shared__ long long red_q[4];
    const int tid = threadIdx.x;
    const unsigned long long *src = part + (size_t)blockIdx.x * ntiles * 2;
    unsigned long long sse = 0ull;
    long long q = 0;
    for (int t = tid; t < ntiles; t += 256) {
        sse += src[2 * t];
        q += (long long)src[2 * t + 1];
    }
    const unsigned long long sse_all = metrics_block_sum(sse, red_u, tid);
    const long long q_all = metrics_block_sum(q, red_q, tid);
    if (tid == 0) {
        out[(size_t)blockIdx.x * 2] = sse_all;
        out[(size_t)blockIdx.x * 2 + 1] = (unsigned long long)q_all;
    }
}

void frame_metrics_tiles(int H, int W, int *tx, int *ty)
{
    *tx = W > METRICS_HALO ? (W - METRICS_HALO + MT - 1) / MT : 1;
    *ty = H > METRICS_HALO ? (H - METRICS_HALO + MT - 1) / MT : 1;
}
int launch_frame_metrics_u8(const unsigned char *a, size_t a_pitch, size_t a_bstride, const unsigned char *b, size_t b_pitch, size_t b_bstride, int B,
                            int H, int W, int C, unsigned long long *out, unsigned long long *part, hipStream_t s)
{
    int tx, ty;
    frame_metrics_tiles(H, W, &tx, &ty);
    MetricArgs p{{a, b}, {a_pitch, b_pitch}, {B > 1 ? a_bstride : 0, B > 1 ? b_bstride : 0}, part, H, W, C, {0, 0}};
    p.wide[0] = mult_of(16, {(size_t)(uintptr_t)a, a_pitch, B > 1 ? a_bstride : 0});
    p.wide[1] = mult_of(16, {(size_t)(uintptr_t)b, b_pitch, B > 1 ? b_bstride : 0});
    frame_metrics_kernel<<<dim3((unsigned)tx, (unsigned)ty, (unsigned)B), 256, 0, s>>>(p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    frame_metrics_finish<<<dim3((unsigned)(B * C)), 256, 0, s>>>(part, tx * ty, out);
    return (int)hipGetLastError();
}

// ---- census of the one-launch packs (deform_pack3.inl, DeformParams::census): one wave per block adds the 64 slots
struct CensusTotals { unsigned long long t[8]; };
__global__ void census_reduce_kernel(const unsigned *__restrict__ census, unsigned long long *__restrict__ out, CensusTotals totals)
{
    const int blk = blockIdx.x, lane = threadIdx.x;   // 64 threads
    const unsigned *c = census + ((size_t)blk * 64 + lane) * 4;
    unsigned long long fix = c[0], par = c[1];
    unsigned mx = c[2];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        fix += __shfl_xor(fix, sh);
        par += __shfl_xor(par, sh);
        const unsigned o = __shfl_xor(mx, sh);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        out[blk * 4 + 0] = fix; out[blk * 4 + 1] = totals.t[blk]; out[blk * 4 + 2] = par; out[blk * 4 + 3] = mx;
    }
}
int launch_census_reduce(const unsigned *census, unsigned long long *out, int nblocks, const unsigned long long *totals, hipStream_t s)
{
    if (nblocks < 1 || nblocks > 8) return (int)hipErrorInvalidValue;
    CensusTotals t{};
    for (int i = 0; i < nblocks; ++i) t.t[i] = totals[i];
    census_reduce_kernel<<<nblocks, 64, 0, s>>>(census, out, t);
    return (int)hipGetLastError();
}

// ---- the adaptive forward's route selector (include/emavfi.h, emavfi_forward_adaptive): one wave, after the last attention block.  Per
// block with a routed pack it adds the census slots of this forward (the counters route_select reads are the ones the packs above just
// wrote: nothing else in a forward touches those bytes), divides by the host's wave-tap total (kernel arguments: fixed under graph
// capture), records the route that ran and the share, and writes the next route with hysteresis.  State words: include/emavfi.h.
struct RouteSelectArgs { unsigned long long totals[8]; float enter, leave; unsigned nblocks, magic; };
__global__ void route_select_kernel(const unsigned *__restrict__ census, unsigned *__restrict__ state, RouteSelectArgs a)
{
    const int lane = threadIdx.x;   // 64 threads
    if (state[0] != a.magic || state[1] != a.nblocks) return;   // not a state of this model: leave it as it is
    unsigned next = 0u, ran = 0u;
    for (unsigned i = 0; i < a.nblocks; ++i) {
        const unsigned cur = state[8 + i] != 0u ? 1u : 0u;
        unsigned nxt = cur;
        if (a.totals[i] != 0ull) {
            unsigned long long fix = census[((size_t)i * 64 + lane) * 4];
#pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) fix += __shfl_xor(fix, sh);
            const float share = (float)((double)fix / (double)a.totals[i]);
            nxt = cur ? (share <= a.leave ? 0u : 1u) : (share >= a.enter ? 1u : 0u);
            if (lane == 0) {
                state[16 + i] = __float_as_uint(share);
                if (nxt != cur) state[24 + i] += 1u;
                state[8 + i] = nxt;
            }
        }
        ran |= cur << i;
        next |= nxt << i;
    }
    if (lane == 0) {
        state[2] = next;
        state[3] = ran;
        state[4] += 1u;
    }
}
int launch_route_select(const unsigned *census, void *state, int nblocks, const unsigned long long *totals, float enter, float leave,
                        unsigned magic, hipStream_t s)
{
    if (nblocks < 1 || nblocks > 8) return (int)hipErrorInvalidValue;
    RouteSelectArgs a{};
    for (int i = 0; i < nblocks; ++i) a.totals[i] = totals[i];
    a.enter = enter; a.leave = leave; a.nblocks = (unsigned)nblocks; a.magic = magic;
    route_select_kernel<<<1, 64, 0, s>>>(census, (unsigned *)state, a);
    return (int)hipGetLastError();
}

// a fresh route state (include/emavfi.h): 32 threads, one word each
__global__ void route_state_init_kernel(unsigned *__restrict__ state, unsigned magic, unsigned nblocks, unsigned start_gather)
{
    const unsigned w = threadIdx.x;   // 32 threads, one word each
    unsigned v = 0u;
    if (w == 0) v = magic;
    else if (w == 1) v = nblocks;
    else if (w == 2) v = start_gather;
    else if (w >= 8 && w < 16) v = (start_gather >> (w - 8)) & 1u;
    else if (w >= 16 && w < 24) v = __float_as_uint(-1.0f);
    state[w] = v;
}
int launch_route_state_init(void *state, unsigned magic, int nblocks, unsigned start_gather, hipStream_t s)
{
    route_state_init_kernel<<<1, 32, 0, s>>>((unsigned *)state, magic, (unsigned)nblocks, start_gather);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Global motion (include/emavfi.h, "ALIGN DEFINITION"; per-element functions: align_elem.h).
//   align_signature_f32_kernel  sig [B][Hc][Wc] u16 = the sum of the 16 quantised lumas of each 4 x 4 cell.  A lane owns one whole cell: grid
//                          (cells / 256, samples - at most 65535 rows of the grid, a workgroup walks the samples beyond), 256 threads, pure
//                          streaming.  Wide form (W % 4 == 0 and x 16-byte aligned, so every plane, row and cell starts on a 16-byte
//                          boundary): a cell is 12 16-byte loads - 4 rows of 3 planes, issued together -, neighbouring lanes read
//                          neighbouring 16 bytes.  Scalar form: 48 loads through the same align_q().  The remainder rows and columns of a
//                          frame that is no multiple of 4 are never read.
//   align_search_kernel    SAD[b][dy][dx] += the absolute differences of one tile: a workgroup takes (sample, dy, 32 rows x 128 columns of Ga).
//                          It stages the tile and the dy-shifted tile of Gb, RMAX columns wider on each side, in LDS.  The u16 cells are
//                          widened to 32 bits on the way in, which leaves room for two marks no cell can hold: 0x80000000 for a cell
//                          outside Ga's grid, 0x40000000 for one outside Gb's.  A difference that involves a mark is above 0x3FFF0000, one
//                          of two cells is at most 0xFFFF, so `d <= 0xFFFF` is "both inside" for any content of the grids, and the inner
//                          loop has no index test.  A lane owns 4 neighbouring cells of a row and all 2 RMAX + 1 dx candidates: it reads
//                          its 4 + 2 RMAX words of Gb once per row (16-byte LDS reads) and keeps one 32-bit sum per candidate in
//                          registers - RMAX is a template argument (8, 16, 32: the least that holds R) so that they stay there;
//                          candidates beyond R are computed and dropped.  A tile's sum is below 2^28.  The sums are reduced across the
//                          wave by shuffles and across the workgroup by LDS adds, and the workgroup issues ONE 64-bit integer atomic per
//                          candidate: integer sums are free of order, the result is the same bits in every run.
//   align_clear_kernel     the sums start from zero: the entry's own launch, whatever the workspace held before.
//   align_finish_kernel    one workgroup per sample: m(d) of every candidate, the least key (align_key) by an LDS minimum, how many
//                          candidates hold it, the acceptance, the four words of the record.
//   shift_f32_kernel       dst [B][C][H][W] = src moved by sign * the half-shift of its sample's record, edges replicated.  The mould of
//                          border_body: a lane owns 4 units of one plane, 256 units apart, loads first, stores after.  The record is read
//                          from device memory at an address that is uniform across the workgroup (a scalar load) and clamped to +-16384
//                          before it meets an index, so any content of `shifts` is safe.  Wide form (W % 4 == 0, dst 16-byte aligned): a
//                          unit is 4 destination columns, one 16-byte store; where its 4 sources are consecutive columns, src is 16-byte
//                          aligned and the move is even (a recorded half-shift always is) they come as one 16-byte or two 8-byte loads,
//                          else as 4 scalar loads through the clamp.  Scalar form: a unit is one element.
// ------------------------------------------------------------------------------------------
struct AlignSigArgs {
    const float *x;
    unsigned short *sig;
    size_t plane;   // H * W
    int B, H, W, Hc, Wc;
};

template <bool WIDE>
__global__ __launch_bounds__(256) void align_signature_f32_kernel(AlignSigArgs p)
{
    const unsigned cells = (unsigned)p.Hc * (unsigned)p.Wc;   // <= 2^24
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    const unsigned i = cell / (unsigned)p.Wc, j = cell - i * (unsigned)p.Wc;
    const size_t at = (size_t)(ALIGN_CELL * i) * (size_t)p.W + ALIGN_CELL * j;   // the cell's first pixel inside a plane
    for (size_t b = blockIdx.y; b < (size_t)p.B; b += gridDim.y) {
        const float *const x0 = p.x + b * 3 * p.plane + at;
        unsigned g = 0;
        if constexpr (WIDE) {
            float4 v[3][ALIGN_CELL];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < ALIGN_CELL; ++r) v[c][r] = *reinterpret_cast<const float4 *>(x0 + c * p.plane + (size_t)r * p.W);
#pragma unroll
            for (int r = 0; r < ALIGN_CELL; ++r)
                g += (unsigned)(align_q(v[0][r].x, v[1][r].x, v[2][r].x) + align_q(v[0][r].y, v[1][r].y, v[2][r].y)
                                + align_q(v[0][r].z, v[1][r].z, v[2][r].z) + align_q(v[0][r].w, v[1][r].w, v[2][r].w));
        } else {
#pragma unroll
            for (int r = 0; r < ALIGN_CELL; ++r)
#pragma unroll
                for (int k = 0; k < ALIGN_CELL; ++k) {
                    const float *const e = x0 + (size_t)r * p.W + k;
                    g += (unsigned)align_q(e[0], e[p.plane], e[2 * p.plane]);
                }
        }
        p.sig[b * cells + cell] = (unsigned short)g;
    }
}

int launch_align_signature_f32(const float *x, unsigned short *sig, int B, int H, int W, hipStream_t s)
{
    AlignSigArgs p{};
    p.x = x; p.sig = sig; p.plane = (size_t)H * W; p.B = B; p.H = H; p.W = W; p.Hc = align_cells(H); p.Wc = align_cells(W);
    const unsigned cells = (unsigned)p.Hc * (unsigned)p.Wc;
    const dim3 grid((cells + 255u) / 256u, (unsigned)(B < 65535 ? B : 65535));
    if ((((uintptr_t)x | (uintptr_t)(W & 3)) & 15) == 0) align_signature_f32_kernel<true><<<grid, 256, 0, s>>>(p);
    else align_signature_f32_kernel<false><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}

struct AlignSearchArgs {
    const unsigned short *ga, *gb;
    unsigned long long *sad;   // [B][2R + 1][2R + 1]
    int B, Hc, Wc, R, tiles_x;
};
constexpr int ALIGN_TR = 32, ALIGN_TC = 128, ALIGN_CPT = 4;   // a tile's rows and columns; the cells of a row a lane owns
constexpr unsigned ALIGN_OUTSIDE_A = 0x80000000u, ALIGN_OUTSIDE_B = 0x40000000u;   // a staged cell outside its grid

template <int RMAX>
__global__ __launch_bounds__(256) void align_search_kernel(AlignSearchArgs p)
{
    constexpr int NDX = 2 * RMAX + 1, GBW = ALIGN_TC + 2 * RMAX, NG = ALIGN_CPT + 2 * RMAX, ROWS = 256 / (ALIGN_TC / ALIGN_CPT);
    static_assert(NG % 4 == 0 && GBW % 4 == 0 && ALIGN_TR % ROWS == 0 && NDX <= 256, "16-byte LDS reads, whole passes, a lane per candidate");
    __shared__ __align__(16) unsigned s_a[ALIGN_TR][ALIGN_TC];
    __shared__ __align__(16) unsigned s_b[ALIGN_TR][GBW];
    __shared__ unsigned s_sum[NDX];
    const int tid = (int)threadIdx.x, n1 = 2 * p.R + 1;
    const int i0 = (int)(blockIdx.x / (unsigned)p.tiles_x) * ALIGN_TR, j0 = (int)(blockIdx.x % (unsigned)p.tiles_x) * ALIGN_TC;
    const int dy = (int)blockIdx.y - p.R;
    const int rp = tid / (ALIGN_TC / ALIGN_CPT), c0 = (tid % (ALIGN_TC / ALIGN_CPT)) * ALIGN_CPT;
    for (size_t b = blockIdx.z; b < (size_t)p.B; b += gridDim.z) {
        const unsigned short *const ga = p.ga + b * (size_t)p.Hc * p.Wc, *const gb = p.gb + b * (size_t)p.Hc * p.Wc;
        for (int e = tid; e < ALIGN_TR * ALIGN_TC; e += 256) {
            const int r = e / ALIGN_TC, c = e - r * ALIGN_TC, i = i0 + r, j = j0 + c;
            s_a[r][c] = i < p.Hc && j < p.Wc ? (unsigned)ga[(size_t)i * p.Wc + j] : ALIGN_OUTSIDE_A;
        }
        for (int e = tid; e < ALIGN_TR * GBW; e += 256) {
            const int r = e / GBW, c = e - r * GBW, i = i0 + r + dy, j = j0 - RMAX + c;
            s_b[r][c] = i >= 0 && i < p.Hc && j >= 0 && j < p.Wc ? (unsigned)gb[(size_t)i * p.Wc + j] : ALIGN_OUTSIDE_B;
        }
        if (tid < NDX) s_sum[tid] = 0u;
        __syncthreads();
        unsigned acc[NDX];
#pragma unroll
        for (int k = 0; k < NDX; ++k) acc[k] = 0u;
        for (int r = rp; r < ALIGN_TR; r += ROWS) {
            const uint4 aw = *reinterpret_cast<const uint4 *>(&s_a[r][c0]);
            const unsigned a[ALIGN_CPT] = {aw.x, aw.y, aw.z, aw.w};
            unsigned g[NG];
#pragma unroll
            for (int k = 0; k < NG / 4; ++k) {
                const uint4 w = *reinterpret_cast<const uint4 *>(&s_b[r][c0 + 4 * k]);
                g[4 * k] = w.x; g[4 * k + 1] = w.y; g[4 * k + 2] = w.z; g[4 * k + 3] = w.w;
            }
#pragma unroll
            for (int k = 0; k < NDX; ++k)
#pragma unroll
                for (int c = 0; c < ALIGN_CPT; ++c) {
                    const unsigned d = align_abs_diff(a[c], g[c + k]);
                    acc[k] += d <= 0xFFFFu ? d : 0u;
                }
        }
#pragma unroll
        for (int k = 0; k < NDX; ++k) {
            unsigned v = acc[k];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63) == 0 && v) atomicAdd(&s_sum[k], v);
        }
        __syncthreads();
        const int dx = tid - RMAX;
        if (tid < NDX && dx >= -p.R && dx <= p.R && s_sum[tid])
            atomicAdd(p.sad + (b * n1 + (size_t)(dy + p.R)) * n1 + (size_t)(dx + p.R), (unsigned long long)s_sum[tid]);
        __syncthreads();
    }
}

// the sums start from zero whatever the workspace held: a kernel of the same stream, so that a captured graph replays it in order
__global__ __launch_bounds__(256) void align_clear_kernel(unsigned long long *__restrict__ sad, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) sad[i] = 0ull;
}

__global__ __launch_bounds__(256) void align_finish_kernel(const unsigned long long *__restrict__ sad, int *__restrict__ shifts, int B, int Hc, int Wc,
                                                           int R, int ratio)
{
    __shared__ unsigned long long s_key, s_m;
    __shared__ unsigned s_win;
    __shared__ int s_dy, s_dx;
    const int tid = (int)threadIdx.x, n1 = 2 * R + 1, n = n1 * n1;
    for (size_t b = blockIdx.x; b < (size_t)B; b += gridDim.x) {
        if (tid == 0) { s_key = ~0ull; s_win = 0u; }
        __syncthreads();
        unsigned long long best = ~0ull, bm = 0ull;
        int bdy = 0, bdx = 0;
        unsigned cnt = 0u;
        for (int c = tid; c < n; c += 256) {
            const int dy = c / n1 - R, dx = c % n1 - R;
            const unsigned long long m = align_m(sad[b * n + c], Hc, Wc, dy, dx), key = align_key(m, dy, dx);
            if (key < best) { best = key; bm = m; bdy = dy; bdx = dx; cnt = 1u; }
            else if (key == best) ++cnt;
        }
        atomicMin(&s_key, best);
        __syncthreads();
        if (cnt && best == s_key) {
            atomicAdd(&s_win, cnt);
            s_dy = bdy; s_dx = bdx; s_m = bm;   // one writer where it matters: several winners make the record zero
        }
        __syncthreads();
        if (tid == 0) {
            int rec[4];
            align_record(s_dy, s_dx, s_win, s_m, align_m(sad[b * n + (size_t)R * n1 + R], Hc, Wc, 0, 0), ratio, rec);
#pragma unroll
            for (int k = 0; k < 4; ++k) shifts[4 * b + k] = rec[k];
        }
        __syncthreads();
    }
}

int launch_align_search(const unsigned short *sig_a, const unsigned short *sig_b, int B, int Hc, int Wc, int R, int ratio, unsigned long long *sad,
                        int *shifts, hipStream_t s)
{
    const size_t n1 = 2 * (size_t)R + 1, sums = (size_t)B * n1 * n1;
    align_clear_kernel<<<(unsigned)((sums + 255) / 256 < 1024 ? (sums + 255) / 256 : 1024), 256, 0, s>>>(sad, sums);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    AlignSearchArgs p{};
    p.ga = sig_a; p.gb = sig_b; p.sad = sad; p.B = B; p.Hc = Hc; p.Wc = Wc; p.R = R;
    p.tiles_x = (Wc + ALIGN_TC - 1) / ALIGN_TC;
    const dim3 grid((unsigned)(p.tiles_x * ((Hc + ALIGN_TR - 1) / ALIGN_TR)), (unsigned)n1, (unsigned)(B < 65535 ? B : 65535));
    if (R <= 8) align_search_kernel<8><<<grid, 256, 0, s>>>(p);
    else if (R <= 16) align_search_kernel<16><<<grid, 256, 0, s>>>(p);
    else align_search_kernel<32><<<grid, 256, 0, s>>>(p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    align_finish_kernel<<<(unsigned)(B < 65535 ? B : 65535), 256, 0, s>>>(sad, shifts, B, Hc, Wc, R, ratio);
    return (int)hipGetLastError();
}

struct ShiftArgs {
    const float *src;
    float *dst;
    const int *shifts;
    size_t planes, plane;   // B * C; H * W
    int C, H, W, sign, vec;
};

template <bool WIDE>
__global__ __launch_bounds__(256) void shift_f32_kernel(ShiftArgs p)
{
    constexpr int U = 4;
    using T = std::conditional_t<WIDE, float4, float>;
    const unsigned Wu = (unsigned)(WIDE ? p.W >> 2 : p.W), units = (unsigned)p.H * Wu;
    const unsigned u0 = blockIdx.x * (256u * U) + threadIdx.x;
    for (size_t pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
        const size_t b = pl / (size_t)p.C;
        const int my = p.sign * align_half(p.shifts[4 * b]), mx = p.sign * align_half(p.shifts[4 * b + 1]);   // uniform: one read per workgroup
        const float *const s = p.src + pl * p.plane;
        T v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            const int y = (int)(u / Wu), q = (int)(u - (unsigned)y * Wu);
            const float *const row = s + (size_t)align_src_index(y, my, p.H) * p.W;
            if constexpr (WIDE) {
                const int x = 4 * q;
                int sx0;
                if (align_unit_inside(x, mx, p.W, &sx0) && p.vec && (sx0 & 1) == 0) {
                    if ((sx0 & 3) == 0) {
                        v[k] = *reinterpret_cast<const float4 *>(row + sx0);
                    } else {
                        const float2 lo = *reinterpret_cast<const float2 *>(row + sx0), hi = *reinterpret_cast<const float2 *>(row + sx0 + 2);
                        v[k] = make_float4(lo.x, lo.y, hi.x, hi.y);
                    }
                } else {
                    v[k] = make_float4(row[align_src_index(x, mx, p.W)], row[align_src_index(x + 1, mx, p.W)], row[align_src_index(x + 2, mx, p.W)],
                                       row[align_src_index(x + 3, mx, p.W)]);
                }
            } else {
                v[k] = row[align_src_index(q, mx, p.W)];
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const unsigned u = u0 + 256u * k;
            if (u >= units) continue;
            reinterpret_cast<T *>(p.dst + pl * p.plane)[u] = v[k];
        }
    }
}

int launch_shift_f32(const float *src, float *dst, int B, int C, int H, int W, const int *shifts, int sign, hipStream_t s)
{
    ShiftArgs p{};
    p.src = src; p.dst = dst; p.shifts = shifts; p.planes = (size_t)B * C; p.plane = (size_t)H * W; p.C = C; p.H = H; p.W = W; p.sign = sign;
    const bool wide = (((uintptr_t)dst | (uintptr_t)(W & 3)) & 15) == 0;
    p.vec = wide && ((uintptr_t)src & 15) == 0;
    const size_t units = (size_t)H * (size_t)(wide ? W >> 2 : W), per_wg = 256u * 4u;   // units <= 2^28
    const dim3 grid((unsigned)((units + per_wg - 1) / per_wg), (unsigned)(p.planes < 65535 ? p.planes : 65535));
    if (wide) shift_f32_kernel<true><<<grid, 256, 0, s>>>(p);
    else shift_f32_kernel<false><<<grid, 256, 0, s>>>(p);
    return (int)hipGetLastError();
}
