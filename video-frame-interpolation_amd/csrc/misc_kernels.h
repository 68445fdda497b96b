// Host-callable launchers of misc_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stddef.h>
#include <stdint.h>

struct PackDesc {
    int cout, cin_raw, cin_off, cin_take;  // raw OIHW tensor: take input channels [cin_off, cin_off + cin_take)
    int ck, nchunk, nf, npass;             // packed geometry
    int perm;                              // 0 = identity, 1 = offset_conv routing (offsets | mask)
    int via_bf16;                          // 1 = round every weight to bf16 first, then store it in the packed type
                                           // (f16 fragments holding the bf16 model's weights exactly: deform_pack.inl)
    int bias_f16;                          // 1 = the fp32 bias table holds fp16-rounded values (autocast casts the bias too)
    int route;                             // ConvRoute (common.h): the layer's weight layout, written by pack_conv_kernel
    int unused_;                           // (keeps first6 / x3 / pack3 where the other pack kernels' code objects read them)
    int first6;                            // conv_first.inl layout (6 -> 64, 16-bit): [kg 5][nf 2][lane (r, h)][8]: W[32 nf + r][channel e][tap 2 kg + h]
    int x3;                                // EMAVFI_F32X3: nchunk counts VIRTUAL chunks 3 c + t; t = 0, 2 carry f16(w), t = 1 carries f16(w - f16(w))
    int pack3;                             // deform_pack3.inl layouts (f16 elements, cin_take = 67): 1 = DCN 67 -> <= 67, 2 = offset_conv 67 -> 27;
                                           // 3 = deform_f32w.inl (fp32 elements, the fp32 DCN on an LDS window)
};

// The packed weight blob is self-describing: its first 256 bytes hold this header, the payload
// (what build_plan lays out) follows.  include/emavfi.h documents the same layout for callers that move blobs around.
struct BlobHeader {
    char magic[8];                                                // "EMAVFIPK"
    uint32_t version, header_bytes;                               // EMAVFI_VERSION of the packing library; 256
    uint32_t in_ch, mid, nb, dtype;                               // the model and the REQUESTED dtype (EMAVFI_AMP16 is a layout of its own)
    uint32_t layout_tag, reserved;                                // emavfi_layout_tag() of the packing process
    uint64_t total_bytes;                                         // header + payload
    uint64_t checksum;                                            // blob_checksum() of the payload
    uint64_t reserved2;
};
static_assert(sizeof(BlobHeader) == 64, "blob header layout");
constexpr unsigned kBlobHeaderBytes = 256;
// order-independent position-weighted sum over the payload's 32-bit words: sum (w[i] + 0x9E3779B9) * (2 i + 1) mod 2^64
inline uint64_t blob_checksum_host(const void *payload, size_t bytes)
{
    const uint32_t *w = (const uint32_t *)payload;
    uint64_t s = 0;
    for (size_t i = 0; i < bytes / 4; ++i) s += ((uint64_t)w[i] + 0x9E3779B9ull) * (2 * (uint64_t)i + 1);
    return s;
}
// forward-time guard: the forward's last launch compares the blob's header with what the call expects and overwrites the frame
// with NaN on a mismatch (misc_kernels.hip, blob_guard_kernel)
struct BlobGuard { const BlobHeader *hdr; BlobHeader expect; };
int launch_blob_guard(const BlobGuard &guard, float *out, size_t n, hipStream_t s);
// `bytes` bytes at `ptr` (any alignment) set to zero by a launch on `s`: the entries' clears, which a captured graph replays in order
int launch_clear_bytes(void *ptr, size_t bytes, hipStream_t s);
// writes the header (pack time) and adds the payload checksum into it
int launch_blob_seal(void *blob, const BlobHeader &h, hipStream_t s);

int launch_pack_conv(const float *w, const float *bias, void *wp, float *bp, const PackDesc &d, int dtype, hipStream_t s);
int launch_pack_ctx(const float *lin_w, const float *lin_b, const float *w9, const float *b9, float *dst, int m, int round16,
                    hipStream_t s);
// channels-last conversion of channels [c0, c0 + nc) of every pixel (nc % 4 == 0): fp16 -> fp32 (widen) or fp32 -> fp16
// lo_off > 0 (EMAVFI_F32X3): the 16-bit side holds [hi | lo] halves, lo at element offset lo_off: widen = hi + lo, narrow writes both
int launch_convert_cl(const void *src, void *dst, size_t npx, int ps_src, int ps_dst, int c0, int nc, int widen, hipStream_t s, int lo_off = 0);
int launch_pack_input(const float *f1, const float *f2, void *dst, int B, int C, int H, int W, int cpad, int dtype, hipStream_t s);
int launch_nchw_to_cl(const float *src, void *dst, int B, int C, int H, int W, int ps, int dtype, hipStream_t s);
// channels [c0, c0 + ctake) of an NCHW tensor with C channels -> channels 0.. of ps-channel pixels (the rest zero)
int launch_nchw_to_cl_sub(const float *src, void *dst, int B, int C, int c0, int ctake, int H, int W, int ps, int dtype, hipStream_t s);
int launch_cl_to_nchw(const void *src, float *dst, int B, int C, int H, int W, int ps, int coff, int dtype, hipStream_t s);
int launch_om_from_nchw(const float *off, const float *msk, float *om, int B, int H, int W, hipStream_t s);
int launch_pool_partial(const void *src, float *part, int B, int npix, int cp, int ps, int nparts, int dtype, hipStream_t s);
// lo_off > 0 (EMAVFI_F32X3): a row of `part` holds the sums of the hi halves and, lo_off floats further, of the lo halves: added
int launch_ctx_finish(const float *part, const float *ctxw, float *ctx_out, float *table, int B, int m, int cp, int nparts,
                      int npix, int coutpad, int round16, hipStream_t s, int lo_off = 0);
// EMAVFI_F32X3 layouts: NCHW fp32 <-> channels-last f16 halves [hi: ps_half | lo: ps_half]; pack_input the same for cat(frame1, frame2)
int launch_nchw_to_cl_x3(const float *src, void *dst, int B, int C, int H, int W, int ps_half, hipStream_t s);
int launch_cl_to_nchw_x3(const void *src, float *dst, int B, int C, int H, int W, int ps_half, int coff, hipStream_t s);
int launch_pack_input_x3(const float *f1, const float *f2, void *dst, int B, int C, int H, int W, int cpad, hipStream_t s);
int launch_warp_nchw(const float *frame2, const float *flow, float *out, int B, int C, int H, int W, hipStream_t s);
// dst16 / ps16 (fp32 variant only, EMAVFI_AMP16): also write the fp16 rounding of the same values into channels [coff, ps16) of a second
// channels-last tensor
int launch_warp_fused(const float *frame2, const float *flow, void *dst, int B, int C, int H, int W, int ps, int coff, int dtype,
                      hipStream_t s, void *dst16 = nullptr, int ps16 = 0);
int launch_preprocess_u8(const unsigned char *src, float *dst, int B, int H, int W, int C, const float *mean, const float *stdv,
                         hipStream_t s);
int launch_postprocess_u8(const float *src, unsigned char *dst, int B, int H, int W, int C, const double *mean, const double *stdv,
                          int denorm, hipStream_t s);
// 4:2:0 frames (include/emavfi.h, "NV12", "HIGH BIT DEPTH", "PLANAR 4:2:0").  yuv_coefficients_depth also takes depth 8, where it returns
// yuv_coefficients' tables
void yuv_coefficients(int standard, int dec[5], int enc[9]);                    // host only
void yuv_coefficients_depth(int standard, int depth, int dec[5], int enc[9]);   // host only
// One frame batch's planes: every operand of a 4:2:0 launch that says where the samples are, by name.
enum Yuv420Layout { YUV420_SEMIPLANAR, YUV420_PLANAR };
struct Yuv420Strides { size_t pitch[3], bstride[3]; };   // bytes between rows / between batch entries of plane [p]
struct Yuv420Frame {
    void *plane[3];          // [0] Y; [1] interleaved U,V pairs (semi-planar) or U (planar); [2] V (planar; null otherwise).  Read only by preprocess
    Yuv420Strides strides;
    int layout;              // Yuv420Layout
    int depth;               // 8: bytes.  10 / 12 / 16: 16-bit words, the sample in the top bits (semi-planar: P010 ..) or the low bits (planar)
};
// layout / depth / standard / order already validated
int launch_preprocess_yuv420(const Yuv420Frame &src, float *dst, int B, int H, int W, int standard, int order, const float *mean, const float *stdv,
                             hipStream_t s);
int launch_postprocess_yuv420(const float *src, const Yuv420Frame &dst, int B, int H, int W, int standard, int order, const double *mean,
                              const double *stdv, int denorm, hipStream_t s);
// frames resized on the device (include/emavfi.h, "RESIZE DEFINITION"): pitches and batch strides in bytes, arguments already validated.
// launch_resize_u8: dst_u8 and / or dst_f32 (dense [B,C,Hd,Wd], normalised with mean / stdv) may be null - one launch writes what is asked for
int launch_resize_u8(const unsigned char *src, size_t src_pitch, size_t src_bstride, unsigned char *dst_u8, size_t dst_pitch, size_t dst_bstride,
                     float *dst_f32, int B, int Hs, int Ws, int Hd, int Wd, int C, const float *mean, const float *stdv, hipStream_t s);
int launch_preprocess_nv12_resized(const unsigned char *y, size_t y_pitch, size_t y_bstride, const unsigned char *uv, size_t uv_pitch,
                                   size_t uv_bstride, float *dst, unsigned char *y_out, size_t yo_pitch, size_t yo_bstride, unsigned char *uv_out,
                                   size_t uvo_pitch, size_t uvo_bstride, int B, int Hs, int Ws, int Hd, int Wd, int standard, int order,
                                   const float *mean, const float *stdv, hipStream_t s);
// scene cuts on the device (include/emavfi.h, "SCENE CUT DEFINITION"): arguments already validated; strides of sig_a / sig_b in u32 words
int launch_luma_signature_u8(const unsigned char *src, size_t pitch, size_t bstride, int B, int H, int W, int C, int order, unsigned *sig, hipStream_t s);
int launch_scene_flags(const unsigned *sig_a, size_t stride_a, const unsigned *sig_b, size_t stride_b, int n, int H, int W, unsigned threshold,
                       unsigned *flags, unsigned *scores, hipStream_t s);
int launch_hold_frames_u8(unsigned char *dst, size_t dst_stride, int rep, const unsigned char *alt, size_t alt_stride, const unsigned *flags, int n,
                          size_t frame_bytes, hipStream_t s);
// duplicate frames (include/emavfi.h, "DUPLICATE FRAME DEFINITION"): arguments already validated
int launch_frame_diff_cells(const unsigned char *a, size_t a_pitch, size_t a_bstride, const unsigned char *b, size_t b_pitch, size_t b_bstride, int n,
                            int H, int W, int C, int order, int sample_bytes, int depth, int shift, unsigned *cells, hipStream_t s);
int launch_duplicate_flags(const unsigned *cells, size_t stride, int n, unsigned threshold, unsigned *flags, unsigned *scores, hipStream_t s);
// temporal resampling (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION"): arguments already validated; `table` is a HOST pointer, read
// before the call returns and passed on as kernel arguments, RESAMPLE_CAP (resample_elem.h) entries per launch
struct ResampleEntry { unsigned a, b, w, f, h; };   // emavfi_resample_entry
int launch_resample_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                           const unsigned char *nodes, size_t node_stride, const ResampleEntry *table, const unsigned *flags, size_t frame_bytes,
                           int sample_bytes, int depth, int shift, hipStream_t s);
// shutter accumulation (include/emavfi.h, "SHUTTER DEFINITION"): arguments already validated; `table` is a HOST pointer, read before the
// call returns and passed on as kernel arguments, SHUTTER_CAP (shutter_elem.h) entries per launch
struct AccumulateEntry { unsigned n, f, h; unsigned tap[33]; unsigned w[33]; };   // emavfi_accumulate_entry
int launch_accumulate_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                             const unsigned char *nodes, size_t node_stride, const AccumulateEntry *table, const unsigned *flags,
                             size_t frame_bytes, int sample_bytes, int depth, int shift, hipStream_t s);
// the same with the first linear_bytes bytes of every frame averaged in light (include/emavfi.h, "LINEAR LIGHT DEFINITION"): arguments
// already validated (depth 8, 10 or 12); `lin` is a DEVICE pointer to 2^depth words
int launch_accumulate_frames_linear(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride,
                                    const unsigned char *nodes, size_t node_stride, const AccumulateEntry *table, const unsigned *flags,
                                    size_t frame_bytes, int sample_bytes, int depth, int shift, const unsigned *lin, size_t linear_bytes,
                                    hipStream_t s);
// static regions held on the device (include/emavfi.h, "STATIC REGION DEFINITION"): arguments already validated; `table` is a HOST pointer, read
// before the call returns and passed on as kernel arguments, STATIC_CAP (static_elem.h) entries per launch; `counts` may be null
struct StaticEntry { unsigned a, b; };   // emavfi_static_entry
int launch_static_guard_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride,
                               const StaticEntry *table, int H, int W, int layout, int C, int sample_bytes, int depth, int shift, int radius,
                               unsigned tol, unsigned *counts, hipStream_t s);
// the active picture (include/emavfi.h, "ACTIVE AREA DEFINITION"): arguments already validated.  launch_active_bounds: an initialising launch,
// then the scan.  launch_fill_outside_frames: `table` is a HOST pointer to n_dst indices into srcs, read before the call returns and passed
// on as kernel arguments, ACTIVE_CAP (active_elem.h) entries per launch; a rectangle that is the frame launches nothing.  The pitched u8
// pair: pitches and batch strides in bytes
int launch_active_bounds(const unsigned char *img, size_t pitch, size_t bstride, int n, int H, int W, int C, int sample_bytes, int depth, int shift,
                         unsigned level, unsigned *bounds, hipStream_t s);
int launch_fill_outside_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, const unsigned *table,
                               int H, int W, int layout, int C, int sample_bytes, int top, int left, int height, int width, hipStream_t s);
int launch_preprocess_u8_pitched(const unsigned char *src, size_t pitch, size_t bstride, float *dst, int B, int H, int W, int C, const float *mean,
                                 const float *stdv, hipStream_t s);
int launch_postprocess_u8_pitched(const float *src, unsigned char *dst, size_t pitch, size_t bstride, int B, int H, int W, int C, const double *mean,
                                  const double *stdv, int denorm, hipStream_t s);
// test-time ensembling (include/emavfi.h, "ENSEMBLE DEFINITION"): arguments already validated; `members` and `flips` are HOST arrays of n
// entries, read before the call returns and passed on as kernel arguments
int launch_flip_f32(const float *src, float *dst, size_t planes, int H, int W, int flip, hipStream_t s);
int launch_ensemble_mean_f32(const float *const *members, const int *flips, int n, float *out, size_t planes, int H, int W, hipStream_t s);
// frame borders (include/emavfi.h, "BORDER DEFINITION"): arguments already validated; H, W are the picture's size in both
int launch_border_pad_f32(const float *src, float *dst, size_t planes, int H, int W, int N, int mode, hipStream_t s);
int launch_border_crop_f32(const float *src, float *dst, size_t planes, int H, int W, int N, hipStream_t s);
// global motion (include/emavfi.h, "ALIGN DEFINITION"): arguments already validated.  launch_align_search clears `sad`
// ([B][2R + 1][2R + 1] u64) with a launch of its own, adds into it and finishes each sample's record; launch_shift_f32's kernel reads the records
// from device memory
int launch_align_signature_f32(const float *x, unsigned short *sig, int B, int H, int W, hipStream_t s);
int launch_align_search(const unsigned short *sig_a, const unsigned short *sig_b, int B, int Hc, int Wc, int R, int ratio, unsigned long long *sad,
                        int *shifts, hipStream_t s);
int launch_shift_f32(const float *src, float *dst, int B, int C, int H, int W, const int *shifts, int sign, hipStream_t s);
// coarse flow (include/emavfi.h, "COARSE FLOW DEFINITION"): arguments already validated; H, W are the FINE tensor's size in both, the
// coarse one is ceil(H / s) x ceil(W / s)
int launch_coarse_down_f32(const float *src, float *dst, size_t planes, int H, int W, int s, hipStream_t st);
int launch_coarse_up_f32(const float *flow_s, float *flow, size_t planes, int H, int W, int s, hipStream_t st);
// agreement guard (include/emavfi.h, "AGREEMENT GUARD DEFINITION"): arguments already validated; `mean` and `std` are HOST arrays of C
// entries, read before the call returns and passed on as kernel arguments
int launch_agreement_guard_f32(const float *u, const float *v, const float *a, const float *b, float *out, int B, int C, int H, int W,
                               int radius, float tol, const float *mean, const float *std, unsigned *counts, hipStream_t s);
// frame metrics on the device (include/emavfi.h, "FRAME METRIC DEFINITION"): arguments already validated; `part` holds 2 u64 per (b, c, tile)
// of frame_metrics_tiles' tx * ty tiles (32 x 32 windows each; one tile where an axis has no window)
void frame_metrics_tiles(int H, int W, int *tx, int *ty);
int launch_frame_metrics_u8(const unsigned char *a, size_t a_pitch, size_t a_bstride, const unsigned char *b, size_t b_pitch, size_t b_bstride, int B,
                            int H, int W, int C, unsigned long long *out, unsigned long long *part, hipStream_t s);
// deform_pack3.inl's census: sums the 64 atomic slots of each of `nblocks` launches ([block][64][4] u32) into out[block][4] u64 =
// {fix-up wave-taps, totals[block], samples outside the window, max |offset| as fp32 bits}
int launch_census_reduce(const unsigned *census, unsigned long long *out, int nblocks, const unsigned long long *totals, hipStream_t s);
