// libemavfi.so host side: the C-ABI of include/emavfi.h, the layer plan (which kernel
// instantiation serves which reference layer), weight packing and workspace carving.
// No device allocation, no synchronisation, no retained pointers.
#include "../../include/emavfi.h"
#include "common.h"
#include "misc_kernels.h"
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
#include "conv_first.inl"

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <string>
#include <vector>

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// common.h, SW_*: the A/B switches of the launch sequence, latched from the environment at first use
std::atomic<unsigned> g_switches{0};
std::once_flag g_switches_once;
void init_switches()
{
    std::call_once(g_switches_once, [] {
        const auto off = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
        unsigned v = 0;
        if (off("EMAVFI_CONV_FIRST")) v |= SW_NO_CONV_FIRST;
        if (off("EMAVFI_CONV_FIRSTRING")) v |= SW_NO_FIRSTRING;
        if (off("EMAVFI_CONV_HEAD")) v |= SW_NO_HEAD;
        if (off("EMAVFI_CONV_TAILFUSE")) v |= SW_NO_TAILFUSE;
        if (off("EMAVFI_CONV_LIGHT")) v |= SW_NO_CONV_LIGHT;
        if (off("EMAVFI_CONV_RING2")) v |= SW_NO_RING2;
        if (off("EMAVFI_CONV_POOLFUSE")) v |= SW_NO_POOLFUSE;
        if (off("EMAVFI_RING_CHUNK")) v |= SW_NO_RING_CHUNK;
        if (getenv("EMAVFI_NO_PERSISTENT_CONV") != nullptr) v |= SW_NO_PERSISTENT_CONV;
        if (const char *e = getenv("EMAVFI_RING_ONE_WG"); e && e[0] == '1') v |= SW_RING_ONE_WG;
        g_switches.store(v, std::memory_order_relaxed);
    });
}

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
inline size_t rup256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// whether the tile-per-workgroup kernel has the (CK, NF, stride) instantiation for elements of esize bytes (the lists of common.h)
bool conv_inst_exists(int ck, int nf, int st, int esize)
{
#define X(CK_, NF_, ST_) if (ck == CK_ && nf == NF_ && st == ST_) return true;
    EMAVFI_CONV_INSTANCES(X)
    if (esize == 2) { EMAVFI_CONV_INSTANCES_16(X) }
    if (esize == 4) { EMAVFI_CONV_INSTANCES_F32(X) }
#undef X
    return false;
}

struct Layer {
    // raw tensor
    int cout = 0, cin_raw = 0, cin_off = 0, cin_take = 0, stride = 1, perm = 0, param = 0;
    // packed geometry
    int cin_pad = 0, ck = 0, nchunk = 0, nf = 0, npass = 0, coutpad = 0;
    size_t w_off = 0, b_off = 0, w_bytes = 0;
    bool deform = false;
    bool f16_of_bf16 = false;  // bf16 model, layer consumed by deform_pack_kernel: bf16-rounded weights stored as f16
    ConvRoute route = CONV_TILE;   // the layer's kernel family and weight layout (common.h); assigned by conv_geometry() and nowhere else
    int pack3 = 0;             // deform_pack3.inl layouts: 1 = DCN, 2 = offset_conv (f16 elements)
    bool first6 = false;       // feat_ext_conv1 at mid_channels 64, 16-bit: a second copy of the weights in conv_first.inl's layout (10 KiB)
    bool fp32 = false;         // Plan::dcn32: fp32 weights, packed for and run by the fp32 kernels whatever the plan's storage type
    bool x3 = false;           // EMAVFI_F32X3: three virtual chunks per real one (w_hi, w_lo, w_hi), activations as [hi | lo] f16 halves
};

// Environment switches the PACKED LAYOUT depends on.  emavfi_pack_weights and emavfi_forward must agree on them, so the plan of
// a model reads them ONCE per process (process_layout_env: a switch flipped between packing and running cannot desynchronise
// the two); only the stage-level entry emavfi_conv3x3, which packs and runs inside one call, reads them per call (the
// parity tests compare kernels inside one process that way).  A blob packed by ANOTHER process under other switches is the
// caller's responsibility: the Python binding keys its caches by them (emavfi/lib.py, layout_switches).
struct LayoutEnv { bool m16_off, ring_off, s2ring_off, wreg_off; };
LayoutEnv read_layout_env()
{
    const auto off = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
    return LayoutEnv{off("EMAVFI_CONV_MFMA16"), off("EMAVFI_CONV_RING"), off("EMAVFI_CONV_S2RING"), off("EMAVFI_CONV_WREG")};
}
const LayoutEnv &process_layout_env()
{
    static const LayoutEnv env = read_layout_env();
    return env;
}

// bit i of emavfi_layout_tag(): every process-wide switch a packed blob's LAYOUT depends on (the blob header carries the tag of the
// packing process; emavfi_packed_check and the forward's guard compare it with this process's)
bool pack_f16_chain();
unsigned layout_tag_of(const LayoutEnv &e)
{
    return (e.m16_off ? 1u : 0u) | (e.ring_off ? 2u : 0u) | (e.s2ring_off ? 4u : 0u) | (pack_f16_chain() ? 0u : 16u) |   // (bit 3 was round 2's EMAVFI_CONV_S2_CK64 experiment, removed in round 4)
          
           (deform16_can_fuse_offset_conv(80, 3, 67, 80, 1) ? 0u : 32u) | (e.wreg_off ? 64u : 0u);   // (EMAVFI_NO_FUSED_OFFSET, latched in deform_bf16.hip)
}

bool conv_geometry(Layer &L, int esize, const LayoutEnv &env_in, bool x3 = false)
{
    // EMAVFI_F32X3 runs every layer on the generic tile kernel (weights through LDS): the weights-in-registers kernels cannot hold three
    // weight sets; the virtual chunks are appended at the end of this function
    const LayoutEnv env = x3 ? LayoutEnv{true, true, true, true} : env_in;
    L.x3 = false;
    L.route = CONV_TILE;
    L.cin_pad = rup(L.cin_take, 16);
    // Stride-2 layers on the tile kernel: 32-channel chunks, two workgroups per CU (round 2 measured 64-channel chunks - every record read
    // once, but one workgroup per CU - SLOWER: 757 vs 513 us, 534 vs 513 us; that experiment and its instances were removed in round 4,
    // when conv_wreg.inl took the 256-channel layers)
    // 64 -> 128 at stride 2 (context_encoding.0): one 64-channel chunk, each wave keeps one output fragment's weights in registers
    // (conv3x3.inl, conv3x3_s2ring_kernel); EMAVFI_CONV_S2RING=0 keeps the 32-channel-chunk plan (changes the packing: set before packing)
    if (L.stride == 2 && esize == 2 && L.cin_pad == 64 && (L.cout + 31) / 32 == 4 && !env.s2ring_off) {
        L.route = CONV_S2RING;
        L.ck = 64; L.nchunk = 1; L.nf = 4; L.npass = 1; L.coutpad = 128;
        L.w_bytes = (size_t)9 * 4 * 4 * 1024;
        return true;
    }
    // 64 -> 64 and 65..67 -> 64 at stride 1 (feat_ext_blocks, motion_estimation.0 / .1, reconstruction.0): conv_ring.inl.
    // EMAVFI_CONV_RING=0 keeps round 2's plans (conv3x3_pingpong16_kernel / the CK = 80 tile kernel; changes the packing: set before packing)
    if (L.stride == 1 && esize == 2 && L.cout > 32 && L.cout <= 64 && L.cin_take >= 64 && L.cin_take <= 67 && !env.ring_off) {
        L.route = L.cin_take == 64 ? CONV_RING : CONV_RING_TAIL3;
        L.ck = L.cin_pad; L.nchunk = 1; L.nf = 2; L.npass = 1; L.coutpad = 64;
        L.w_bytes = (size_t)9 * 4 * 2 * 1024 + (L.route == CONV_RING_TAIL3 ? 3 * 2 * 1024 : 0);
        return true;
    }
    // 256 output channels from >= 128 inputs (context_encoding.1 / .2 at mid_channels 64): conv_wreg.inl - all eight output fragments in one
    // pass, weights streamed into registers.  EMAVFI_CONV_WREG=0 keeps round 3's plans (changes the packing: set before packing)
    if (esize == 2 && L.cout > 224 && L.cout <= 256 && L.cin_pad >= 128 && !env.wreg_off &&
        ((L.stride == 1 && L.cin_pad % 64 == 0) || (L.stride == 2 && L.cin_pad % 32 == 0))) {
        L.route = CONV_WREG;
        L.ck = L.stride == 1 ? 64 : 32; L.nchunk = L.cin_pad / L.ck; L.nf = 8; L.npass = 1; L.coutpad = 256;
        L.w_bytes = (size_t)L.nchunk * 9 * (L.ck / 16) * 8 * 1024;
        return true;
    }
    if (L.stride == 2) L.ck = (L.cin_pad % 32 == 0) ? 32 : 16;
    else if (esize == 4 && L.cin_take > 64 && L.cin_take <= 72) { L.ck = 72; L.cin_pad = 72; }   // fp32 k-groups are 8 channels: 9 instead of 10
    else if (L.cin_pad <= 80) L.ck = L.cin_pad;
    else if (L.cin_pad % 64 == 0) L.ck = 64;
    else return false;
    L.nchunk = L.cin_pad / L.ck;
    const int frags = (L.cout + 31) / 32;
    L.nf = (frags % 4 == 0) ? 4 : (frags % 2 == 0) ? 2 : 1;
    // 16-bit stride-2 layers with >= 256 output channels take all of them in ONE pass (8 fragments, 128 accumulator
    // registers per lane): every extra pass re-reads the whole input from HBM (FETCH_SIZE calibration,
    // tools/microbench/fetch_calib.hip: reading 64 bytes of every record fetches every 128-byte line)
    if (L.stride == 2 && esize == 2 && frags % 8 == 0 && L.ck == 32) L.nf = 8;
    if (L.stride == 2 && L.ck == 16) L.nf = 1;
    if (L.stride == 2 && L.ck == 32 && L.nf == 1) { L.ck = 16; L.nchunk = L.cin_pad / 16; }
    L.npass = frags / L.nf;
    L.coutpad = frags * 32;
    // fall back to narrower fragments if the preferred width has no instantiation
    while (!conv_inst_exists(L.ck, L.nf, L.stride, esize) && L.nf > 1) { L.nf /= 2; L.npass = frags / L.nf; }
    if (!conv_inst_exists(L.ck, L.nf, L.stride, esize)) return false;
    L.w_bytes = (size_t)L.npass * L.nchunk * 9 * (L.ck * esize / 32) * L.nf * 1024;
    // 16-bit full-resolution layers of one chunk and one pass leave the tile kernel (same w_bytes: the 16x16x32 packing regroups the elements):
    const bool one = esize == 2 && L.stride == 1 && L.nchunk == 1 && L.npass == 1, head = L.nf == 1 && L.cout <= 4;
    // 64 channels in, <= 64 out on 16x16x32 MFMAs, planar heads (motion_estimation.2, reconstruction.2) on conv_light.inl; EMAVFI_CONV_MFMA16=0:
    // the 32x32x16 kernels, the persistent one where it beats the tile kernel (launch_conv16, conv3x3.inl: 64 -> 64, 64 -> 32 / 64 -> 2, 67 -> 27)
    if (one && !env.m16_off && L.ck == 64 && (L.nf == 2 || L.nf == 1)) L.route = head ? CONV_LIGHT : CONV_PERSIST16;
    else if (one && !env.m16_off && L.ck == 32 && head) L.route = CONV_LIGHT;
    else if (one && ((L.ck == 64 && (L.nf == 2 || L.nf == 1)) || (L.ck == 80 && L.nf == 1))) L.route = CONV_PERSIST;
    if (x3) {   // (every switch is off above: the route is CONV_TILE or CONV_PERSIST; three weight sets leave the tile kernel only)
        if (esize != 2) return false;
        L.x3 = true;
        L.route = CONV_TILE;
        L.nchunk *= 3;      // virtual chunks 3 c + t
        L.w_bytes *= 3;
    }
    return true;
}

bool deform_geometry(Layer &L, int esize)
{
    const int cpad = rup(L.cin_take, 16), frags = (L.cout + 31) / 32;
    int ck = 0, nf = 0;   // the narrowest instantiation that holds the layer
#define X(CK_, NF_) if (!ck && CK_ >= cpad && NF_ >= frags) { ck = CK_; nf = NF_; }
    EMAVFI_DEFORM_INSTANCES(X)
#undef X
    if (!ck) return false;
    L.cin_pad = L.ck = ck; L.nchunk = 1; L.nf = nf; L.npass = 1; L.coutpad = nf * 32;
    L.w_bytes = (size_t)9 * (L.ck * esize / 32) * L.nf * 1024;
    L.deform = true;
    return true;
}

// ---- which layers run as ONE launch: the fusion rules, each stated once (sw: the switch word, common.h SW_*) ----
// conv_ring2.inl: two consecutive 64 -> 64 layers, the tensor between them only an LDS ring
bool can_pair(const Layer &a, const Layer &b, unsigned sw) { return a.route == CONV_RING && b.route == CONV_RING && !a.f16_of_bf16 && !b.f16_of_bf16 && !(sw & SW_NO_RING2); }
// conv_ring_first.inl: the 64 -> 64 layer behind feat_ext_conv1 (conv_first.inl) in the same launch
bool can_follow_first(const Layer &blk0, unsigned sw) { return blk0.route == CONV_RING && !(sw & SW_NO_FIRSTRING); }
// conv_ring.inl, HEAD: a planar head of <= 2 channels computed from the 64 -> 64 layer's rows in LDS (motion_estimation.1 + .2)
bool can_fuse_head(const Layer &a, const Layer &head, unsigned sw) { return a.route == CONV_RING && head.route == CONV_LIGHT && head.ck == 64 && head.cout <= 2 && !(sw & SW_NO_HEAD); }
// conv_ring_tail.inl: 64 -> 32 -> <= 3 planes through a second LDS ring (reconstruction.1 + .2)
bool can_fuse_tail(const Layer &r1, const Layer &r2, unsigned sw) { return r1.route == CONV_PERSIST16 && r1.nf == 1 && r1.cout == 32 && r2.route == CONV_LIGHT && r2.ck == 32 && r2.cout <= 3 && !(sw & SW_NO_TAILFUSE); }
// conv_wreg.inl: per-tile channel sums of the p4 = 256 channels instead of the layer's output (context_encoding.2 feeds the pool only)
bool can_pool_fuse(const Layer &c2, int p4, unsigned sw) { return c2.route == CONV_WREG && p4 == 256 && !(sw & SW_NO_POOLFUSE); }

// bf16 model: consecutive one-launch packs hand each other f16 bit patterns (the window is f16 on chip anyway; the
// receiving pack skips its in-LDS conversion pass).  EMAVFI_PACK_F16_CHAIN=0 keeps bf16 between them (A/B switch).
bool pack_f16_chain()
{
    static const bool off = [] { const char *e = getenv("EMAVFI_PACK_F16_CHAIN"); return e && e[0] == '0'; }();
    return !off;
}

constexpr int kMaxBlocks = 8;

struct Plan {
    bool feat16 = false;       // bf16 model with the one-launch packs: `feat` (and the warped tail) is stored as IEEE f16 - what the first
                               // pack wants on chip (no conversion pass in it) -; its other readers (context_encoding.0,
                               // motion_estimation.0) run the f16 ring kernels on bf16-rounded weights and hand bf16 on
    int in_ch, mid, nb, dtype, esize;  // dtype = the KERNEL storage type (EMAVFI_AMP16 runs the f16 kernels)
    bool amp;                          // EMAVFI_AMP16: autocast op policy (fp32 DCN on an fp32 fusion tensor, fp16 roundings)
    bool x3;                           // EMAVFI_F32X3: fp32-accurate three-term f16 split in every convolution, fp32 DCN (its contraction on the split too where dcn32[i].x3); the data flow of
                                       // the autocast mode (an fp32 fusion tensor beside the 16-bit one) without any of its roundings
    bool wide() const { return amp || x3; }   // the fusion tensor also exists in fp32 (what the fp32 DCN reads and writes)
    Layer dcn32[kMaxBlocks];           // amp: the deformable convolutions' fp32 master weights
    int fpad, p_mid;  // padded fusion / feature widths
    int fps;          // pixel stride (elements) of the fusion buffers: 72 when the 16-bit LDS-window pack serves them (the
                      // only channels any consumer reads; 144-byte pixels instead of 160: -10 % HBM traffic on every tensor
                      // the three packs and reconstruction.0 touch), else fpad
    Layer conv1, blk[kMaxBlocks], c0, c1, c2, m0, m1, m2, off[kMaxBlocks], dcn[kMaxBlocks], r0, r1, r2;
    Layer offh[kMaxBlocks];  // bf16 model at the reference width: second copy of offset_conv for the one-launch pack
    bool has_offh;
    int lin_param;
    size_t ctx_off, zero_off, total;
    const char *why;
};

Layer mk(int param, int cout, int cin_raw, int stride = 1, int cin_off = 0, int cin_take = -1, int perm = 0)
{
    Layer L;
    L.param = param; L.cout = cout; L.cin_raw = cin_raw; L.stride = stride;
    L.cin_off = cin_off; L.cin_take = cin_take < 0 ? cin_raw : cin_take; L.perm = perm;
    return L;
}

bool build_plan(Plan &P, int in_ch, int mid, int nb, int dtype)
{
    P.why = "";
    if (dtype != EMAVFI_F32 && dtype != EMAVFI_BF16 && dtype != EMAVFI_F16 && dtype != EMAVFI_AMP16 && dtype != EMAVFI_F32X3) {
        P.why = "dtype must be EMAVFI_F32, EMAVFI_BF16, EMAVFI_F16, EMAVFI_AMP16 or EMAVFI_F32X3";
        return false;
    }
    P.amp = dtype == EMAVFI_AMP16;
    P.x3 = dtype == EMAVFI_F32X3;
    if (P.wide()) dtype = EMAVFI_F16;  // every convolution runs the f16 kernels; what differs is in forward_impl / pack
    // the reference's fusion width is the literal mid_channels + 3 (ema_vfi.py:97): with any other in_channels its
    // forward raises a channel mismatch at the first attention block, so this build refuses instead of padding / dropping
    if (in_ch != 3) { P.why = "in_channels must be 3 (the reference's fusion width is mid_channels + 3, ema_vfi.py:97)"; return false; }
    if (nb < 1 || nb > kMaxBlocks) { P.why = "num_blocks must be 1..8"; return false; }
    if (mid < 8 || mid % 8 != 0) { P.why = "mid_channels must be a positive multiple of 8"; return false; }
    P.in_ch = in_ch; P.mid = mid; P.nb = nb; P.dtype = dtype; P.esize = dtype == EMAVFI_F32 ? 4 : 2;
    const int f = mid + 3;  // ema_vfi.py:97 (the +3 is literal in the reference)
    P.fpad = rup(f, 16); P.p_mid = rup(mid, 16);
    int q = 0;  // running index into the state_dict tensor list (weight, bias pairs)
    P.conv1 = mk(q, mid, 2 * in_ch); q += 2;
    for (int i = 0; i < nb; ++i) { P.blk[i] = mk(q, mid, mid); q += 2; }
    P.c0 = mk(q, 2 * mid, mid, 2); q += 2;
    P.c1 = mk(q, 4 * mid, 2 * mid, 2); q += 2;
    P.c2 = mk(q, 4 * mid, 4 * mid); q += 2;
    P.lin_param = q; q += 2;
    P.m0 = mk(q, mid, 2 * mid, 1, 0, mid); q += 2;  // feat half only; ctx half is folded into the bias table
    P.m1 = mk(q, mid, mid); q += 2;
    P.m2 = mk(q, 2, mid); q += 2;
    for (int i = 0; i < nb; ++i) {
        P.off[i] = mk(q, 27, f, 1, 0, -1, 1); q += 2;
        P.dcn[i] = mk(q, f, f); q += 2;
    }
    P.r0 = mk(q, mid, f); q += 2;
    P.r1 = mk(q, mid / 2, mid); q += 2;
    P.r2 = mk(q, in_ch, mid / 2); q += 2;

    size_t o = kBlobHeaderBytes;   // the blob's header (misc_kernels.h, BlobHeader) comes first
    auto place = [&](Layer &L, bool deform) {
        const bool ok = deform ? deform_geometry(L, P.esize) : conv_geometry(L, P.esize, process_layout_env(), P.x3);
        if (!ok) return false;
        L.w_off = o; o = rup256(o + L.w_bytes);
        L.b_off = o; o = rup256(o + (size_t)L.coutpad * sizeof(float));
        return true;
    };
    // 16-bit, 6 -> 64: the fused cat + conv kernel (conv_first.inl) reads its own 10 KiB fragment copy behind the regular one
    // (the blob always carries both layouts: EMAVFI_CONV_FIRST=0, read per forward, runs pack_input + conv3x3<16,2,1> - A/B, parity test)
    bool ok = conv_geometry(P.conv1, P.esize, process_layout_env(), P.x3);
    if (ok) {
        P.conv1.first6 = P.esize == 2 && P.conv1.cout == 64 && P.conv1.cin_take == 6 && !P.x3;
        P.conv1.w_off = o; o = rup256(o + P.conv1.w_bytes + (P.conv1.first6 ? 10240 : 0));
        P.conv1.b_off = o; o = rup256(o + (size_t)P.conv1.coutpad * sizeof(float));
    }
    for (int i = 0; i < nb && ok; ++i) ok = place(P.blk[i], false);
    ok = ok && place(P.c0, false) && place(P.c1, false) && place(P.c2, false);
    ok = ok && place(P.m0, false) && place(P.m1, false) && place(P.m2, false);
    for (int i = 0; i < nb && ok; ++i) ok = place(P.off[i], false) && place(P.dcn[i], true);
    ok = ok && place(P.r0, false) && place(P.r1, false) && place(P.r2, false);
    // The one-launch pack kernel (deform_pack.inl) keeps its window in f16 on chip whatever the storage type: in a bf16
    // model its two weight sets are the bf16-rounded values stored as f16.  The stand-alone offset_conv (conv3x3, used
    // when the pack is not fused) still reads the bf16 copy.
    P.fps = P.fpad;
    if (ok && !P.wide() && dtype != EMAVFI_F32 && nb > 0 && deform_pack3_shape(P.dcn[0].ck, P.dcn[0].nf, P.dcn[0].cin_take, P.dcn[0].cout)) P.fps = 72;
    if (ok && P.wide()) {
        for (int i = 0; i < nb && ok; ++i) {
            P.dcn32[i] = mk(P.dcn[i].param, f, f);
            ok = deform_geometry(P.dcn32[i], 4);
            P.dcn32[i].fp32 = true;
            P.dcn32[i].w_off = o; o = rup256(o + P.dcn32[i].w_bytes);
            P.dcn32[i].b_off = o; o = rup256(o + (size_t)P.dcn32[i].coutpad * sizeof(float));
        }
        if (!ok) { P.why = "no fp32 deformable-conv instantiation for these channel widths"; return false; }
    }
    if (ok && dtype == EMAVFI_F32)
        for (int i = 0; i < nb; ++i)
            if (deform_f32w_shape(P.dcn[i].ck, P.dcn[i].nf, P.dcn[i].cin_take, P.dcn[i].cout)) P.dcn[i].pack3 = 3;
    if (ok && P.wide())
        for (int i = 0; i < nb; ++i)
            if (deform_f32w_shape(P.dcn32[i].ck, P.dcn32[i].nf, P.dcn32[i].cin_take, P.dcn32[i].cout)) {
                P.dcn32[i].pack3 = 3;
                // deform_f32w.inl's x3 form (weights as f16 (hi, lo) pairs, three 16x16x16 f16 MFMAs per K = 16 step: 22 bits of each operand,
                // exact products, fp32 accumulation - the error class of an fp32 convolution's own summation order).  Also the autocast-policy
                // mode's DCN since round 6: torchvision's CUDA kernel is an fp32 computation in ANOTHER summation order, every result of this
                // mode is rounded to fp16 behind it, and the op is 73 % of that mode's step (6.9 -> 4.7 ms per launch).  EMAVFI_F32 stays exact.
                P.dcn32[i].x3 = P.x3 || P.amp;
            }
    P.has_offh = false;
    P.feat16 = false;
    const bool p3 = ok && !P.wide() && dtype != EMAVFI_F32 && nb > 0 && deform_pack3_shape(P.dcn[0].ck, P.dcn[0].nf, P.dcn[0].cin_take, P.dcn[0].cout) &&
                    P.off[0].nchunk == 1 && P.off[0].npass == 1 && P.off[0].ck == 80 && P.off[0].nf == 1;
    if (p3) {
        // a second copy of offset_conv for the one-launch pack: f16 fragments (bf16 model: the bf16-rounded values), and in
        // the deform_pack3.inl layout where that kernel serves the shape (both 16-bit models); off[i] keeps the conv3x3 layout
        P.has_offh = true;
        // (feat16: see Plan; needs the ring kernels on both sides of `feat` and at least one block in front of the last one)
        P.feat16 = dtype == EMAVFI_BF16 && pack_f16_chain() && nb >= 2 && P.blk[nb - 1].route == CONV_RING && P.c0.route == CONV_S2RING && P.m0.route == CONV_RING && P.fpad - mid == 16 &&
                   deform16_can_fuse_offset_conv(P.dcn[0].ck, P.dcn[0].nf, P.dcn[0].cin_take, P.off[0].ck, P.off[0].nf);   // (EMAVFI_NO_FUSED_OFFSET: once per process)
        if (P.feat16) P.c0.f16_of_bf16 = P.m0.f16_of_bf16 = true;
        for (int i = 0; i < nb && ok; ++i) {
            P.dcn[i].f16_of_bf16 = dtype == EMAVFI_BF16;
            P.dcn[i].pack3 = p3 ? 1 : 0;
            P.offh[i] = P.off[i];
            P.offh[i].f16_of_bf16 = dtype == EMAVFI_BF16;
            P.offh[i].pack3 = p3 ? 2 : 0;
            P.offh[i].w_off = o; o = rup256(o + P.offh[i].w_bytes);  // shares off[i]'s bias
        }
    }
    if (!ok) { P.why = "no kernel instantiation for these channel widths (built: mid_channels 8, 16, 32, 64)"; return false; }
    if (256 % rup(4 * mid, 16) != 0) { P.why = "4*mid_channels must divide 256 for the pooling kernel"; return false; }
    P.ctx_off = o;
    o = rup256(o + ((size_t)mid * 4 * mid + mid + (size_t)mid * mid * 9 + mid) * sizeof(float));
    P.zero_off = o;
    o += 256;
    P.total = o;
    return true;
}

#if defined(EMAVFI_DEFORM_STAMPS) && EMAVFI_DEFORM_STAMPS
// diagnostic build only (never the shipped library): a lazily allocated stamp buffer and its reader
unsigned long long *debug_stamp_buffer()
{
    static unsigned long long *buf = nullptr;
    if (!buf && hipMalloc(&buf, (size_t)DEFORM_STAMP_ROWS * 8 * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(buf, 0, (size_t)DEFORM_STAMP_ROWS * 8 * sizeof(unsigned long long));
    return buf;
}
#endif

inline const char *blob_at(const void *packed, size_t off) { return (const char *)packed + off; }   // Layer::w_off / b_off, Plan::zero_off

// One conv launch as its call site names it, `ConvCall{}.from(...).to(...)`: a setter per group of operands that travel together, an
// operand no setter names is absent.  The setters fill the call's half of the kernels' ConvParams, run_conv adds the layer's half.
struct ConvCall {
    ConvParams c{};
    const Layer *head = nullptr, *second = nullptr;
    const FirstParams *first = nullptr;
    ConvCall &from(const void *p, int ps, int H, int W) { c.in = p; c.in_ps = ps; c.Hin = H; c.Win = W; return *this; }    // channels-last input, its pixel stride (elements), its size
    // conv_ring_first.inl: feat_ext_conv1 on the frames runs in front of L in the same launch; its ps-channel pixels exist only as an LDS ring
    ConvCall &from(const FirstParams &fp, int ps) { first = &fp; c.in_ps = ps; c.Hin = fp.H; c.Win = fp.W; return *this; }
    ConvCall &to(void *p, int ps, int stored) { c.out = p; c.out_ps = ps; c.cstore = stored; return *this; }   // channels-last output, its pixel stride, the channels stored
    ConvCall &to_planes(float *p, int n) { c.out_planar = p; c.nplanes = n; return *this; }                    // NCHW fp32 output (EPI_PLANAR*), the fused head's where there is one
    ConvCall &to_pool_sums(float *p, int channels) { c.pool_part = p; c.out_ps = c.cstore = channels; return *this; }   // conv_wreg.inl: per-tile channel sums, no output tensor
    ConvCall &to_f32(float *p, int ps) { c.out32 = p; c.out32_ps = ps; return *this; }                         // EMAVFI_F32X3: the fp32 side output (or null), its pixel stride
    ConvCall &act(int epi) { c.epi = epi; return *this; }
    ConvCall &bias_rows(const float *table) { c.bias = table; c.bias_mode = 1; return *this; }                 // per-sample, per-border-class bias rows instead of the layer's bias
    // conv_ring.inl / conv_ring_tail.inl: L's rows stay in LDS, the planar head l is computed from them (conv_ring_tail.inl's with the epilogue epi)
    ConvCall &then_head(const Layer &l, int epi = 0) { head = &l; c.epi2 = epi; return *this; }
    ConvCall &then_layer(const Layer &l) { second = &l; return *this; }   // conv_ring2.inl: l runs behind L in the same launch; the output operands are ITS output's
    ConvCall &other16(bool on) { c.out_alt = on ? 1 : 0; return *this; }  // ConvParams::out_alt
};

// the conv3x3 launcher of kernel type kd (behind conv_ring_first.inl's layer where `first` is given: 16-bit types only)
int launch_conv(int kd, const FirstParams *first, const ConvParams &c, hipStream_t s)
{
    if (first) return kd == EMAVFI_F16 ? launch_conv_ringfirst_f16(*first, c, s) : launch_conv_ringfirst_bf16(*first, c, s);
    return kd == EMAVFI_F32 ? launch_conv3x3_f32(c, s) : kd == EMAVFI_F16 ? launch_conv3x3_f16(c, s) : launch_conv3x3_bf16(c, s);
}

int run_conv(const Plan &P, const Layer &L, const void *packed, int B, hipStream_t s, const ConvCall &a)
{
    const bool head = a.head != nullptr, first = a.first != nullptr;
    ConvParams c = a.c;
    if (!L.x3) c.out32 = nullptr;
    if (a.second) { c.w2 = blob_at(packed, a.second->w_off); c.bias2 = (const float *)blob_at(packed, a.second->b_off); }
    c.out_fill = (L.route == CONV_RING && !head && !first && c.out && c.cstore == 64 && (size_t)c.out_ps * P.esize == 144) ? 1 : 0;   // (also the fused pair's second layer)
    if (head) { c.head_w = blob_at(packed, a.head->w_off); c.head_bias = (const float *)blob_at(packed, a.head->b_off); }
    // a single-chunk layer wider than its input's pixel stride (CK = 80 fed from the 72-channel fusion buffers) reads the missing pieces as zeros
    if (L.nchunk == 1 && c.in_ps < L.ck) c.in_pieces = c.in_ps * P.esize / 16;
    c.round16 = P.amp ? 1 : 0;
    if (L.x3) {   // EMAVFI_F32X3: pixels are [hi | lo] halves of the widths the caller names
        c.x3 = 1; c.x3_lo_off = c.in_ps; c.in_ps *= 2;
        if (c.epi == EPI_NONE || c.epi == EPI_RELU) { c.out_lo_off = c.out_ps; c.out_ps *= 2; }   // (EPI_OM / planar outputs are fp32 as in every mode)
    }
    c.zeros = blob_at(packed, P.zero_off); c.w = blob_at(packed, L.w_off);
    if (!c.bias_mode) c.bias = (const float *)blob_at(packed, L.b_off);
    c.Hout = (c.Hin + L.stride - 1) / L.stride; c.Wout = (c.Win + L.stride - 1) / L.stride;   // (out_coff stays 0: no layer writes into the middle of a pixel)
    c.B = B; c.nchunk = L.nchunk; c.npass = L.npass; c.ck = L.ck; c.nf = L.nf; c.stride = L.stride; c.route = L.route;
    const bool f16_kernels = L.f16_of_bf16 && !L.deform;   // feat16: f16 activations in, bf16-rounded weights stored as f16
    const int kd = f16_kernels ? (int)EMAVFI_F16 : P.dtype;
#if defined(EMAVFI_DEFORM_STAMPS) && EMAVFI_DEFORM_STAMPS
    if (L.route == CONV_WREG && !a.c.out_planar && !getenv("EMAVFI_STAMP_RING")) c.out_planar = reinterpret_cast<float *>(debug_stamp_buffer());   // diagnostic build: conv_wreg.inl's stamps (tools/wreg_stamps.py)
    {   // diagnostic build: the LDS-ring kernels' stamps (tools/ring_stamps.py); EMAVFI_STAMP_RING = ring | tail | head | ringtail | ringfirst
        const char *sel = getenv("EMAVFI_STAMP_RING");
        const char *kind = first ? "ringfirst" : head ? (L.route == CONV_RING ? "head" : L.route == CONV_PERSIST16 ? "ringtail" : "")
                                                  : L.route == CONV_RING_TAIL3 ? "tail" : (L.route == CONV_RING && !a.second) ? "ring" : "";
        if (sel && kind[0] && strcmp(sel, kind) == 0) c.stamps = debug_stamp_buffer();
    }
    if (const char *rep = getenv("EMAVFI_DEBUG_REPEAT_CONV"))   // diagnostic build: as EMAVFI_DEBUG_REPEAT_PACK, for the plain layers
        if (!first && !f16_kernels)
            for (int i = 1; i < atoi(rep); ++i)
                if (const int rc = launch_conv(kd, nullptr, c, s)) return rc;
#endif
    return launch_conv(kd, a.first, c, s);
}

// Which kernel runs a one-launch pack: EMAVFI_ROUTE_WINDOW (deform_pack3_kernel), EMAVFI_ROUTE_GATHER (deform_gather3_kernel: same
// operands, same output, no window) or kRouteAdaptive (the routed pack, deform_route3.inl, reading the route word `word`:
// emavfi_forward_adaptive).  The two non-window kinds exist only where require_gather_route() holds.
constexpr int kRouteAdaptive = 2;
struct PackRoute { int kind = EMAVFI_ROUTE_WINDOW; const unsigned *word = nullptr; };

// One deformable launch as its call site names it (as ConvCall, on DeformParams); a layer stores all out_ps channels of its output pixels
struct DeformCall {
    DeformParams d{};
    const Layer *off = nullptr;
    int route = EMAVFI_ROUTE_WINDOW;
    // channels-last input, its pixel stride (elements), its size; the offsets / masks: read, or written first by the fused pack
    DeformCall &from(const void *p, int ps, int H, int W, float *om) { d.x = p; d.x_ps = ps; d.H = H; d.W = W; d.om = om; return *this; }
    DeformCall &to(void *p, int ps) { d.out = p; d.out_ps = d.cstore = ps; return *this; }
    // fp32 DCN: ALSO the 16-bit rounding (or null), its pixel stride and, EMAVFI_F32X3, the offset of its lo half
    DeformCall &to_16(void *p, int ps, int lo_off) { d.out16 = p; d.out16_ps = ps; d.out16_lo_off = lo_off; return *this; }
    DeformCall &fused(const Layer &l) { off = &l; return *this; }   // fused ModulatedDeformConvPack: the kernel computes om itself (l = offset_conv in the kernel's on-chip type)
    DeformCall &tail(const void *p, int ps) { d.x_tail = p; d.tail_ps = ps; return *this; }   // split input: the compact tail buffer (or null), its pixel stride
    DeformCall &f16_link(int in, int out) { d.in_f16 = in; d.out_f16 = out; return *this; }   // the bf16 model's f16 hand-off
    // one-launch pack: its census slots and its kernel (the route word shares out16's bytes: the routed pack has no fp16 side output)
    DeformCall &routed(unsigned *census, PackRoute r) { d.census = census; route = r.kind; if (r.kind == kRouteAdaptive) d.route = r.word; return *this; }
};

// the deformable launcher of kernel type kd on a route; the gather and the routed pack are 16-bit only: -2 (no instantiation) otherwise
int launch_deform(int kd, int route, const DeformParams &d, hipStream_t s)
{
    if (route == kRouteAdaptive) return kd == EMAVFI_F16 ? launch_deform_routed_f16(d, s) : kd == EMAVFI_BF16 ? launch_deform_routed_bf16(d, s) : -2;
    if (route == EMAVFI_ROUTE_GATHER) return kd == EMAVFI_F16 ? launch_deform_gather_f16(d, s) : kd == EMAVFI_BF16 ? launch_deform_gather_bf16(d, s) : -2;
    return kd == EMAVFI_F32 ? launch_deform_f32(d, s) : kd == EMAVFI_F16 ? launch_deform_f16(d, s) : launch_deform_bf16(d, s);
}

int run_deform(const Plan &P, const Layer &L, const void *packed, int B, hipStream_t s, const DeformCall &a)
{
    const int kd = L.fp32 ? (int)EMAVFI_F32 : P.dtype;
    DeformParams d = a.d;
    d.x3 = L.x3 && L.pack3 == 3 ? 1 : 0;
    if (a.off) { d.off_w = blob_at(packed, a.off->w_off); d.off_bias = (const float *)blob_at(packed, a.off->b_off); }
    d.zeros = blob_at(packed, P.zero_off); d.w = blob_at(packed, L.w_off); d.bias = (const float *)blob_at(packed, L.b_off);
    d.B = B; d.cin_real = L.cin_take; d.cout_real = L.cout; d.ck = L.ck; d.nf = L.nf; d.pack3 = L.pack3;
#if defined(EMAVFI_DEFORM_STAMPS) && EMAVFI_DEFORM_STAMPS
    {   // diagnostic build: EMAVFI_STAMP_PACK=i records only the i-th deformable launch of every 3 (default: every launch,
        // i.e. what is read back is the last pack of a forward)
        static int calls = 0;
        const char *sel = getenv("EMAVFI_STAMP_PACK");
        if ((!sel || (calls % 3) == atoi(sel)) && !getenv("EMAVFI_STAMP_RING")) d.stamps = debug_stamp_buffer();   // (the ring kernels' stamps share the buffer)
        ++calls;
    }
    // diagnostic build: EMAVFI_DEBUG_REPEAT_PACK=n launches the kernel n times back to back (same operands, same result: the input is
    // not the output) - what the board's power and clock are under THIS kernel alone (tools/power_per_kernel.py)
    if (const char *rep = getenv("EMAVFI_DEBUG_REPEAT_PACK"))
        for (int i = 1; i < atoi(rep); ++i)
            if (const int rc = launch_deform(kd, EMAVFI_ROUTE_WINDOW, d, s)) return rc;
#endif
    return launch_deform(kd, a.route, d, s);
}

// (L.param, L.param + 1 of `params`: the layer's weight and bias; L.w_off / L.b_off: where they go in `packed`)
int pack_layer(const Layer &L, const void *const *params, void *packed, int dtype, hipStream_t s, bool bias_f16 = false)
{
    PackDesc d{L.cout, L.cin_raw, L.cin_off, L.cin_take, L.ck, L.nchunk, L.nf, L.npass, L.perm, L.f16_of_bf16 ? 1 : 0, bias_f16 ? 1 : 0};
    d.route = L.route; d.first6 = L.first6 ? 1 : 0; d.pack3 = L.pack3; d.x3 = L.x3 ? 1 : 0;
    return launch_pack_conv((const float *)params[L.param], (const float *)params[L.param + 1], (char *)packed + L.w_off,
                            (float *)((char *)packed + L.b_off), d, L.f16_of_bf16 ? (int)EMAVFI_F16 : L.fp32 ? (int)EMAVFI_F32 : dtype, s);
}

struct Workspace {
    char *base; size_t cap, used;
    void *take(size_t bytes) { void *p = base ? base + used : nullptr; used = rup256(used + bytes); return p; }
};

constexpr size_t kCensusBlock = (size_t)DEFORM_CENSUS_SLOTS * 4 * sizeof(unsigned);   // one launch's census
constexpr size_t kCensusBytes = (size_t)kMaxBlocks * kCensusBlock;

// The compact tail of the fusion input (channels mid .. mid + 2, the warped frame): FOUR 16-bit channels = 8 bytes per pixel (round 6; was 8
// channels = 16 bytes).  The pack kernel's window DMA fetches 16 bytes per pixel from it - the pixel's tail and its right neighbour's,
// which land in channels 68..71 of the window slot.  No arithmetic ever sees those 8 bytes, whatever they hold (for the last pixel of the
// buffer they are slack that nothing in this mode writes: the workspace contract of include/emavfi.h owes no finite data there): every
// LDS read of a slot's tail is 8 bytes wide (deform3_stages.inl, lds_read8: channels 64..67 only), and channels 68..71 of the OUTPUT are
// stored from the bias alone (its epilogue).  The over-fetch only has to stay inside the allocation, so the buffer keeps 8 bytes of
// slack behind its last pixel (it lives in the 16-channel packed-input buffer: plenty).  The warp then moves 8 + 12 + 8 = 28 bytes per
// pixel instead of 36.
constexpr int kTailPs = 4;

struct FwdBuffers {
    void *in16, *fA, *fB, *fu0, *fu1, *c1, *c2, *c3;
    float *fuF0, *fuF1;  // amp: fp32 copies of the fusion tensor (input / output of the fp32 DCN)
    float *part, *ctx, *table, *flow, *om;
    float *tpart;        // context_encoding.2 fused with the pool (conv_wreg.inl): per-tile channel sums [B][ntiles][p4]
    int ntiles, nparts2; // ... and the partial sums avg_pool_partial reduces them to
    unsigned *census;    // deform_pack3.inl's per-launch census: [kMaxBlocks][DEFORM_CENSUS_SLOTS][4] u32, zeroed at the head of every forward
    int nparts, H2, W2, H4, W4, p2, p4, p_half;
};

void carve_forward(const Plan &P, Workspace &ws, FwdBuffers &f, int B, int H, int W)
{
    const size_t px = (size_t)B * H * W, e = (size_t)P.esize * (P.x3 ? 2 : 1);   // (EMAVFI_F32X3: [hi | lo] halves per pixel)
    f.H2 = (H + 1) / 2; f.W2 = (W + 1) / 2; f.H4 = (f.H2 + 1) / 2; f.W4 = (f.W2 + 1) / 2;
    f.p2 = rup(2 * P.mid, 16); f.p4 = rup(4 * P.mid, 16); f.p_half = rup(P.mid / 2, 16);
    const int npix4 = f.H4 * f.W4;
    f.nparts = npix4 >= 256 * 64 ? 256 : (npix4 >= 64 ? npix4 / 64 : 1);  // >= 64 pixels per partial sum
    f.in16 = ws.take(px * 16 * e);
    f.fA = ws.take(px * P.p_mid * e);
    f.fB = ws.take(px * P.p_mid * e);
    f.fu0 = ws.take(px * P.fps * e);
    f.fu1 = ws.take(px * P.fps * e);
    f.c1 = ws.take((size_t)B * f.H2 * f.W2 * f.p2 * e);
    f.c2 = ws.take((size_t)B * npix4 * f.p4 * e);
    f.c3 = ws.take((size_t)B * npix4 * f.p4 * e);
    f.part = (float *)ws.take((size_t)B * f.nparts * f.p4 * sizeof(float) * (P.x3 ? 2 : 1));
    f.ntiles = ((f.W4 + 31) / 32) * ((f.H4 + 3) / 4);   // conv_wreg_tiles()
    f.nparts2 = f.ntiles >= 32 ? (f.ntiles / 16 < 32 ? f.ntiles / 16 : 32) : 1;
    if (f.nparts2 > f.nparts) f.nparts2 = f.nparts;
    f.tpart = P.c2.route == CONV_WREG ? (float *)ws.take((size_t)B * f.ntiles * f.p4 * sizeof(float)) : nullptr;
    f.ctx = (float *)ws.take((size_t)B * P.mid * sizeof(float));
    f.table = (float *)ws.take((size_t)B * 16 * P.m0.coutpad * sizeof(float));
    f.flow = (float *)ws.take(px * 2 * sizeof(float));
    f.om = (float *)ws.take(px * 32 * sizeof(float));
    f.fuF0 = f.fuF1 = nullptr;
    if (P.wide()) {
        f.fuF0 = (float *)ws.take(px * P.fpad * sizeof(float));
        f.fuF1 = (float *)ws.take(px * P.fpad * sizeof(float));
    }
    f.census = (unsigned *)ws.take(kCensusBytes);   // (last: every other offset is what it was before round 6)
}

// ---- launch recorder: names every kernel launch of a forward, its algorithmic work, and can
// bracket each launch with caller-owned hipEvents on the launch stream (bench.py's roofline leg).
struct LaunchRec { std::string name; double flops, bytes; };
struct Recorder {
    std::vector<LaunchRec> *recs = nullptr;  // filled when enumerating
    void *const *events = nullptr;           // 2 per launch: start, stop
    int n_events = 0, idx = 0;
    bool dry = false;                        // enumerate only, launch nothing
    void *const *stage_events = nullptr;     // up to 3 hipEvent_t recorded behind the front / the attention blocks / the reconstruction
};

// the one rule for the per-launch events of every entry that takes them: NULL = none; a non-NULL array needs n_events >= 2
int set_events(Recorder &rec, void *const *events, int n_events, const char *what)
{
    if (events && n_events < 2) return fail(EMAVFI_E_ARG, "%s: events given, n_events must be >= 2", what);
    rec.events = events;
    rec.n_events = events ? n_events : 0;
    return EMAVFI_OK;
}

// records stage event i of a forward on the launch stream (no-op without stage events)
#define EMAVFI_STAGE_EVENT(rec, i)                                                                       \
    do {                                                                                                 \
        if (!(rec).dry && (rec).stage_events && (rec).stage_events[i] &&                                 \
            hipEventRecord((hipEvent_t)(rec).stage_events[i], s) != hipSuccess)                          \
            return fail(EMAVFI_E_LAUNCH, "forward: hipEventRecord of stage event %d failed", (int)(i));  \
    } while (0)

const char *dtype_name(int dtype) { return dtype == EMAVFI_F32 ? "f32" : dtype == EMAVFI_F16 ? "f16" : "bf16"; }

std::string conv_name(const Plan &P, const Layer &L)
{
    char b[96];
    snprintf(b, sizeof b, "conv3x3<%s,ck=%d,nf=%d,s=%d>", L.f16_of_bf16 ? "f16" : dtype_name(P.dtype), L.ck, L.nf, L.stride);   // (feat16: f16 kernels in a bf16 model)
    return b;
}
std::string deform_name(const Plan &P, const Layer &L)
{
    char b[96];
    snprintf(b, sizeof b, "deform<%s,ck=%d,nf=%d>", dtype_name(P.dtype), L.ck, L.nf);
    return b;
}
// algorithmic work of one conv launch: real (unpadded) channels, every tensor touched once
void conv_work(const Plan &P, const Layer &L, int B, int Hin, int Win, double out_esize, double &flops, double &bytes)
{
    const double Ho = (Hin + L.stride - 1) / L.stride, Wo = (Win + L.stride - 1) / L.stride;
    flops = 2.0 * 9.0 * L.cin_take * L.cout * Ho * Wo * B;
    bytes = (double)P.esize * L.cin_take * Hin * Win * B + out_esize * L.cout * Ho * Wo * B + 9.0 * L.cin_take * L.cout * P.esize;
}

#define EMAVFI_TRY(expr, what)                                                                       \
    do {                                                                                             \
        const int e_ = (expr);                                                                       \
        if (e_ == -2) return fail(EMAVFI_E_UNSUPPORTED, "%s: no kernel instantiation", what);        \
        if (e_ != 0) return fail(EMAVFI_E_LAUNCH, "%s: %s", what, hipGetErrorString((hipError_t)e_)); \
    } while (0)

#define EMAVFI_STEP(rec, label, fl, by, expr)                                                          \
    do {                                                                                               \
        if ((rec).recs) (rec).recs->push_back(LaunchRec{(label), (double)(fl), (double)(by)});         \
        if (!(rec).dry) {                                                                              \
            const bool ev_ = (rec).events && 2 * (rec).idx + 1 < (rec).n_events;                       \
            if (ev_ && hipEventRecord((hipEvent_t)(rec).events[2 * (rec).idx], s) != hipSuccess)       \
                return fail(EMAVFI_E_LAUNCH, "hipEventRecord failed");                                 \
            EMAVFI_TRY(expr, "forward");                                                               \
            if (ev_ && hipEventRecord((hipEvent_t)(rec).events[2 * (rec).idx + 1], s) != hipSuccess)   \
                return fail(EMAVFI_E_LAUNCH, "hipEventRecord failed");                                 \
        }                                                                                              \
        (rec).idx++;                                                                                   \
    } while (0)

// ---- one ModulatedDeformConvPack.forward (ema_vfi.py:53-60) as the forward runs it; shared by forward_impl and the stage-level entry
// emavfi_mdcn so that the stage test exercises exactly the product's routing, packing and flags.
// Whether block i runs as ONE launch (offset_conv computed on the staged window, offsets / masks never leave the registers)
bool pack_fuses(const Plan &P, int i)
{
    return P.dtype != EMAVFI_F32 && !P.amp && P.off[i].nchunk == 1 && P.off[i].npass == 1 && P.off[i].stride == 1 &&
           deform16_can_fuse_offset_conv(P.dcn[i].ck, P.dcn[i].nf, P.dcn[i].cin_take, P.off[i].ck, P.off[i].nf) &&
           (P.dcn[i].pack3 == 0 || P.has_offh);
}
// bf16 model, consecutive one-launch packs in the deform_pack3 layout: pack i writes f16 bit patterns for pack i + 1
bool pack_f16_link(const Plan &P, int i)
{
    return P.dtype == EMAVFI_BF16 && pack_f16_chain() && i >= 0 && i + 1 < P.nb && P.dcn[i].pack3 && P.dcn[i + 1].pack3 && pack_fuses(P, i) &&
           pack_fuses(P, i + 1);
}
// Whether block i may take the window-free route (deform_gather3.inl): exactly where the one-launch pack runs in the deform_pack3 layout
// (16-bit modes at the reference width); fp32, EMAVFI_AMP16, EMAVFI_F32X3 and other widths keep their kernels
bool pack_gather_ok(const Plan &P, int i) { return pack_fuses(P, i) && P.dcn[i].pack3 == 1; }
// the one check that block i has the gather route (and with it the routed pack) in this plan
int require_gather_route(const Plan &P, int i, const char *what)
{
    if (pack_gather_ok(P, i)) return EMAVFI_OK;
    return fail(EMAVFI_E_UNSUPPORTED, "%s: attention block %d has no gather route in this mode (the one-launch pack of the 16-bit modes at the reference width only)",
                what, i);
}
// 16-bit / fp32 models: x -> y (channels-last, pixel stride P.fps).  x_tail: the compact tail buffer (kTailPs channels per pixel) the first pack takes channels
// 64.. from (or null); in_f16 / out_f16: the bf16 model's f16 hand-off (DeformParams).  route: the kernel of the one-launch pack (PackRoute)
int attention_block(const Plan &P, int i, const void *packed, const void *x, void *y, float *om, const void *x_tail, int in_f16, int out_f16,
                    int B, int H, int W, hipStream_t s, Recorder &rec, unsigned *census = nullptr, PackRoute route = {})
{
    const double px = (double)B * H * W, e = P.esize, cf = P.mid + 3;
    double fl, by;
    conv_work(P, P.off[i], B, H, W, 4.0, fl, by);
    if (route.kind != EMAVFI_ROUTE_WINDOW && route.kind != EMAVFI_ROUTE_GATHER && route.kind != kRouteAdaptive)
        return fail(EMAVFI_E_ARG, "attention block %d: unknown route %d", i, route.kind);
    if (route.kind != EMAVFI_ROUTE_WINDOW)
        if (const int rc = require_gather_route(P, i, "attention block"); rc != EMAVFI_OK) return rc;
    if (pack_fuses(P, i)) {
        // one launch for the whole pack (ema_vfi.py:54-60): offset_conv on the staged window, then the DCN;
        // the input is read once and the offsets / masks never leave the registers.  Every route is listed with the window
        // kernel's algorithmic work (the gather kernel's corner reads are L1 / L2 traffic, not HBM; the routed kernel picks its body on the device)
        static const char *const kPrefix[] = {"deform<", "deform_gather<", "deform_routed<"};
        char nm[96];
        snprintf(nm, sizeof nm, "%s%s,ck=%d,nf=%d> offset_conv+dcn_v2", kPrefix[route.kind], dtype_name(P.dtype), P.dcn[i].ck, P.dcn[i].nf);
        EMAVFI_STEP(rec, nm, fl + 2.0 * 9.0 * cf * cf * px, px * (2.0 * cf * e) + 9.0 * cf * (cf + 27.0) * e,
                    run_deform(P, P.dcn[i], packed, B, s, DeformCall{}.from(x, P.fps, H, W, om).to(y, P.fps).fused(P.has_offh ? P.offh[i] : P.off[i])
                                                              .tail(x_tail, kTailPs).f16_link(in_f16, out_f16).routed(census, route)));
    } else {
        if (x_tail || in_f16 || out_f16) return fail(EMAVFI_E_UNSUPPORTED, "attention block: split tail / f16 hand-off need the one-launch pack kernel");
        EMAVFI_STEP(rec, conv_name(P, P.off[i]) + " offset_conv", fl, by, run_conv(P, P.off[i], packed, B, s, ConvCall{}.from(x, P.fps, H, W).to(om, 32, 32).act(EPI_OM)));
        EMAVFI_STEP(rec, deform_name(P, P.dcn[i]) + " dcn_v2", 2.0 * 9.0 * cf * cf * px, px * (2.0 * cf * e + 27.0 * 4.0) + 9.0 * cf * cf * e,
                    run_deform(P, P.dcn[i], packed, B, s, DeformCall{}.from(x, P.fps, H, W, om).to(y, P.fps)));
    }
    return EMAVFI_OK;
}
// EMAVFI_AMP16: fp16 offset_conv on the fp16 rounding x16 of the fusion tensor, fp32 deform_conv2d on the fp32 tensor xF -> yF; y16 receives
// the fp16 rounding of yF - from the DCN's own epilogue where the fp32 LDS-window kernel serves the shape (round 5: was a conversion
// pass per block), else from launch_convert_cl
bool amp_dcn_writes_fp16(const Plan &P, int i) { return P.dcn32[i].pack3 == 3; }
int attention_block_amp(const Plan &P, int i, const void *packed, const void *x16, const float *xF, float *yF, bool want16, void *y16, float *om, int B,
                        int H, int W, hipStream_t s, Recorder &rec)
{
    const double px = (double)B * H * W, cf = P.mid + 3;
    const size_t npx = (size_t)B * H * W;
    double fl, by;
    conv_work(P, P.off[i], B, H, W, 4.0, fl, by);
    EMAVFI_STEP(rec, conv_name(P, P.off[i]) + " offset_conv", fl, by, run_conv(P, P.off[i], packed, B, s, ConvCall{}.from(x16, P.fps, H, W).to(om, 32, 32).act(EPI_OM)));
    // (want16, not the pointer, decides: the enumeration-only pass has no buffers and must list the launches the real pass runs)
    const bool both = amp_dcn_writes_fp16(P, i) && want16;
    EMAVFI_STEP(rec, both ? (P.x3 ? "deform<f32,ck=80,nf=3> dcn_v2 (fp32 sampling, three-term f16 split contraction; writes fp32 + its f16 hi / lo halves)" : "deform<f32,ck=80,nf=3> dcn_v2 (fp32 under autocast; writes fp32 + its fp16 rounding)")
                          : "deform<f32,ck=80,nf=3> dcn_v2 (fp32 under autocast)",
                2.0 * 9.0 * cf * cf * px, px * (2.0 * cf * 4.0 + 27.0 * 4.0 + (both ? cf * 2.0 * (P.x3 ? 2 : 1) : 0.0)) + 9.0 * cf * cf * 4.0,
                run_deform(P, P.dcn32[i], packed, B, s, DeformCall{}.from(xF, P.fpad, H, W, om).to(yF, P.fpad)
                                                            .to_16(both ? y16 : nullptr, P.fps * (P.x3 ? 2 : 1), both && P.x3 ? P.fps : 0)));
    if (!both && want16)
        EMAVFI_STEP(rec, "fusion_round", 0, px * cf * 6.0, launch_convert_cl(yF, y16, npx, P.fpad, P.fps * (P.x3 ? 2 : 1), 0, P.fpad, 0, s, P.x3 ? P.fps : 0));
    return EMAVFI_OK;
}

// ---- context_encoding (ema_vfi.py:79-86, called at :120) and reconstruction (ema_vfi.py:102-107, called at :144-146) as the forward
// runs them; shared by forward_impl and the stage-level entries emavfi_context / emavfi_reconstruct
int context_stage(const Plan &P, const void *packed, const void *feat_cl, const FwdBuffers &f, int B, int H, int W, hipStream_t s, Recorder &rec)
{
    const double e = P.esize;
    const int mid = P.mid, dtype = P.dtype;
    double fl, by;
    conv_work(P, P.c0, B, H, W, e, fl, by);
    EMAVFI_STEP(rec, conv_name(P, P.c0) + " context_encoding.0", fl, by,
                run_conv(P, P.c0, packed, B, s, ConvCall{}.from(feat_cl, P.fps, H, W).to(f.c1, f.p2, f.p2).act(EPI_RELU).other16(P.feat16)));
    conv_work(P, P.c1, B, f.H2, f.W2, e, fl, by);
    EMAVFI_STEP(rec, conv_name(P, P.c1) + " context_encoding.1", fl, by,
                run_conv(P, P.c1, packed, B, s, ConvCall{}.from(f.c1, f.p2, f.H2, f.W2).to(f.c2, f.p4, f.p4).act(EPI_RELU)));
    conv_work(P, P.c2, B, f.H4, f.W4, e, fl, by);
    // conv_wreg.inl at the reference width: the layer's only reader is the pool, so the kernel writes per-tile channel sums instead of the
    // tensor (no 236 MB store + read at B = 8 x 720p); avg_pool_partial then adds tiles instead of pixels.  EMAVFI_CONV_POOLFUSE=0: A/B
    const bool poolfuse = can_pool_fuse(P.c2, f.p4, emavfi_switches());
    if (poolfuse) {
        EMAVFI_STEP(rec, conv_name(P, P.c2) + " context_encoding.2 + pool (tile sums)", fl, by - (double)B * f.H4 * f.W4 * 4 * mid * e,
                    run_conv(P, P.c2, packed, B, s, ConvCall{}.from(f.c2, f.p4, f.H4, f.W4).to_pool_sums(f.tpart, f.p4).act(EPI_RELU)));
        EMAVFI_STEP(rec, "avg_pool_partial", 0, (double)B * f.ntiles * 4 * mid * 4,
                    launch_pool_partial(f.tpart, f.part, B, f.ntiles, f.p4, f.p4, f.nparts2, EMAVFI_F32, s));
    } else {
        EMAVFI_STEP(rec, conv_name(P, P.c2) + " context_encoding.2", fl, by,
                    run_conv(P, P.c2, packed, B, s, ConvCall{}.from(f.c2, f.p4, f.H4, f.W4).to(f.c3, f.p4, f.p4).act(EPI_RELU)));
        const int hw = P.x3 ? 2 : 1;   // EMAVFI_F32X3: the hi and the lo halves are pooled as 2 x p4 channels and added in the fold
        EMAVFI_STEP(rec, "avg_pool_partial", 0, (double)B * f.H4 * f.W4 * 4 * mid * e * hw,
                    launch_pool_partial(f.c3, f.part, B, f.H4 * f.W4, hw * f.p4, hw * f.p4, f.nparts, dtype, s));
    }
    const int np = poolfuse ? f.nparts2 : f.nparts;
    EMAVFI_STEP(rec, "context_linear_fold", 0, (double)B * np * 4 * mid * 4,
                launch_ctx_finish(f.part, packed ? (const float *)((const char *)packed + P.ctx_off) : nullptr, f.ctx, f.table, B, mid,
                                  P.x3 ? 2 * f.p4 : f.p4, np, f.H4 * f.W4, P.m0.coutpad, P.amp ? 1 : 0, s, P.x3 ? f.p4 : 0));
    return EMAVFI_OK;
}

int reconstruction_stage(const Plan &P, const void *packed, const void *x, const FwdBuffers &f, float *out, int B, int H, int W, hipStream_t s, Recorder &rec)
{
    const double e = P.esize;
    const int C = P.in_ch;
    const unsigned sw = emavfi_switches();
    double fl, by;
    conv_work(P, P.r0, B, H, W, e, fl, by);
    EMAVFI_STEP(rec, conv_name(P, P.r0) + " reconstruction.0", fl, by,
                run_conv(P, P.r0, packed, B, s, ConvCall{}.from(x, P.fps, H, W).to(f.fA, P.p_mid, P.p_mid).act(EPI_RELU)));
    // reconstruction.1 + .2 in one launch (conv_ring_tail.inl): .1's rows never leave the LDS.  EMAVFI_CONV_TAILFUSE=0: two
    if (can_fuse_tail(P.r1, P.r2, sw)) {
        double fl2, by2;
        conv_work(P, P.r1, B, H, W, e, fl, by);
        conv_work(P, P.r2, B, H, W, 4.0, fl2, by2);
        const double mid_bytes = (double)B * H * W * P.r1.cout * e;
        EMAVFI_STEP(rec, "conv3x3+tail<" + std::string(dtype_name(P.dtype)) + ",64->32->" + std::to_string(P.r2.cout) + "> reconstruction.1+.2(tanh)",
                    fl + fl2, by + by2 - 2 * mid_bytes,
                    run_conv(P, P.r1, packed, B, s, ConvCall{}.from(f.fA, P.p_mid, H, W).act(EPI_RELU).then_head(P.r2, EPI_PLANAR_TANH01).to_planes(out, C)));
    } else {
        conv_work(P, P.r1, B, H, W, e, fl, by);
        EMAVFI_STEP(rec, conv_name(P, P.r1) + " reconstruction.1", fl, by,
                    run_conv(P, P.r1, packed, B, s, ConvCall{}.from(f.fA, P.p_mid, H, W).to(f.fB, f.p_half, f.p_half).act(EPI_RELU)));
        conv_work(P, P.r2, B, H, W, 4.0, fl, by);
        EMAVFI_STEP(rec, conv_name(P, P.r2) + " reconstruction.2(tanh)", fl, by,
                    run_conv(P, P.r2, packed, B, s, ConvCall{}.from(f.fB, f.p_half, H, W).act(EPI_PLANAR_TANH01).to_planes(out, C)));
    }
    return EMAVFI_OK;
}

BlobHeader expected_header(const Plan &P, int requested_dtype)
{
    BlobHeader h{};
    memcpy(h.magic, "EMAVFIPK", 8);
    h.version = EMAVFI_VERSION; h.header_bytes = kBlobHeaderBytes;
    h.in_ch = (uint32_t)P.in_ch; h.mid = (uint32_t)P.mid; h.nb = (uint32_t)P.nb; h.dtype = (uint32_t)requested_dtype;
    h.layout_tag = layout_tag_of(process_layout_env());
    h.total_bytes = P.total;
    return h;
}

// The pack routes of one forward: the per-block gather mask (emavfi_forward_routed) or, adaptive, the route state (device,
// include/emavfi.h; null when only enumerating) and the hysteresis thresholds (emavfi_forward_adaptive)
struct Routes { unsigned gather_mask = 0; bool adaptive = false; unsigned *state = nullptr; float enter = 0.0f, leave = 0.0f; };
// all (wave, tap) groups of one one-launch pack: the census denominator (emavfi_forward_census, route_select)
// Where one forward's flow comes from and where the forward ends (include/emavfi.h, "COARSE FLOW DEFINITION"): PLAIN computes it and goes
// on - every entry older than the coarse flow; STOP ends behind the launch that writes it and copies it to `out` (emavfi_forward_flow);
// GIVEN launches neither context encoding nor motion estimation and warps by the caller's `given`, read in place
// (emavfi_forward_given_flow).  When only enumerating, both pointers are null and the kind alone decides.
struct FlowPlan { enum Kind { PLAIN, STOP, GIVEN } kind = PLAIN; float *out = nullptr; const float *given = nullptr; };
static unsigned long long pack3_wave_taps(int B, int H, int W) { return (unsigned long long)B * ((H + 15) / 16) * ((W + 15) / 16) * 4ull * 9ull; }
// a forward in this mode has routed packs: every block runs the one-launch pack of the deform_pack3 layout (16-bit modes at the
// reference width; not EMAVFI_AMP16 / EMAVFI_F32X3, whose blocks run the fp32-family DCN)
static bool adaptive_applies(const Plan &P)
{
    if (P.nb < 1) return false;
    for (int i = 0; i < P.nb; ++i)
        if (!pack_gather_ok(P, i)) return false;
    return true;
}

int forward_impl(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                 const float *frame2, float *out, void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype,
                 float *const *taps, void *stream, Recorder &rec, const Routes &routes = Routes{}, const FlowPlan &flowp = FlowPlan{})
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s", P.why);
    // emavfi_forward_adaptive: every block of a mode with the one-launch pack runs the routed pack; elsewhere it is emavfi_forward
    const bool adaptive = routes.adaptive && adaptive_applies(P);
    // per-block route (emavfi_forward_routed): bit i sends attention block i to the window-free kernel
    const unsigned gather_mask = routes.gather_mask;
    if (P.nb < 32 && (gather_mask >> P.nb) != 0u)
        return fail(EMAVFI_E_ARG, "forward: gather_blocks 0x%x names blocks at or above num_blocks = %d", gather_mask, P.nb);
    for (int i = 0; i < P.nb; ++i)
        if ((gather_mask >> i) & 1u)
            if (const int rc = require_gather_route(P, i, "forward"); rc != EMAVFI_OK) return rc;
    const int requested_dtype = dtype;
    dtype = P.dtype;  // the kernel storage type from here on (EMAVFI_AMP16 -> EMAVFI_F16, with P.amp set)
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "forward: B, H, W must be >= 1 (got %d, %d, %d)", B, H, W);
    if ((size_t)B * H * W >= ((size_t)1 << 31)) return fail(EMAVFI_E_ARG, "forward: B*H*W must be < 2^31");
    // the kernels' byte offsets inside one sample are 32-bit: guard with the WIDEST element any kernel of the plan reads
    // (EMAVFI_AMP16 runs the fp32 deformable kernel on an fp32 fusion tensor: 4-byte elements beside P.esize = 2)
    const size_t widest = P.wide() ? sizeof(float) : (size_t)P.esize;
    if ((size_t)H * W * P.fpad * widest >= ((size_t)1 << 32)) return fail(EMAVFI_E_ARG, "forward: one sample's activation plane must be < 4 GiB");
    if ((size_t)H * W >= ((size_t)1 << 24)) return fail(EMAVFI_E_ARG, "forward: H*W must be < 2^24 (24-bit pixel index arithmetic in the gather kernels)");
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    FwdBuffers f;
    carve_forward(P, ws, f, B, H, W);
    if (!rec.dry) {
        // (a forward that stops behind the flow has no frame: its output is flowp.out)
        const void *const result = flowp.kind == FlowPlan::STOP ? (const void *)flowp.out : (const void *)out;
        if (!packed || !frame1 || !frame2 || !result || !workspace || (flowp.kind == FlowPlan::GIVEN && !flowp.given))
            return fail(EMAVFI_E_ARG, "forward: null pointer");
        if (!aligned16(packed) || !aligned16(workspace) || !aligned16(frame1) || !aligned16(frame2) || !aligned16(result) || !aligned16(flowp.given))
            return fail(EMAVFI_E_ARG, "forward: pointers must be 16-byte aligned");
        if (flowp.kind == FlowPlan::GIVEN && taps && (taps[1] || taps[2]))
            return fail(EMAVFI_E_ARG, "forward_given_flow: taps[1] (ctx) and taps[2] (flow) must be NULL: a forward with a given flow computes neither");
        if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "forward: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
        // every kernel reads the blob at offsets of THIS plan: a shorter buffer is another model's, another dtype's or a truncated one
        if (packed_bytes < P.total)
            return fail(EMAVFI_E_ARG, "forward: packed blob has %zu bytes, EMA_VFI(%d, %d, %d) in this dtype needs %zu (wrong model / dtype / version?)",
                        packed_bytes, in_channels, mid_channels, num_blocks, P.total);
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned sw = emavfi_switches();
    // the one-launch packs count what left their window (emavfi_forward_census reads it back): 8 KiB, zeroed per forward
    // (a clearing launch outside the recorded launch table, as the memset it replaced was: a captured graph replays it in order)
    if (!rec.dry) EMAVFI_TRY(launch_clear_bytes(f.census, kCensusBytes, s), "forward: census clear");
    // the header of the blob is compared ON THE DEVICE with what this call expects (the forward's last launch, blob_guard_kernel): a
    // blob of another version / model / dtype / layout-switch setting yields an all-NaN frame instead of plausible garbage.
    // emavfi_packed_check() is the (synchronising) entry that returns a code for it.
    BlobGuard guard{rec.dry ? nullptr : (const BlobHeader *)packed, expected_header(P, requested_dtype)};
    const int mid = P.mid, C = P.in_ch;
    const double px = (double)B * H * W, e = P.esize;
    const size_t npx = (size_t)B * H * W;
    double fl, by;

    // bf16 model: `feat` and the warped tail as f16 (Plan::feat16) when the first pack is the one-launch kernel that wants them so
    const bool feat16 = P.feat16;
    const int feat_dtype = feat16 ? (int)EMAVFI_F16 : dtype;
    // --- feature extraction: cat + conv + ReLU, then num_blocks x (conv + ReLU)  (ema_vfi.py:112-116)
    conv_work(P, P.conv1, B, H, W, e, fl, by);
    int first_blk = 0;
    void *cur = f.fA, *nxt = f.fB;
    {
        // EMAVFI_CONV_FIRST=0 / EMAVFI_CONV_FIRSTRING=0 (the blob carries both layouts; the switch word is latched once per process and
        // flipped by the parity tests through emavfi_debug_switches)
        if (P.conv1.first6 && !(sw & SW_NO_CONV_FIRST)) {
            // cat(frame1, frame2) + conv + ReLU in one launch, straight from the NCHW fp32 frames (ema_vfi.py:112-113)
            // (the enumeration-only pass has no blob: no arithmetic on its null pointer - found by the UBSan build, tests/host/host_check.cpp)
            const char *blob = (const char *)packed;
            FirstParams fp{frame1, frame2, f.fA, blob ? blob + P.conv1.w_off + P.conv1.w_bytes : nullptr,
                           blob ? (const float *)(blob + P.conv1.b_off) : nullptr, P.p_mid, H, W, B, 1};
            if (P.nb >= 1 && can_follow_first(P.blk[0], sw)) {
                // ... and feat_ext_blocks.conv_block_0 + ReLU behind it in the SAME launch (conv_ring_first.inl): feat_ext_conv1's
                // tensor exists only as an LDS ring.  EMAVFI_CONV_FIRSTRING=0 (read per call): two launches
                double fl2, by2;
                const bool last = P.nb == 1;
                void *dst = last ? f.fu0 : f.fB;
                conv_work(P, P.blk[0], B, H, W, e, fl2, by2);
                EMAVFI_STEP(rec, std::string("conv_first+conv3x3<") + dtype_name(dtype) + ",6->64->64> cat+feat_ext_conv1+conv_block_0", fl + fl2,
                            px * (8.0 * C + mid * e) + 9.0 * 2 * C * mid * e + 9.0 * mid * mid * e,
                            run_conv(P, P.blk[0], packed, B, s, ConvCall{}.from(fp, P.p_mid).to(dst, last ? P.fps : P.p_mid, P.p_mid).act(EPI_RELU)));
                first_blk = 1;
                cur = f.fB; nxt = f.fA;
            } else {
                EMAVFI_STEP(rec, std::string("conv_first<") + dtype_name(dtype) + ",6->64> cat+feat_ext_conv1", fl, px * (8.0 * C + mid * e) + 9.0 * 2 * C * mid * e,
                            dtype == EMAVFI_F16 ? launch_conv_first_f16(fp, s) : launch_conv_first_bf16(fp, s));
            }
        } else {
            EMAVFI_STEP(rec, "pack_input", 0, px * (8.0 * C + 2.0 * C * e * (P.x3 ? 2 : 1)),
                        P.x3 ? launch_pack_input_x3(frame1, frame2, f.in16, B, C, H, W, 16, s) : launch_pack_input(frame1, frame2, f.in16, B, C, H, W, 16, dtype, s));
            EMAVFI_STEP(rec, conv_name(P, P.conv1) + " feat_ext_conv1", fl, by,
                        run_conv(P, P.conv1, packed, B, s, ConvCall{}.from(f.in16, 16, H, W).to(f.fA, P.p_mid, P.p_mid).act(EPI_RELU)));
        }
    }
    for (int i = first_blk; i < P.nb; ++i) {
        // two consecutive conv_blocks as ONE launch (conv_ring2.inl): the tensor between them exists only as an LDS ring.
        // EMAVFI_CONV_RING2=0: one launch each
        const bool pair = i + 1 < P.nb && can_pair(P.blk[i], P.blk[i + 1], sw);
        const int j = pair ? i + 1 : i;   // the layer whose output leaves the launch
        const bool last = j == P.nb - 1;  // the last block writes feat straight into the fusion buffer
        void *dst = last ? f.fu0 : nxt;
        conv_work(P, P.blk[i], B, H, W, e, fl, by);
        if (pair) {
            double fl2, by2;
            conv_work(P, P.blk[j], B, H, W, e, fl2, by2);
            const double mid_bytes = (double)B * H * W * mid * e;   // the intermediate tensor is neither written nor read
            EMAVFI_STEP(rec, "conv3x3+conv3x3<" + std::string(dtype_name(dtype)) + ",64->64->64> feat_ext_blocks." + std::to_string(i) + "+" + std::to_string(j),
                        fl + fl2, by + by2 - 2 * mid_bytes,
                        run_conv(P, P.blk[i], packed, B, s, ConvCall{}.from(cur, P.p_mid, H, W).act(EPI_RELU).then_layer(P.blk[j])
                                                                .to(dst, last ? P.fps : P.p_mid, P.p_mid).other16(last && feat16)));
            i = j;
        } else {
            // (EMAVFI_F32X3: the last block also writes `feat` in fp32 into the fusion tensor the fp32 DCN reads)
            EMAVFI_STEP(rec, conv_name(P, P.blk[i]) + " feat_ext_blocks", fl, by + (last && P.x3 ? px * mid * 4.0 : 0.0),
                        run_conv(P, P.blk[i], packed, B, s, ConvCall{}.from(cur, P.p_mid, H, W).to(dst, last ? P.fps : P.p_mid, P.p_mid).act(EPI_RELU)
                                                                .other16(last && feat16).to_f32(last && P.x3 ? f.fuF0 : nullptr, P.fpad)));
        }
        if (!last) { void *t = cur; cur = nxt; nxt = t; }
    }
    if (!rec.dry && taps && taps[0])
        EMAVFI_TRY(P.x3 ? launch_cl_to_nchw_x3(f.fu0, taps[0], B, mid, H, W, P.fps, 0, s) : launch_cl_to_nchw(f.fu0, taps[0], B, mid, H, W, P.fps, 0, feat_dtype, s), "tap feat");

    // (a given flow replaces everything between `feat` and the warp: context encoding and motion estimation have no other consumer)
    if (flowp.kind != FlowPlan::GIVEN) {
        // --- context encoding (ema_vfi.py:120): two stride-2 convs, one conv, global mean, linear
        if (const int rc = context_stage(P, packed, f.fu0, f, B, H, W, s, rec); rc != EMAVFI_OK) return rc;
        if (!rec.dry && taps && taps[1])
            if (hipMemcpyAsync(taps[1], f.ctx, (size_t)B * mid * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
                return fail(EMAVFI_E_LAUNCH, "tap ctx copy failed");

        // --- motion estimation (ema_vfi.py:124-126); the broadcast-context concat is a per-border-class bias
        conv_work(P, P.m0, B, H, W, e, fl, by);
        EMAVFI_STEP(rec, conv_name(P, P.m0) + " motion_estimation.0(ctx folded)", fl, by,
                    run_conv(P, P.m0, packed, B, s, ConvCall{}.from(f.fu0, P.fps, H, W).bias_rows(f.table).to(f.fA, P.p_mid, P.p_mid).act(EPI_RELU).other16(feat16)));
        // motion_estimation.1 + .2 in one launch (conv_ring.inl, HEAD): .1's rows never leave the LDS.  EMAVFI_CONV_HEAD=0: two launches
        if (can_fuse_head(P.m1, P.m2, sw)) {
            double fl2, by2;
            conv_work(P, P.m1, B, H, W, e, fl, by);
            conv_work(P, P.m2, B, H, W, 4.0, fl2, by2);
            // bytes: .1's input and weights, .2's weights and output (the intermediate tensor is neither written nor read)
            const double mid_bytes = (double)B * H * W * mid * e;
            EMAVFI_STEP(rec, "conv3x3+head<" + std::string(dtype_name(P.dtype)) + ",64->64->" + std::to_string(P.m2.cout) + "> motion_estimation.1+.2(flow)",
                        fl + fl2, by + by2 - 2 * mid_bytes,
                        run_conv(P, P.m1, packed, B, s, ConvCall{}.from(f.fA, P.p_mid, H, W).act(EPI_RELU).then_head(P.m2).to_planes(f.flow, 2)));
        } else {
            conv_work(P, P.m1, B, H, W, e, fl, by);
            EMAVFI_STEP(rec, conv_name(P, P.m1) + " motion_estimation.1", fl, by,
                        run_conv(P, P.m1, packed, B, s, ConvCall{}.from(f.fA, P.p_mid, H, W).to(f.fB, P.p_mid, P.p_mid).act(EPI_RELU)));
            conv_work(P, P.m2, B, H, W, 4.0, fl, by);
            EMAVFI_STEP(rec, conv_name(P, P.m2) + " motion_estimation.2(flow)", fl, by,
                        run_conv(P, P.m2, packed, B, s, ConvCall{}.from(f.fB, P.p_mid, H, W).act(EPI_PLANAR).to_planes(f.flow, 2)));
        }
        if (!rec.dry && taps && taps[2])
            if (hipMemcpyAsync(taps[2], f.flow, npx * 2 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
                return fail(EMAVFI_E_LAUNCH, "tap flow copy failed");
    }
    if (flowp.kind == FlowPlan::STOP) {
        if (!rec.dry && hipMemcpyAsync(flowp.out, f.flow, npx * 2 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(EMAVFI_E_LAUNCH, "forward_flow: flow copy failed");
        return EMAVFI_OK;
    }
    const float *const flow = flowp.kind == FlowPlan::GIVEN ? flowp.given : f.flow;

    void *x = f.fu0, *y = f.fu1;
    if (P.wide()) {
        // --- EMAVFI_F32X3 takes the same data flow without any rounding: the fp32 fusion tensor is what the fp32 DCN reads and
        // writes, its [hi | lo] f16 halves (22 bits) are what the split convolutions read.
        // --- EMAVFI_AMP16: the autocast op policy for ema_vfi.py:130-138.  grid_sample runs in fp32 on the fp16-valued
        // flow and cat(feat, warped) promotes to fp32, so the fusion tensor exists twice: fp32 (fuF: what the fp32
        // deform_conv2d reads and writes, never rounded between blocks) and its fp16 rounding (fu: what the fp16
        // offset_conv / reconstruction.0 read).
        float *xF = f.fuF0, *yF = f.fuF1;
        // (round 5: the warp writes the fp32 values AND their fp16 rounding - was the conversion pass fusion_round_warped)
        if (P.x3) {
            EMAVFI_STEP(rec, "warp_fused<f32>", 24.0 * px, px * (8.0 + 8.0 * C), launch_warp_fused(frame2, flow, xF, B, C, H, W, P.fpad, mid, EMAVFI_F32, s));
            EMAVFI_STEP(rec, "fusion_split_warped", 0, px * (P.fpad - mid) * 8.0, launch_convert_cl(xF, f.fu0, npx, P.fpad, 2 * P.fps, mid, P.fpad - mid, 0, s, P.fps));
            // (`feat`'s fp32 copy is already in xF: the last feature layer wrote it beside its f16 halves; nb == 0 has no such layer)
            if (P.nb == 0) EMAVFI_STEP(rec, "fusion_widen_feat", 0, px * mid * 8.0, launch_convert_cl(f.fu0, xF, npx, 2 * P.fps, P.fpad, 0, mid, 1, s, P.fps));
        } else {
            EMAVFI_STEP(rec, "warp_fused<f32>", 24.0 * px, px * (8.0 + 8.0 * C + 2.0 * C),
                        launch_warp_fused(frame2, flow, xF, B, C, H, W, P.fpad, mid, EMAVFI_F32, s, f.fu0, P.fps));
            EMAVFI_STEP(rec, "fusion_widen_feat", 0, px * mid * 6.0, launch_convert_cl(f.fu0, xF, npx, P.fps, P.fpad, 0, mid, 1, s));
        }
        if (!rec.dry && taps && taps[3])
            EMAVFI_TRY(launch_cl_to_nchw(xF, taps[3], B, C, H, W, P.fpad, mid, EMAVFI_F32, s), "tap warped");
        EMAVFI_STAGE_EVENT(rec, 0);
        for (int i = 0; i < P.nb; ++i) {
            if (const int rc = attention_block_amp(P, i, packed, x, xF, yF, true, y, f.om, B, H, W, s, rec); rc != EMAVFI_OK) return rc;
            if (!rec.dry && taps && taps[5 + i])
                EMAVFI_TRY(launch_cl_to_nchw(yF, taps[5 + i], B, mid + 3, H, W, P.fpad, 0, EMAVFI_F32, s), "tap fused");
            void *t = x; x = y; y = t;
            float *tf = xF; xF = yF; yF = tf;
        }
    } else {
        // --- warp frame2 by the flow into channels [mid, fpad) of the fusion buffer (ema_vfi.py:130,134).
        // When the first pack runs as the one-launch LDS kernel, those 16 channels go to a compact buffer of their own
        // (kTailPs = 4 channels = 8 bytes per pixel, in the packed-input buffer, free since conv1) and the kernel's window DMA picks
        // them up from there: contiguous 16-byte pixels instead of 6 useful bytes scattered into every 160-byte fusion pixel.
        const bool split_tail = P.nb > 0 && pack_fuses(P, 0) && P.fpad - mid == 16;
        EMAVFI_STEP(rec, std::string("warp_fused<") + dtype_name(dtype) + ">", 24.0 * px, px * (8.0 + 4.0 * C + C * e),
                    split_tail ? launch_warp_fused(frame2, flow, f.in16, B, C, H, W, kTailPs, 0, feat_dtype, s)
                               : launch_warp_fused(frame2, flow, f.fu0, B, C, H, W, P.fps, mid, feat_dtype, s));
        if (!rec.dry && taps && taps[3])
            EMAVFI_TRY(split_tail ? launch_cl_to_nchw(f.in16, taps[3], B, C, H, W, kTailPs, 0, feat_dtype, s)
                                  : launch_cl_to_nchw(f.fu0, taps[3], B, C, H, W, P.fps, mid, feat_dtype, s), "tap warped");
        EMAVFI_STAGE_EVENT(rec, 0);

        // --- multi-attention fusion: num_blocks x ModulatedDeformConvPack, no activation (ema_vfi.py:136-138)
        for (int i = 0; i < P.nb; ++i) {
            const PackRoute route = adaptive ? PackRoute{kRouteAdaptive, routes.state ? routes.state + 8 + i : nullptr}
                                             : PackRoute{((gather_mask >> i) & 1u) ? EMAVFI_ROUTE_GATHER : EMAVFI_ROUTE_WINDOW};
            if (const int rc = attention_block(P, i, packed, x, y, f.om, i == 0 && split_tail ? f.in16 : nullptr,
                                               (i == 0 ? feat16 : pack_f16_link(P, i - 1)) ? 1 : 0, pack_f16_link(P, i) ? 1 : 0, B, H, W, s, rec,
                                               rec.dry ? nullptr : f.census + (size_t)i * DEFORM_CENSUS_SLOTS * 4, route);
                rc != EMAVFI_OK)
                return rc;
            if (!rec.dry && taps && taps[5 + i])
                EMAVFI_TRY(launch_cl_to_nchw(y, taps[5 + i], B, mid + 3, H, W, P.fps, 0, pack_f16_link(P, i) ? (int)EMAVFI_F16 : dtype, s), "tap fused");
            void *t = x; x = y; y = t;
        }
        if (adaptive) {
            // the next forward's routes from this one's census (read here, before anything reuses those bytes)
            unsigned long long totals[kMaxBlocks] = {};
            for (int i = 0; i < P.nb; ++i) totals[i] = pack3_wave_taps(B, H, W);
            EMAVFI_STEP(rec, "route_select", 0.0, (double)P.nb * kCensusBlock + 128.0,
                        launch_route_select(f.census, routes.state, P.nb, totals, routes.enter, routes.leave, EMAVFI_ROUTE_MAGIC, s));
        }
    }

    EMAVFI_STAGE_EVENT(rec, 1);
    // --- reconstruction (ema_vfi.py:144-146)
    if (const int rc = reconstruction_stage(P, packed, x, f, out, B, H, W, s, rec); rc != EMAVFI_OK) return rc;
    EMAVFI_STEP(rec, "blob_guard", 0, 64.0, launch_blob_guard(guard, out, npx * (size_t)C, s));
    EMAVFI_STAGE_EVENT(rec, 2);
    return EMAVFI_OK;
}

}  // namespace

unsigned emavfi_switches()
{
    init_switches();
    return g_switches.load(std::memory_order_relaxed);
}

extern "C" {

#if defined(EMAVFI_DEFORM_STAMPS) && EMAVFI_DEFORM_STAMPS
// rows of {prologue, offset_conv, geometry, steps, epilogue, total, valid, start time} per sampled wave
int emavfi_debug_deform_stamps(unsigned long long *out, int rows, int reset)
{
    unsigned long long *buf = debug_stamp_buffer();
    if (!buf || rows > DEFORM_STAMP_ROWS) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (out && hipMemcpy(out, buf, (size_t)rows * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -3;
    if (reset && hipMemset(buf, 0, (size_t)DEFORM_STAMP_ROWS * 8 * sizeof(unsigned long long)) != hipSuccess) return -4;
    return 0;
}
#endif

int emavfi_version(void) { return EMAVFI_VERSION; }
const char *emavfi_last_error(void) { return g_err; }
int emavfi_param_count(int num_blocks) { return 2 * (11 + 3 * num_blocks); }

int emavfi_supported(int in_channels, int mid_channels, int num_blocks, int dtype)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s", P.why);
    return EMAVFI_OK;
}

size_t emavfi_packed_bytes(int in_channels, int mid_channels, int num_blocks, int dtype)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) { fail(EMAVFI_E_UNSUPPORTED, "%s", P.why); return 0; }
    return P.total;
}

int emavfi_pack_weights(int in_channels, int mid_channels, int num_blocks, const void *const *params, int n_params,
                        void *packed, size_t packed_bytes, int dtype, void *stream)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s", P.why);
    if (!params || !packed) return fail(EMAVFI_E_ARG, "pack_weights: null pointer");
    if (n_params != emavfi_param_count(num_blocks))
        return fail(EMAVFI_E_ARG, "pack_weights: expected %d tensors, got %d", emavfi_param_count(num_blocks), n_params);
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return fail(EMAVFI_E_ARG, "pack_weights: params[%d] is null", i);
    if (packed_bytes < P.total) return fail(EMAVFI_E_WORKSPACE, "pack_weights: need %zu bytes, got %zu", P.total, packed_bytes);
    if (!aligned16(packed)) return fail(EMAVFI_E_ARG, "pack_weights: packed buffer must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const BlobHeader hdr = expected_header(P, dtype);
    dtype = P.dtype;            // kernel storage type (EMAVFI_AMP16 -> EMAVFI_F16)
    const bool b16 = P.amp;     // autocast casts a convolution's bias to fp16 as well (EMAVFI_F32X3 keeps every bias in fp32)
    // (the gaps between the 256-byte aligned layers are part of the checksummed payload: zero, not whatever the buffer held)
    EMAVFI_TRY(launch_clear_bytes(packed, P.total, s), "pack: blob clear");
    EMAVFI_TRY(pack_layer(P.conv1, params, packed, dtype, s, b16), "pack conv1");
    for (int i = 0; i < P.nb; ++i) EMAVFI_TRY(pack_layer(P.blk[i], params, packed, dtype, s, b16), "pack feat block");
    EMAVFI_TRY(pack_layer(P.c0, params, packed, dtype, s, b16), "pack ctx0");
    EMAVFI_TRY(pack_layer(P.c1, params, packed, dtype, s, b16), "pack ctx1");
    EMAVFI_TRY(pack_layer(P.c2, params, packed, dtype, s, b16), "pack ctx2");
    EMAVFI_TRY(pack_layer(P.m0, params, packed, dtype, s, b16), "pack motion0");
    EMAVFI_TRY(pack_layer(P.m1, params, packed, dtype, s, b16), "pack motion1");
    EMAVFI_TRY(pack_layer(P.m2, params, packed, dtype, s, b16), "pack motion2");
    for (int i = 0; i < P.nb; ++i) {
        EMAVFI_TRY(pack_layer(P.off[i], params, packed, dtype, s, b16), "pack offset_conv");
        if (P.has_offh) EMAVFI_TRY(pack_layer(P.offh[i], params, packed, dtype, s), "pack offset_conv (f16 fragments)");
        EMAVFI_TRY(pack_layer(P.dcn[i], params, packed, dtype, s), "pack dcn_v2");
        if (P.wide()) EMAVFI_TRY(pack_layer(P.dcn32[i], params, packed, dtype, s), "pack dcn_v2 (fp32 master weights)");
    }
    EMAVFI_TRY(pack_layer(P.r0, params, packed, dtype, s, b16), "pack recon0");
    EMAVFI_TRY(pack_layer(P.r1, params, packed, dtype, s, b16), "pack recon1");
    EMAVFI_TRY(pack_layer(P.r2, params, packed, dtype, s, b16), "pack recon2");
    EMAVFI_TRY(launch_pack_ctx((const float *)params[P.lin_param], (const float *)params[P.lin_param + 1],
                               (const float *)params[P.m0.param], (const float *)params[P.m0.param + 1],
                               (float *)((char *)packed + P.ctx_off), P.mid, P.amp ? 1 : 0, s),
               "pack context");
    EMAVFI_TRY(launch_blob_seal(packed, hdr, s), "pack: blob header");
    return EMAVFI_OK;
}

int emavfi_layout_tag(void) { return (int)layout_tag_of(process_layout_env()); }

int emavfi_debug_switches(int and_mask, int or_mask)
{
    init_switches();
    unsigned old = g_switches.load(std::memory_order_relaxed), want;
    do want = (old & (unsigned)and_mask) | (unsigned)or_mask;
    while (!g_switches.compare_exchange_weak(old, want, std::memory_order_relaxed));
    return (int)old;
}

int emavfi_packed_check(int in_channels, int mid_channels, int num_blocks, int dtype, const void *packed, size_t packed_bytes)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s", P.why);
    if (!packed) return fail(EMAVFI_E_ARG, "packed_check: null pointer");
    if (packed_bytes < P.total) return fail(EMAVFI_E_ARG, "packed_check: blob has %zu bytes, this model / dtype needs %zu", packed_bytes, P.total);
    // device memory is copied to the host (this entry synchronises: it is for the moment a blob arrives - from a file, another rank,
    // another process -, not for the per-frame path); anything HIP does not know as device memory is read in place
    std::vector<unsigned char> host;
    const unsigned char *bytes = (const unsigned char *)packed;
    hipPointerAttribute_t attr{};
    const bool on_device = hipPointerGetAttributes(&attr, packed) == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
    (void)hipGetLastError();   // (a plain host pointer makes hipPointerGetAttributes fail: not an error of this call)
    if (on_device) {
        // The blob's producer (the pack kernels on the caller's stream, an RCCL broadcast, a cache upload) may have run on ANY stream of
        // the blob's device - also a non-blocking one, which the legacy null stream of a plain hipMemcpy does not wait for - and that
        // device need not be the current one.  So: make the blob's device current, wait for ALL of its streams, then copy.
        int cur_dev = 0;
        if (hipGetDevice(&cur_dev) != hipSuccess) return fail(EMAVFI_E_LAUNCH, "packed_check: hipGetDevice failed");
        const bool other = attr.device != cur_dev;
        if (other && hipSetDevice(attr.device) != hipSuccess) return fail(EMAVFI_E_LAUNCH, "packed_check: cannot select the blob's device %d", attr.device);
        host.resize(P.total);
        const bool ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(host.data(), packed, P.total, hipMemcpyDeviceToHost) == hipSuccess;
        if (other) (void)hipSetDevice(cur_dev);
        if (!ok) { (void)hipGetLastError(); return fail(EMAVFI_E_LAUNCH, "packed_check: device synchronise / device-to-host copy failed"); }
        bytes = host.data();
    }
    BlobHeader got;
    memcpy(&got, bytes, sizeof got);
    const BlobHeader want = expected_header(P, dtype);
    if (memcmp(got.magic, want.magic, 8) != 0) return fail(EMAVFI_E_ARG, "packed_check: no EMAVFIPK header (a blob of a library older than 0.4.0, or not a blob)");
    if (got.version != want.version) return fail(EMAVFI_E_ARG, "packed_check: blob packed by library version %u, this is %u: re-pack", got.version, want.version);
    if (got.in_ch != want.in_ch || got.mid != want.mid || got.nb != want.nb)
        return fail(EMAVFI_E_ARG, "packed_check: blob is for EMA_VFI(%u, %u, %u), not (%d, %d, %d)", got.in_ch, got.mid, got.nb, in_channels, mid_channels, num_blocks);
    if (got.dtype != want.dtype) return fail(EMAVFI_E_ARG, "packed_check: blob was packed for dtype %u, asked for %d", got.dtype, dtype);
    if (got.layout_tag != want.layout_tag)
        return fail(EMAVFI_E_ARG, "packed_check: blob was packed under layout switches 0x%x, this process runs 0x%x (EMAVFI_CONV_MFMA16 / _RING / _WREG / _S2RING / EMAVFI_PACK_F16_CHAIN / EMAVFI_NO_FUSED_OFFSET)",
                    got.layout_tag, want.layout_tag);
    if (got.header_bytes != want.header_bytes || got.total_bytes != want.total_bytes)
        return fail(EMAVFI_E_ARG, "packed_check: blob size fields (%u, %llu) do not match this build's layout (%u, %llu)", got.header_bytes,
                    (unsigned long long)got.total_bytes, want.header_bytes, (unsigned long long)want.total_bytes);
    const uint64_t sum = blob_checksum_host(bytes + kBlobHeaderBytes, P.total - kBlobHeaderBytes);
    if (sum != got.checksum) return fail(EMAVFI_E_ARG, "packed_check: payload checksum %016llx, header says %016llx (corrupted blob)", (unsigned long long)sum, (unsigned long long)got.checksum);
    return EMAVFI_OK;
}

size_t emavfi_workspace_bytes(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) { fail(EMAVFI_E_UNSUPPORTED, "%s", P.why); return 0; }
    if (B < 1 || H < 1 || W < 1) { fail(EMAVFI_E_ARG, "workspace_bytes: B, H, W must be >= 1"); return 0; }
    Workspace ws{nullptr, 0, 0};
    FwdBuffers f;
    carve_forward(P, ws, f, B, H, W);
    return ws.used;
}

int emavfi_forward(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                   const float *frame2, float *out, void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype,
                   float *const *taps, void *stream)
{
    Recorder rec;
    return forward_impl(in_channels, mid_channels, num_blocks, packed, packed_bytes, frame1, frame2, out, workspace, workspace_bytes, B, H, W,
                        dtype, taps, stream, rec);
}

int emavfi_forward_routed(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                          const float *frame2, float *out, void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype,
                          float *const *taps, void *const *stage_events, void *const *events, int n_events, unsigned gather_blocks, void *stream)
{
    Recorder rec;
    rec.stage_events = stage_events;
    if (const int rc = set_events(rec, events, n_events, "forward_routed"); rc != EMAVFI_OK) return rc;
    Routes routes;
    routes.gather_mask = gather_blocks;
    return forward_impl(in_channels, mid_channels, num_blocks, packed, packed_bytes, frame1, frame2, out, workspace, workspace_bytes, B, H, W,
                        dtype, taps, stream, rec, routes);
}

int emavfi_forward_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                            char *names, size_t names_bytes, double *flops, double *bytes, int capacity)
{
    return emavfi_forward_launches_routed(in_channels, mid_channels, num_blocks, B, H, W, dtype, 0u, names, names_bytes, flops, bytes, capacity);
}

static int list_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, const Routes &routes,
                         char *names, size_t names_bytes, double *flops, double *bytes, int capacity, const FlowPlan &flowp = FlowPlan{})
{
    std::vector<LaunchRec> recs;
    Recorder rec;
    rec.recs = &recs; rec.dry = true;
    const int rc = forward_impl(in_channels, mid_channels, num_blocks, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, B, H, W,
                                dtype, nullptr, nullptr, rec, routes, flowp);
    if (rc != EMAVFI_OK) return rc;
    const int n = (int)recs.size();
    if (capacity <= 0) return n;
    if (capacity < n) return fail(EMAVFI_E_ARG, "forward_launches: capacity %d < %d launches", capacity, n);
    size_t used = 0;
    for (int i = 0; i < n; ++i) {
        if (flops) flops[i] = recs[i].flops;
        if (bytes) bytes[i] = recs[i].bytes;
        if (names) {
            if (used + recs[i].name.size() + 2 > names_bytes) return fail(EMAVFI_E_ARG, "forward_launches: names buffer too small");
            memcpy(names + used, recs[i].name.c_str(), recs[i].name.size());
            used += recs[i].name.size();
            names[used++] = '\n';
            names[used] = 0;
        }
    }
    return n;
}

int emavfi_forward_launches_routed(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, unsigned gather_blocks,
                                   char *names, size_t names_bytes, double *flops, double *bytes, int capacity)
{
    Routes routes;
    routes.gather_mask = gather_blocks;
    return list_launches(in_channels, mid_channels, num_blocks, B, H, W, dtype, routes, names, names_bytes, flops, bytes, capacity);
}

int emavfi_forward_launches_adaptive(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                                     char *names, size_t names_bytes, double *flops, double *bytes, int capacity)
{
    Routes routes;
    routes.adaptive = true;
    return list_launches(in_channels, mid_channels, num_blocks, B, H, W, dtype, routes, names, names_bytes, flops, bytes, capacity);
}

// ---- coarse flow (include/emavfi.h, "COARSE FLOW DEFINITION"): the two halves of the forward, split at the flow
int emavfi_forward_flow(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                        const float *frame2, float *flow_out, void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype, void *stream)
{
    Recorder rec;
    FlowPlan flowp;
    flowp.kind = FlowPlan::STOP; flowp.out = flow_out;
    return forward_impl(in_channels, mid_channels, num_blocks, packed, packed_bytes, frame1, frame2, nullptr, workspace, workspace_bytes, B, H, W,
                        dtype, nullptr, stream, rec, Routes{}, flowp);
}

int emavfi_forward_given_flow(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                              const float *frame2, const float *flow, float *out, void *workspace, size_t workspace_bytes, int B, int H, int W,
                              int dtype, float *const *taps, void *const *stage_events, void *const *events, int n_events, unsigned gather_blocks,
                              void *stream)
{
    Recorder rec;
    rec.stage_events = stage_events;
    if (const int rc = set_events(rec, events, n_events, "forward_given_flow"); rc != EMAVFI_OK) return rc;
    Routes routes;
    routes.gather_mask = gather_blocks;
    FlowPlan flowp;
    flowp.kind = FlowPlan::GIVEN; flowp.given = flow;
    return forward_impl(in_channels, mid_channels, num_blocks, packed, packed_bytes, frame1, frame2, out, workspace, workspace_bytes, B, H, W,
                        dtype, taps, stream, rec, routes, flowp);
}

int emavfi_forward_flow_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype,
                                 char *names, size_t names_bytes, double *flops, double *bytes, int capacity)
{
    FlowPlan flowp;
    flowp.kind = FlowPlan::STOP;
    return list_launches(in_channels, mid_channels, num_blocks, B, H, W, dtype, Routes{}, names, names_bytes, flops, bytes, capacity, flowp);
}

int emavfi_forward_given_flow_launches(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, unsigned gather_blocks,
                                       char *names, size_t names_bytes, double *flops, double *bytes, int capacity)
{
    Routes routes;
    routes.gather_mask = gather_blocks;
    FlowPlan flowp;
    flowp.kind = FlowPlan::GIVEN;
    return list_launches(in_channels, mid_channels, num_blocks, B, H, W, dtype, routes, names, names_bytes, flops, bytes, capacity, flowp);
}

// ---- adaptive per-block route (include/emavfi.h): the states emavfi_route_state_init wrote, by address -> num_blocks.  The forward
// checks a state here instead of reading its magic back (that would be a host sync in every forward).
static std::mutex g_route_states_mu;
static std::unordered_map<const void *, int> g_route_states;
constexpr size_t kRouteStateBytes = 32 * sizeof(unsigned);

size_t emavfi_route_state_bytes(void) { return kRouteStateBytes; }

int emavfi_route_state_init(void *route_state, int num_blocks, unsigned start_gather_mask, void *stream)
{
    if (!route_state) return fail(EMAVFI_E_ARG, "route_state_init: null state");
    if (!aligned16(route_state)) return fail(EMAVFI_E_ARG, "route_state_init: the state must be 16-byte aligned");
    if (num_blocks < 1 || num_blocks > kMaxBlocks) return fail(EMAVFI_E_ARG, "route_state_init: num_blocks must be 1..%d (got %d)", kMaxBlocks, num_blocks);
    if ((start_gather_mask >> num_blocks) != 0u)
        return fail(EMAVFI_E_ARG, "route_state_init: start_gather_mask 0x%x names blocks at or above num_blocks = %d", start_gather_mask, num_blocks);
    EMAVFI_TRY(launch_route_state_init(route_state, EMAVFI_ROUTE_MAGIC, num_blocks, start_gather_mask, (hipStream_t)stream), "route_state_init");
    std::lock_guard<std::mutex> lk(g_route_states_mu);
    g_route_states[route_state] = num_blocks;
    return EMAVFI_OK;
}

int emavfi_forward_adaptive(int in_channels, int mid_channels, int num_blocks, const void *packed, size_t packed_bytes, const float *frame1,
                            const float *frame2, float *out, void *workspace, size_t workspace_bytes, int B, int H, int W, int dtype,
                            float *const *taps, void *const *stage_events, void *const *events, int n_events, void *route_state,
                            float enter_share, float leave_share, void *stream)
{
    if (!(leave_share >= 0.0f && leave_share < enter_share && enter_share <= 1.0f))
        return fail(EMAVFI_E_ARG, "forward_adaptive: thresholds need 0 <= leave_share < enter_share <= 1 (got enter %g, leave %g)", (double)enter_share,
                    (double)leave_share);
    if (!route_state) return fail(EMAVFI_E_ARG, "forward_adaptive: null route state");
    {
        std::lock_guard<std::mutex> lk(g_route_states_mu);
        const auto it = g_route_states.find(route_state);
        if (it == g_route_states.end())
            return fail(EMAVFI_E_ARG, "forward_adaptive: bad route state magic (not written by emavfi_route_state_init)");
        if (it->second != num_blocks)
            return fail(EMAVFI_E_ARG, "forward_adaptive: the route state was written for num_blocks = %d, the model has %d", it->second, num_blocks);
    }
    Recorder rec;
    rec.stage_events = stage_events;
    if (const int rc = set_events(rec, events, n_events, "forward_adaptive"); rc != EMAVFI_OK) return rc;
    Routes routes;
    routes.adaptive = true; routes.state = (unsigned *)route_state; routes.enter = enter_share; routes.leave = leave_share;
    return forward_impl(in_channels, mid_channels, num_blocks, packed, packed_bytes, frame1, frame2, out, workspace, workspace_bytes, B, H, W,
                        dtype, taps, stream, rec, routes);
}

int emavfi_warp(const float *frame2, const float *flow, float *out, int B, int C, int H, int W, void *stream)
{
    if (!frame2 || !flow || !out) return fail(EMAVFI_E_ARG, "warp: null pointer");
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "warp: B, C, H, W must be >= 1");
    if ((size_t)H * W >= ((size_t)1 << 31)) return fail(EMAVFI_E_ARG, "warp: H*W must be < 2^31 (32-bit pixel offsets inside a plane)");
    if (!aligned16(frame2) || !aligned16(flow) || !aligned16(out)) return fail(EMAVFI_E_ARG, "warp: pointers must be 16-byte aligned");
    EMAVFI_TRY(launch_warp_nchw(frame2, flow, out, B, C, H, W, (hipStream_t)stream), "warp");
    return EMAVFI_OK;
}

int emavfi_preprocess_u8(const unsigned char *frames_hwc, float *out_nchw, int B, int H, int W, int C, const float *mean,
                         const float *std, void *stream)
{
    if (!frames_hwc || !out_nchw || !mean || !std) return fail(EMAVFI_E_ARG, "preprocess_u8: null pointer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || C > 4) return fail(EMAVFI_E_ARG, "preprocess_u8: bad shape (C must be 1..4)");
    for (int c = 0; c < C; ++c)
        if (!(std[c] != 0.0f)) return fail(EMAVFI_E_ARG, "preprocess_u8: std[%d] must be non-zero", c);
    EMAVFI_TRY(launch_preprocess_u8(frames_hwc, out_nchw, B, H, W, C, mean, std, (hipStream_t)stream), "preprocess_u8");
    return EMAVFI_OK;
}

int emavfi_postprocess_u8(const float *frames_nchw, unsigned char *out_hwc, int B, int H, int W, int C, const double *mean,
                          const double *std, int denormalize, void *stream)
{
    if (!frames_nchw || !out_hwc || !mean || !std) return fail(EMAVFI_E_ARG, "postprocess_u8: null pointer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || C > 4) return fail(EMAVFI_E_ARG, "postprocess_u8: bad shape (C must be 1..4)");
    EMAVFI_TRY(launch_postprocess_u8(frames_nchw, out_hwc, B, H, W, C, mean, std, denormalize ? 1 : 0, (hipStream_t)stream),
               "postprocess_u8");
    return EMAVFI_OK;
}

// ---- 4:2:0 frames (include/emavfi.h, "NV12", "HIGH BIT DEPTH", "PLANAR 4:2:0"): one check for the six entries.  An entry names its planes and
// its format's rules in a table; yuv420_check walks it in an order that lets a caller without a device reach every refusal.
struct Yuv420PlaneRule {
    const char *name;
    size_t row, rows;               // bytes of a row, rows of the plane
    size_t ptr_align, step_align;   // what the pointer / the pitch and (B > 1) the batch stride must be a multiple of; 1: anything
};
struct Yuv420Table {
    Yuv420Frame fr;                 // the planes, as the launcher takes them
    int nplanes;
    Yuv420PlaneRule rule[3];
    const char *depths;             // null: fr.depth is one of the format's; else the list of those, for the message
    int last_standard;              // EMAVFI_YUV_BT601_LIMITED .. last_standard
    const char *last_standard_name;
};
static size_t half_up(int n) { return ((size_t)n + 1) / 2; }
// NV12: bytes; both pointers 2-byte aligned, any pitch; the four 8-bit standards
static Yuv420Table nv12_table(const void *y, size_t y_pitch, size_t y_bstride, const void *uv, size_t uv_pitch, size_t uv_bstride, int H, int W)
{
    return {{{(void *)y, (void *)uv, nullptr}, {{y_pitch, uv_pitch, 0}, {y_bstride, uv_bstride, 0}}, YUV420_SEMIPLANAR, 8}, 2,
            {{"y", (size_t)W, (size_t)H, 2, 1}, {"uv", 2 * half_up(W), half_up(H), 2, 1}, {}},
            nullptr, EMAVFI_YUV_BT709_FULL, "EMAVFI_YUV_BT709_FULL"};
}
// P010 / P012 / P016: words; the Y plane keeps word alignment, the UV plane pair (4-byte) alignment; all six standards
static Yuv420Table p010_table(const void *y, size_t y_pitch, size_t y_bstride, const void *uv, size_t uv_pitch, size_t uv_bstride, int H, int W, int depth)
{
    return {{{(void *)y, (void *)uv, nullptr}, {{y_pitch, uv_pitch, 0}, {y_bstride, uv_bstride, 0}}, YUV420_SEMIPLANAR, depth}, 2,
            {{"y", 2 * (size_t)W, (size_t)H, 2, 2}, {"uv", 4 * half_up(W), half_up(H), 4, 4}, {}},
            depth == 10 || depth == 12 || depth == 16 ? nullptr : "10, 12 or 16 (P010, P012, P016)", EMAVFI_YUV_BT2020_FULL, "EMAVFI_YUV_BT2020_FULL"};
}
// planar: bytes with no alignment rule and the 8-bit standards, or words that keep word alignment and all six standards
static Yuv420Table yuv420p_table(const void *y, size_t y_pitch, size_t y_bstride, const void *u, size_t u_pitch, size_t u_bstride, const void *v,
                                 size_t v_pitch, size_t v_bstride, int H, int W, int depth)
{
    const size_t es = depth == 8 ? 1 : 2;   // bytes per sample
    return {{{(void *)y, (void *)u, (void *)v}, {{y_pitch, u_pitch, v_pitch}, {y_bstride, u_bstride, v_bstride}}, YUV420_PLANAR, depth}, 3,
            {{"y", es * (size_t)W, (size_t)H, es, es}, {"u", es * half_up(W), half_up(H), es, es}, {"v", es * half_up(W), half_up(H), es, es}},
            depth == 8 || depth == 10 || depth == 12 || depth == 16 ? nullptr : "8, 10, 12 or 16",
            depth == 8 ? EMAVFI_YUV_BT709_FULL : EMAVFI_YUV_BT2020_FULL, depth == 8 ? "EMAVFI_YUV_BT709_FULL" : "EMAVFI_YUV_BT2020_FULL"};
}
// mean / std come as float (preprocess) or as double (postprocess); sizes are compared in 128 bits
static int yuv420_check(const char *what, const Yuv420Table &t, const void *f32, int B, int H, int W, int standard, int order, const float *mean32,
                        const float *std32, const double *mean64, const double *std64)
{
    typedef unsigned __int128 u128;
    const Yuv420Strides &st = t.fr.strides;
    if (!(mean32 && std32) && !(mean64 && std64)) return fail(EMAVFI_E_ARG, "%s: null mean / std", what);
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "%s: B, H, W must be >= 1", what);
    if (t.depths) return fail(EMAVFI_E_ARG, "%s: depth %d is not %s", what, t.fr.depth, t.depths);
    if (standard < EMAVFI_YUV_BT601_LIMITED || standard > t.last_standard)
        return fail(EMAVFI_E_ARG, "%s: unknown standard %d at depth %d (EMAVFI_YUV_BT601_LIMITED .. %s)", what, standard, t.fr.depth, t.last_standard_name);
    if (order != EMAVFI_ORDER_BGR && order != EMAVFI_ORDER_RGB)
        return fail(EMAVFI_E_ARG, "%s: unknown order %d (EMAVFI_ORDER_BGR or EMAVFI_ORDER_RGB)", what, order);
    for (int p = 0; p < t.nplanes; ++p) {
        const Yuv420PlaneRule &r = t.rule[p];
        if (st.pitch[p] < r.row) return fail(EMAVFI_E_ARG, "%s: %s_pitch %zu is smaller than its row of %zu bytes", what, r.name, st.pitch[p], r.row);
        if (st.pitch[p] % r.step_align) return fail(EMAVFI_E_ARG, "%s: %s_pitch %zu must be a multiple of %zu", what, r.name, st.pitch[p], r.step_align);
    }
    for (int p = 0; p < t.nplanes && B > 1; ++p) {
        const Yuv420PlaneRule &r = t.rule[p];
        if ((u128)st.bstride[p] < (u128)(r.rows - 1) * st.pitch[p] + r.row)
            return fail(EMAVFI_E_ARG, "%s: the %s batch stride %zu is smaller than its plane", what, r.name, st.bstride[p]);
        if (st.bstride[p] % r.step_align)
            return fail(EMAVFI_E_ARG, "%s: the %s batch stride %zu must be a multiple of %zu (it breaks the alignment of its plane)", what, r.name,
                        st.bstride[p], r.step_align);
    }
    for (int c = 0; c < 3; ++c)
        if (std32 ? !(std32[c] != 0.0f) : !(std64[c] != 0.0)) return fail(EMAVFI_E_ARG, "%s: std[%d] must be non-zero", what, c);
    for (int p = 0; p < t.nplanes; ++p)
        if (!t.fr.plane[p]) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if (!f32) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    for (int p = 0; p < t.nplanes; ++p)
        if ((uintptr_t)t.fr.plane[p] % t.rule[p].ptr_align)
            return fail(EMAVFI_E_ARG, "%s: the %s pointer must be %zu-byte aligned", what, t.rule[p].name, t.rule[p].ptr_align);
    if ((uintptr_t)f32 & 3) return fail(EMAVFI_E_ARG, "%s: the fp32 pointer must be 4-byte aligned", what);
    return EMAVFI_OK;
}
static int preprocess_yuv420(const char *what, const Yuv420Table &t, float *out_nchw, int B, int H, int W, int standard, int order, const float *mean,
                             const float *std, void *stream)
{
    if (const int rc = yuv420_check(what, t, out_nchw, B, H, W, standard, order, mean, std, nullptr, nullptr); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_preprocess_yuv420(t.fr, out_nchw, B, H, W, standard, order, mean, std, (hipStream_t)stream), what);
    return EMAVFI_OK;
}
static int postprocess_yuv420(const char *what, const float *frames_nchw, const Yuv420Table &t, int B, int H, int W, int standard, int order,
                              const double *mean, const double *std, int denormalize, void *stream)
{
    if (const int rc = yuv420_check(what, t, frames_nchw, B, H, W, standard, order, nullptr, nullptr, mean, std); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_postprocess_yuv420(frames_nchw, t.fr, B, H, W, standard, order, mean, std, denormalize ? 1 : 0, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_yuv_coefficients(int standard, int decode[5], int encode[9])
{
    if (standard < EMAVFI_YUV_BT601_LIMITED || standard > EMAVFI_YUV_BT709_FULL)
        return fail(EMAVFI_E_ARG, "yuv_coefficients: unknown standard %d (EMAVFI_YUV_BT601_LIMITED .. EMAVFI_YUV_BT709_FULL)", standard);
    if (!decode || !encode) return fail(EMAVFI_E_ARG, "yuv_coefficients: null pointer");
    yuv_coefficients(standard, decode, encode);
    return EMAVFI_OK;
}

int emavfi_yuv_coefficients_depth(int standard, int depth, int decode[5], int encode[9])
{
    if (standard < EMAVFI_YUV_BT601_LIMITED || standard > EMAVFI_YUV_BT2020_FULL)
        return fail(EMAVFI_E_ARG, "yuv_coefficients_depth: unknown standard %d (EMAVFI_YUV_BT601_LIMITED .. EMAVFI_YUV_BT2020_FULL)", standard);
    if (depth != 8 && depth != 10 && depth != 12 && depth != 16)
        return fail(EMAVFI_E_ARG, "yuv_coefficients_depth: depth %d is not 8, 10, 12 or 16", depth);
    if (!decode || !encode) return fail(EMAVFI_E_ARG, "yuv_coefficients_depth: null pointer");
    yuv_coefficients_depth(standard, depth, decode, encode);
    return EMAVFI_OK;
}

int emavfi_preprocess_nv12(const unsigned char *y, size_t y_pitch, size_t y_batch_stride, const unsigned char *uv, size_t uv_pitch,
                           size_t uv_batch_stride, float *out_nchw, int B, int H, int W, int standard, int order, const float *mean,
                           const float *std, void *stream)
{
    return preprocess_yuv420("preprocess_nv12", nv12_table(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, H, W), out_nchw, B, H, W,
                             standard, order, mean, std, stream);
}

int emavfi_postprocess_nv12(const float *frames_nchw, unsigned char *y, size_t y_pitch, size_t y_batch_stride, unsigned char *uv, size_t uv_pitch,
                            size_t uv_batch_stride, int B, int H, int W, int standard, int order, const double *mean, const double *std,
                            int denormalize, void *stream)
{
    return postprocess_yuv420("postprocess_nv12", frames_nchw, nv12_table(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, H, W), B, H, W,
                              standard, order, mean, std, denormalize, stream);
}

int emavfi_preprocess_p010(const void *y, size_t y_pitch, size_t y_batch_stride, const void *uv, size_t uv_pitch, size_t uv_batch_stride,
                           float *out_nchw, int B, int H, int W, int depth, int standard, int order, const float *mean, const float *std,
                           void *stream)
{
    return preprocess_yuv420("preprocess_p010", p010_table(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, H, W, depth), out_nchw, B, H,
                             W, standard, order, mean, std, stream);
}

int emavfi_postprocess_p010(const float *frames_nchw, void *y, size_t y_pitch, size_t y_batch_stride, void *uv, size_t uv_pitch,
                            size_t uv_batch_stride, int B, int H, int W, int depth, int standard, int order, const double *mean,
                            const double *std, int denormalize, void *stream)
{
    return postprocess_yuv420("postprocess_p010", frames_nchw, p010_table(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, H, W, depth), B,
                              H, W, standard, order, mean, std, denormalize, stream);
}

int emavfi_preprocess_yuv420p(const void *y, size_t y_pitch, size_t y_batch_stride, const void *u, size_t u_pitch, size_t u_batch_stride,
                              const void *v, size_t v_pitch, size_t v_batch_stride, float *out_nchw, int B, int H, int W, int depth,
                              int standard, int order, const float *mean, const float *std, void *stream)
{
    return preprocess_yuv420("preprocess_yuv420p",
                             yuv420p_table(y, y_pitch, y_batch_stride, u, u_pitch, u_batch_stride, v, v_pitch, v_batch_stride, H, W, depth), out_nchw,
                             B, H, W, standard, order, mean, std, stream);
}

int emavfi_postprocess_yuv420p(const float *frames_nchw, void *y, size_t y_pitch, size_t y_batch_stride, void *u, size_t u_pitch,
                               size_t u_batch_stride, void *v, size_t v_pitch, size_t v_batch_stride, int B, int H, int W, int depth,
                               int standard, int order, const double *mean, const double *std, int denormalize, void *stream)
{
    return postprocess_yuv420("postprocess_yuv420p", frames_nchw,
                              yuv420p_table(y, y_pitch, y_batch_stride, u, u_pitch, u_batch_stride, v, v_pitch, v_batch_stride, H, W, depth), B, H, W,
                              standard, order, mean, std, denormalize, stream);
}

// ---- frames resized on the device (include/emavfi.h, "RESIZE DEFINITION"): checks in an order that lets a caller without a device reach each
static int resize_dims_check(const char *what, int B, int Hs, int Ws, int Hd, int Wd)
{
    if (B < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return fail(EMAVFI_E_ARG, "%s: B, Hs, Ws, Hd, Wd must be >= 1", what);
    if (Hs > EMAVFI_RESIZE_MAX_DIM || Ws > EMAVFI_RESIZE_MAX_DIM || Hd > EMAVFI_RESIZE_MAX_DIM || Wd > EMAVFI_RESIZE_MAX_DIM)
        return fail(EMAVFI_E_ARG, "%s: a dimension (%d x %d -> %d x %d) is above 16384", what, Hs, Ws, Hd, Wd);
    if (B > 65535) return fail(EMAVFI_E_ARG, "%s: B = %d is above 65535", what, B);
    return EMAVFI_OK;
}
// one pitched byte plane of `rows` rows of `row` bytes
static int resize_plane_check(const char *what, const char *name, size_t pitch, size_t bstride, size_t rows, size_t row, int B)
{
    if (pitch < row) return fail(EMAVFI_E_ARG, "%s: %s_pitch %zu is smaller than its row of %zu bytes", what, name, pitch, row);
    if (B > 1 && bstride < (rows - 1) * pitch + row) return fail(EMAVFI_E_ARG, "%s: the %s batch stride %zu is smaller than its plane", what, name, bstride);
    return EMAVFI_OK;
}

int emavfi_resize_u8(const unsigned char *src, size_t src_pitch, size_t src_batch_stride, unsigned char *dst, size_t dst_pitch,
                     size_t dst_batch_stride, int B, int Hs, int Ws, int Hd, int Wd, int C, void *stream)
{
    if (const int rc = resize_dims_check("resize_u8", B, Hs, Ws, Hd, Wd); rc != EMAVFI_OK) return rc;
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "resize_u8: C = %d (C must be 1..4)", C);
    if (const int rc = resize_plane_check("resize_u8", "src", src_pitch, src_batch_stride, (size_t)Hs, (size_t)Ws * C, B); rc != EMAVFI_OK) return rc;
    if (const int rc = resize_plane_check("resize_u8", "dst", dst_pitch, dst_batch_stride, (size_t)Hd, (size_t)Wd * C, B); rc != EMAVFI_OK) return rc;
    if (!src || !dst) return fail(EMAVFI_E_ARG, "resize_u8: null pointer");
    EMAVFI_TRY(launch_resize_u8(src, src_pitch, src_batch_stride, dst, dst_pitch, dst_batch_stride, nullptr, B, Hs, Ws, Hd, Wd, C, nullptr, nullptr,
                                (hipStream_t)stream), "resize_u8");
    return EMAVFI_OK;
}

int emavfi_preprocess_u8_resized(const unsigned char *frames_hwc, float *out_nchw, unsigned char *resized_hwc, int B, int Hs, int Ws, int Hd,
                                 int Wd, int C, const float *mean, const float *std, void *stream)
{
    if (!mean || !std) return fail(EMAVFI_E_ARG, "preprocess_u8_resized: null mean / std");
    if (const int rc = resize_dims_check("preprocess_u8_resized", B, Hs, Ws, Hd, Wd); rc != EMAVFI_OK) return rc;
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "preprocess_u8_resized: C = %d (C must be 1..4)", C);
    for (int c = 0; c < C; ++c)
        if (!(std[c] != 0.0f)) return fail(EMAVFI_E_ARG, "preprocess_u8_resized: std[%d] must be non-zero", c);
    if (!frames_hwc || !out_nchw) return fail(EMAVFI_E_ARG, "preprocess_u8_resized: null pointer");
    if ((uintptr_t)out_nchw & 3) return fail(EMAVFI_E_ARG, "preprocess_u8_resized: the fp32 pointer must be 4-byte aligned");
    const size_t srow = (size_t)Ws * C, drow = (size_t)Wd * C;
    EMAVFI_TRY(launch_resize_u8(frames_hwc, srow, srow * Hs, resized_hwc, drow, drow * Hd, out_nchw, B, Hs, Ws, Hd, Wd, C, mean, std,
                                (hipStream_t)stream), "preprocess_u8_resized");
    return EMAVFI_OK;
}

int emavfi_preprocess_nv12_resized(const unsigned char *y, size_t y_pitch, size_t y_batch_stride, const unsigned char *uv, size_t uv_pitch,
                                   size_t uv_batch_stride, float *out_nchw, unsigned char *y_out, size_t y_out_pitch, size_t y_out_batch_stride,
                                   unsigned char *uv_out, size_t uv_out_pitch, size_t uv_out_batch_stride, int B, int Hs, int Ws, int Hd, int Wd,
                                   int standard, int order, const float *mean, const float *std, void *stream)
{
    const char *const what = "preprocess_nv12_resized";
    if (!mean || !std) return fail(EMAVFI_E_ARG, "%s: null mean / std", what);
    if (const int rc = resize_dims_check(what, B, Hs, Ws, Hd, Wd); rc != EMAVFI_OK) return rc;
    // the source planes: emavfi_preprocess_nv12's checks (standard, order, pitches, batch strides, std, null, alignment), under this entry's name
    if (const int rc = yuv420_check(what, nv12_table(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, Hs, Ws), out_nchw, B, Hs, Ws, standard,
                                    order, mean, std, nullptr, nullptr); rc != EMAVFI_OK) return rc;
    const size_t uv_row = 2 * (((size_t)Wd + 1) / 2), uv_rows = ((size_t)Hd + 1) / 2;
    if (y_out)
        if (const int rc = resize_plane_check(what, "y_out", y_out_pitch, y_out_batch_stride, (size_t)Hd, (size_t)Wd, B); rc != EMAVFI_OK) return rc;
    if (uv_out)
        if (const int rc = resize_plane_check(what, "uv_out", uv_out_pitch, uv_out_batch_stride, uv_rows, uv_row, B); rc != EMAVFI_OK) return rc;
    if (((uintptr_t)y_out | (uintptr_t)uv_out) & 1) return fail(EMAVFI_E_ARG, "%s: the y_out and uv_out pointers must be 2-byte aligned", what);
    EMAVFI_TRY(launch_preprocess_nv12_resized(y, y_pitch, y_batch_stride, uv, uv_pitch, uv_batch_stride, out_nchw, y_out, y_out_pitch,
                                              y_out_batch_stride, uv_out, uv_out_pitch, uv_out_batch_stride, B, Hs, Ws, Hd, Wd, standard, order, mean,
                                              std, (hipStream_t)stream), "preprocess_nv12_resized");
    return EMAVFI_OK;
}

// ---- scene cuts on the device (include/emavfi.h, "SCENE CUT DEFINITION"): every check runs on the host, pointers are looked at last
static int scene_dims_check(const char *what, int H, int W)
{
    if (H < 1 || W < 1) return fail(EMAVFI_E_ARG, "%s: H, W must be >= 1", what);
    if (H > EMAVFI_RESIZE_MAX_DIM || W > EMAVFI_RESIZE_MAX_DIM) return fail(EMAVFI_E_ARG, "%s: a dimension (%d x %d) is above 16384", what, H, W);
    return EMAVFI_OK;
}

int emavfi_luma_signature_u8(const unsigned char *src, size_t pitch, size_t batch_stride, int B, int H, int W, int C, int order, unsigned *sig,
                             void *stream)
{
    const char *const what = "luma_signature_u8";
    if (B < 1) return fail(EMAVFI_E_ARG, "%s: B must be >= 1", what);
    if (B > 65535) return fail(EMAVFI_E_ARG, "%s: B = %d is above 65535", what, B);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (C != 1 && C != 3) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1 or 3)", what, C);
    if (order != EMAVFI_ORDER_BGR && order != EMAVFI_ORDER_RGB)
        return fail(EMAVFI_E_ARG, "%s: unknown order %d (EMAVFI_ORDER_BGR or EMAVFI_ORDER_RGB)", what, order);
    const size_t row = (size_t)W * C;
    if (pitch < row) return fail(EMAVFI_E_ARG, "%s: pitch %zu is smaller than its row of %zu bytes", what, pitch, row);
    size_t plane, span;
    if (__builtin_mul_overflow((size_t)(H - 1), pitch, &plane) || __builtin_add_overflow(plane, row, &plane))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (pitch %zu)", what, pitch);
    if (B > 1 && batch_stride < plane) return fail(EMAVFI_E_ARG, "%s: the batch stride %zu is smaller than its plane", what, batch_stride);
    if (B > 1 && (__builtin_mul_overflow((size_t)(B - 1), batch_stride, &span) || __builtin_add_overflow(span, plane, &span)))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (batch stride %zu)", what, batch_stride);
    if (!src || !sig) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if ((uintptr_t)sig & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer must be 4-byte aligned", what);
    EMAVFI_TRY(launch_luma_signature_u8(src, pitch, batch_stride, B, H, W, C, order, sig, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_scene_flags(const unsigned *sig_a, size_t stride_a_words, const unsigned *sig_b, size_t stride_b_words, int n, int H, int W,
                       unsigned threshold, unsigned *flags, unsigned *scores, void *stream)
{
    const char *const what = "scene_flags";
    if (n < 1) return fail(EMAVFI_E_ARG, "%s: n must be >= 1", what);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    for (const size_t st : {stride_a_words, stride_b_words}) {
        size_t span;
        if (st != 0 && st < EMAVFI_SCENE_SIG_WORDS)
            return fail(EMAVFI_E_ARG, "%s: a signature stride of %zu words is neither 0 nor at least %d", what, st, EMAVFI_SCENE_SIG_WORDS);
        if (__builtin_mul_overflow((size_t)(n - 1), st, &span) || __builtin_add_overflow(span, (size_t)EMAVFI_SCENE_SIG_WORDS, &span) ||
            __builtin_mul_overflow(span, sizeof(unsigned), &span))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (stride %zu words)", what, st);
    }
    if (!sig_a || !sig_b || !flags) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if (((uintptr_t)sig_a | (uintptr_t)sig_b | (uintptr_t)flags | (uintptr_t)scores) & 3)
        return fail(EMAVFI_E_ARG, "%s: the u32 pointers must be 4-byte aligned", what);
    EMAVFI_TRY(launch_scene_flags(sig_a, stride_a_words, sig_b, stride_b_words, n, H, W, threshold, flags, scores, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_hold_frames_u8(unsigned char *dst, size_t dst_stride, int rep, const unsigned char *alt, size_t alt_stride, const unsigned *flags, int n,
                          size_t frame_bytes, void *stream)
{
    const char *const what = "hold_frames_u8";
    if (n < 1 || rep < 1) return fail(EMAVFI_E_ARG, "%s: n, rep must be >= 1", what);
    if (n > 65535 || rep > 65535) return fail(EMAVFI_E_ARG, "%s: n = %d, rep = %d: above 65535", what, n, rep);
    if (frame_bytes < 1) return fail(EMAVFI_E_ARG, "%s: frame_bytes must be >= 1", what);
    if (frame_bytes > ((size_t)1 << 40)) return fail(EMAVFI_E_ARG, "%s: frame_bytes %zu is above 2^40", what, frame_bytes);
    if ((size_t)n * rep > 1 && (dst_stride < frame_bytes || alt_stride < frame_bytes))
        return fail(EMAVFI_E_ARG, "%s: a stride (dst %zu, alt %zu) is smaller than frame_bytes %zu", what, dst_stride, alt_stride, frame_bytes);
    size_t span;
    if (__builtin_mul_overflow((size_t)n * rep - 1, dst_stride, &span) || __builtin_add_overflow(span, frame_bytes, &span) ||
        __builtin_mul_overflow((size_t)(n - 1), alt_stride, &span) || __builtin_add_overflow(span, frame_bytes, &span))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (strides dst %zu, alt %zu)", what, dst_stride, alt_stride);
    if (!dst || !alt || !flags) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if ((uintptr_t)flags & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer must be 4-byte aligned", what);
    EMAVFI_TRY(launch_hold_frames_u8(dst, dst_stride, rep, alt, alt_stride, flags, n, frame_bytes, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- duplicate frames (include/emavfi.h, "DUPLICATE FRAME DEFINITION"): every check runs on the host, pointers are looked at last
static_assert(DEDUP_CELLS == EMAVFI_SCENE_SIG_WORDS, "header and dedup_elem.h disagree");

int emavfi_frame_diff_cells(const unsigned char *a, size_t a_pitch, size_t a_batch_stride, const unsigned char *b, size_t b_pitch,
                            size_t b_batch_stride, int n, int H, int W, int C, int order, int sample_bytes, int depth, int shift,
                            unsigned *cells, void *stream)
{
    const char *const what = "frame_diff_cells";
    if (n < 1) return fail(EMAVFI_E_ARG, "%s: n must be >= 1", what);
    if (n > 65535) return fail(EMAVFI_E_ARG, "%s: n = %d is above 65535", what, n);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (C != 1 && C != 3) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1 or 3)", what, C);
    if (order != EMAVFI_ORDER_BGR && order != EMAVFI_ORDER_RGB)
        return fail(EMAVFI_E_ARG, "%s: unknown order %d (EMAVFI_ORDER_BGR or EMAVFI_ORDER_RGB)", what, order);
    if (sample_bytes != 1 && sample_bytes != 2) return fail(EMAVFI_E_ARG, "%s: sample_bytes = %d (sample_bytes must be 1 or 2)", what, sample_bytes);
    if (sample_bytes == 1 ? depth != 8 : (depth != 10 && depth != 12 && depth != 16))
        return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8 at sample_bytes 1 and 10, 12 or 16 at sample_bytes 2)", what, depth);
    if (shift < 0 || shift > 8 * sample_bytes - depth)
        return fail(EMAVFI_E_ARG, "%s: shift = %d (shift must lie in 0..%d at depth %d)", what, shift, 8 * sample_bytes - depth, depth);
    if (C == 3 && sample_bytes == 2) return fail(EMAVFI_E_ARG, "%s: C = 3 at sample_bytes 2 (interleaved colour is scored as bytes only)", what);
    const size_t odd = sample_bytes == 2 ? 1 : 0, row = (size_t)W * C * sample_bytes;
    const struct { const char *name; size_t pitch, bstride; } side[2] = {{"a", a_pitch, a_batch_stride}, {"b", b_pitch, b_batch_stride}};
    for (const auto &sd : side) {
        if (sd.pitch < row) return fail(EMAVFI_E_ARG, "%s: %s_pitch %zu is smaller than its row of %zu bytes", what, sd.name, sd.pitch, row);
        if (sd.pitch & odd) return fail(EMAVFI_E_ARG, "%s: %s_pitch %zu is odd at sample_bytes 2", what, sd.name, sd.pitch);
        size_t plane, span;
        if (__builtin_mul_overflow((size_t)(H - 1), sd.pitch, &plane) || __builtin_add_overflow(plane, row, &plane))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s_pitch %zu)", what, sd.name, sd.pitch);
        if (n > 1 && sd.bstride < plane)
            return fail(EMAVFI_E_ARG, "%s: the batch stride %s_batch_stride %zu is smaller than its plane", what, sd.name, sd.bstride);
        if (n > 1 && (sd.bstride & odd)) return fail(EMAVFI_E_ARG, "%s: %s_batch_stride %zu is odd at sample_bytes 2", what, sd.name, sd.bstride);
        if (n > 1 && (__builtin_mul_overflow((size_t)(n - 1), sd.bstride, &span) || __builtin_add_overflow(span, plane, &span)))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s_batch_stride %zu)", what, sd.name, sd.bstride);
    }
    if (!a || !b || !cells) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if (((uintptr_t)a | (uintptr_t)b) & odd) return fail(EMAVFI_E_ARG, "%s: the image pointers a, b must be 2-byte aligned at sample_bytes 2", what);
    if ((uintptr_t)cells & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer must be 4-byte aligned", what);
    EMAVFI_TRY(launch_frame_diff_cells(a, a_pitch, a_batch_stride, b, b_pitch, b_batch_stride, n, H, W, C, order, sample_bytes, depth, shift, cells,
                                       (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_duplicate_flags(const unsigned *cells, size_t stride_words, int n, unsigned threshold, unsigned *flags, unsigned *scores, void *stream)
{
    const char *const what = "duplicate_flags";
    if (n < 1) return fail(EMAVFI_E_ARG, "%s: n must be >= 1", what);
    if (stride_words < EMAVFI_SCENE_SIG_WORDS)
        return fail(EMAVFI_E_ARG, "%s: a stride of %zu words is below %d", what, stride_words, EMAVFI_SCENE_SIG_WORDS);
    size_t span;
    if (__builtin_mul_overflow((size_t)(n - 1), stride_words, &span) || __builtin_add_overflow(span, (size_t)EMAVFI_SCENE_SIG_WORDS, &span) ||
        __builtin_mul_overflow(span, sizeof(unsigned), &span))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (stride %zu words)", what, stride_words);
    if (!cells || !flags) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if (((uintptr_t)cells | (uintptr_t)flags | (uintptr_t)scores) & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointers must be 4-byte aligned", what);
    EMAVFI_TRY(launch_duplicate_flags(cells, stride_words, n, threshold, flags, scores, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- temporal resampling (include/emavfi.h, "TEMPORAL RESAMPLE DEFINITION"): every check runs on the host, the table is read here and not kept
static_assert(sizeof(emavfi_resample_entry) == sizeof(ResampleEntry) && EMAVFI_RESAMPLE_LAUNCH_CAP == RESAMPLE_CAP &&
              EMAVFI_RESAMPLE_NODES == RESAMPLE_POOL_NODES, "header, misc_kernels.h and resample_elem.h disagree");

// bytes from the first byte of frame 0 to the last byte of frame n - 1; false when the arithmetic overflows
static bool resample_span(int n, size_t stride, size_t frame_bytes, size_t *span)
{
    return !(__builtin_mul_overflow((size_t)(n - 1), stride, span) || __builtin_add_overflow(*span, frame_bytes, span));
}

// what emavfi_resample_frames and emavfi_accumulate_frames refuse alike: everything but the entries of the table
static int resample_pools_check(const char *what, const unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs,
                                size_t src_stride, int n_srcs, const unsigned char *nodes, size_t node_stride, int n_nodes, const void *table,
                                const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift)
{
    if (n_out < 1) return fail(EMAVFI_E_ARG, "%s: n_out must be >= 1", what);
    if (n_srcs < 0 || n_nodes < 0 || n_flags < 0) return fail(EMAVFI_E_ARG, "%s: n_srcs, n_nodes, n_flags must be >= 0", what);
    if (sample_bytes != 1 && sample_bytes != 2) return fail(EMAVFI_E_ARG, "%s: sample_bytes = %d (sample_bytes must be 1 or 2)", what, sample_bytes);
    if (sample_bytes == 1 ? depth != 8 : (depth != 10 && depth != 12 && depth != 16))
        return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8 at sample_bytes 1 and 10, 12 or 16 at sample_bytes 2)", what, depth);
    if (shift < 0 || shift > 8 * sample_bytes - depth)
        return fail(EMAVFI_E_ARG, "%s: shift = %d (shift must lie in 0..%d at depth %d)", what, shift, 8 * sample_bytes - depth, depth);
    if (frame_bytes < 1) return fail(EMAVFI_E_ARG, "%s: frame_bytes must be >= 1", what);
    if (frame_bytes > ((size_t)1 << 40)) return fail(EMAVFI_E_ARG, "%s: frame_bytes %zu is above 2^40", what, frame_bytes);
    const size_t odd = sample_bytes == 2 ? 1 : 0;
    if (frame_bytes & odd) return fail(EMAVFI_E_ARG, "%s: frame_bytes %zu is odd at sample_bytes 2", what, frame_bytes);
    const struct { const char *name; size_t stride; int n; } pools[3] = {{"dst_stride", dst_stride, n_out}, {"src_stride", src_stride, n_srcs},
                                                                         {"node_stride", node_stride, n_nodes}};
    size_t span[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        if (pools[k].n < 1) continue;
        if (pools[k].stride < frame_bytes)
            return fail(EMAVFI_E_ARG, "%s: %s %zu is smaller than frame_bytes %zu", what, pools[k].name, pools[k].stride, frame_bytes);
        if (pools[k].stride & odd) return fail(EMAVFI_E_ARG, "%s: %s %zu is odd at sample_bytes 2", what, pools[k].name, pools[k].stride);
        if (!resample_span(pools[k].n, pools[k].stride, frame_bytes, &span[k]))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s %zu)", what, pools[k].name, pools[k].stride);
    }
    if (!dst) return fail(EMAVFI_E_ARG, "%s: null pointer dst", what);
    if (!table) return fail(EMAVFI_E_ARG, "%s: null pointer table", what);
    if (n_srcs > 0 && !srcs) return fail(EMAVFI_E_ARG, "%s: null pointer srcs with n_srcs = %d", what, n_srcs);
    if (n_nodes > 0 && !nodes) return fail(EMAVFI_E_ARG, "%s: null pointer nodes with n_nodes = %d", what, n_nodes);
    if (n_flags > 0 && !flags) return fail(EMAVFI_E_ARG, "%s: null pointer flags with n_flags = %d", what, n_flags);
    if (((uintptr_t)dst | (uintptr_t)srcs | (uintptr_t)nodes) & odd)
        return fail(EMAVFI_E_ARG, "%s: the frame pointers dst, srcs, nodes must be 2-byte aligned at sample_bytes 2", what);
    if ((uintptr_t)flags & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer flags must be 4-byte aligned", what);
    const uintptr_t d0 = (uintptr_t)dst;
    const uintptr_t base[3] = {d0, (uintptr_t)srcs, (uintptr_t)nodes};
    for (int k = 1; k < 3; ++k)
        if (pools[k].n > 0 && d0 < base[k] + span[k] && base[k] < d0 + span[0])
            return fail(EMAVFI_E_ARG, "%s: dst overlaps %s", what, k == 1 ? "srcs" : "nodes");
    return EMAVFI_OK;
}

int emavfi_resample_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                           const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_resample_entry *table,
                           const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift, void *stream)
{
    const char *const what = "resample_frames";
    if (const int rc = resample_pools_check(what, dst, dst_stride, n_out, srcs, src_stride, n_srcs, nodes, node_stride, n_nodes, table, flags,
                                            n_flags, frame_bytes, sample_bytes, depth, shift))
        return rc;
    for (int k = 0; k < n_out; ++k) {
        const emavfi_resample_entry &e = table[k];
        if (e.w > 256u) return fail(EMAVFI_E_ARG, "%s: table[%d].w = %u is above 256", what, k, e.w);
        const unsigned idx[2] = {e.a, e.b};
        for (int q = 0; q < 2; ++q) {
            const bool node = idx[q] & EMAVFI_RESAMPLE_NODES;
            const unsigned i = idx[q] & ~EMAVFI_RESAMPLE_NODES;
            if (i >= (unsigned)(node ? n_nodes : n_srcs))
                return fail(EMAVFI_E_ARG, "%s: table[%d].%c = %s index %u is outside its pool of %d frames", what, k, q ? 'b' : 'a',
                            node ? "nodes" : "srcs", i, node ? n_nodes : n_srcs);
        }
        if (e.f > (unsigned)n_flags) return fail(EMAVFI_E_ARG, "%s: table[%d].f = %u is beyond n_flags = %d", what, k, e.f, n_flags);
        if (e.f != 0 && e.h >= (unsigned)n_srcs)
            return fail(EMAVFI_E_ARG, "%s: table[%d].h = %u is outside the srcs pool of %d frames", what, k, e.h, n_srcs);
    }
    EMAVFI_TRY(launch_resample_frames(dst, dst_stride, n_out, srcs, src_stride, nodes, node_stride, reinterpret_cast<const ResampleEntry *>(table),
                                      flags, frame_bytes, sample_bytes, depth, shift, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- shutter accumulation (include/emavfi.h, "SHUTTER DEFINITION"): every check runs on the host, the table is read here and not kept
static_assert(sizeof(emavfi_accumulate_entry) == sizeof(AccumulateEntry) && EMAVFI_ACCUMULATE_LAUNCH_CAP == SHUTTER_CAP &&
              EMAVFI_ACCUMULATE_MAX_TAPS == SHUTTER_MAX_TAPS, "header, misc_kernels.h and shutter_elem.h disagree");

// what emavfi_accumulate_frames and emavfi_accumulate_frames_linear refuse alike: everything but the light table
static int accumulate_check(const char *what, const unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs,
                            size_t src_stride, int n_srcs, const unsigned char *nodes, size_t node_stride, int n_nodes,
                            const emavfi_accumulate_entry *table, const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes,
                            int depth, int shift)
{
    if (const int rc = resample_pools_check(what, dst, dst_stride, n_out, srcs, src_stride, n_srcs, nodes, node_stride, n_nodes, table, flags,
                                            n_flags, frame_bytes, sample_bytes, depth, shift))
        return rc;
    for (int k = 0; k < n_out; ++k) {
        const emavfi_accumulate_entry &e = table[k];
        if (e.n < 1u || e.n > (unsigned)EMAVFI_ACCUMULATE_MAX_TAPS)
            return fail(EMAVFI_E_ARG, "%s: table[%d].n = %u is outside 1..%d", what, k, e.n, EMAVFI_ACCUMULATE_MAX_TAPS);
        unsigned sum = 0u;                                            // at most 33 weights below 2^16 each once the loop has passed
        for (unsigned t = 0; t < e.n; ++t) {
            const bool node = e.tap[t] & EMAVFI_RESAMPLE_NODES;
            const unsigned i = e.tap[t] & ~EMAVFI_RESAMPLE_NODES;
            if (i >= (unsigned)(node ? n_nodes : n_srcs))
                return fail(EMAVFI_E_ARG, "%s: table[%d].tap[%u] = %s index %u is outside its pool of %d frames", what, k, t,
                            node ? "nodes" : "srcs", i, node ? n_nodes : n_srcs);
            if (e.w[t] == 0u) return fail(EMAVFI_E_ARG, "%s: table[%d].w[%u] is zero (a frame without weight is no tap)", what, k, t);
            if (e.w[t] > SHUTTER_MAX_SUM || (sum += e.w[t]) > SHUTTER_MAX_SUM)
                return fail(EMAVFI_E_ARG, "%s: table[%d].w sums to more than %u at w[%u] = %u", what, k, SHUTTER_MAX_SUM, t, e.w[t]);
        }
        if (e.f > (unsigned)n_flags) return fail(EMAVFI_E_ARG, "%s: table[%d].f = %u is beyond n_flags = %d", what, k, e.f, n_flags);
        if (e.f != 0 && e.h >= (unsigned)n_srcs)
            return fail(EMAVFI_E_ARG, "%s: table[%d].h = %u is outside the srcs pool of %d frames", what, k, e.h, n_srcs);
    }
    return EMAVFI_OK;
}

int emavfi_accumulate_frames(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                             const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_accumulate_entry *table,
                             const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift, void *stream)
{
    const char *const what = "accumulate_frames";
    if (const int rc = accumulate_check(what, dst, dst_stride, n_out, srcs, src_stride, n_srcs, nodes, node_stride, n_nodes, table, flags,
                                        n_flags, frame_bytes, sample_bytes, depth, shift))
        return rc;
    EMAVFI_TRY(launch_accumulate_frames(dst, dst_stride, n_out, srcs, src_stride, nodes, node_stride,
                                        reinterpret_cast<const AccumulateEntry *>(table), flags, frame_bytes, sample_bytes, depth, shift,
                                        (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- linear light (include/emavfi.h, "LINEAR LIGHT DEFINITION"): the tables are built and checked on the host, in double and in integers
static_assert(EMAVFI_LIGHT_ONE == LIGHT_ONE && EMAVFI_LIGHT_BIAS == LIGHT_BIAS && EMAVFI_LIGHT_LIMIT == LIGHT_LIMIT,
              "header and light_elem.h disagree");

// the inverse transfer function on x >= 0
static double light_inverse(int transfer, double x)
{
    if (transfer == EMAVFI_TRANSFER_SRGB) return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    if (transfer == EMAVFI_TRANSFER_BT709) {
        const double alpha = 1.09929682680944, beta = 0.018053968510807;
        return x < 4.5 * beta ? x / 4.5 : pow((x + alpha - 1.0) / alpha, 1.0 / 0.45);
    }
    const double a = 0.17883277, b = 0.28466892, c = 0.55991073;     // EMAVFI_TRANSFER_HLG
    return x <= 0.5 ? x * x / 3.0 : (exp((x - c) / a) + b) / 12.0;
}

static bool light_depth_ok(int depth) { return depth == 8 || depth == 10 || depth == 12; }

int emavfi_transfer_table(int transfer, int depth, int full_range, unsigned *lin_host)
{
    const char *const what = "transfer_table";
    if (transfer != EMAVFI_TRANSFER_SRGB && transfer != EMAVFI_TRANSFER_BT709 && transfer != EMAVFI_TRANSFER_HLG)
        return fail(EMAVFI_E_ARG, "%s: transfer = %d (EMAVFI_TRANSFER_SRGB, _BT709 or _HLG expected)", what, transfer);
    if (!light_depth_ok(depth)) return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8, 10 or 12)", what, depth);
    if (!lin_host) return fail(EMAVFI_E_ARG, "%s: null pointer lin_host", what);
    const int lo = full_range ? 0 : 16 << (depth - 8), hi = full_range ? (1 << depth) - 1 : 235 << (depth - 8);
    for (int v = 0; v < 1 << depth; ++v) {
        const double x = (double)(v - lo) / (double)(hi - lo);
        const double g = x < 0.0 ? -light_inverse(transfer, -x) : light_inverse(transfer, x);
        lin_host[v] = (unsigned)((long long)EMAVFI_LIGHT_BIAS + llround((double)EMAVFI_LIGHT_ONE * g));
    }
    return EMAVFI_OK;
}

int emavfi_transfer_table_check(const unsigned *lin_host, int depth)
{
    const char *const what = "transfer_table_check";
    if (!light_depth_ok(depth)) return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8, 10 or 12)", what, depth);
    if (!lin_host) return fail(EMAVFI_E_ARG, "%s: null pointer lin_host", what);
    for (int v = 0; v < 1 << depth; ++v) {
        if (lin_host[v] >= EMAVFI_LIGHT_LIMIT) return fail(EMAVFI_E_ARG, "%s: lin[%d] = %u is not below 2^30", what, v, lin_host[v]);
        if (v > 0 && lin_host[v] <= lin_host[v - 1])
            return fail(EMAVFI_E_ARG, "%s: lin[%d] = %u is not above lin[%d] = %u (the table must be strictly increasing)", what, v, lin_host[v],
                        v - 1, lin_host[v - 1]);
    }
    return EMAVFI_OK;
}

int emavfi_accumulate_frames_linear(unsigned char *dst, size_t dst_stride, int n_out, const unsigned char *srcs, size_t src_stride, int n_srcs,
                                    const unsigned char *nodes, size_t node_stride, int n_nodes, const emavfi_accumulate_entry *table,
                                    const unsigned *flags, int n_flags, size_t frame_bytes, int sample_bytes, int depth, int shift,
                                    const unsigned *lin, size_t linear_bytes, void *stream)
{
    const char *const what = "accumulate_frames_linear";
    if (const int rc = accumulate_check(what, dst, dst_stride, n_out, srcs, src_stride, n_srcs, nodes, node_stride, n_nodes, table, flags,
                                        n_flags, frame_bytes, sample_bytes, depth, shift))
        return rc;
    if (!light_depth_ok(depth))
        return fail(EMAVFI_E_ARG, "%s: depth = %d (linear light takes depth 8, 10 or 12: a table of 2^16 words does not fit LDS)", what, depth);
    if (!lin) return fail(EMAVFI_E_ARG, "%s: null pointer lin", what);
    if ((uintptr_t)lin & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer lin must be 4-byte aligned", what);
    if (linear_bytes > frame_bytes) return fail(EMAVFI_E_ARG, "%s: linear_bytes %zu is above frame_bytes %zu", what, linear_bytes, frame_bytes);
    if (linear_bytes % (size_t)sample_bytes)
        return fail(EMAVFI_E_ARG, "%s: linear_bytes %zu is not a multiple of sample_bytes %d", what, linear_bytes, sample_bytes);
    EMAVFI_TRY(launch_accumulate_frames_linear(dst, dst_stride, n_out, srcs, src_stride, nodes, node_stride,
                                               reinterpret_cast<const AccumulateEntry *>(table), flags, frame_bytes, sample_bytes, depth, shift,
                                               lin, linear_bytes, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- static regions (include/emavfi.h, "STATIC REGION DEFINITION"): every check runs on the host, the table is read here and not kept
static_assert(sizeof(emavfi_static_entry) == sizeof(StaticEntry) && EMAVFI_RESAMPLE_LAUNCH_CAP == STATIC_CAP &&
              EMAVFI_STATIC_MAX_RADIUS == STATIC_MAX_RADIUS && EMAVFI_LAYOUT_INTERLEAVED == STATIC_LAYOUT_INTERLEAVED &&
              EMAVFI_LAYOUT_NV12 == STATIC_LAYOUT_NV12 && EMAVFI_LAYOUT_I420 == STATIC_LAYOUT_I420, "header, misc_kernels.h and static_elem.h disagree");

int emavfi_static_guard_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, int n_srcs,
                               const emavfi_static_entry *table, int H, int W, int layout, int C, int sample_bytes, int depth, int shift,
                               int radius, unsigned tol, unsigned *counts, void *stream)
{
    const char *const what = "static_guard_frames";
    if (n_dst < 1) return fail(EMAVFI_E_ARG, "%s: n_dst must be >= 1", what);
    if (n_srcs < 1) return fail(EMAVFI_E_ARG, "%s: n_srcs must be >= 1", what);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (layout != EMAVFI_LAYOUT_INTERLEAVED && layout != EMAVFI_LAYOUT_NV12 && layout != EMAVFI_LAYOUT_I420)
        return fail(EMAVFI_E_ARG, "%s: unknown layout %d (EMAVFI_LAYOUT_INTERLEAVED, EMAVFI_LAYOUT_NV12 or EMAVFI_LAYOUT_I420)", what, layout);
    if (layout != EMAVFI_LAYOUT_INTERLEAVED && ((H | W) & 1))
        return fail(EMAVFI_E_ARG, "%s: H = %d, W = %d: a 4:2:0 layout needs an even H and W", what, H, W);
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1..4)", what, C);
    if (layout != EMAVFI_LAYOUT_INTERLEAVED && C != 1) return fail(EMAVFI_E_ARG, "%s: C = %d at a 4:2:0 layout (C must be 1 there)", what, C);
    if (sample_bytes != 1 && sample_bytes != 2) return fail(EMAVFI_E_ARG, "%s: sample_bytes = %d (sample_bytes must be 1 or 2)", what, sample_bytes);
    if (sample_bytes == 1 ? depth != 8 : (depth != 10 && depth != 12 && depth != 16))
        return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8 at sample_bytes 1 and 10, 12 or 16 at sample_bytes 2)", what, depth);
    if (shift < 0 || shift > 8 * sample_bytes - depth)
        return fail(EMAVFI_E_ARG, "%s: shift = %d (shift must lie in 0..%d at depth %d)", what, shift, 8 * sample_bytes - depth, depth);
    if (radius < 0 || radius > EMAVFI_STATIC_MAX_RADIUS)
        return fail(EMAVFI_E_ARG, "%s: radius = %d (radius must lie in 0..%d)", what, radius, EMAVFI_STATIC_MAX_RADIUS);
    if (tol > (1u << depth) - 1u) return fail(EMAVFI_E_ARG, "%s: tol = %u is above 2^depth - 1 = %u", what, tol, (1u << depth) - 1u);
    StaticPlane planes[3];
    size_t frame_bytes;                                   // at most 16384^2 * 4 * 2 = 2^31
    static_planes(layout, C, H, W, sample_bytes, planes, &frame_bytes);
    const size_t odd = sample_bytes == 2 ? 1 : 0;
    const struct { const char *name; size_t stride; int n; } pools[2] = {{"dst_stride", dst_stride, n_dst}, {"src_stride", src_stride, n_srcs}};
    size_t span[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        if (pools[k].stride < frame_bytes)
            return fail(EMAVFI_E_ARG, "%s: %s %zu is smaller than the frame's %zu bytes", what, pools[k].name, pools[k].stride, frame_bytes);
        if (pools[k].stride & odd) return fail(EMAVFI_E_ARG, "%s: %s %zu is odd at sample_bytes 2", what, pools[k].name, pools[k].stride);
        if (!resample_span(pools[k].n, pools[k].stride, frame_bytes, &span[k]))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s %zu)", what, pools[k].name, pools[k].stride);
    }
    size_t count_bytes;
    if (__builtin_mul_overflow((size_t)n_dst, sizeof(unsigned), &count_bytes)) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (n_dst)", what);
    if (!dst) return fail(EMAVFI_E_ARG, "%s: null pointer dst", what);
    if (!srcs) return fail(EMAVFI_E_ARG, "%s: null pointer srcs", what);
    if (!table) return fail(EMAVFI_E_ARG, "%s: null pointer table", what);
    if (((uintptr_t)dst | (uintptr_t)srcs) & odd)
        return fail(EMAVFI_E_ARG, "%s: the frame pointers dst, srcs must be 2-byte aligned at sample_bytes 2", what);
    if ((uintptr_t)counts & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer counts must be 4-byte aligned", what);
    const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)srcs;
    if (d0 + span[0] < d0 || s0 + span[1] < s0) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (a pool wraps the address space)", what);
    if (d0 < s0 + span[1] && s0 < d0 + span[0]) return fail(EMAVFI_E_ARG, "%s: dst overlaps srcs", what);
    for (int k = 0; k < n_dst; ++k) {
        if (table[k].a >= (unsigned)n_srcs)
            return fail(EMAVFI_E_ARG, "%s: table[%d].a = %u is outside srcs (%d frames)", what, k, table[k].a, n_srcs);
        if (table[k].b >= (unsigned)n_srcs)
            return fail(EMAVFI_E_ARG, "%s: table[%d].b = %u is outside srcs (%d frames)", what, k, table[k].b, n_srcs);
    }
    EMAVFI_TRY(launch_static_guard_frames(dst, dst_stride, n_dst, srcs, src_stride, reinterpret_cast<const StaticEntry *>(table), H, W, layout, C,
                                          sample_bytes, depth, shift, radius, tol, counts, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- the active picture (include/emavfi.h, "ACTIVE AREA DEFINITION"): every check runs on the host, pointers are looked at last, the table is
// read here and not kept
static_assert(EMAVFI_RESAMPLE_LAUNCH_CAP == ACTIVE_CAP, "header and active_elem.h disagree");

// what the four entries refuse alike about a sample format
static int active_sample_check(const char *what, int sample_bytes, int depth, int shift)
{
    if (sample_bytes != 1 && sample_bytes != 2) return fail(EMAVFI_E_ARG, "%s: sample_bytes = %d (sample_bytes must be 1 or 2)", what, sample_bytes);
    if (sample_bytes == 1 ? depth != 8 : (depth != 10 && depth != 12 && depth != 16))
        return fail(EMAVFI_E_ARG, "%s: depth = %d (depth must be 8 at sample_bytes 1 and 10, 12 or 16 at sample_bytes 2)", what, depth);
    if (shift < 0 || shift > 8 * sample_bytes - depth)
        return fail(EMAVFI_E_ARG, "%s: shift = %d (shift must lie in 0..%d at depth %d)", what, shift, 8 * sample_bytes - depth, depth);
    return EMAVFI_OK;
}
// one pitched image batch of n images of H rows of `row` bytes
static int active_image_check(const char *what, size_t pitch, size_t bstride, int n, int H, size_t row, size_t odd)
{
    if (pitch < row) return fail(EMAVFI_E_ARG, "%s: pitch %zu is smaller than its row of %zu bytes", what, pitch, row);
    if (pitch & odd) return fail(EMAVFI_E_ARG, "%s: pitch %zu is odd at sample_bytes 2", what, pitch);
    size_t plane, span;
    if (__builtin_mul_overflow((size_t)(H - 1), pitch, &plane) || __builtin_add_overflow(plane, row, &plane))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (pitch %zu)", what, pitch);
    if (n > 1 && bstride < plane) return fail(EMAVFI_E_ARG, "%s: the batch stride batch_stride %zu is smaller than its plane", what, bstride);
    if (n > 1 && (bstride & odd)) return fail(EMAVFI_E_ARG, "%s: batch_stride %zu is odd at sample_bytes 2", what, bstride);
    if (n > 1 && (__builtin_mul_overflow((size_t)(n - 1), bstride, &span) || __builtin_add_overflow(span, plane, &span)))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (batch_stride %zu)", what, bstride);
    return EMAVFI_OK;
}

int emavfi_active_bounds(const unsigned char *img, size_t pitch, size_t batch_stride, int n, int H, int W, int C, int sample_bytes, int depth,
                         int shift, unsigned level, unsigned *bounds, void *stream)
{
    const char *const what = "active_bounds";
    if (n < 1) return fail(EMAVFI_E_ARG, "%s: n must be >= 1", what);
    if (n > 65535) return fail(EMAVFI_E_ARG, "%s: n = %d is above 65535", what, n);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (C != 1 && C != 3) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1 or 3)", what, C);
    if (const int rc = active_sample_check(what, sample_bytes, depth, shift); rc != EMAVFI_OK) return rc;
    if (C == 3 && sample_bytes == 2) return fail(EMAVFI_E_ARG, "%s: C = 3 at sample_bytes 2 (interleaved colour is scanned as bytes only)", what);
    if (level > (1u << depth) - 1u) return fail(EMAVFI_E_ARG, "%s: level = %u is above 2^depth - 1 = %u", what, level, (1u << depth) - 1u);
    const size_t odd = sample_bytes == 2 ? 1 : 0;
    if (const int rc = active_image_check(what, pitch, batch_stride, n, H, (size_t)W * C * sample_bytes, odd); rc != EMAVFI_OK) return rc;
    if (!img) return fail(EMAVFI_E_ARG, "%s: null pointer img", what);
    if (!bounds) return fail(EMAVFI_E_ARG, "%s: null pointer bounds", what);
    if ((uintptr_t)img & odd) return fail(EMAVFI_E_ARG, "%s: the image pointer img must be 2-byte aligned at sample_bytes 2", what);
    if ((uintptr_t)bounds & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer bounds must be 4-byte aligned", what);
    EMAVFI_TRY(launch_active_bounds(img, pitch, batch_stride, n, H, W, C, sample_bytes, depth, shift, level, bounds, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_fill_outside_frames(unsigned char *dst, size_t dst_stride, int n_dst, const unsigned char *srcs, size_t src_stride, int n_srcs,
                               const unsigned *table, int H, int W, int layout, int C, int sample_bytes, int top, int left, int height, int width,
                               void *stream)
{
    const char *const what = "fill_outside_frames";
    if (n_dst < 1) return fail(EMAVFI_E_ARG, "%s: n_dst must be >= 1", what);
    if (n_srcs < 1) return fail(EMAVFI_E_ARG, "%s: n_srcs must be >= 1", what);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (layout != EMAVFI_LAYOUT_INTERLEAVED && layout != EMAVFI_LAYOUT_NV12 && layout != EMAVFI_LAYOUT_I420)
        return fail(EMAVFI_E_ARG, "%s: unknown layout %d (EMAVFI_LAYOUT_INTERLEAVED, EMAVFI_LAYOUT_NV12 or EMAVFI_LAYOUT_I420)", what, layout);
    const bool sub = layout != EMAVFI_LAYOUT_INTERLEAVED;
    if (sub && ((H | W) & 1)) return fail(EMAVFI_E_ARG, "%s: H = %d, W = %d: a 4:2:0 layout needs an even H and W", what, H, W);
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1..4)", what, C);
    if (sub && C != 1) return fail(EMAVFI_E_ARG, "%s: C = %d at a 4:2:0 layout (C must be 1 there)", what, C);
    if (sample_bytes != 1 && sample_bytes != 2) return fail(EMAVFI_E_ARG, "%s: sample_bytes = %d (sample_bytes must be 1 or 2)", what, sample_bytes);
    if (height < 1 || width < 1) return fail(EMAVFI_E_ARG, "%s: the rectangle has no area (height = %d, width = %d)", what, height, width);
    if (top < 0 || left < 0 || top > H - height || left > W - width)
        return fail(EMAVFI_E_ARG, "%s: the rectangle (top = %d, left = %d, height = %d, width = %d) leaves the %d x %d frame", what, top, left, height,
                    width, H, W);
    if (sub && ((top | left | height | width) & 1))
        return fail(EMAVFI_E_ARG, "%s: the rectangle (top = %d, left = %d, height = %d, width = %d) is odd at a 4:2:0 layout", what, top, left, height,
                    width);
    StaticPlane planes[3];
    size_t frame_bytes;                                   // at most 16384^2 * 4 * 2 = 2^31
    static_planes(layout, C, H, W, sample_bytes, planes, &frame_bytes);
    const size_t odd = sample_bytes == 2 ? 1 : 0;
    const struct { const char *name; size_t stride; int n; } pools[2] = {{"dst_stride", dst_stride, n_dst}, {"src_stride", src_stride, n_srcs}};
    size_t span[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        if (pools[k].stride < frame_bytes)
            return fail(EMAVFI_E_ARG, "%s: %s %zu is smaller than the frame's %zu bytes", what, pools[k].name, pools[k].stride, frame_bytes);
        if (pools[k].stride & odd) return fail(EMAVFI_E_ARG, "%s: %s %zu is odd at sample_bytes 2", what, pools[k].name, pools[k].stride);
        if (!resample_span(pools[k].n, pools[k].stride, frame_bytes, &span[k]))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s %zu)", what, pools[k].name, pools[k].stride);
    }
    if (!dst) return fail(EMAVFI_E_ARG, "%s: null pointer dst", what);
    if (!srcs) return fail(EMAVFI_E_ARG, "%s: null pointer srcs", what);
    if (!table) return fail(EMAVFI_E_ARG, "%s: null pointer table", what);
    if (((uintptr_t)dst | (uintptr_t)srcs) & odd)
        return fail(EMAVFI_E_ARG, "%s: the frame pointers dst, srcs must be 2-byte aligned at sample_bytes 2", what);
    const uintptr_t d0 = (uintptr_t)dst, s0 = (uintptr_t)srcs;
    if (d0 + span[0] < d0 || s0 + span[1] < s0) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (a pool wraps the address space)", what);
    if (d0 < s0 + span[1] && s0 < d0 + span[0]) return fail(EMAVFI_E_ARG, "%s: dst overlaps srcs", what);
    for (int k = 0; k < n_dst; ++k)
        if (table[k] >= (unsigned)n_srcs) return fail(EMAVFI_E_ARG, "%s: table[%d] = %u is outside srcs (%d frames)", what, k, table[k], n_srcs);
    EMAVFI_TRY(launch_fill_outside_frames(dst, dst_stride, n_dst, srcs, src_stride, table, H, W, layout, C, sample_bytes, top, left, height, width,
                                          (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// what the pitched u8 pair refuses alike: everything but the pointers
static int u8_pitched_check(const char *what, size_t pitch, size_t batch_stride, int B, int H, int W, int C)
{
    if (B < 1) return fail(EMAVFI_E_ARG, "%s: B must be >= 1", what);
    if (B > 65535) return fail(EMAVFI_E_ARG, "%s: B = %d is above 65535", what, B);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1..4)", what, C);
    return active_image_check(what, pitch, batch_stride, B, H, (size_t)W * C, 0);
}

int emavfi_preprocess_u8_pitched(const unsigned char *frames, size_t pitch, size_t batch_stride, float *out_nchw, int B, int H, int W, int C,
                                 const float *mean, const float *std, void *stream)
{
    const char *const what = "preprocess_u8_pitched";
    if (const int rc = u8_pitched_check(what, pitch, batch_stride, B, H, W, C); rc != EMAVFI_OK) return rc;
    if (!mean || !std) return fail(EMAVFI_E_ARG, "%s: null mean / std", what);
    for (int c = 0; c < C; ++c)
        if (!(std[c] != 0.0f)) return fail(EMAVFI_E_ARG, "%s: std[%d] must be non-zero", what, c);
    if (!frames) return fail(EMAVFI_E_ARG, "%s: null pointer frames", what);
    if (!out_nchw) return fail(EMAVFI_E_ARG, "%s: null pointer out_nchw", what);
    if ((uintptr_t)out_nchw & 3) return fail(EMAVFI_E_ARG, "%s: the fp32 pointer out_nchw must be 4-byte aligned", what);
    EMAVFI_TRY(launch_preprocess_u8_pitched(frames, pitch, batch_stride, out_nchw, B, H, W, C, mean, std, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_postprocess_u8_pitched(const float *frames_nchw, unsigned char *out, size_t pitch, size_t batch_stride, int B, int H, int W, int C,
                                  const double *mean, const double *std, int denormalize, void *stream)
{
    const char *const what = "postprocess_u8_pitched";
    if (const int rc = u8_pitched_check(what, pitch, batch_stride, B, H, W, C); rc != EMAVFI_OK) return rc;
    if (!mean || !std) return fail(EMAVFI_E_ARG, "%s: null mean / std", what);
    if (!frames_nchw) return fail(EMAVFI_E_ARG, "%s: null pointer frames_nchw", what);
    if (!out) return fail(EMAVFI_E_ARG, "%s: null pointer out", what);
    if ((uintptr_t)frames_nchw & 3) return fail(EMAVFI_E_ARG, "%s: the fp32 pointer frames_nchw must be 4-byte aligned", what);
    EMAVFI_TRY(launch_postprocess_u8_pitched(frames_nchw, out, pitch, batch_stride, B, H, W, C, mean, std, denormalize ? 1 : 0, (hipStream_t)stream),
               what);
    return EMAVFI_OK;
}

// ---- test-time ensembling (include/emavfi.h, "ENSEMBLE DEFINITION"): every check runs on the host, the member list is read here and not kept
static_assert(EMAVFI_FLIP_H == ENSEMBLE_FLIP_H && EMAVFI_FLIP_V == ENSEMBLE_FLIP_V && EMAVFI_ENSEMBLE_MAX_MEMBERS == ENSEMBLE_MAX_MEMBERS,
              "header and ensemble_elem.h disagree");

// the bytes of a dense fp32 [planes][H][W] tensor, refused where the arithmetic overflows size_t
static int ensemble_shape_check(const char *what, size_t planes, int H, int W, size_t *bytes)
{
    if (planes < 1) return fail(EMAVFI_E_ARG, "%s: planes must be >= 1", what);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (__builtin_mul_overflow(planes, (size_t)H * W * sizeof(float), bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (planes %zu)", what, planes);
    return EMAVFI_OK;
}

// a tensor of `bytes` bytes at p: 4-byte aligned, inside the address space
static int ensemble_pointer_check(const char *what, const char *name, int index, const void *p, size_t bytes)
{
    char label[32];
    if (index >= 0) snprintf(label, sizeof label, "%s[%d]", name, index);
    else snprintf(label, sizeof label, "%s", name);
    if (!p) return fail(EMAVFI_E_ARG, "%s: null pointer %s", what, label);
    if ((uintptr_t)p & 3) return fail(EMAVFI_E_ARG, "%s: the fp32 pointer %s must be 4-byte aligned", what, label);
    if ((uintptr_t)p + bytes < (uintptr_t)p) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s wraps the address space)", what, label);
    return EMAVFI_OK;
}

int emavfi_flip_f32(const float *src, float *dst, size_t planes, int H, int W, int flip, void *stream)
{
    const char *const what = "flip_f32";
    size_t bytes;
    if (const int rc = ensemble_shape_check(what, planes, H, W, &bytes); rc != EMAVFI_OK) return rc;
    if (!ensemble_flip_ok(flip)) return fail(EMAVFI_E_ARG, "%s: flip = %d (flip must lie in 0..3: EMAVFI_FLIP_H | EMAVFI_FLIP_V)", what, flip);
    if (const int rc = ensemble_pointer_check(what, "src", -1, src, bytes); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "dst", -1, dst, bytes); rc != EMAVFI_OK) return rc;
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    if (d0 < s0 + bytes && s0 < d0 + bytes) return fail(EMAVFI_E_ARG, "%s: dst overlaps src", what);
    EMAVFI_TRY(launch_flip_f32(src, dst, planes, H, W, flip, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_ensemble_mean_f32(const float *const *members, const int *flips, int n, float *out, size_t planes, int H, int W, void *stream)
{
    const char *const what = "ensemble_mean_f32";
    if (!ensemble_count_ok(n)) return fail(EMAVFI_E_ARG, "%s: n = %d (n must be 1, 2, 4 or 8)", what, n);
    size_t bytes;
    if (const int rc = ensemble_shape_check(what, planes, H, W, &bytes); rc != EMAVFI_OK) return rc;
    if (!members) return fail(EMAVFI_E_ARG, "%s: null pointer members", what);
    if (!flips) return fail(EMAVFI_E_ARG, "%s: null pointer flips", what);
    if (const int rc = ensemble_pointer_check(what, "out", -1, out, bytes); rc != EMAVFI_OK) return rc;
    const uintptr_t o0 = (uintptr_t)out;
    for (int k = 0; k < n; ++k) {
        if (!ensemble_flip_ok(flips[k])) return fail(EMAVFI_E_ARG, "%s: flips[%d] = %d (a flip must lie in 0..3)", what, k, flips[k]);
        if (const int rc = ensemble_pointer_check(what, "members", k, members[k], bytes); rc != EMAVFI_OK) return rc;
        const uintptr_t m0 = (uintptr_t)members[k];
        if (o0 < m0 + bytes && m0 < o0 + bytes) return fail(EMAVFI_E_ARG, "%s: out overlaps members[%d]", what, k);
    }
    EMAVFI_TRY(launch_ensemble_mean_f32(members, flips, n, out, planes, H, W, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- frame borders (include/emavfi.h, "BORDER DEFINITION"): every check runs on the host; H, W are the picture's size in both entries
static_assert(EMAVFI_BORDER_REPLICATE == BORDER_REPLICATE && EMAVFI_BORDER_REFLECT == BORDER_REFLECT && EMAVFI_BORDER_MAX == BORDER_MAX
              && EMAVFI_RESIZE_MAX_DIM == BORDER_MAX_DIM, "header and border_elem.h disagree");

// the bytes of the picture [planes][H][W] and of its extension [planes][H + 2N][W + 2N], refused where a size or the arithmetic is out of range
static int border_shape_check(const char *what, size_t planes, int H, int W, int N, size_t *picture_bytes, size_t *padded_bytes)
{
    if (planes < 1) return fail(EMAVFI_E_ARG, "%s: planes must be >= 1", what);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (!border_n_ok(N)) return fail(EMAVFI_E_ARG, "%s: N = %d (N must lie in 0..%d: EMAVFI_BORDER_MAX)", what, N, BORDER_MAX);
    const int Hp = border_padded_dim(H, N), Wp = border_padded_dim(W, N);
    if (!border_dim_ok(Hp) || !border_dim_ok(Wp))
        return fail(EMAVFI_E_ARG, "%s: a dimension of the padded tensor (%d x %d: %d x %d with N = %d) is above 16384", what, Hp, Wp, H, W, N);
    if (__builtin_mul_overflow(planes, (size_t)H * W * sizeof(float), picture_bytes)
        || __builtin_mul_overflow(planes, (size_t)Hp * Wp * sizeof(float), padded_bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (planes %zu)", what, planes);
    return EMAVFI_OK;
}

static int border_overlap_check(const char *what, const void *src, size_t src_bytes, const void *dst, size_t dst_bytes)
{
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    if (d0 < s0 + src_bytes && s0 < d0 + dst_bytes) return fail(EMAVFI_E_ARG, "%s: dst overlaps src", what);
    return EMAVFI_OK;
}

int emavfi_border_pad_f32(const float *src, float *dst, size_t planes, int H, int W, int N, int mode, void *stream)
{
    const char *const what = "border_pad_f32";
    size_t picture, padded;
    if (const int rc = border_shape_check(what, planes, H, W, N, &picture, &padded); rc != EMAVFI_OK) return rc;
    if (!border_mode_ok(mode))
        return fail(EMAVFI_E_ARG, "%s: mode = %d (mode must be EMAVFI_BORDER_REPLICATE = 0 or EMAVFI_BORDER_REFLECT = 1)", what, mode);
    if (const int rc = ensemble_pointer_check(what, "src", -1, src, picture); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "dst", -1, dst, padded); rc != EMAVFI_OK) return rc;
    if (const int rc = border_overlap_check(what, src, picture, dst, padded); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_border_pad_f32(src, dst, planes, H, W, N, mode, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_border_crop_f32(const float *src, float *dst, size_t planes, int H, int W, int N, void *stream)
{
    const char *const what = "border_crop_f32";
    size_t picture, padded;
    if (const int rc = border_shape_check(what, planes, H, W, N, &picture, &padded); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "src", -1, src, padded); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "dst", -1, dst, picture); rc != EMAVFI_OK) return rc;
    if (const int rc = border_overlap_check(what, src, padded, dst, picture); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_border_crop_f32(src, dst, planes, H, W, N, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- global motion (include/emavfi.h, "ALIGN DEFINITION"): every check runs on the host, before any work goes on the stream
static_assert(EMAVFI_ALIGN_CELL == ALIGN_CELL && EMAVFI_ALIGN_MAX_RADIUS == ALIGN_MAX_RADIUS && EMAVFI_ALIGN_MAX_RATIO == ALIGN_MAX_RATIO
              && EMAVFI_RESIZE_MAX_DIM == ALIGN_MAX_DIM, "header and align_elem.h disagree");

// a tensor of `bytes` bytes at p whose elements are `align` bytes wide
static int align_pointer_check(const char *what, const char *name, const void *p, size_t bytes, unsigned align)
{
    if (!p) return fail(EMAVFI_E_ARG, "%s: null pointer %s", what, name);
    if ((uintptr_t)p & (align - 1)) return fail(EMAVFI_E_ARG, "%s: the pointer %s must be %u-byte aligned", what, name, align);
    if ((uintptr_t)p + bytes < (uintptr_t)p) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (%s wraps the address space)", what, name);
    return EMAVFI_OK;
}

int emavfi_align_signature_f32(const float *x, unsigned short *sig, int B, int H, int W, void *stream)
{
    const char *const what = "align_signature_f32";
    if (B < 1) return fail(EMAVFI_E_ARG, "%s: B = %d (B must be >= 1)", what, B);
    if (!align_sig_dim_ok(H) || !align_sig_dim_ok(W))
        return fail(EMAVFI_E_ARG, "%s: H, W = %d, %d (each must lie in %d..%d)", what, H, W, ALIGN_MIN_DIM, ALIGN_MAX_DIM);
    size_t x_bytes, sig_bytes;
    if (__builtin_mul_overflow((size_t)B, (size_t)3 * H * W * sizeof(float), &x_bytes)
        || __builtin_mul_overflow((size_t)B, (size_t)align_cells(H) * align_cells(W) * sizeof(unsigned short), &sig_bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (B %d)", what, B);
    if (const int rc = align_pointer_check(what, "x", x, x_bytes, 4); rc != EMAVFI_OK) return rc;
    if (const int rc = align_pointer_check(what, "sig", sig, sig_bytes, 2); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_align_signature_f32(x, sig, B, H, W, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

size_t emavfi_align_workspace_bytes(int B, int R)
{
    if (B < 1 || !align_radius_ok(R)) return 0;
    size_t bytes;
    if (__builtin_mul_overflow((size_t)B, (size_t)align_candidates(R) * sizeof(unsigned long long), &bytes)) return 0;
    return bytes;
}

int emavfi_align_search(const unsigned short *sig_a, const unsigned short *sig_b, int B, int Hc, int Wc, int R, int ratio, void *workspace,
                        size_t workspace_bytes, int *shifts, void *stream)
{
    const char *const what = "align_search";
    if (B < 1) return fail(EMAVFI_E_ARG, "%s: B = %d (B must be >= 1)", what, B);
    if (!align_grid_dim_ok(Hc) || !align_grid_dim_ok(Wc))
        return fail(EMAVFI_E_ARG, "%s: Hc, Wc = %d, %d (each must lie in %d..%d cells)", what, Hc, Wc, ALIGN_MIN_DIM / ALIGN_CELL, ALIGN_MAX_DIM / ALIGN_CELL);
    if (!align_radius_ok(R)) return fail(EMAVFI_E_ARG, "%s: R = %d (R must lie in 1..%d cells: EMAVFI_ALIGN_MAX_RADIUS)", what, R, ALIGN_MAX_RADIUS);
    if (!align_radius_fits(R, Hc, Wc))
        return fail(EMAVFI_E_ARG, "%s: R = %d with a grid of %d x %d cells (2 R must not exceed min(Hc, Wc))", what, R, Hc, Wc);
    if (!align_ratio_ok(ratio)) return fail(EMAVFI_E_ARG, "%s: ratio = %d (ratio must lie in 0..%d: EMAVFI_ALIGN_MAX_RATIO)", what, ratio, ALIGN_MAX_RATIO);
    size_t sig_bytes;
    if (__builtin_mul_overflow((size_t)B, (size_t)Hc * Wc * sizeof(unsigned short), &sig_bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (B %d)", what, B);
    const size_t need = emavfi_align_workspace_bytes(B, R);
    if (need == 0) return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (B %d)", what, B);
    if (const int rc = align_pointer_check(what, "sig_a", sig_a, sig_bytes, 2); rc != EMAVFI_OK) return rc;
    if (const int rc = align_pointer_check(what, "sig_b", sig_b, sig_bytes, 2); rc != EMAVFI_OK) return rc;
    if (const int rc = align_pointer_check(what, "workspace", workspace, need, 8); rc != EMAVFI_OK) return rc;
    if (workspace_bytes < need)
        return fail(EMAVFI_E_ARG, "%s: workspace_bytes = %zu is too small (emavfi_align_workspace_bytes gives %zu)", what, workspace_bytes, need);
    if (const int rc = align_pointer_check(what, "shifts", shifts, (size_t)B * 4 * sizeof(int), 4); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_align_search(sig_a, sig_b, B, Hc, Wc, R, ratio, (unsigned long long *)workspace, shifts, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_shift_f32(const float *src, float *dst, int B, int C, int H, int W, const int *shifts, int sign, void *stream)
{
    const char *const what = "shift_f32";
    if (B < 1 || C < 1) return fail(EMAVFI_E_ARG, "%s: B, C = %d, %d (each must be >= 1)", what, B, C);
    if (!align_dim_ok(H) || !align_dim_ok(W)) return fail(EMAVFI_E_ARG, "%s: H, W = %d, %d (each must lie in 1..%d)", what, H, W, ALIGN_MAX_DIM);
    if (!align_sign_ok(sign)) return fail(EMAVFI_E_ARG, "%s: sign = %d (sign must be +1 or -1)", what, sign);
    size_t planes, bytes;
    if (__builtin_mul_overflow((size_t)B, (size_t)C, &planes) || __builtin_mul_overflow(planes, (size_t)H * W * sizeof(float), &bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (B %d, C %d)", what, B, C);
    if (const int rc = align_pointer_check(what, "src", src, bytes, 4); rc != EMAVFI_OK) return rc;
    if (const int rc = align_pointer_check(what, "dst", dst, bytes, 4); rc != EMAVFI_OK) return rc;
    if (const int rc = align_pointer_check(what, "shifts", shifts, (size_t)B * 4 * sizeof(int), 4); rc != EMAVFI_OK) return rc;
    if (const int rc = border_overlap_check(what, src, bytes, dst, bytes); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_shift_f32(src, dst, B, C, H, W, shifts, sign, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- coarse flow, steps 1 and 3 (include/emavfi.h, "COARSE FLOW DEFINITION"): every check runs on the host; H, W are the FINE tensor's size
static_assert(EMAVFI_RESIZE_MAX_DIM == COARSE_MAX_DIM, "header and coarse_elem.h disagree");

// the bytes of the fine [planes][H][W] and of the coarse [planes][ceil(H / s)][ceil(W / s)] tensor, refused where s, a size or the arithmetic
// is out of range; `given` (upsample) is the caller's {Hs, Ws}, which must be those ceilings
static int coarse_shape_check(const char *what, size_t planes, int H, int W, int s, const int *given, size_t *fine_bytes, size_t *coarse_bytes)
{
    if (planes < 1) return fail(EMAVFI_E_ARG, "%s: planes must be >= 1", what);
    if (!coarse_scale_ok(s)) return fail(EMAVFI_E_ARG, "%s: s = %d (s must be 2, 4 or 8)", what, s);
    if (!coarse_dim_ok(H) || !coarse_dim_ok(W)) return fail(EMAVFI_E_ARG, "%s: H, W must lie in 1..16384 (got %d, %d)", what, H, W);
    const int Hs = coarse_dim(H, s), Ws = coarse_dim(W, s);
    if (given && (!coarse_dim_ok(given[0]) || !coarse_dim_ok(given[1])))
        return fail(EMAVFI_E_ARG, "%s: Hs, Ws must lie in 1..16384 (got %d, %d)", what, given[0], given[1]);
    if (given && (given[0] != Hs || given[1] != Ws))
        return fail(EMAVFI_E_ARG, "%s: Hs x Ws = %d x %d, but ceil(H / s) x ceil(W / s) = %d x %d for %d x %d at s = %d", what, given[0], given[1], Hs, Ws,
                    H, W, s);
    if (__builtin_mul_overflow(planes, (size_t)H * W * sizeof(float), fine_bytes)
        || __builtin_mul_overflow(planes, (size_t)Hs * Ws * sizeof(float), coarse_bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (planes %zu)", what, planes);
    return EMAVFI_OK;
}

int emavfi_downscale_f32(const float *src, float *dst, size_t planes, int H, int W, int s, void *stream)
{
    const char *const what = "downscale_f32";
    size_t fine, coarse;
    if (const int rc = coarse_shape_check(what, planes, H, W, s, nullptr, &fine, &coarse); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "src", -1, src, fine); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "dst", -1, dst, coarse); rc != EMAVFI_OK) return rc;
    if (const int rc = border_overlap_check(what, src, fine, dst, coarse); rc != EMAVFI_OK) return rc;
    EMAVFI_TRY(launch_coarse_down_f32(src, dst, planes, H, W, s, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

int emavfi_upsample_flow_f32(const float *flow_s, float *flow, size_t planes, int Hs, int Ws, int H, int W, int s, void *stream)
{
    const char *const what = "upsample_flow_f32";
    size_t fine, coarse;
    const int given[2] = {Hs, Ws};
    if (const int rc = coarse_shape_check(what, planes, H, W, s, given, &fine, &coarse); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "flow_s", -1, flow_s, coarse); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "flow", -1, flow, fine); rc != EMAVFI_OK) return rc;
    const uintptr_t s0 = (uintptr_t)flow_s, d0 = (uintptr_t)flow;
    if (d0 < s0 + coarse && s0 < d0 + fine) return fail(EMAVFI_E_ARG, "%s: flow overlaps flow_s", what);
    EMAVFI_TRY(launch_coarse_up_f32(flow_s, flow, planes, H, W, s, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- agreement guard (include/emavfi.h, "AGREEMENT GUARD DEFINITION"): every check runs on the host; mean and std are read here and not kept
static_assert(EMAVFI_AGREEMENT_MAX_BATCH == AGREEMENT_MAX_BATCH, "header and agreement_elem.h disagree");

int emavfi_agreement_guard_f32(const float *u, const float *v, const float *a, const float *b, float *out, int B, int C, int H, int W,
                               int radius, float tol, const float *mean, const float *std, unsigned *counts, void *stream)
{
    const char *const what = "agreement_guard_f32";
    if (B < 1 || B > EMAVFI_AGREEMENT_MAX_BATCH) return fail(EMAVFI_E_ARG, "%s: B = %d (B must lie in 1..%d)", what, B, EMAVFI_AGREEMENT_MAX_BATCH);
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1..4)", what, C);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (radius < 0 || radius > EMAVFI_STATIC_MAX_RADIUS)
        return fail(EMAVFI_E_ARG, "%s: radius = %d (radius must lie in 0..%d)", what, radius, EMAVFI_STATIC_MAX_RADIUS);
    if (!agreement_tol_ok(tol)) return fail(EMAVFI_E_ARG, "%s: tol = %g (tol must lie in 0..1)", what, (double)tol);
    size_t bytes;                                         // at most 65535 * 4 * 16384^2 * 4 < 2^48
    if (__builtin_mul_overflow((size_t)B * C, (size_t)H * W * sizeof(float), &bytes))
        return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (B %d)", what, B);
    if (!mean) return fail(EMAVFI_E_ARG, "%s: null pointer mean", what);
    if (!std) return fail(EMAVFI_E_ARG, "%s: null pointer std", what);
    for (int c = 0; c < C; ++c) {
        if (!(mean[c] - mean[c] == 0.0f)) return fail(EMAVFI_E_ARG, "%s: mean[%d] must be finite", what, c);
        if (!agreement_std_ok(std[c])) return fail(EMAVFI_E_ARG, "%s: std[%d] must be finite and non-zero", what, c);
    }
    const struct { const char *name; const void *p; } in[4] = {{"u", u}, {"v", v}, {"a", a}, {"b", b}};
    for (int k = 0; k < 4; ++k)
        if (const int rc = ensemble_pointer_check(what, in[k].name, -1, in[k].p, bytes); rc != EMAVFI_OK) return rc;
    if (const int rc = ensemble_pointer_check(what, "out", -1, out, bytes); rc != EMAVFI_OK) return rc;
    if ((uintptr_t)counts & 3) return fail(EMAVFI_E_ARG, "%s: the u32 pointer counts must be 4-byte aligned", what);
    const uintptr_t o0 = (uintptr_t)out;
    for (int k = 0; k < 4; ++k) {
        const uintptr_t i0 = (uintptr_t)in[k].p;
        if (o0 < i0 + bytes && i0 < o0 + bytes) return fail(EMAVFI_E_ARG, "%s: out overlaps %s", what, in[k].name);
    }
    EMAVFI_TRY(launch_agreement_guard_f32(u, v, a, b, out, B, C, H, W, radius, tol, mean, std, counts, (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- frame metrics on the device (include/emavfi.h, "FRAME METRIC DEFINITION"): every check runs on the host, pointers are looked at last
static int metrics_shape_check(const char *what, int B, int H, int W, int C)
{
    if (B < 1) return fail(EMAVFI_E_ARG, "%s: B must be >= 1", what);
    if (B > 65535) return fail(EMAVFI_E_ARG, "%s: B = %d is above 65535", what, B);
    if (const int rc = scene_dims_check(what, H, W); rc != EMAVFI_OK) return rc;
    if (C < 1 || C > 4) return fail(EMAVFI_E_ARG, "%s: C = %d (C must be 1..4)", what, C);
    return EMAVFI_OK;
}

size_t emavfi_frame_metrics_workspace_bytes(int B, int H, int W, int C)
{
    if (metrics_shape_check("frame_metrics_workspace_bytes", B, H, W, C) != EMAVFI_OK) return 0;
    int tx, ty;
    frame_metrics_tiles(H, W, &tx, &ty);
    return (size_t)B * C * tx * ty * 2 * sizeof(unsigned long long);   // at most 65535 * 4 * 512 * 512 * 16 < 2^41
}

int emavfi_frame_metrics_u8(const unsigned char *a, size_t a_pitch, size_t a_batch_stride, const unsigned char *b, size_t b_pitch,
                            size_t b_batch_stride, int B, int H, int W, int C, long long *out, void *workspace, size_t workspace_bytes,
                            void *stream)
{
    const char *const what = "frame_metrics_u8";
    if (const int rc = metrics_shape_check(what, B, H, W, C); rc != EMAVFI_OK) return rc;
    const size_t row = (size_t)W * C;
    const size_t pitch[2] = {a_pitch, b_pitch}, bstride[2] = {a_batch_stride, b_batch_stride};
    for (int i = 0; i < 2; ++i) {
        const char *const side = i ? "b" : "a";
        if (pitch[i] < row) return fail(EMAVFI_E_ARG, "%s: the pitch of %s, %zu, is smaller than its row of %zu bytes", what, side, pitch[i], row);
        size_t plane, span;
        if (__builtin_mul_overflow((size_t)(H - 1), pitch[i], &plane) || __builtin_add_overflow(plane, row, &plane))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (pitch of %s %zu)", what, side, pitch[i]);
        if (B > 1 && bstride[i] < plane)
            return fail(EMAVFI_E_ARG, "%s: the batch stride of %s, %zu, is smaller than its plane", what, side, bstride[i]);
        if (B > 1 && (__builtin_mul_overflow((size_t)(B - 1), bstride[i], &span) || __builtin_add_overflow(span, plane, &span)))
            return fail(EMAVFI_E_ARG, "%s: the size arithmetic overflows (batch stride of %s %zu)", what, side, bstride[i]);
    }
    if (!a || !b || !out || !workspace) return fail(EMAVFI_E_ARG, "%s: null pointer", what);
    if (((uintptr_t)out | (uintptr_t)workspace) & 7) return fail(EMAVFI_E_ARG, "%s: out and the workspace must be 8-byte aligned", what);
    const size_t need = emavfi_frame_metrics_workspace_bytes(B, H, W, C);
    if (workspace_bytes < need) return fail(EMAVFI_E_WORKSPACE, "%s: workspace needs %zu bytes, got %zu", what, need, workspace_bytes);
    EMAVFI_TRY(launch_frame_metrics_u8(a, a_pitch, a_batch_stride, b, b_pitch, b_batch_stride, B, H, W, C, (unsigned long long *)out, (unsigned long long *)workspace,
                                       (hipStream_t)stream), what);
    return EMAVFI_OK;
}

// ---- stage-level entries (diagnostics / parity tests of single operators): one layer, packed into the workspace and run inside one call ----
// Their plan - the kernel storage type (EMAVFI_F32X3: the f16 kernels on [hi | lo] halves) and, from op_carve, the zero page - and
// their layer, as the plan of a model lays it out: a bf16 DCN on the LDS-window kernel contracts bf16-rounded weights stored as f16
static bool op_layer(Plan &P, Layer &L, bool deform, int Cin, int Cout, int stride, int dtype)
{
    P = Plan{};
    P.x3 = dtype == EMAVFI_F32X3; P.dtype = P.x3 ? (int)EMAVFI_F16 : dtype; P.esize = P.dtype == EMAVFI_F32 ? 4 : 2;
    L = mk(0, Cout, Cin, stride);
    if (!deform) return conv_geometry(L, P.esize, read_layout_env(), P.x3);   // (the layout switches per call: packs and runs inside one call)
    if (!deform_geometry(L, P.esize)) return false;
    if (dtype != EMAVFI_F32 && deform_pack3_shape(L.ck, L.nf, L.cin_take, L.cout)) L.pack3 = 1;
    if (dtype == EMAVFI_F32 && deform_f32w_shape(L.ck, L.nf, L.cin_take, L.cout)) L.pack3 = 3;
    L.f16_of_bf16 = dtype == EMAVFI_BF16 && L.pack3 == 1;
    return true;
}
// the workspace of both: channels-last input, offsets / masks (deformable), the packed layer - `packed` is the workspace itself, the
// layer's and the plan's offsets are relative to it -, channels-last output, zero page
struct OpBuffers { void *xcl, *ycl, *zpage; float *om; };
static OpBuffers op_carve(Plan &P, Layer &L, Workspace &ws, int B, int H, int W)
{
    const size_t e = (size_t)P.esize * (L.x3 ? 2 : 1), px = (size_t)B * H * W;   // (EMAVFI_F32X3 convolution: [hi | lo] halves per pixel)
    OpBuffers b{};
    b.xcl = ws.take(px * L.cin_pad * e);
    if (L.deform) b.om = (float *)ws.take(px * 32 * sizeof(float));
    L.w_off = ws.used; ws.take(L.w_bytes);
    L.b_off = ws.used; ws.take((size_t)L.coutpad * sizeof(float));
    b.ycl = ws.take((size_t)B * ((H + L.stride - 1) / L.stride) * ((W + L.stride - 1) / L.stride) * rup(L.cout, 16) * e);
    P.zero_off = ws.used; b.zpage = ws.take(256);
    return b;
}

size_t emavfi_conv3x3_workspace_bytes(int B, int Cin, int Cout, int H, int W, int stride, int dtype)
{
    Plan P;
    Layer L;
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || !op_layer(P, L, false, Cin, Cout, stride, dtype)) {
        fail(EMAVFI_E_UNSUPPORTED, "conv3x3: no kernel instantiation for Cin=%d Cout=%d stride=%d", Cin, Cout, stride);
        return 0;
    }
    Workspace ws{nullptr, 0, 0};
    op_carve(P, L, ws, B, H, W);
    return ws.used;
}

int emavfi_conv3x3(const float *x, const float *weight, const float *bias, float *y, int B, int Cin, int Cout, int H, int W,
                   int stride, int act, int dtype, void *workspace, size_t workspace_bytes, void *stream)
{
    if (dtype != EMAVFI_F32 && dtype != EMAVFI_BF16 && dtype != EMAVFI_F16 && dtype != EMAVFI_F32X3) return fail(EMAVFI_E_ARG, "conv3x3: bad dtype %d", dtype);
    if (!x || !weight || !y || !workspace) return fail(EMAVFI_E_ARG, "conv3x3: null pointer");
    if (B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return fail(EMAVFI_E_ARG, "conv3x3: bad shape");
    if (act < EMAVFI_ACT_NONE || act > EMAVFI_ACT_TANH01) return fail(EMAVFI_E_ARG, "conv3x3: bad activation %d", act);
    if (act == EMAVFI_ACT_TANH01 && Cout > 4) return fail(EMAVFI_E_UNSUPPORTED, "conv3x3: TANH01 epilogue needs Cout <= 4");
    Plan P;
    Layer L;
    if (!op_layer(P, L, false, Cin, Cout, stride, dtype))
        return fail(EMAVFI_E_UNSUPPORTED, "conv3x3: no kernel instantiation for Cin=%d Cout=%d stride=%d", Cin, Cout, stride);
    const bool x3 = P.x3;   // the three-term f16 split: [hi | lo] halves in, fp32-accurate result out; dtype: the kernel storage type from here on
    dtype = P.dtype;
    // the kernels' DMA source offsets inside one sample are 32-bit (conv3x3.inl, conv_dma_src)
    if ((size_t)H * W * L.cin_pad * P.esize >= ((size_t)1 << 32)) return fail(EMAVFI_E_ARG, "conv3x3: one sample's input plane must be < 4 GiB");
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride, ops = rup(Cout, 16);
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    const OpBuffers b = op_carve(P, L, ws, B, H, W);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "conv3x3: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const void *const params[2] = {weight, bias};
    EMAVFI_TRY(launch_clear_bytes(b.zpage, 256, s), "conv3x3: zero page clear");
    EMAVFI_TRY(pack_layer(L, params, workspace, dtype, s), "conv3x3 pack");
    EMAVFI_TRY(x3 ? launch_nchw_to_cl_x3(x, b.xcl, B, Cin, H, W, L.cin_pad, s) : launch_nchw_to_cl(x, b.xcl, B, Cin, H, W, L.cin_pad, dtype, s), "conv3x3 layout in");
    if (act == EMAVFI_ACT_TANH01) {
        EMAVFI_TRY(run_conv(P, L, workspace, B, s, ConvCall{}.from(b.xcl, L.cin_pad, H, W).act(EPI_PLANAR_TANH01).to_planes(y, Cout)), "conv3x3");
    } else {
        EMAVFI_TRY(run_conv(P, L, workspace, B, s, ConvCall{}.from(b.xcl, L.cin_pad, H, W).to(b.ycl, ops, ops).act(act == EMAVFI_ACT_RELU ? EPI_RELU : EPI_NONE)), "conv3x3");
        EMAVFI_TRY(x3 ? launch_cl_to_nchw_x3(b.ycl, y, B, Cout, Ho, Wo, ops, 0, s) : launch_cl_to_nchw(b.ycl, y, B, Cout, Ho, Wo, ops, 0, dtype, s), "conv3x3 layout out");
    }
    return EMAVFI_OK;
}

size_t emavfi_deform_conv2d_workspace_bytes(int B, int C, int O, int H, int W, int dtype)
{
    Plan P;
    Layer L;
    if (B < 1 || C < 1 || O < 1 || H < 1 || W < 1 || !op_layer(P, L, true, C, O, 1, dtype)) {
        fail(EMAVFI_E_UNSUPPORTED, "deform_conv2d: no kernel instantiation for C=%d O=%d", C, O);
        return 0;
    }
    if ((size_t)H * W >= ((size_t)1 << 24) || (size_t)H * W * L.ck * P.esize >= ((size_t)1 << 32)) {
        fail(EMAVFI_E_ARG, "deform_conv2d: H*W must be < 2^24 and one sample's input plane < 4 GiB");
        return 0;
    }
    Workspace ws{nullptr, 0, 0};
    op_carve(P, L, ws, B, H, W);
    return ws.used;
}

int emavfi_deform_conv2d(const float *x, const float *offset, const float *mask, const float *weight, const float *bias,
                         float *y, int B, int C, int O, int H, int W, int dtype, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    if (dtype != EMAVFI_F32 && dtype != EMAVFI_BF16 && dtype != EMAVFI_F16) return fail(EMAVFI_E_ARG, "deform_conv2d: bad dtype %d", dtype);
    if (!x || !offset || !mask || !weight || !y || !workspace) return fail(EMAVFI_E_ARG, "deform_conv2d: null pointer");
    if (B < 1 || C < 1 || O < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "deform_conv2d: bad shape");
    if ((size_t)H * W >= ((size_t)1 << 24)) return fail(EMAVFI_E_ARG, "deform_conv2d: H*W must be < 2^24");
    Plan P;
    Layer L;
    if (!op_layer(P, L, true, C, O, 1, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "deform_conv2d: no kernel instantiation for C=%d O=%d", C, O);
    if ((size_t)H * W * L.ck * P.esize >= ((size_t)1 << 32))
        return fail(EMAVFI_E_ARG, "deform_conv2d: one sample's input plane must be < 4 GiB (32-bit byte offsets in the gather)");
    const int ops = rup(O, 16);
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    const OpBuffers b = op_carve(P, L, ws, B, H, W);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "deform_conv2d: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const void *const params[2] = {weight, bias};
    EMAVFI_TRY(launch_clear_bytes(b.zpage, 256, s), "deform_conv2d: zero page clear");
    EMAVFI_TRY(pack_layer(L, params, workspace, dtype, s), "deform pack");
    EMAVFI_TRY(launch_nchw_to_cl(x, b.xcl, B, C, H, W, L.ck, dtype, s), "deform layout in");
    EMAVFI_TRY(launch_om_from_nchw(offset, mask, b.om, B, H, W, s), "deform offsets");
    EMAVFI_TRY(run_deform(P, L, workspace, B, s, DeformCall{}.from(b.xcl, L.ck, H, W, b.om).to(b.ycl, ops)), "deform_conv2d");
    EMAVFI_TRY(launch_cl_to_nchw(b.ycl, y, B, O, H, W, ops, 0, dtype, s), "deform layout out");
    return EMAVFI_OK;
}

// ---- ModulatedDeformConvPack.forward (ema_vfi.py:53-60) as ONE stage-level entry, routed through attention_block() - i.e. exactly as
// block i of emavfi_forward runs it: in the 16-bit modes at the reference width the one-launch kernel deform_pack3_kernel<T, FUSE_OFF = true>
// (offset_conv on the staged window, fast sigmoid, geometry, taps, fix-up), in fp32 conv3x3(EPI_OM) + the fp32 LDS-window DCN, under
// EMAVFI_AMP16 the fp16 offset_conv + fp32 DCN pair.  The model is EMA_VFI(3, C - 3, 1): the reference only ever builds this pack at
// mid_channels + 3 channels (ema_vfi.py:97).
static int mdcn_plan(Plan &P, int C, int dtype, int flags, bool &split, int &in_f16, int &out_f16)
{
    if (dtype == EMAVFI_F32X3) return fail(EMAVFI_E_UNSUPPORTED, "mdcn: EMAVFI_F32X3 has no stage entry of its own (its DCN samples in fp32 and, at the reference width, contracts on the three-term f16 split, as EMAVFI_AMP16's does; EMAVFI_F32 is the exact fp32 pack)");
    if (C < 11 || !build_plan(P, 3, C - 3, 1, dtype))
        return fail(EMAVFI_E_UNSUPPORTED, "mdcn: C = %d is not mid_channels + 3 of a supported model (%s)", C, C < 11 ? "C < 11" : P.why);
    if (flags & ~(EMAVFI_MDCN_IN_F16 | EMAVFI_MDCN_OUT_F16 | EMAVFI_MDCN_SPLIT_TAIL)) return fail(EMAVFI_E_ARG, "mdcn: unknown flag bits 0x%x", flags);
    split = (flags & EMAVFI_MDCN_SPLIT_TAIL) != 0;
    in_f16 = (flags & EMAVFI_MDCN_IN_F16) ? 1 : 0;
    out_f16 = (flags & EMAVFI_MDCN_OUT_F16) ? 1 : 0;
    const bool one_launch = pack_fuses(P, 0) && P.dcn[0].pack3 != 0;
    if ((in_f16 || out_f16) && !(one_launch && P.dtype == EMAVFI_BF16 && !P.amp))
        return fail(EMAVFI_E_UNSUPPORTED, "mdcn: the f16 hand-off flags belong to the bf16 one-launch pack (C = 65..67)");
    if (split && !(pack_fuses(P, 0) && P.fpad - P.mid == 16)) return fail(EMAVFI_E_UNSUPPORTED, "mdcn: the split tail belongs to the one-launch pack");
    return EMAVFI_OK;
}

struct MdcnBuffers { void *blob, *xcl, *tail, *ycl; float *om, *xF, *yF; unsigned *census; };
static void mdcn_carve(const Plan &P, Workspace &ws, MdcnBuffers &m, int B, int H, int W, bool split)
{
    const size_t px = (size_t)B * H * W;
    m.blob = ws.take(P.total);
    m.xcl = ws.take(px * P.fps * P.esize);
    m.tail = split ? ws.take(px * 8 * P.esize) : nullptr;
    m.ycl = ws.take(px * P.fps * P.esize);
    m.om = (float *)ws.take(px * 32 * sizeof(float));
    m.xF = m.yF = nullptr;
    if (P.amp) {
        m.xF = (float *)ws.take(px * P.fpad * sizeof(float));
        m.yF = (float *)ws.take(px * P.fpad * sizeof(float));
    }
    m.census = (unsigned *)ws.take(kCensusBlock);
}

size_t emavfi_mdcn_workspace_bytes(int B, int C, int H, int W, int dtype, int flags)
{
    Plan P;
    bool split; int in_f16, out_f16;
    if (mdcn_plan(P, C, dtype, flags, split, in_f16, out_f16) != EMAVFI_OK) return 0;
    if (B < 1 || H < 1 || W < 1) { fail(EMAVFI_E_ARG, "mdcn: B, H, W must be >= 1"); return 0; }
    Workspace ws{nullptr, 0, 0};
    MdcnBuffers m;
    mdcn_carve(P, ws, m, B, H, W, split);
    return ws.used;
}

static int mdcn_impl(const float *x, const float *offset_weight, const float *offset_bias, const float *dcn_weight, const float *dcn_bias, float *y,
                     int B, int C, int H, int W, int dtype, int flags, void *workspace, size_t workspace_bytes, void *stream, Recorder &rec,
                     int route = EMAVFI_ROUTE_WINDOW)
{
    Plan P;
    bool split; int in_f16, out_f16;
    if (const int rc = mdcn_plan(P, C, dtype, flags, split, in_f16, out_f16); rc != EMAVFI_OK) return rc;
    if (route != EMAVFI_ROUTE_WINDOW && route != EMAVFI_ROUTE_GATHER) return fail(EMAVFI_E_ARG, "mdcn: unknown route %d", route);
    if (route == EMAVFI_ROUTE_GATHER)
        if (const int rc = require_gather_route(P, 0, "mdcn"); rc != EMAVFI_OK) return rc;
    if (!x || !offset_weight || !offset_bias || !dcn_weight || !y || !workspace) return fail(EMAVFI_E_ARG, "mdcn: null pointer");
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "mdcn: B, H, W must be >= 1");
    if (!aligned16(x) || !aligned16(y) || !aligned16(workspace)) return fail(EMAVFI_E_ARG, "mdcn: pointers must be 16-byte aligned");
    if ((size_t)B * H * W >= ((size_t)1 << 31) || (size_t)H * W >= ((size_t)1 << 24)) return fail(EMAVFI_E_ARG, "mdcn: B*H*W must be < 2^31 and H*W < 2^24");
    if ((size_t)H * W * P.fpad * (P.amp ? sizeof(float) : (size_t)P.esize) >= ((size_t)1 << 32)) return fail(EMAVFI_E_ARG, "mdcn: one sample's activation plane must be < 4 GiB");
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    MdcnBuffers m;
    mdcn_carve(P, ws, m, B, H, W, split);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "mdcn: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int kd = P.dtype, mid = P.mid;   // kernel storage type
    // pack the two layers exactly as emavfi_pack_weights packs attention_blocks.0 (both offset_conv copies where the plan has them)
    std::vector<const void *> params((size_t)emavfi_param_count(1), nullptr);
    params[P.off[0].param] = offset_weight; params[P.off[0].param + 1] = offset_bias;
    params[P.dcn[0].param] = dcn_weight; params[P.dcn[0].param + 1] = dcn_bias;
    EMAVFI_TRY(launch_clear_bytes(m.blob, P.total, s), "mdcn: blob clear");
    EMAVFI_TRY(launch_clear_bytes(m.census, kCensusBlock, s), "mdcn: census clear");
    EMAVFI_TRY(pack_layer(P.off[0], params.data(), m.blob, kd, s, P.amp), "mdcn pack offset_conv");
    if (P.has_offh) EMAVFI_TRY(pack_layer(P.offh[0], params.data(), m.blob, kd, s), "mdcn pack offset_conv (f16 fragments)");
    EMAVFI_TRY(pack_layer(P.dcn[0], params.data(), m.blob, kd, s), "mdcn pack dcn_v2");
    if (P.amp) EMAVFI_TRY(pack_layer(P.dcn32[0], params.data(), m.blob, kd, s), "mdcn pack dcn_v2 (fp32 master weights)");
    if (P.amp) {
        EMAVFI_TRY(launch_nchw_to_cl(x, m.xF, B, C, H, W, P.fpad, EMAVFI_F32, s), "mdcn layout in (fp32)");
        EMAVFI_TRY(launch_nchw_to_cl(x, m.xcl, B, C, H, W, P.fps, EMAVFI_F16, s), "mdcn layout in (fp16 rounding)");
        if (const int rc = attention_block_amp(P, 0, m.blob, m.xcl, m.xF, m.yF, false, nullptr, m.om, B, H, W, s, rec); rc != EMAVFI_OK) return rc;
        EMAVFI_TRY(launch_cl_to_nchw(m.yF, y, B, C, H, W, P.fpad, 0, EMAVFI_F32, s), "mdcn layout out");
        return EMAVFI_OK;
    }
    const int xdt = in_f16 ? (int)EMAVFI_F16 : kd, ydt = out_f16 ? (int)EMAVFI_F16 : kd;
    if (split) {   // the first pack's input form: channels 0..mid-1 in the fusion pixels, channels mid.. in the compact tail buffer
        EMAVFI_TRY(launch_nchw_to_cl_sub(x, m.xcl, B, C, 0, mid, H, W, P.fps, xdt, s), "mdcn layout in");
        EMAVFI_TRY(launch_nchw_to_cl_sub(x, m.tail, B, C, mid, C - mid, H, W, kTailPs, xdt, s), "mdcn layout in (tail)");
    } else {
        EMAVFI_TRY(launch_nchw_to_cl(x, m.xcl, B, C, H, W, P.fps, xdt, s), "mdcn layout in");
    }
    if (const int rc = attention_block(P, 0, m.blob, m.xcl, m.ycl, m.om, m.tail, in_f16, out_f16, B, H, W, s, rec, m.census, PackRoute{route}); rc != EMAVFI_OK)
        return rc;
    EMAVFI_TRY(launch_cl_to_nchw(m.ycl, y, B, C, H, W, P.fps, 0, ydt, s), "mdcn layout out");
    return EMAVFI_OK;
}

int emavfi_mdcn(const float *x, const float *offset_weight, const float *offset_bias, const float *dcn_weight, const float *dcn_bias, float *y,
                int B, int C, int H, int W, int dtype, int flags, void *workspace, size_t workspace_bytes, void *stream)
{
    Recorder rec;
    return mdcn_impl(x, offset_weight, offset_bias, dcn_weight, dcn_bias, y, B, C, H, W, dtype, flags, workspace, workspace_bytes, stream, rec);
}

int emavfi_mdcn_routed(const float *x, const float *offset_weight, const float *offset_bias, const float *dcn_weight, const float *dcn_bias, float *y,
                       int B, int C, int H, int W, int dtype, int flags, int route, void *workspace, size_t workspace_bytes, void *const *events,
                       int n_events, void *stream)
{
    Recorder rec;
    if (const int rc = set_events(rec, events, n_events, "mdcn_routed"); rc != EMAVFI_OK) return rc;
    return mdcn_impl(x, offset_weight, offset_bias, dcn_weight, dcn_bias, y, B, C, H, W, dtype, flags, workspace, workspace_bytes, stream, rec, route);
}

// ---- census of the one-launch packs (round 6): what deform_pack3_kernel itself counted while it ran - the (wave, tap)
// groups that took the fix-up, the samples outside the staged window, the largest |offset| - reduced over the launch's 64 atomic slots
// into out[block][4] (u64, DEVICE memory): {fix-up wave-taps, all wave-taps, samples outside, max |offset| as fp32 bits}.  All wave-taps
// is 0 for a block that did not run the one-launch kernel (fp32 / autocast modes, other widths): nothing was counted.

int emavfi_forward_census(int in_channels, int mid_channels, int num_blocks, int B, int H, int W, int dtype, const void *workspace,
                          size_t workspace_bytes, unsigned long long *out, void *stream)
{
    Plan P;
    if (!build_plan(P, in_channels, mid_channels, num_blocks, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s", P.why);
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "forward_census: B, H, W must be >= 1");
    if (!workspace || !out) return fail(EMAVFI_E_ARG, "forward_census: null pointer");
    Workspace ws{(char *)const_cast<void *>(workspace), workspace_bytes, 0};
    FwdBuffers f;
    carve_forward(P, ws, f, B, H, W);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "forward_census: this forward's workspace has %zu bytes, got %zu", ws.used, workspace_bytes);
    unsigned long long totals[kMaxBlocks] = {};
    for (int i = 0; i < P.nb; ++i) totals[i] = pack_gather_ok(P, i) ? pack3_wave_taps(B, H, W) : 0ull;
    EMAVFI_TRY(launch_census_reduce(f.census, out, P.nb, totals, (hipStream_t)stream), "forward_census");
    return EMAVFI_OK;
}

int emavfi_mdcn_census(int B, int C, int H, int W, int dtype, int flags, const void *workspace, size_t workspace_bytes, unsigned long long *out, void *stream)
{
    Plan P;
    bool split; int in_f16, out_f16;
    if (const int rc = mdcn_plan(P, C, dtype, flags, split, in_f16, out_f16); rc != EMAVFI_OK) return rc;
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "mdcn_census: B, H, W must be >= 1");
    if (!workspace || !out) return fail(EMAVFI_E_ARG, "mdcn_census: null pointer");
    Workspace ws{(char *)const_cast<void *>(workspace), workspace_bytes, 0};
    MdcnBuffers m;
    mdcn_carve(P, ws, m, B, H, W, split);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "mdcn_census: this stage's workspace has %zu bytes, got %zu", ws.used, workspace_bytes);
    unsigned long long totals[kMaxBlocks] = {};
    totals[0] = pack_gather_ok(P, 0) ? pack3_wave_taps(B, H, W) : 0ull;
    EMAVFI_TRY(launch_census_reduce(m.census, out, 1, totals, (hipStream_t)stream), "mdcn_census");
    return EMAVFI_OK;
}

// ---- context_encoding and reconstruction as stage-level entries (SURVEY 8b's proposed emavfi_context / emavfi_reconstruct): the model is
// EMA_VFI(3, mid_channels, 3) - the stage does not depend on num_blocks -, the layers are packed and run exactly as emavfi_forward
// packs and runs them (context_stage / reconstruction_stage above), the tensors cross the boundary as NCHW fp32.
static int stage_plan(Plan &P, int mid, int dtype, int B, int H, int W, const char *what)
{
    if (dtype == EMAVFI_F32X3) return fail(EMAVFI_E_UNSUPPORTED, "%s: EMAVFI_F32X3 has stage entries for conv3x3 only", what);
    if (!build_plan(P, 3, mid, 3, dtype)) return fail(EMAVFI_E_UNSUPPORTED, "%s: %s", what, P.why);
    if (B < 1 || H < 1 || W < 1) return fail(EMAVFI_E_ARG, "%s: B, H, W must be >= 1", what);
    if ((size_t)B * H * W >= ((size_t)1 << 31) || (size_t)H * W >= ((size_t)1 << 24) || (size_t)H * W * P.fpad * (P.amp ? sizeof(float) : (size_t)P.esize) >= ((size_t)1 << 32))
        return fail(EMAVFI_E_ARG, "%s: B*H*W must be < 2^31, H*W < 2^24 and one sample's activation plane < 4 GiB", what);
    return EMAVFI_OK;
}
struct StageBuffers { void *blob; float *zeros9; FwdBuffers f; };
static void stage_carve(const Plan &P, Workspace &ws, StageBuffers &b, int B, int H, int W)
{
    b.blob = ws.take(P.total);
    b.zeros9 = (float *)ws.take(((size_t)P.mid * 2 * P.mid * 9 + P.mid) * sizeof(float));   // a zero motion_estimation.0 for the context fold
    carve_forward(P, ws, b.f, B, H, W);
}

size_t emavfi_context_workspace_bytes(int B, int mid_channels, int H, int W, int dtype)
{
    Plan P;
    if (stage_plan(P, mid_channels, dtype, B, H, W, "context") != EMAVFI_OK) return 0;
    Workspace ws{nullptr, 0, 0};
    StageBuffers b;
    stage_carve(P, ws, b, B, H, W);
    return ws.used;
}

int emavfi_context(const float *feat, const float *const *params, float *ctx, int B, int mid_channels, int H, int W, int dtype,
                   void *workspace, size_t workspace_bytes, void *stream)
{
    Plan P;
    if (const int rc = stage_plan(P, mid_channels, dtype, B, H, W, "context"); rc != EMAVFI_OK) return rc;
    if (!feat || !params || !ctx || !workspace) return fail(EMAVFI_E_ARG, "context: null pointer");
    for (int i = 0; i < 8; ++i)
        if (!params[i]) return fail(EMAVFI_E_ARG, "context: params[%d] is null", i);
    if (!aligned16(feat) || !aligned16(workspace)) return fail(EMAVFI_E_ARG, "context: pointers must be 16-byte aligned");
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    StageBuffers b;
    stage_carve(P, ws, b, B, H, W);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "context: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int kd = P.dtype, mid = P.mid;
    std::vector<const void *> all((size_t)emavfi_param_count(3), nullptr);
    all[P.c0.param] = params[0]; all[P.c0.param + 1] = params[1];
    all[P.c1.param] = params[2]; all[P.c1.param + 1] = params[3];
    all[P.c2.param] = params[4]; all[P.c2.param + 1] = params[5];
    EMAVFI_TRY(launch_clear_bytes(b.blob, P.total, s), "context: blob clear");
    EMAVFI_TRY(launch_clear_bytes(b.zeros9, ((size_t)mid * 2 * mid * 9 + mid) * sizeof(float), s), "context: zero weights clear");
    EMAVFI_TRY(pack_layer(P.c0, all.data(), b.blob, kd, s, P.amp), "context pack 0");
    EMAVFI_TRY(pack_layer(P.c1, all.data(), b.blob, kd, s, P.amp), "context pack 1");
    EMAVFI_TRY(pack_layer(P.c2, all.data(), b.blob, kd, s, P.amp), "context pack 2");
    EMAVFI_TRY(launch_pack_ctx(params[6], params[7], b.zeros9, b.zeros9 + (size_t)mid * 2 * mid * 9, (float *)((char *)b.blob + P.ctx_off), mid, P.amp ? 1 : 0, s),
               "context pack linear");
    // `feat` as the forward stores it: channels 0..mid-1 of the fusion pixels, f16 in the bf16 model with the one-launch packs (Plan::feat16)
    EMAVFI_TRY(launch_nchw_to_cl(feat, b.f.fu0, B, mid, H, W, P.fps, P.feat16 ? (int)EMAVFI_F16 : kd, s), "context layout in");
    Recorder rec;
    if (const int rc = context_stage(P, b.blob, b.f.fu0, b.f, B, H, W, s, rec); rc != EMAVFI_OK) return rc;
    if (hipMemcpyAsync(ctx, b.f.ctx, (size_t)B * mid * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(EMAVFI_E_LAUNCH, "context: copy out failed");
    return EMAVFI_OK;
}

size_t emavfi_reconstruct_workspace_bytes(int B, int mid_channels, int H, int W, int dtype)
{
    return emavfi_context_workspace_bytes(B, mid_channels, H, W, dtype);   // the same carving
}

int emavfi_reconstruct(const float *fused, const float *const *params, float *out, int B, int mid_channels, int H, int W, int dtype,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    Plan P;
    if (const int rc = stage_plan(P, mid_channels, dtype, B, H, W, "reconstruct"); rc != EMAVFI_OK) return rc;
    if (!fused || !params || !out || !workspace) return fail(EMAVFI_E_ARG, "reconstruct: null pointer");
    for (int i = 0; i < 6; ++i)
        if (!params[i]) return fail(EMAVFI_E_ARG, "reconstruct: params[%d] is null", i);
    if (!aligned16(fused) || !aligned16(out) || !aligned16(workspace)) return fail(EMAVFI_E_ARG, "reconstruct: pointers must be 16-byte aligned");
    Workspace ws{(char *)workspace, workspace_bytes, 0};
    StageBuffers b;
    stage_carve(P, ws, b, B, H, W);
    if (ws.used > workspace_bytes) return fail(EMAVFI_E_WORKSPACE, "reconstruct: workspace needs %zu bytes, got %zu", ws.used, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int kd = P.dtype, mid = P.mid;
    std::vector<const void *> all((size_t)emavfi_param_count(3), nullptr);
    all[P.r0.param] = params[0]; all[P.r0.param + 1] = params[1];
    all[P.r1.param] = params[2]; all[P.r1.param + 1] = params[3];
    all[P.r2.param] = params[4]; all[P.r2.param + 1] = params[5];
    EMAVFI_TRY(launch_clear_bytes(b.blob, P.total, s), "reconstruct: blob clear");
    EMAVFI_TRY(pack_layer(P.r0, all.data(), b.blob, kd, s, P.amp), "reconstruct pack 0");
    EMAVFI_TRY(pack_layer(P.r1, all.data(), b.blob, kd, s, P.amp), "reconstruct pack 1");
    EMAVFI_TRY(pack_layer(P.r2, all.data(), b.blob, kd, s, P.amp), "reconstruct pack 2");
    // the fusion tensor as the last attention block leaves it: mid + 3 channels in P.fps-channel pixels of the storage type
    EMAVFI_TRY(launch_nchw_to_cl(fused, b.f.fu0, B, mid + 3, H, W, P.fps, kd, s), "reconstruct layout in");
    Recorder rec;
    return reconstruction_stage(P, b.blob, b.f.fu0, b.f, out, B, H, W, s, rec);
}

}  // extern "C"
