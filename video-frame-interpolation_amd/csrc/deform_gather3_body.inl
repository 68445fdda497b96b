// The body of deform_gather3_kernel<TS> (deform_gather3.inl), the WINDOW-FREE route, in a file of its own because the routed pack
// (deform_route3.inl) runs it as its gather branch.  Included inside a function body that defines TS and the DeformParams `p`.  The
// stages it has in common with the window body are included from deform3_stages.inl (deform3_shared.inl).
    using C = Gather3;
    static_assert(sizeof(TS) == 2, "16-bit storage types only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lds_cchar_t *lds_r = (lds_cchar_t *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int H = p.H, W = p.W;
    const unsigned lane16 = (unsigned)lane * 16u;

#define DEFORM3_STAGE DEFORM3_TILE
#include "deform3_stages.inl"
    const unsigned ps_bytes = (unsigned)p.x_ps * 2u, tail_bytes = (unsigned)p.tail_ps * 2u;
    const int ty0 = tile_y * C::TROWS - 1, tx0 = tile_x * C::TCOLS - 1;                      // staged halo window
    const int wy0 = tile_y * C::TROWS - 1 - Pack3::R, wx0 = tile_x * C::TCOLS - 1 - Pack3::R;  // the window route's window (census only)
    const char *gplane = (const char *)p.x + (size_t)b * H * W * ps_bytes;
    const char *tplane = p.x_tail ? (const char *)p.x_tail + (size_t)b * H * W * tail_bytes : nullptr;
    const char *zeros = (const char *)p.zeros;
    const char *wbase_g = (const char *)p.w;
    const char *owbase_g = (const char *)p.off_w;
    const unsigned npx = (unsigned)H * (unsigned)W;
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(gplane), 0, (int)(npx * ps_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_t =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(tplane ? tplane : gplane), 0, (int)(npx * (tplane ? tail_bytes : ps_bytes)), 0x00020000);
    const unsigned t_ps = tplane ? tail_bytes : ps_bytes, t_off = tplane ? 0u : 128u;   // tail record of pixel i: t_ps * i + t_off in rs_t
    const bool convert = std::is_same<TS, bf16_t>::value && !p.in_f16;

    f16x8 ow[3][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) ow[t][kg] = *reinterpret_cast<const f16x8 *>(owbase_g + (t * 4 + kg) * 1024 + lane16);

    // ---- stage the 18 x 18 window: load k of wave w fetches 16-byte pieces [64 (4k + w), 64 (4k + w) + 64) of the window in memory order
    // (pixel-major, 9 pieces per pixel) into registers; out-of-image pixels read the zero page, pieces past the window are masked off.
    // Plain loads and LDS stores, not LDS-DMA: the bf16 -> f16 conversion happens on the way (to_f16_piece, as in the window route's
    // in-LDS pass, so the same f16 values), and the kernel has no DMA whose completion it would have to count.
    constexpr int NK = (C::NCHUNK + 3) / 4;
    u32x4_t stage[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int chunk = 4 * k + wave, pi = chunk * 64 + lane;
        if (chunk < C::NCHUNK && pi < C::NPIECE) {
            const int px = pi / C::SP, pc = pi - px * C::SP, ly = px / C::TC, lx = px - ly * C::TC;
            const int gy = ty0 + ly, gx = tx0 + lx;
            const bool ok = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            const long long pix = (long long)gy * W + gx;
            const char *src = !ok ? zeros : (tplane && pc == C::SP - 1) ? tplane + pix * (long long)tail_bytes : gplane + pix * (long long)ps_bytes + pc * 16;
            stage[k] = *reinterpret_cast<const u32x4_t *>(src);
        }
    }
    // the third fragment's A operands (4 608 B = 288 pieces)
    const u32x4_t w3a0 = *reinterpret_cast<const u32x4_t *>(wbase_g + C::DCN_W3 + tid * 16);
    const u32x4_t w3a1 = tid < 32 ? *reinterpret_cast<const u32x4_t *>(wbase_g + C::DCN_W3 + 4096 + tid * 16) : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int chunk = 4 * k + wave, pi = chunk * 64 + lane;
        if (chunk < C::NCHUNK && pi < C::NPIECE)
            *reinterpret_cast<__attribute__((address_space(3))) u32x4_t *>((lds_char_t *)smem + chunk * 1024 + lane16) =
                convert ? to_f16_piece<TS>(stage[k]) : stage[k];
    }
    *reinterpret_cast<__attribute__((address_space(3))) u32x4_t *>((lds_char_t *)smem + C::W3_OFF + tid * 16) = w3a0;
    if (tid < 32) *reinterpret_cast<__attribute__((address_space(3))) u32x4_t *>((lds_char_t *)smem + C::W3_OFF + 4096 + tid * 16) = w3a1;

#define DEFORM3_STAGE DEFORM3_LANE
#include "deform3_stages.inl"
    constexpr int HALO = 0;
#define DEFORM3_STAGE DEFORM3_LANE_CONST
#include "deform3_stages.inl"
    __syncthreads();

    // ---- offset_conv and the mask's sigmoid on the staged window
    f32x16 omr[2];
    constexpr bool KG0_ONLY = false;
#define DEFORM3_STAGE DEFORM3_OFFSET_CONV
#include "deform3_stages.inl"

#define DEFORM3_STAGE DEFORM3_ACC_INIT
#include "deform3_stages.inl"

    // ---- sampling geometry of all nine taps.  Per tap a lane keeps three words - in LDS, in the window
    // that offset_conv no longer reads (27 KiB: registers are what limits this kernel, the tap loop reads them once per tap):
    //   GM0: corner descriptor = clamped top-left pixel index | x1 - x0 << 24 | y1 - y0 << 25 | validity of the 4 corners << 26
    //   GM1 / GM2: the corner weights (w00, w01) | (w10, w11) as f16 pairs, NOT validity-masked: an out-of-image corner reads 0, which
    //   is what the window route's window holds there
    typedef __attribute__((address_space(3))) unsigned lds_u32_t;
    lds_u32_t *gm = reinterpret_cast<lds_u32_t *>((lds_char_t *)smem) + tid;   // word (tap, k) at gm[(3 tap + k) * 256]
    __syncthreads();   // every wave has left offset_conv: the window is dead
    unsigned lane_fb = 0, fb_taps = 0;   // census: samples the window route would have parked for its fix-up
    float omax = 0.0f;
    unsigned tl[12][2];
#pragma unroll
    for (int t = 9; t < 12; ++t) tl[t][0] = tl[t][1] = 0u;
    // corner c's byte offset (record stride ps, +off) of descriptor d, BAD for an out-of-image corner
    auto corner_off = [&](unsigned d, int c, unsigned ps, unsigned off) -> unsigned {
        const unsigned idx = (d & 0xffffffu) + ((c & 1) ? ((d >> 24) & 1u) : 0u) + ((c & 2) && ((d >> 25) & 1u) ? (unsigned)W : 0u);
        return ((d >> (26 + c)) & 1u) ? __umul24(idx, ps) + off : C::BAD;
    };
    auto geom_tap = [&](auto tc) {
        constexpr int tap = decltype(tc)::value, ti = tap / 3, tj = tap - 3 * ti;
        OmTap o;
#define DEFORM3_STAGE DEFORM3_PICK
#include "deform3_stages.inl"
        constexpr bool CENSUS = true, PIN = true;
#define DEFORM3_STAGE DEFORM3_SAMPLE
#include "deform3_stages.inl"
        // census: would the window route's 23 x 23 window have held all four corners?
        const int ly0 = hl - wy0, lx0 = wl - wx0;
        const bool inside = (unsigned)ly0 <= (unsigned)(Pack3::TR - 2) && (unsigned)lx0 <= (unsigned)(Pack3::TC - 2);
        const bool need_fb = !EMAVFI_DEFORM_ABL_NO_FALLBACK && !inside && my_in;
        lane_fb |= need_fb ? 1u << tap : 0u;
        fb_taps |= __any(need_fb) ? 1u << tap : 0u;
        typedef unsigned valid_t;
#define DEFORM3_STAGE DEFORM3_CORNERS
#include "deform3_stages.inl"
#define DEFORM3_STAGE DEFORM3_CORNER_DESC
#include "deform3_stages.inl"
        const unsigned d = cdesc | ((vhl & vwl) << 26) | ((vhl & vwh) << 27) | ((vhh & vwl) << 28) | ((vhh & vwh) << 29);
        const unsigned w01h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[0], (half_t)w4[1]});
        const unsigned w23h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[2], (half_t)w4[3]});
        gm[(3 * tap + 0) * C::THREADS] = d; gm[(3 * tap + 1) * C::THREADS] = w01h; gm[(3 * tap + 2) * C::THREADS] = w23h;
        // tail of this half-lane's own pixel: four 8-byte corner reads
        u32x4_t vt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x2_t t2 = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(rs_t, corner_off(d, c, t_ps, t_off), 0, 0));
            vt[c] = u32x4_t{t2[0], t2[1], 0u, 0u};
            if (convert) vt[c] = to_f16_piece<TS>(vt[c]);
        }
        const u32x4_t td = __builtin_bit_cast(u32x4_t, blend_corners<2>(vt, w01h, w23h));
        tl[tap][0] = td[0]; tl[tap][1] = td[1];
    };
    geom_tap(std::integral_constant<int, 0>{}); geom_tap(std::integral_constant<int, 1>{}); geom_tap(std::integral_constant<int, 2>{});
    geom_tap(std::integral_constant<int, 3>{}); geom_tap(std::integral_constant<int, 4>{}); geom_tap(std::integral_constant<int, 5>{});
    geom_tap(std::integral_constant<int, 6>{}); geom_tap(std::integral_constant<int, 7>{}); geom_tap(std::integral_constant<int, 8>{});

#define DEFORM3_STAGE DEFORM3_TAIL_MMA
#include "deform3_stages.inl"

    // ---- 9 taps x 4 k-groups x 2 rows, step s = 2 kg + m (the window route's order per accumulator).  The corner pieces of step s travel four
    // steps ahead in a ring of four operand buffers; steps 4..7 of a tap fetch steps 0..3 of the next one.
    // byte offsets of the four corners of pixel r of fragment row m (lane half h: its piece), for tap t
    auto tap_offs = [&](int t, unsigned (&o)[2][4]) {
        const unsigned d = gm[3 * t * C::THREADS];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned own = corner_off(d, c, ps_bytes, 0u);
            const auto sw = __builtin_amdgcn_permlane32_swap(own, own, false, false);   // {row 0's, row 1's} in both halves
            o[0][c] = sw[0] + (unsigned)(h * 16);
            o[1][c] = sw[1] + (unsigned)(h * 16);
        }
    };
    auto issue = [&](const unsigned (&o)[2][4], int s, u32x4_t (&d)[4]) {
        const int kg = s >> 1, m = s & 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) d[c] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_x, o[m][c] + (unsigned)(kg * 32), 0, 0));
    };
    unsigned ocur[2][4], onxt[2][4];
    u32x4_t vb[4][4];
    tap_offs(0, ocur);
#pragma unroll
    for (int s = 0; s < 4; ++s) issue(ocur, s, vb[s]);
    f16x8 wq[2][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) wq[0][n] = *reinterpret_cast<const f16x8 *>(wbase_g + n * 1024 + lane16);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const char *wtap = wbase_g + (size_t)tap * C::DCN_TAP;
        unsigned w01[2], w23[2];
        {
            const unsigned g1 = gm[(3 * tap + 1) * C::THREADS], g2 = gm[(3 * tap + 2) * C::THREADS];
            const auto s1 = __builtin_amdgcn_permlane32_swap(g1, g1, false, false);
            const auto s2 = __builtin_amdgcn_permlane32_swap(g2, g2, false, false);
            w01[0] = s1[0]; w01[1] = s1[1]; w23[0] = s2[0]; w23[1] = s2[1];
        }
        const unsigned w3a = w3lane + (unsigned)(tap * C::W3_TAP);
        const bool more = tap < 8;
        f16x8 w3 = {};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kg = s >> 1, m = s & 1;
            if (s == 4 && more) tap_offs(tap + 1, onxt);
            if (m == 0) {
                w3 = __builtin_bit_cast(f16x8, lds_read16(lds_r + w3a + (unsigned)(kg * 128)));
                if (kg + 1 < 4) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) wq[(kg + 1) & 1][n] = *reinterpret_cast<const f16x8 *>(wtap + ((kg + 1) * 2 + n) * 1024 + lane16);
                } else if (more) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) wq[0][n] = *reinterpret_cast<const f16x8 *>(wtap + C::DCN_TAP + n * 1024 + lane16);
                }
            }
            u32x4_t (&d)[4] = vb[s & 3];
            if (convert) {
#pragma unroll
                for (int c = 0; c < 4; ++c) d[c] = to_f16_piece<TS>(d[c]);
            }
            const f16x8 xf = blend_corners<4>(d, w01[m], w23[m]);
            if (s < 4) issue(ocur, s + 4, d);
            else if (more) issue(onxt, s - 4, d);
            mma_kg(acc[m][0], wq[kg & 1][0], xf);
            mma_kg(acc[m][1], wq[kg & 1][1], xf);
            mma_k32(acc3[m], w3, xf);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int c = 0; c < 4; ++c) ocur[m][c] = onxt[m][c];
    }

    // ---- census: only a wave with a sample beyond the window route's window pays for it
    if (__builtin_expect(fb_taps != 0, 0) && p.census) {
        unsigned n_parked = 0;
#define DEFORM3_STAGE DEFORM3_COUNT_PARKED
#include "deform3_stages.inl"
#define DEFORM3_STAGE DEFORM3_CENSUS_RECORD
#include "deform3_stages.inl"
    }

#define DEFORM3_STAGE DEFORM3_EPILOGUE
#include "deform3_stages.inl"
