// The body of deform_gather3_kernel<TS> (deform_gather3.inl), in a file of its own for the same reason as deform_pack3_body.inl: the
// routed pack (deform_route3.inl) runs it as its gather branch.  Included inside a function body that defines TS and the DeformParams `p`.
    using C = Gather3;
    static_assert(sizeof(TS) == 2, "16-bit storage types only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lds_cchar_t *lds_r = (lds_cchar_t *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int H = p.H, W = p.W;
    const unsigned lane16 = (unsigned)lane * 16u;

    // ---- tile of this workgroup (the pack's XCD-aware order)
    const int ntx = (W + C::TCOLS - 1) / C::TCOLS, nty = (H + C::TROWS - 1) / C::TROWS, nt = ntx * nty;
    int tile_x, tile_y, b;
    {
        constexpr int SROWS = 4;
        const int nwg = gridDim.x, grp = blockIdx.x & 7, kk = blockIdx.x >> 3, qq = nwg >> 3, rr = nwg & 7;
        const int wg = (grp < rr ? grp * (qq + 1) : rr * (qq + 1) + (grp - rr) * qq) + kk;
        b = wg / nt;
        const int t = wg - b * nt, strip = t / (SROWS * ntx), tt = t - strip * SROWS * ntx;
        const int rows = min(SROWS, nty - strip * SROWS);
        tile_x = tt / rows;
        tile_y = strip * SROWS + (tt - tile_x * rows);
    }
    const unsigned ps_bytes = (unsigned)p.x_ps * 2u, tail_bytes = (unsigned)p.tail_ps * 2u;
    const int ty0 = tile_y * C::TROWS - 1, tx0 = tile_x * C::TCOLS - 1;                      // staged halo window
    const int wy0 = tile_y * C::TROWS - 1 - Pack3::R, wx0 = tile_x * C::TCOLS - 1 - Pack3::R;  // the pack's window (census only)
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
    // Plain loads and LDS stores, not LDS-DMA: the bf16 -> f16 conversion happens on the way (the same conversion as the pack's in-LDS
    // pass, so the same f16 values), and the kernel has no DMA whose completion it would have to count.
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

    // ---- this lane's pixel in each of its wave's two fragments (the pack's assignment)
    const bool g2 = (r >= 4 && r < 12) || (r >= 16 && r < 20) || r >= 28;
    const int fr_row = g2 ? 1 : 0;
    const int fr_col = g2 ? (r < 12 ? r - 4 : (r < 20 ? r - 8 : r - 16)) : (r < 4 ? r : (r < 16 ? r - 8 : r - 12));
    const int px_x = tile_x * C::TCOLS + fr_col;
    int py_y[2], wrow[2];
    bool in_img[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        wrow[m] = (wave * 2 + m) * 2 + fr_row;
        py_y[m] = tile_y * C::TROWS + wrow[m];
        in_img[m] = py_y[m] < H && px_x < W;
    }
    const int my_y = h ? py_y[1] : py_y[0];
    const bool my_in = h ? in_img[1] : in_img[0];
    const float fy_base = (float)(my_y - 1), fx_base = (float)(px_x - 1);
    const float fy_max = (float)(H + 1), fx_max = (float)(W + 1);
    unsigned xbase[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) xbase[m] = (unsigned)((wrow[m] * C::TC + fr_col) * C::PSB + h * 16);
    const int a3i = lane & 15, a3kb = lane >> 4;
    const bool a3real = (a3i >> 2) < 2 && (a3i & 3) < 3 && (a3kb & 1) == (a3i >> 2);
    const int a3row = a3real ? (a3i & 3) : 3, a3half = a3kb >> 1;
    const unsigned w3lane = (unsigned)(C::W3_OFF + (a3row * 2 + a3half) * 16);
    const int t3lane16 = (a3half * 32 + a3row) * 16;
    __syncthreads();

    // ---- offset_conv (ema_vfi.py:41,56) on the staged window: the pack's k-group order, then the three im2col tail k-groups
    f32x16 omr[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) omr[m][i] = p.off_bias[acc_channel(i, h)];
    {
        u32x4_t xq[2][2][4];
        auto load_x = [&](auto tc, u32x4_t (&dst)[2][4]) {
            constexpr int toff = gather3_tap_off(decltype(tc)::value);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kg = 0; kg < 4; ++kg) dst[m][kg] = lds_read16(lds_r + xbase[m] + (unsigned)(toff + kg * 32));
        };
        load_x(std::integral_constant<int, 0>{}, xq[0]);
        auto off_tap = [&](auto tc) {
            constexpr int tap = decltype(tc)::value;
            if constexpr (tap < 7) {
#pragma unroll
                for (int kg = 0; kg < 4; ++kg) ow[(tap + 2) % 3][kg] = *reinterpret_cast<const f16x8 *>(owbase_g + ((tap + 2) * 4 + kg) * 1024 + lane16);
            }
            if constexpr (tap < 8) load_x(std::integral_constant<int, tap + 1>{}, xq[(tap + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kg = 0; kg < 4; ++kg) mma_kg(omr[m], ow[tap % 3][kg], __builtin_bit_cast(f16x8, xq[tap & 1][m][kg]));
            __builtin_amdgcn_sched_barrier(0);
        };
        off_tap(std::integral_constant<int, 0>{}); off_tap(std::integral_constant<int, 1>{}); off_tap(std::integral_constant<int, 2>{});
        off_tap(std::integral_constant<int, 3>{}); off_tap(std::integral_constant<int, 4>{}); off_tap(std::integral_constant<int, 5>{});
        off_tap(std::integral_constant<int, 6>{}); off_tap(std::integral_constant<int, 7>{}); off_tap(std::integral_constant<int, 8>{});
        f16x8 ot[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) ot[j] = *reinterpret_cast<const f16x8 *>(owbase_g + C::OFF_TAIL + j * 1024 + lane16);
        u32x2_t ta[2][3][2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const unsigned tb = xbase[m] - (unsigned)(h * 16) + 128u;
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned o = h ? (unsigned)gather3_tap_off(4 * j + 2 + u) : (unsigned)gather3_tap_off(4 * j + u);
                    ta[m][j][u] = lds_read8(lds_r + tb + o);
                }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x4_t bq = {ta[m][j][0][0], ta[m][j][0][1], ta[m][j][1][0], ta[m][j][1][1]};
                mma_kg(omr[m], ot[j], __builtin_bit_cast(f16x8, bq));
            }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = acc_channel(i, h);
            const float v = omr[m][i];
            const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
            omr[m][i] = (c >= 18 && c < 27) ? sg : v;
        }

    // ---- DCN accumulators
    f32x16 acc[2][2];
    f32x4 acc3[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][n][i] = p.bias[n * 32 + acc_channel(i, h)];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc3[m][e] = lane < 32 ? p.bias[64 + e] : 0.0f;
    }

    // ---- sampling geometry of all nine taps (the pack's fp32 arithmetic).  Per tap a lane keeps three words - in LDS, in the window
    // that offset_conv no longer reads (27 KiB: registers are what limits this kernel, the tap loop reads them once per tap):
    //   GM0: corner descriptor = clamped top-left pixel index | x1 - x0 << 24 | y1 - y0 << 25 | validity of the 4 corners << 26
    //   GM1 / GM2: the corner weights (w00, w01) | (w10, w11) as f16 pairs, NOT validity-masked (the pack's window path: an
    //   out-of-image corner reads 0)
    typedef __attribute__((address_space(3))) unsigned lds_u32_t;
    lds_u32_t *gm = reinterpret_cast<lds_u32_t *>((lds_char_t *)smem) + tid;   // word (tap, k) at gm[(3 tap + k) * 256]
    __syncthreads();   // every wave has left offset_conv: the window is dead
    unsigned lane_fb = 0, fb_taps = 0;   // census: samples the pack would have parked for its fix-up
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
        auto pick = [&](auto cc) {
            constexpr int c = decltype(cc)::value;
            constexpr int reg = (c & 3) + 4 * (c >> 3);
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(omr[0][reg]), __float_as_uint(omr[1][reg]), false, false);
            return __uint_as_float(((c >> 2) & 1) ? sw[1] : sw[0]);
        };
        o.dy = pick(std::integral_constant<int, 2 * tap>{});
        o.dx = pick(std::integral_constant<int, 2 * tap + 1>{});
        o.mk = pick(std::integral_constant<int, 18 + tap>{});
        if (!my_in) o.mk = 0.0f;
        omax = fmaxf(omax, fmaxf(fabsf(o.dy), fabsf(o.dx)));
        const float py = fminf(fmaxf((fy_base + (float)ti) + o.dy, -2.0f), fy_max);
        const float px = fminf(fmaxf((fx_base + (float)tj) + o.dx, -2.0f), fx_max);
        const float fy = floorf(py), fx = floorf(px);
        const int hl = (int)fy, wl = (int)fx, hh = hl + 1, wh = wl + 1;
        const float lh = py - fy, lw = px - fx, uh = 1.0f - lh, uw = 1.0f - lw;
        float w4[4] = {o.mk * (uh * uw), o.mk * (uh * lw), o.mk * (lh * uw), o.mk * (lh * lw)};
        // the products are rounded to fp32 and THEN to f16, as in the pack: left alone, hipcc folds mul + f16 conversion into one
        // v_fma_mixlo_f16 (a single rounding) here but not there, and 1 in ~10^3 weights came out one f16 ulp apart (no instruction emitted)
        asm("" : "+v"(w4[0]), "+v"(w4[1]), "+v"(w4[2]), "+v"(w4[3]));
        // census: would the pack's 23 x 23 window have held all four corners?
        const int ly0 = hl - wy0, lx0 = wl - wx0;
        const bool inside = (unsigned)ly0 <= (unsigned)(Pack3::TR - 2) && (unsigned)lx0 <= (unsigned)(Pack3::TC - 2);
        const bool need_fb = !EMAVFI_DEFORM_ABL_NO_FALLBACK && !inside && my_in;
        lane_fb |= need_fb ? 1u << tap : 0u;
        fb_taps |= __any(need_fb) ? 1u << tap : 0u;
        const int hlc = min(max(hl, 0), H - 1), wlc = min(max(wl, 0), W - 1);
        const int hhc = min(max(hh, 0), H - 1), whc = min(max(wh, 0), W - 1);
        const unsigned vhl = (unsigned)hl < (unsigned)H, vhh = (unsigned)hh < (unsigned)H;
        const unsigned vwl = (unsigned)wl < (unsigned)W, vwh = (unsigned)wh < (unsigned)W;
        const unsigned d = (__umul24((unsigned)hlc, (unsigned)W) + (unsigned)wlc) | ((unsigned)(whc - wlc) << 24) | ((unsigned)(hhc - hlc) << 25) |
                           ((vhl & vwl) << 26) | ((vhl & vwh) << 27) | ((vhh & vwl) << 28) | ((vhh & vwh) << 29);
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

    // ---- the tail channels of all nine taps: three im2col k-groups, contracted first (the pack's order)
    const char *wtl = wbase_g + C::DCN_TAIL;
    auto tail_mma = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        f16x8 wt[3];
#pragma unroll
        for (int n = 0; n < 3; ++n) wt[n] = *reinterpret_cast<const f16x8 *>(wtl + (j * 3 + n) * 1024 + (n < 2 ? lane16 : t3lane16));
        unsigned bm[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const auto sw = __builtin_amdgcn_permlane32_swap(tl[4 * j + u][d], tl[4 * j + 2 + u][d], false, false);
                bm[0][2 * u + d] = sw[0];
                bm[1][2 * u + d] = sw[1];
            }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f16x8 xf = __builtin_bit_cast(f16x8, u32x4_t{bm[m][0], bm[m][1], bm[m][2], bm[m][3]});
#pragma unroll
            for (int n = 0; n < 2; ++n) mma_kg(acc[m][n], wt[n], xf);
            mma_k32(acc3[m], wt[2], xf);
        }
    };
    tail_mma(std::integral_constant<int, 0>{}); tail_mma(std::integral_constant<int, 1>{}); tail_mma(std::integral_constant<int, 2>{});

    // ---- 9 taps x 4 k-groups x 2 rows, step s = 2 kg + m (the pack's order per accumulator).  The corner pieces of step s travel four
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

    // ---- census (the pack's record, deform_pack3.inl): only waves with a sample beyond the pack's window pay for it
    if (__builtin_expect(fb_taps != 0, 0) && p.census) {
        unsigned n_parked = 0;
#pragma unroll 1
        for (unsigned left = fb_taps; left != 0; left &= left - 1)
            n_parked += (unsigned)__popcll(__ballot(((lane_fb >> __builtin_ctz(left)) & 1u) != 0));
        float om = my_in ? omax : 0.0f;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) om = fmaxf(om, __shfl_xor(om, sh));
        if (lane == 0) {
            unsigned *cs = p.census + (blockIdx.x & 63u) * 4u;
            (void)__hip_atomic_fetch_add(cs, (unsigned)__popc(fb_taps), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(cs + 1, n_parked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(cs + 2, __float_as_uint(om), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- epilogue (the pack's)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!in_img[m]) continue;
        TS *op = reinterpret_cast<TS *>(p.out) + (((size_t)b * H + py_y[m]) * W + px_x) * p.out_ps;
        auto store_third = [&](auto *o16) {
            typedef typename std::remove_pointer<decltype(o16)>::type O;
            typedef __attribute__((ext_vector_type(2))) O pair_t;
            if (p.cstore > 64 && h == 0) {
                const pair_t q0 = {(O)acc3[m][0], (O)acc3[m][1]}, q1 = {(O)acc3[m][2], (O)acc3[m][3]};
                const pair_t q2 = {(O)p.bias[68], (O)p.bias[69]}, q3 = {(O)p.bias[70], (O)p.bias[71]};
                *reinterpret_cast<uint4 *>(o16 + 64) = make_uint4(__builtin_bit_cast(unsigned, q0), __builtin_bit_cast(unsigned, q1),
                                                                  __builtin_bit_cast(unsigned, q2), __builtin_bit_cast(unsigned, q3));
            }
        };
        if (std::is_same<TS, bf16_t>::value && p.out_f16) {
            half_t *oh = reinterpret_cast<half_t *>(op);
#pragma unroll
            for (int n = 0; n < 2; ++n) store_frag(oh + n * 32, acc[m][n], h, p.cstore - n * 32, [](float v, int) { return v; });
            store_third(oh);
        } else {
#pragma unroll
            for (int n = 0; n < 2; ++n) store_frag(op + n * 32, acc[m][n], h, p.cstore - n * 32, [](float v, int) { return v; });
            store_third(op);
        }
    }
