// The stages that the two bodies of the one-launch ModulatedDeformConvPack (deform_pack3_body.inl, deform_gather3_body.inl) share, as
// statements (deform3_shared.inl says why not as functions, and holds the stage ids).  A body includes this file once per stage, where
// the stage runs:
//     #define DEFORM3_STAGE DEFORM3_LANE
//     #include "deform3_stages.inl"
// Every stage reads C (Pack3 / Gather3), `p`, H, W, tid-derived lane, wave, h, lane16 and lds_r of the body, and what is listed with it;
// what it declares stays in the body's scope.  No stage branches on the route: what differs comes in through the names it expects.
// Hazards of the idiom, so that nobody has to find them: a stage is several statements, so a body never puts one directly under an
// unbraced `if` / `for`; a stage that declares names can run once per scope; this file has no include guard on purpose, and
// DEFORM3_STAGE is undefined again at its end, so a forgotten #define is an error, not the previous stage.
#ifndef DEFORM3_STAGE
#error "define DEFORM3_STAGE to one of the DEFORM3_* stages before including deform3_stages.inl"

#elif DEFORM3_STAGE == DEFORM3_TILE
    // ---- tile of this workgroup -> tile_x, tile_y, b.  XCD-aware order (deform_pack.inl): strips of SROWS tile rows, column by column
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

#elif DEFORM3_STAGE == DEFORM3_LANE
    // ---- this lane's pixel in each of its wave's two fragments (2 rows x 16 columns; hardware ds_read_b128 lane groups get one row of
    // 16 consecutive pixels each: deform_pack.inl) -> px_x, py_y[m], in_img[m]; half-lane h OWNS the pixel of fragment h: my_y, my_in.
    // expects: r, tile_x, tile_y
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

#elif DEFORM3_STAGE == DEFORM3_LANE_CONST
    // ---- per-lane constants: tap (0, 0)'s undeformed sample position and the clamp's bounds, xbase[m], and the third fragment's
    // w3lane / t3lane16.  expects: stage LANE; HALO = pixels between the staged window's edge and offset_conv's 1 px ring (Pack3::R / 0)
    const float fy_base = (float)(my_y - 1), fx_base = (float)(px_x - 1);
    const float fy_max = (float)(H + 1), fx_max = (float)(W + 1);
    // LDS byte offset of this lane's piece (h) of the plain tap-0 pixel of fragment row m
    unsigned xbase[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) xbase[m] = (unsigned)(((wrow[m] + HALO) * C::TC + fr_col + HALO) * C::PSB + h * 16);
    // The third output fragment (channels 64..66) runs on v_mfma_f32_16x16x32 (half the matrix-pipe cycles of the 32x32x16 it
    // replaces, 4 accumulator registers per row instead of 16) on the SAME B register: read as a 16x16x32 operand, lane
    // L = 32 h + r supplies column j = r & 15, K slice kb = 2 h + (r >> 4) - the two pixel halves of the fragment row sit in
    // different K slices.  The A operand separates them again: row 4 ph + c holds W[64 + c][slice h] in K slice 2 h + ph and zeros in
    // the other pixel half's slices, so D[4 ph + c][j] is channel 64 + c of pixel 16 ph + j - lane L < 32 ends with channels
    // 64..67 of ITS OWN pixel in its four registers.  Same LDS table (rows 0..2 | zero row, two halves), another lane mapping.
    // (Non-finite data: the other pixel's contribution is removed by ZERO weights, so an Inf / NaN blended value at pixel r +- 16 - reachable
    // only through an f16 overflow - makes channels 64..66 of pixel r NaN too, where the 32x32x16 form and the reference confine it to the
    // offending pixel.  Documented in include/emavfi.h; not masked: a frame with a non-finite activation is garbage either way.)
    const int a3i = lane & 15, a3kb = lane >> 4;
    const bool a3real = (a3i >> 2) < 2 && (a3i & 3) < 3 && (a3kb & 1) == (a3i >> 2);
    const int a3row = a3real ? (a3i & 3) : 3, a3half = a3kb >> 1;
    const unsigned w3lane = (unsigned)(C::W3_OFF + (a3row * 2 + a3half) * 16);
    const int t3lane16 = (a3half * 32 + a3row) * 16;   // the same operand out of a 32x32x16 fragment of the blob (its row 3 is a zero row)

#elif DEFORM3_STAGE == DEFORM3_OFFSET_CONV
    // ---- offset_conv (ema_vfi.py:41,56: 3x3, pad 1, 67 -> 27) on the staged window into omr[2]: 4 k-groups per tap on the window pieces
    // as they lie, then the three tail channels of all nine taps as three im2col k-groups; then the mask's sigmoid.
    // expects: omr, ow (taps 0 and 1 loaded), xbase, owbase_g; KG0_ONLY = EMAVFI_P3_ABL bit 5 (the window body passes the bit, the
    // gather body false: the ablation bits act in the window body alone)
    {
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) omr[m][i] = p.off_bias[acc_channel(i, h)];
        u32x4_t xq[2][2][4];
        auto load_x = [&](auto tc, u32x4_t (&dst)[2][4]) {
            constexpr int toff = deform3_tap_off<C>(decltype(tc)::value);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kg = 0; kg < 4; ++kg) dst[m][kg] = lds_read16(lds_r + xbase[m] + (unsigned)(toff + kg * 32));
        };
        load_x(std::integral_constant<int, 0>{}, xq[0]);
        auto off_tap = [&](auto tc) {
            constexpr int tap = decltype(tc)::value;
            if constexpr (tap < 7) {  // weight fragments two taps ahead
#pragma unroll
                for (int kg = 0; kg < 4; ++kg) ow[(tap + 2) % 3][kg] = *reinterpret_cast<const f16x8 *>(owbase_g + ((tap + 2) * 4 + kg) * 1024 + lane16);
            }
            if constexpr (tap < 8) load_x(std::integral_constant<int, tap + 1>{}, xq[(tap + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kg = 0; kg < 4; ++kg)
                    if (!KG0_ONLY || kg == 0) mma_kg(omr[m], ow[tap % 3][kg], __builtin_bit_cast(f16x8, xq[tap & 1][m][kg]));
            __builtin_amdgcn_sched_barrier(0);
        };
        off_tap(std::integral_constant<int, 0>{}); off_tap(std::integral_constant<int, 1>{}); off_tap(std::integral_constant<int, 2>{});
        off_tap(std::integral_constant<int, 3>{}); off_tap(std::integral_constant<int, 4>{}); off_tap(std::integral_constant<int, 5>{});
        off_tap(std::integral_constant<int, 6>{}); off_tap(std::integral_constant<int, 7>{}); off_tap(std::integral_constant<int, 8>{});
        // tail: k-group j, lane (r, h) holds K = 16j + 8h + e = tap slot 4j + 2h + (e >> 2), channel 64 + (e & 3)
        {
            f16x8 ot[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) ot[j] = *reinterpret_cast<const f16x8 *>(owbase_g + C::OFF_TAIL + j * 1024 + lane16);
            u32x2_t ta[2][3][2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const unsigned tb = xbase[m] - (unsigned)(h * 16) + 128u;   // tail piece of the plain tap-0 pixel
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const unsigned o = h ? (unsigned)deform3_tap_off<C>(4 * j + 2 + u) : (unsigned)deform3_tap_off<C>(4 * j + u);
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
        // mask = sigmoid(third chunk), ema_vfi.py:59 (channels 18..26 after the pack-time routing)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = acc_channel(i, h);
                const float v = omr[m][i];
                // v_exp_f32 + v_rcp_f32 (1 ulp each): the value becomes an f16 blend weight; the IEEE division and libm expf of
                // the stand-alone layer cost ~25 instructions per value, 18 values per lane
                const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
                omr[m][i] = (c >= 18 && c < 27) ? sg : v;
            }
    }

#elif DEFORM3_STAGE == DEFORM3_ACC_INIT
    // ---- the DCN accumulators acc[m][n], acc3[m], from the bias (the third fragment's four registers: channels 64..67, lanes < 32)
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

#elif DEFORM3_STAGE == DEFORM3_PICK
    // ---- o = this tap's (dy, dx, mask) of the half-lane's own pixel out of offset_conv's accumulators.  expects: tap, o, omr, my_in
            // channel c of (row 0 | row 1) of this lane's pixels, delivered to (half 0 | half 1): one swap.
            // swap(a, b) -> {(a.lo, b.lo), (a.hi, b.hi)}; the channel lives in half-lane (c >> 2) & 1, register (c & 3) + 4 * (c >> 3)
            auto pick = [&](auto cc) {
                constexpr int c = decltype(cc)::value;
                constexpr int reg = (c & 3) + 4 * (c >> 3);
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(omr[0][reg]), __float_as_uint(omr[1][reg]), false, false);
                return __uint_as_float(((c >> 2) & 1) ? sw[1] : sw[0]);
            };
            o.dy = pick(std::integral_constant<int, 2 * tap>{});
            o.dx = pick(std::integral_constant<int, 2 * tap + 1>{});
            o.mk = pick(std::integral_constant<int, 18 + tap>{});
            if (!my_in) o.mk = 0.0f;   // pixels of the tile overhang contribute nothing (and are never stored)

#elif DEFORM3_STAGE == DEFORM3_SAMPLE
    // ---- this tap's sample (py, px) of the half-lane's own pixel (compare-free clamps: NaN -> -2; positions <= -1 or >= size sample
    // zeros), its top-left and bottom-right corners (hl, wl), (hh, wh), the four mask-weighted bilinear weights w4, and the census' largest |offset|.
    // expects: o, ti, tj, omax; CENSUS = !EMAVFI_P3_NO_CENSUS in the window body, true in the gather body (the switch acts in the window
    // body alone); PIN = false in the window body, true in the gather body:
    // both routes must round the weight products twice (fp32 here, f16 by the body).  In the gather body hipcc otherwise folds
    // multiplication and conversion into one v_fma_mixlo_f16 - a single rounding, which it does not do in the window body - and 1 in
    // ~10^3 weights came out one f16 ulp apart.  The empty asm (no instruction emitted) keeps the fp32 product.
        if (CENSUS) omax = fmaxf(omax, fmaxf(fabsf(o.dy), fabsf(o.dx)));   // (one v_max3_f32 with |.| modifiers; NaN offsets are ignored)
        const float py = fminf(fmaxf((fy_base + (float)ti) + o.dy, -2.0f), fy_max);
        const float px = fminf(fmaxf((fx_base + (float)tj) + o.dx, -2.0f), fx_max);
        const float fy = floorf(py), fx = floorf(px);
        const int hl = (int)fy, wl = (int)fx;
        [[maybe_unused]] const int hh = hl + 1, wh = wl + 1;   // (the gather body's corners; computed HERE, ahead of the products, in both)
        const float lh = py - fy, lw = px - fx, uh = 1.0f - lh, uw = 1.0f - lw;
        float w4[4] = {o.mk * (uh * uw), o.mk * (uh * lw), o.mk * (lh * uw), o.mk * (lh * lw)};
        if (PIN) asm("" : "+v"(w4[0]), "+v"(w4[1]), "+v"(w4[2]), "+v"(w4[3]));

#elif DEFORM3_STAGE == DEFORM3_CORNERS
    // ---- a sample's four corners clamped into the image, and which rows / columns of them lie inside it (an out-of-image corner
    // contributes nothing: the window body zeroes its weight, the gather body reads a zero).
    // expects: (hl, wl), (hh, wh) = the sample's top-left and bottom-right corners; valid_t = the flags' type (bool in the window body,
    // unsigned in the gather body: each kernel's code object depends on it)
            const int hlc = min(max(hl, 0), H - 1), wlc = min(max(wl, 0), W - 1);
            const int hhc = min(max(hh, 0), H - 1), whc = min(max(wh, 0), W - 1);
            const valid_t vhl = (unsigned)hl < (unsigned)H, vhh = (unsigned)hh < (unsigned)H;
            const valid_t vwl = (unsigned)wl < (unsigned)W, vwh = (unsigned)wh < (unsigned)W;

#elif DEFORM3_STAGE == DEFORM3_CORNER_DESC
    // ---- cdesc = the clamped corners' descriptor: top-left pixel index | x1 - x0 << 24 | y1 - y0 << 25 (bits 26.. are the body's).
    // expects: stage CORNERS
            const unsigned cdesc = (__umul24((unsigned)hlc, (unsigned)W) + (unsigned)wlc) | ((unsigned)(whc - wlc) << 24) | ((unsigned)(hhc - hlc) << 25);

#elif DEFORM3_STAGE == DEFORM3_TAIL_MMA
    // ---- the tail channels of all nine taps: three im2col k-groups, contracted first.  Half-lane h holds its OWN row's values;
    // one swap per dword hands tap slots (4j + 2h, 4j + 2h + 1) of row m to lane (r, h) of fragment m.
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

#elif DEFORM3_STAGE == DEFORM3_COUNT_PARKED
    // ---- n_parked += this wave's samples outside the window route's window.  expects: n_parked; fb_taps = the wave's taps that have
    // one, bit `tap` of lane_fb = this lane's is
#pragma unroll 1
        for (unsigned left = fb_taps; left != 0; left &= left - 1)
            n_parked += (unsigned)__popcll(__ballot(((lane_fb >> __builtin_ctz(left)) & 1u) != 0));

#elif DEFORM3_STAGE == DEFORM3_CENSUS_RECORD
    // ---- census of this launch (emavfi_forward_census / emavfi_mdcn_census): (wave, tap) groups that took / would take the fix-up,
    // samples outside the window, and the largest |offset| of a wave that had one - ONLY such waves pay for it (a same-box A/B priced an
    // unconditional wave reduction + atomic at 40-55 us per launch, 3-4 %: profiles/r06_experiments_that_lost.txt).  64 slots of
    // {u32 x 4} per launch, no-return atomics.  A launch without a flagged wave reports max |offset| 0 = "every sample inside the +-2 px
    // window".  expects: fb_taps, n_parked, my_in, omax; the body's guard around it decides whether the wave records
        float om = my_in ? omax : 0.0f;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) om = fmaxf(om, __shfl_xor(om, sh));
        if (lane == 0) {
            unsigned *cs = p.census + (blockIdx.x & 63u) * 4u;
            (void)__hip_atomic_fetch_add(cs, (unsigned)__popc(fb_taps), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(cs + 1, n_parked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(cs + 2, __float_as_uint(om), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }

#elif DEFORM3_STAGE == DEFORM3_EPILOGUE
    // ---- epilogue (no activation: ema_vfi.py:136-138 chains the blocks directly).  expects: b, px_x, py_y, in_img, acc, acc3
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!in_img[m]) continue;
        TS *op = reinterpret_cast<TS *>(p.out) + (((size_t)b * H + py_y[m]) * W + px_x) * p.out_ps;
        // the third fragment: lanes < 32 hold channels 64..67 of their own pixel; 68..71 have zero weights (their bias alone)
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

#else
#error "DEFORM3_STAGE is not one of the DEFORM3_* stages"
#endif
#undef DEFORM3_STAGE
