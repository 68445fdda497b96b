// The body of deform_pack3_kernel<TS, FUSE_OFF> (deform_pack3.inl), the WINDOW route, kept in a file of its own so that the routed pack
// (deform_route3.inl) runs the same statements as its window branch.  Included inside a function body that defines TS, FUSE_OFF and the
// DeformParams `p`.  The stages it has in common with the gather body are included from deform3_stages.inl (deform3_shared.inl).
    using C = Pack3;
    constexpr int R = C::R;
    static_assert(sizeof(TS) == 2, "16-bit storage types only");
    typedef __attribute__((address_space(1))) const void gptr_t;
    typedef __attribute__((address_space(3))) void lptr_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lds_cchar_t *lds_r = (lds_cchar_t *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int H = p.H, W = p.W;
    const unsigned lane16 = (unsigned)lane * 16u;
    DEFORM_STAMP(ts_begin);
#if EMAVFI_DEFORM_STAMPS
    unsigned long long sum_steps = 0, cnt_out = 0;
#endif

#define DEFORM3_STAGE DEFORM3_TILE
#include "deform3_stages.inl"
    const unsigned ps_bytes = (unsigned)p.x_ps * 2u, tail_bytes = (unsigned)p.tail_ps * 2u;
    const int ty0 = tile_y * C::TROWS - 1 - R, tx0 = tile_x * C::TCOLS - 1 - R;
    const char *gplane = (const char *)p.x + (size_t)b * H * W * ps_bytes;
    const char *tplane = p.x_tail ? (const char *)p.x_tail + (size_t)b * H * W * tail_bytes : nullptr;
    const char *zeros = (const char *)p.zeros;
    const char *wbase_g = (const char *)p.w;       // wave-uniform bases: fragment loads are base + lane16 + immediate
    const char *owbase_g = (const char *)p.off_w;

    // ---- small loads first (L2-resident): the first two taps' offset_conv fragments
    f16x8 ow[FUSE_OFF ? 3 : 1][4];
    if constexpr (FUSE_OFF) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) ow[t][kg] = *reinterpret_cast<const f16x8 *>(owbase_g + (t * 4 + kg) * 1024 + lane16);
    }

    // ---- DMA the window, row by row: wave w fetches pixels [7w, 7w + 7) (wave 3: 2 pixels) x 9 pieces of every row.
    // A lane's pixel column and piece never change; out-of-image pixels read the zero page.
    const bool dact = wave < 3 ? lane < C::SEG_PX * C::SP : lane < C::LAST_PX * C::SP;
    {
        const int dp = lane / C::SP, dpc = lane - dp * C::SP;
        const int dgx = tx0 + wave * C::SEG_PX + dp;
        const bool dcol = (unsigned)dgx < (unsigned)W;
        const long long pix0 = (long long)ty0 * W + dgx;
        const bool from_tail = tplane != nullptr && dpc == C::SP - 1;   // channels 64..71 from the compact tail buffer
        const char *src = from_tail ? tplane + pix0 * (long long)tail_bytes : gplane + pix0 * (long long)ps_bytes + dpc * 16;
        const unsigned inc = (unsigned)W * (from_tail ? tail_bytes : ps_bytes);
        if (dact && !(EMAVFI_P3_ABL & 16)) {
#pragma unroll
            for (int ly = 0; ly < C::TR; ++ly) {
                const bool ok = dcol && (unsigned)(ty0 + ly) < (unsigned)H;
                const char *s = ok ? src : zeros;
                __builtin_amdgcn_global_load_lds((gptr_t *)s, (lptr_t *)(smem + ly * C::ROWB + wave * C::SEG_BYTES), 16, 0, 0);
                src += inc;
            }
        }
        // the third fragment's A operands (4 608 B): one DMA instruction per wave + half an instruction
        const char *w3g = wbase_g + C::DCN_W3;
        __builtin_amdgcn_global_load_lds((gptr_t *)(w3g + wave * 1024 + lane16), (lptr_t *)(smem + C::W3_OFF + wave * 1024), 16, 0, 0);
        if (wave == 0 && lane < 32)
            __builtin_amdgcn_global_load_lds((gptr_t *)(w3g + 4096 + lane16), (lptr_t *)(smem + C::W3_OFF + 4096), 16, 0, 0);
    }
    DEFORM_STAMP(ts_issued);
#if EMAVFI_DEFORM_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    DEFORM_STAMP(ts_landed);
    if constexpr (std::is_same<TS, bf16_t>::value) {
        // bf16 -> f16 in place: every wave converts exactly the pieces its own DMA instructions fetched, so its own
        // vmcnt(0) is the only wait needed before it reads them back.  Skipped when the producer already wrote f16.
        if (!p.in_f16) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (dact) {
#pragma unroll
                for (int ly = 0; ly < C::TR; ++ly) {
                    lds_char_t *q = (lds_char_t *)smem + ly * C::ROWB + wave * C::SEG_BYTES + lane16;
                    const u32x4_t v = to_f16_piece<TS>(lds_read16(q));
                    *reinterpret_cast<__attribute__((address_space(3))) u32x4_t *>(q) = v;
                }
            }
        }
    }

#define DEFORM3_STAGE DEFORM3_LANE
#include "deform3_stages.inl"
    const float *om_my = p.om + (((size_t)b * H + (my_in ? my_y : 0)) * W + (my_in ? px_x : 0)) * 32;
    constexpr int HALO = R;
#define DEFORM3_STAGE DEFORM3_LANE_CONST
#include "deform3_stages.inl"
    DEFORM_STAMP(ts_converted);
    if (tid == 0) *reinterpret_cast<__attribute__((address_space(3))) unsigned *>((lds_char_t *)smem + C::SYNC_OFF) = 0u;   // (fix-up hand-shake below)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the window DMA has landed (hipcc emits this wait today; not relied upon - ADVICE r5)
    __syncthreads();
    DEFORM_STAMP(ts_window);

    f32x16 omr[FUSE_OFF ? 2 : 1];
    if constexpr (FUSE_OFF) {
        constexpr bool KG0_ONLY = (EMAVFI_P3_ABL & 32) != 0;
#define DEFORM3_STAGE DEFORM3_OFFSET_CONV
#include "deform3_stages.inl"
    }

    // ---- DCN.  Accumulators; the first weight fragments.
    f16x8 wq[2][2];  // [kg & 1][n]
#pragma unroll
    for (int n = 0; n < 2; ++n) wq[0][n] = *reinterpret_cast<const f16x8 *>(wbase_g + n * 1024 + lane16);
#define DEFORM3_STAGE DEFORM3_ACC_INIT
#include "deform3_stages.inl"
    DEFORM_STAMP(ts_offconv);

    // ---- sampling geometry of ALL NINE taps up front (fp32, compare-free clamps: NaN -> -2; positions <= -1 or >= size sample
    // zeros).  Half-lane h handles the pixel of fragment row h.  Nine independent chains in one block instead of one dependent
    // chain in front of every tap's steps; the offset_conv's accumulators die here.  Per tap a lane keeps three registers:
    //   sample inside the staged window:  window byte offset of its top-left corner | (w00, w01) | (w10, w11) as f16 pairs
    //   sample outside (|offset| > R near the tile edge: rare):  py | px | mask as fp32 bits, bit `tap` of lane_fb set.
    // Such a sample contributes NOTHING in the tap loop (zero weights, window offset 0); the fix-up loop behind it adds the
    // missing samples from global memory.  The common path carries no fallback code.
    constexpr int OFF[4] = {0, C::PSB, C::ROWB, C::ROWB + C::PSB};
    // (three 16-element register vectors: a wave-uniform runtime index into an ext_vector lowers to an indexed register move,
    // where a switch over nine scalars was turned into a scratch-memory table by hipcc)
    typedef unsigned u32x16_t __attribute__((ext_vector_type(9)));
    u32x16_t gm0 = {}, gm1 = {}, gm2 = {};
    unsigned lane_fb = 0, fb_taps = 0;   // per-lane / wave-uniform masks over taps
    float omax = 0.0f;                   // census (DeformParams::census): largest |offset| this lane computed
    unsigned tl[12][2];                  // blended tail (channels 64..66 of this half-lane's own pixel) per tap slot; 9..11 zero
#pragma unroll
    for (int t = 9; t < 12; ++t) tl[t][0] = tl[t][1] = 0u;
    auto geom_tap = [&](auto tc) {
        constexpr int tap = decltype(tc)::value, ti = tap / 3, tj = tap - 3 * ti;
        OmTap o;
        if constexpr (FUSE_OFF) {
#define DEFORM3_STAGE DEFORM3_PICK
#include "deform3_stages.inl"
        } else {
            o = load_om(om_my, tap, my_in);
        }
        constexpr bool CENSUS = !EMAVFI_P3_NO_CENSUS, PIN = false;
#define DEFORM3_STAGE DEFORM3_SAMPLE
#include "deform3_stages.inl"
        // window-local top-left corner; all four corners inside the staged window <=> 0 <= ly0 <= TR-2 and 0 <= lx0 <= TC-2
        const int ly0 = hl - ty0, lx0 = wl - tx0;
        const bool inside = (unsigned)ly0 <= (unsigned)(C::TR - 2) && (unsigned)lx0 <= (unsigned)(C::TC - 2);
        // pixels of the tile overhang (mask forced to 0) read their clamped window position: 0 x finite data
        const bool need_fb = !EMAVFI_DEFORM_ABL_NO_FALLBACK && !inside && my_in;
        const unsigned mybase = __umul24((unsigned)min(max(ly0, 0), C::TR - 2), (unsigned)C::ROWB) +
                                __umul24((unsigned)min(max(lx0, 0), C::TC - 2), (unsigned)C::PSB);
        // branch-free on purpose (bit masks, not ?: - hipcc turns the selects into EXEC branches that cut the block in nine)
        const unsigned keep = need_fb ? 0u : 0xffffffffu;
        const unsigned w01h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[0], (half_t)w4[1]}) & keep;
        const unsigned w23h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[2], (half_t)w4[3]}) & keep;
        gm0[tap] = (mybase & keep) | (__float_as_uint(py) & ~keep);
        gm1[tap] = w01h | (__float_as_uint(px) & ~keep);
        gm2[tap] = w23h | (__float_as_uint(o.mk) & ~keep);
        lane_fb |= ~keep & (1u << tap);
        fb_taps |= __any(need_fb) ? 1u << tap : 0u;
        // tail of this half-lane's own pixel: four 8-byte corner reads (clamped position: always a valid window address)
        // (no scheduling fences in this blend: the nine taps' chains are meant to interleave)
        u32x4_t vt[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x2_t t2 = lds_read8(lds_r + mybase + (unsigned)(128 + OFF[c]));
            vt[c] = u32x4_t{t2[0], t2[1], 0u, 0u};
        }
        const u32x4_t td = __builtin_bit_cast(u32x4_t, blend_corners<2>(vt, w01h, w23h));
        tl[tap][0] = td[0]; tl[tap][1] = td[1];
    };
    geom_tap(std::integral_constant<int, 0>{}); geom_tap(std::integral_constant<int, 1>{}); geom_tap(std::integral_constant<int, 2>{});
    geom_tap(std::integral_constant<int, 3>{}); geom_tap(std::integral_constant<int, 4>{}); geom_tap(std::integral_constant<int, 5>{});
    geom_tap(std::integral_constant<int, 6>{}); geom_tap(std::integral_constant<int, 7>{}); geom_tap(std::integral_constant<int, 8>{});

#define DEFORM3_STAGE DEFORM3_TAIL_MMA
#include "deform3_stages.inl"
    DEFORM_STAMP(ts_geom_all);

    // ---- 9 taps x 4 k-groups x 2 rows: two fragments from global weight fragments, the third from the LDS table.
    // The tap body is a generic lambda because it runs from TWO operand sources: the staged window (corners one pixel / one row apart)
    // and, for the samples that left the window, the fix-up arena (round 6: four consecutive 144-byte corner records per entry).
    f16x8 xf_prev = {}, w3_prev = {}, w3_cur = {};   // software pipeline: the MFMAs of a step run inside the NEXT step's blend
#pragma unroll
    for (int n = 0; n < 2; ++n) wq[1][n] = f16x8{};  // read (against the zero xf_prev) by the first tap's first step
    // one tap: operands (g0, g1, g2) = {LDS byte offset of the top-left corner | (w00, w01) | (w10, w11)} of this half-lane's OWN pixel;
    // wnext = the NEXT tap's first weight fragments (null: none).  The last step's MFMAs stay pending in (xf_prev, w3_prev, wq[1]).
    auto tap_body = [&](auto arena_tag, const int tap, const char *wnext, const unsigned g0, const unsigned g1, const unsigned g2) {
        constexpr bool ARENA = decltype(arena_tag)::value;
        constexpr int OFFC[4] = {0, ARENA ? C::A_C1 : C::PSB, ARENA ? C::A_C2 : C::ROWB, ARENA ? C::A_C1 + C::A_C2 : C::ROWB + C::PSB};
        constexpr int KGS = ARENA ? C::A_KG : 32, HS = ARENA ? C::A_H : 16;   // byte strides of a k-group (two pieces) / of this half-lane's piece
        const char *wtap = wbase_g + (size_t)tap * C::DCN_TAP;   // wave-uniform
        unsigned base[2], w01[2], w23[2];
        {
            auto both = [&](unsigned x, unsigned (&out)[2]) {
                const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
                out[0] = sw[0]; out[1] = sw[1];
            };
            both(g1, w01); both(g2, w23);
            // swap(a, b) = {(a.lo, b.lo), (a.hi, b.hi)}: the h = 1 receivers take b = base + 16 (their piece of the pixel)
            const auto sw = __builtin_amdgcn_permlane32_swap(g0, g0 + (unsigned)HS, false, false);
            base[0] = sw[0]; base[1] = sw[1];
            if (!ARENA && (EMAVFI_P3_ABL & 2)) { base[0] = xbase[0] + (unsigned)(tap * 16); base[1] = xbase[1] + (unsigned)(tap * 16); }
        }
        const unsigned w3a = w3lane + (unsigned)(tap * C::W3_TAP);
        // ---- the eight (k-group, row) steps, scheduled by hand.  Left to hipcc the block came out as runs of 4-6 back-to-back
        // MFMAs (the wave parked behind the matrix pipe, 32 cycles each) between runs of 16-32 blend instructions (the pipe
        // idle) - and the SIMD's other wave runs the same program.  Here the three MFMAs of step s - 1 are issued between the
        // thirds of step s's blend (5 / 5 / 6 packed FMAs, corner-major: 8 + ~24 issue cycles per 32-cycle MFMA), the corner
        // reads of step s + 1 and the next k-group's weight fragments go out at the head of step s, and sched_barrier(0)
        // pins that order.  The last step's MFMAs are carried into the next tap's first blend (into the final three behind
        // the loop); the first tap's "previous" B operand is zero.
        auto gather = [&](int s, unsigned (&d)[4][4]) {
            const int kg = s >> 1, m = s & 1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const u32x4_t v = lds_read16(lds_r + base[m] + (unsigned)(kg * KGS + OFFC[c]));
                d[c][0] = v[0]; d[c][1] = v[1]; d[c][2] = v[2]; d[c][3] = v[3];
            }
        };
        unsigned vb[2][4][4];
        gather(0, vb[0]);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int kg = s >> 1, m = s & 1;
            const int pm = (s + 7) & 1;              // row of the previous step (step 7 of the previous tap for s = 0)
            const int pkg = ((s + 7) & 7) >> 1;      // its k-group: weights still in wq[pkg & 1]
            if (s + 1 < 8 && !(EMAVFI_P3_ABL & 128)) gather(s + 1, vb[(s + 1) & 1]);
            f16x8 w3n;
            if (m == 0) w3n = __builtin_bit_cast(f16x8, lds_read16(lds_r + w3a + (unsigned)(kg * 128)));
            __builtin_amdgcn_sched_barrier(0);
            f16x2_t a[4];
            const unsigned (&d)[4][4] = vb[s & 1];
            const unsigned wa = w01[m], wb = w23[m];
            // ---- MFMA 0 of the previous step | blend ops 0..4
            if (!(EMAVFI_P3_ABL & 8)) mma_kg(acc[pm][0], wq[pkg & 1][0], xf_prev);
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = __builtin_bit_cast(f16x2_t, d[0][q]) * bcast_half<0>(wa);
            if (!(EMAVFI_P3_ABL & 4)) a[0] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2_t, d[1][0]), bcast_half<1>(wa), a[0]);
            PACK3_PIN(a);
            // ---- MFMA 1 | blend ops 5..9
            if (!(EMAVFI_P3_ABL & 8)) mma_kg(acc[pm][1], wq[pkg & 1][1], xf_prev);
            if (!(EMAVFI_P3_ABL & 4)) {
#pragma unroll
                for (int q = 1; q < 4; ++q) a[q] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2_t, d[1][q]), bcast_half<1>(wa), a[q]);
#pragma unroll
                for (int q = 0; q < 2; ++q) a[q] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2_t, d[2][q]), bcast_half<0>(wb), a[q]);
            }
            PACK3_PIN(a);
            // ---- MFMA 2 | blend ops 10..15, then the weight fragments of the next k-group (behind the MFMAs that read wq[(kg+1)&1])
            if (!(EMAVFI_P3_ABL & 64)) mma_k32(acc3[pm], w3_prev, xf_prev);   // (ablation bit 6: no third-fragment MFMA in the tap loop - results wrong in channels 64..66 only)
            if (!(EMAVFI_P3_ABL & 4)) {
#pragma unroll
                for (int q = 2; q < 4; ++q) a[q] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2_t, d[2][q]), bcast_half<0>(wb), a[q]);
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2_t, d[3][q]), bcast_half<1>(wb), a[q]);
            }
            if (m == 0 && !(EMAVFI_P3_ABL & 1)) {
                if (kg + 1 < 4) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) wq[(kg + 1) & 1][n] = *reinterpret_cast<const f16x8 *>(wtap + ((kg + 1) * 2 + n) * 1024 + lane16);
                } else if (wnext) {
#pragma unroll
                    for (int n = 0; n < 2; ++n) wq[0][n] = *reinterpret_cast<const f16x8 *>(wnext + n * 1024 + lane16);
                }
            }
            if (m == 0) w3_cur = w3n;
            PACK3_PIN(a);
            xf_prev = f16x8{a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1], a[3][0], a[3][1]};
            w3_prev = w3_cur;
        }
    };
    // the pending last step (k-group 3, row 1) of a tap sequence
    auto flush_taps = [&]() {
        mma_kg(acc[1][0], wq[1][0], xf_prev);
        mma_kg(acc[1][1], wq[1][1], xf_prev);
        mma_k32(acc3[1], w3_prev, xf_prev);
    };
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        DEFORM_STAMP(ts_tap);
        unsigned g0 = gm0[tap], g1 = gm1[tap], g2 = gm2[tap];   // wave-uniform index: indexed register moves
        if (__builtin_expect((fb_taps >> tap) & 1u, 0)) {   // wave-uniform, rare: lanes parked for the fix-up hold (py, px, mask)
            if ((lane_fb >> tap) & 1u) { g0 = 0u; g1 = 0u; g2 = 0u; }
        }
        tap_body(std::false_type{}, tap, tap < 8 ? wbase_g + (size_t)(tap + 1) * C::DCN_TAP : nullptr, g0, g1, g2);
#if EMAVFI_DEFORM_STAMPS
        DEFORM_STAMP(ts_end);
        sum_steps += ts_end - ts_tap;
#endif
    }
    flush_taps();
    DEFORM_STAMP(ts_taps_done);

    // ---- fix-up (round 6): the samples that left the window.  Round 5 gathered them from global memory in a second copy of the tap
    // body - a full wave contraction per flagged tap with its corner loads in front of the blend, 2-4 tap times each.
    // Now: every wave signals that it has left the tap loop; a wave with parked samples waits until all four have (the window is dead
    // then), takes ITS quarter of the window as an arena, fetches the parked samples' four corner records (4 x 144 B) into it with
    // LDS-DMA - up to 31 samples of ANY of its taps per round, one exposed round trip per round instead of one per tap -, and runs the
    // very tap body of the main loop on the arena (zero weights and the zero entry for every lane without a sample in the round).
    // Corners are clamped into the image and the weights of out-of-image corners are zero: the value deform_kernel computes.
    typedef __attribute__((address_space(3))) unsigned lds_u32_t;
    lds_u32_t *sync_word = reinterpret_cast<lds_u32_t *>((lds_char_t *)smem + C::SYNC_OFF);
    if (!EMAVFI_P3_NO_HANDSHAKE) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's last window reads have returned
        if (lane == 0) __hip_atomic_fetch_add(sync_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    unsigned n_parked = 0;
#if EMAVFI_DEFORM_STAMPS
    unsigned long long fx_wait = 0, fx_issue = 0, fx_land = 0, fx_taps = 0;
#endif
    if (__builtin_expect(fb_taps != 0, 0)) {
#if EMAVFI_DEFORM_STAMPS
        cnt_out += __popc(fb_taps);
#endif
        const unsigned lds0 = (unsigned)(size_t)(lds_char_t *)smem;
        const unsigned arena = (unsigned)__builtin_amdgcn_readfirstlane(wave * C::ARENA_BYTES);   // (an SGPR: the DMA's M0 operand)
        lds_u32_t *table = reinterpret_cast<lds_u32_t *>((lds_char_t *)smem + C::TAB_OFF + wave * 128);
        const unsigned long long below = (1ull << lane) - 1ull;
        // (py, px, mask) of a parked lane -> clamped corner descriptor (top-left pixel | x1 - x0 << 24 | y1 - y0 << 25) and the
        // validity-masked corner weights; lanes without `sel` get zero weights
        // (its floor and weight products are its own, not stage SAMPLE's: they start from the stored position and mask, and the
        // products sit inside the validity selects)
        auto fix_geom = [&](int tap, bool sel, unsigned &desc, unsigned &w01h, unsigned &w23h) {
            typedef bool valid_t;
            const unsigned g0 = gm0[tap], g1 = gm1[tap], g2 = gm2[tap];
            const float py = sel ? __uint_as_float(g0) : 0.0f, px = sel ? __uint_as_float(g1) : 0.0f;
            const float mk = sel ? __uint_as_float(g2) : 0.0f;
            const float fy = floorf(py), fx = floorf(px);
            const int hl = (int)fy, wl = (int)fx, hh = hl + 1, wh = wl + 1;
            const float lh = py - fy, lw = px - fx, uh = 1.0f - lh, uw = 1.0f - lw;
#define DEFORM3_STAGE DEFORM3_CORNERS
#include "deform3_stages.inl"
            const float w4[4] = {vhl && vwl ? mk * (uh * uw) : 0.0f, vhl && vwh ? mk * (uh * lw) : 0.0f,
                                 vhh && vwl ? mk * (lh * uw) : 0.0f, vhh && vwh ? mk * (lh * lw) : 0.0f};
#define DEFORM3_STAGE DEFORM3_CORNER_DESC
#include "deform3_stages.inl"
            desc = cdesc;
            w01h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[0], (half_t)w4[1]});
            w23h = __builtin_bit_cast(unsigned, f16x2_t{(half_t)w4[2], (half_t)w4[3]});
        };
        // one LDS-DMA instruction = 64 consecutive 16-byte slots = two rows of the arena (Pack3: piece-major layout)
        auto dma = [&](const char *src, unsigned dst) {
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(__builtin_amdgcn_readfirstlane(dst)) : "memory", "m0");
        };
#define DEFORM3_STAGE DEFORM3_COUNT_PARKED
#include "deform3_stages.inl"
        const bool convert = std::is_same<TS, bf16_t>::value && !p.in_f16;
        const char *wtl_fx = wbase_g + C::DCN_TAIL;
        const unsigned my_slot = (unsigned)lane & 31u, hb = (unsigned)lane >> 5;
#pragma unroll 1
        for (unsigned rbase = 0; rbase < n_parked; rbase += (unsigned)C::NENT) {
            const unsigned n_ent = min((unsigned)C::NENT, n_parked - rbase);
            DEFORM_STAMP(tr0);
            // -- A: the round's corner descriptors, slot by slot
            unsigned round_taps = 0, prefix = 0;
#pragma unroll 1
            for (unsigned left = fb_taps; left != 0; left &= left - 1) {
                const int tap = __builtin_ctz(left);
                const bool parked = ((lane_fb >> tap) & 1u) != 0;
                const unsigned long long bal = __ballot(parked);
                const unsigned cnt = (unsigned)__popcll(bal);
                if (prefix < rbase + n_ent && prefix + cnt > rbase) {
                    round_taps |= 1u << tap;
                    const unsigned slot = prefix + (unsigned)__popcll(bal & below) - rbase;
                    unsigned desc, wa_, wb_;
                    fix_geom(tap, parked, desc, wa_, wb_);
                    if (parked && slot < n_ent) table[slot] = desc;
                }
                prefix += cnt;
            }
            // (the first round's descriptors were computed while the other waves finished their tap loops: the window is needed from here on)
            if (rbase == 0) {
#if EMAVFI_DEFORM_STAMPS
                DEFORM_STAMP(tw0);
#endif
                // every wave of the workgroup reaches the increment above unconditionally: the wait ends
                while (*reinterpret_cast<volatile lds_u32_t *>(sync_word) < (unsigned)C::WAVES) __builtin_amdgcn_s_sleep(1);
#if EMAVFI_DEFORM_STAMPS
                { DEFORM_STAMP(tw1); fx_wait = tw1 - tw0; }
#endif
            }
            // -- B: fetch.  Lane (slot, hb) owns corners 2 hb and 2 hb + 1 of its slot: instructions 0..8 their first, 9..17 their second,
            // piece by piece (piece 8 = the tail channels, from the compact tail buffer when the pack has one).  Slots past the round's
            // entries and slot 31 read the zero page.  The DMA is inline asm: hipcc places no waits for it, C below does.
            {
                const unsigned d = table[my_slot];
                const bool live = my_slot < n_ent;
                const unsigned cpa = (d & 0xffffffu) + (hb && ((d >> 25) & 1u) ? (unsigned)W : 0u), cpb = cpa + ((d >> 24) & 1u);
                // (HIP declares __umul24 as returning int: widened directly, an offset with bit 31 set - a plane above 2 GiB - would be
                // sign-extended and the corner fetched from 4 GiB below it; through unsigned it is zero-extended)
                const char *pa = live ? gplane + (size_t)(unsigned)__umul24(cpa, ps_bytes) : zeros, *pb = live ? gplane + (size_t)(unsigned)__umul24(cpb, ps_bytes) : zeros;
                const char *ta = !live ? zeros : (tplane ? tplane + (size_t)(unsigned)__umul24(cpa, tail_bytes) : pa + 128);
                const char *tb = !live ? zeros : (tplane ? tplane + (size_t)(unsigned)__umul24(cpb, tail_bytes) : pb + 128);
                const unsigned step = live ? 16u : 0u;
                const unsigned dst0 = lds0 + arena;
#pragma unroll
                for (int i = 0; i < C::SP - 1; ++i) { dma(pa, dst0 + (unsigned)(i * 1024)); pa += step; }
                dma(ta, dst0 + (unsigned)((C::SP - 1) * 1024));
#pragma unroll
                for (int i = 0; i < C::SP - 1; ++i) { dma(pb, dst0 + (unsigned)((C::SP + i) * 1024)); pb += step; }
                dma(tb, dst0 + (unsigned)((2 * C::SP - 1) * 1024));
            }
            // the round's first weight fragments travel under the DMA
            {
                const char *w0 = wbase_g + (size_t)__builtin_ctz(round_taps) * C::DCN_TAP;
#pragma unroll
                for (int n = 0; n < 2; ++n) { wq[0][n] = *reinterpret_cast<const f16x8 *>(w0 + n * 1024 + lane16); wq[1][n] = f16x8{}; }
                xf_prev = f16x8{}; w3_prev = f16x8{};
            }
            // -- C: landed (in-order return: the fragments above too); bf16 storage: every lane converts the slots it fetched
            DEFORM_STAMP(tr1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            DEFORM_STAMP(tr2);
            if (convert && my_slot < n_ent) {   // (the other slots hold zeros)
#pragma unroll
                for (int i = 0; i < C::ADMA; ++i) {
                    lds_char_t *q = (lds_char_t *)smem + arena + (unsigned)(i * 1024) + lane16;
                    const u32x4_t v = to_f16_piece<TS>(lds_read16(q));
                    *reinterpret_cast<__attribute__((address_space(3))) u32x4_t *>(q) = v;
                }
            }
            // -- D: the round's taps on the arena
            DEFORM_STAMP(tr3);
            prefix = 0;
#pragma unroll 1
            for (unsigned left = fb_taps; left != 0; left &= left - 1) {
                const int tap = __builtin_ctz(left);
                const bool parked = ((lane_fb >> tap) & 1u) != 0;
                const unsigned long long bal = __ballot(parked);
                const unsigned cnt = (unsigned)__popcll(bal);
                const unsigned slot = prefix + (unsigned)__popcll(bal & below) - rbase;
                prefix += cnt;
                if (!((round_taps >> tap) & 1u)) continue;
                const bool mine = parked && slot < n_ent;
                unsigned desc, w01h, w23h;
                fix_geom(tap, mine, desc, w01h, w23h);
                const unsigned ent = arena + (mine ? slot : (unsigned)C::NENT) * 16u;
                // the tail's weight fragments (one im2col k-group with this tap's slot alone) travel under the tap's steps
                const int j = tap >> 2, hsel = (tap >> 1) & 1, u = tap & 1;
                f16x8 wt[3];
#pragma unroll
                for (int n = 0; n < 3; ++n) wt[n] = *reinterpret_cast<const f16x8 *>(wtl_fx + (j * 3 + n) * 1024 + (n < 2 ? lane16 : t3lane16));
                const unsigned later = round_taps & ~((2u << tap) - 1u);
                tap_body(std::true_type{}, tap, later ? wbase_g + (size_t)__builtin_ctz(later) * C::DCN_TAP : nullptr, ent, w01h, w23h);
                // the tail channels (64..66) of the same samples
                {
                    constexpr int OC[4] = {0, C::A_C1, C::A_C2, C::A_C1 + C::A_C2};
                    u32x4_t vt[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const u32x2_t t2 = lds_read8(lds_r + ent + (unsigned)((C::SP - 1) * C::A_H + OC[c]));
                        vt[c] = u32x4_t{t2[0], t2[1], 0u, 0u};
                    }
                    const u32x4_t td = __builtin_bit_cast(u32x4_t, blend_corners<2>(vt, w01h, w23h));
                    // K = 16 j + 8 h' + 4 u + channel with tap = 4 j + 2 h' + u: only lanes of half h' carry it, in dwords (2u, 2u + 1)
                    unsigned tm[2][2];
#pragma unroll
                    for (int dd = 0; dd < 2; ++dd) {
                        const auto sw = __builtin_amdgcn_permlane32_swap(td[dd], td[dd], false, false);   // {row 0's, row 1's} in both halves
                        tm[0][dd] = h == hsel ? sw[0] : 0u;
                        tm[1][dd] = h == hsel ? sw[1] : 0u;
                    }
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        const u32x4_t bq = u ? u32x4_t{0u, 0u, tm[m][0], tm[m][1]} : u32x4_t{tm[m][0], tm[m][1], 0u, 0u};
                        const f16x8 xf = __builtin_bit_cast(f16x8, bq);
#pragma unroll
                        for (int n = 0; n < 2; ++n) mma_kg(acc[m][n], wt[n], xf);
                        mma_k32(acc3[m], wt[2], xf);
                    }
                }
            }
            flush_taps();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the round's arena reads have returned before the next round's DMA overwrites them
#if EMAVFI_DEFORM_STAMPS
            { DEFORM_STAMP(tr4); fx_issue += tr1 - tr0; fx_land += tr3 - tr1; fx_taps += tr4 - tr3; }
#endif
        }
    }
    DEFORM_STAMP(ts_loop);
    // ---- census: only a wave that had a sample outside its window pays for it
    if (!EMAVFI_P3_NO_CENSUS && __builtin_expect(fb_taps != 0, 0) && p.census) {
#define DEFORM3_STAGE DEFORM3_CENSUS_RECORD
#include "deform3_stages.inl"
    }

#define DEFORM3_STAGE DEFORM3_EPILOGUE
#include "deform3_stages.inl"
#if EMAVFI_DEFORM_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DEFORM_STAMP(ts_done);
    if (p.stamps && lane == 0 && blockIdx.x % DEFORM_STAMP_STRIDE == 0) {
        const unsigned row = (blockIdx.x / DEFORM_STAMP_STRIDE) * C::WAVES + wave;
        if (row < DEFORM_STAMP_ROWS) {
            unsigned long long *o = p.stamps + (size_t)row * 8;
            // (o[2] bits 32..63: the fix-up pass - hand-shake wait, arena rounds, its taps; o[4]: flagged taps << 32, parked samples << 40)
            // (bits 32..63 of o[0] / o[1] / o[3] / o[5]: the fix-up's hand-shake wait / descriptor + DMA issue / DMA landing + conversion / taps)
            o[0] = (ts_window - ts_begin) | (fx_wait << 32); o[1] = (ts_offconv - ts_window) | ((fx_issue - fx_wait) << 32);
            o[2] = (ts_geom_all - ts_offconv) | ((ts_loop - ts_taps_done) << 32); o[3] = sum_steps | (fx_land << 32);
            o[4] = (ts_done - ts_loop) | (cnt_out << 32) | ((unsigned long long)n_parked << 40); o[5] = (ts_done - ts_begin) | (fx_taps << 32); o[6] = 1;
            auto q16 = [](unsigned long long v) { v >>= 2; return v > 0xffffull ? 0xffffull : v; };
            o[7] = q16(ts_issued - ts_begin) | (q16(ts_landed - ts_issued) << 16) | (q16(ts_converted - ts_landed) << 32) | (q16(ts_window - ts_converted) << 48);
        }
    }
#endif
