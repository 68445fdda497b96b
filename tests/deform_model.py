"""A float64 reference of the modulated deformable 3x3 convolution (DCNv2 as oracle/emavfi_oracle.py restates it), the worst-case error
a correct kernel may show against it WHEN ITS OFFSETS ARE EXACT, and the named set of offsets on which the sampling rule bends
(lattice_cases / carrier_cases).  Plain torch on the CPU; knows nothing of the library.  tests/test_deform_model_cpu.py tests this module
with the CPU as "kernel" (and shows that each of a list of injected defects fails the gate); tests/test_gpu_deform_lattice.py gates
the HIP kernels with it.

Positions are computed in fp32 in the kernels' and the oracle's order, ((y - 1 + i) + dy), and widened afterwards: every offset of
the lattice is a dyadic rational chosen so that this sum is exact, so reference and kernel sample at the SAME position and no element
has to be excused for sitting near an edge.  Everything behind the position is float64.

The bounds (u = 2^-11, the f16 unit roundoff; n = 9 C + 1 accumulated terms; s = sum over a tap's corners of |w_c x_c|):

  16-bit LDS-window / gather kernels (deform_pack3_body.inl, deform_gather3_body.inl) - bound_pack16.  tests/test_gpu_mdcn.py's
  error_model without its position term b_offset:
    * corner weights mask * bilinear are computed in fp32 (three roundings of 2^-24 each: 2^-22 with slack) and rounded to f16: u s -
      unless the exact product is itself an f16 number (then every fp32 intermediate is exact too): 0;
    * blend_corners (deform_pack.inl) is one rounded f16 product and three rounded f16 FMAs.  A corner whose weight is zero (outside
      the image, or lh = 0 at an exact integer) adds exactly nothing, so the blend rounds once per NON-ZERO corner: nz u s, nz <= 4.
      Together <= 5 u s - error_model's figure - and exactly 0 at integer positions with mask 1 (one corner, weight 1);
    * results or weights below f16's normal range (2^-14) round absolutely, not relatively: 2^-25 each - four blend roundings and four
      weights times |x| per blended value: 2^-25 (4 + 4 max|x|) sum|W|.  A bf16 tensor staged as f16 loses at most 2^-25 per value below
      2^-14: 2^-25 sum|W| more;
    * a mask that the kernel's own sigmoid produced (v_exp_f32, v_rcp_f32): 2^-21 sum|W| bilin(|x|); an explicit mask: 0;
    * the contraction is exact-product fp32 MFMA: n 2^-24 sum|terms|; the store rounds to nearest: half a unit.
  generic gather kernel in a 16-bit type (deform.inl, blend4 in fp32 then ONE rounding to the storage type) - bound_generic16:
    (u_T + 2^-21) per blended value - 3 weight roundings + 4 FMA roundings in fp32 are 7 * 2^-24 < 2^-21 - and the same contraction
    and store.
  fp32: deform_f32w_kernel<false> and deform_kernel<float> - bound_fp32.  uh = 1 - lh, uw = 1 - lw (lh, lw are exact differences),
    uh * uw, mask * (.): three roundings per corner weight; blend4(float): four FMAs, each partial sum <= s: 7 * 2^-24 s per blended
    value; the fp32 MFMA rounds the products too: 2 n 2^-24 sum|terms| (rounding_model.conv_model(fp32_products=True)).
  deform_f32w_kernel<true> (the three-term f16 split, deform_f32w.inl split_f16x4 / mma_x3) - bound_x3.  Each operand v is carried as
    hi = f16(v), lo = f16(v - hi): |v - hi| <= u |v|, |(v - hi) - lo| <= u^2 |v| = 2^-22 |v|, or 2^-25 absolutely once lo is
    subnormal.  Contracted: w_hi x_hi + w_lo x_hi + w_hi x_lo = (w_hi + w_lo)(x_hi + x_lo) - w_lo x_lo, so per product
    |error| <= 2^-22 |w x| (w) + 2^-22 |w x| (x) + u^2 |w x| (the dropped lo x lo) + 2^-25 (|w| + |x|): 3 * 2^-22 sum|terms| +
    2^-25 (sum|W| + sum|blended|), to first order like every term here.  The three f16 MFMAs have exact products and add 3 n terms in
    fp32: 3 n 2^-24 sum|terms|.  The blend in front is the fp32 one (7 * 2^-24)."""
import torch

from rounding_model import U32, UNIT, round64

U16 = 2.0 ** -11
EPS = 2.0 ** -10      # the lattice's step beside an edge: exact in fp32 beside any coordinate below 2^13
TILE = 16             # deform_pack3 / deform_f32w: 16 x 16 output tiles, window = tile + 3 left / above, 23 wide: rows / columns [0, 21] hold a top-left corner


# ------------------------------------------------------------------------------------------------------------ the operator
def tap_positions(off, H, W):
    """[(py, px)] of the nine taps, fp32 [B,H,W], in the kernels' order ((y - 1 + i) + dy): the only fp32 step of the model."""
    off = off.float()
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    return [((ys - 1 + (k // 3)) + off[:, 2 * k], (xs - 1 + (k % 3)) + off[:, 2 * k + 1]) for k in range(9)]


def corners64(py, px, H, W):
    """The four corners of a sample: [(row, col, weight, ok)] with float64 weights and ok = the corner counts.  A position <= -1 or
    >= size, a NaN and an infinity make all four not ok (selected with where: nothing non-finite is ever multiplied)."""
    py, px = py.double(), px.double()
    live = torch.isfinite(py) & torch.isfinite(px) & (py > -1) & (py < H) & (px > -1) & (px < W)
    pys, pxs = torch.where(live, py, torch.zeros_like(py)), torch.where(live, px, torch.zeros_like(px))
    fy, fx = torch.floor(pys), torch.floor(pxs)
    lh, lw = pys - fy, pxs - fx
    hl, wl = fy.long(), fx.long()
    out = []
    for r, c, wgt in ((hl, wl, (1 - lh) * (1 - lw)), (hl, wl + 1, (1 - lh) * lw), (hl + 1, wl, lh * (1 - lw)), (hl + 1, wl + 1, lh * lw)):
        ok = live & (r >= 0) & (r <= H - 1) & (c >= 0) & (c <= W - 1)
        out.append((r.clamp(0, H - 1), c.clamp(0, W - 1), torch.where(ok, wgt, torch.zeros_like(wgt)), ok))
    return out


def _gather(x64, r, c):
    B, C, H, W = x64.shape
    idx = (r * W + c).reshape(B, 1, H * W).expand(B, C, H * W)
    return torch.gather(x64.reshape(B, C, H * W), 2, idx).reshape(B, C, H, W)


def sample64(x, py, px):
    """bilin(x, py, px) for all channels, float64 [B,C,H,W].  The bilinear rule with the early return: exactly 0 for a position <= -1
    or >= size and for a NaN or infinite one; corners outside the image add 0."""
    x64 = x.double()
    out = torch.zeros_like(x64)
    for r, c, wgt, ok in corners64(py, px, x.shape[2], x.shape[3]):
        out = out + torch.where(ok.unsqueeze(1), _gather(x64, r, c) * wgt.unsqueeze(1), torch.zeros_like(x64))
    return out


def contract64(cols, w):
    out = 0
    for k in range(9):
        out = out + torch.einsum("oc,bchw->bohw", w[:, :, k // 3, k % 3].double(), cols[k])
    return out


def dcn64(x, off, msk, w, b, sampler=sample64):
    """(ref, terms): the float64 DCNv2 on fp32 positions and sum|terms| = sum |W| |mask| bilin(|x|) + |b| for the bounds."""
    H, W = x.shape[2:]
    pos = tap_positions(off, H, W)
    m = msk.double()
    cols = [sampler(x, *pos[k]) * m[:, k].unsqueeze(1) for k in range(9)]
    acols = [sample64(x.abs(), *pos[k]) * m[:, k].abs().unsqueeze(1) for k in range(9)]
    ref, terms = contract64(cols, w), contract64(acols, w.abs())
    if b is not None:
        ref, terms = ref + b.double().view(1, -1, 1, 1), terms + b.double().abs().view(1, -1, 1, 1)
    return ref, terms


def dead_taps(off, H, W):
    """[B,9,H,W] bool: taps whose sample contributes exactly nothing whatever the image holds (no corner counts)."""
    pos = tap_positions(off, H, W)
    return torch.stack([~torch.stack([ok for _, _, _, ok in corners64(*pos[k], H, W)]).any(dim=0) for k in range(9)], dim=1)


def integer_taps(off, H, W):
    """[B,9,H,W] bool: the sample sits on an exact integer in both axes (or is dead): the blend is a copy."""
    pos = tap_positions(off, H, W)
    out = []
    for py, px in pos:
        whole = torch.isfinite(py) & torch.isfinite(px) & (py == torch.floor(py)) & (px == torch.floor(px))
        out.append(whole)
    return torch.stack(out, dim=1) | dead_taps(off, H, W)


# ------------------------------------------------------------------------------------------------------------ the bounds
def _blend_terms(x, off, msk, w, factor):
    """sum over taps of |W| (x) [factor_k * |mask_k| bilin(|x|)], factor(k, corners, mask_k) -> [B,H,W] roundings per blended value."""
    H, W = x.shape[2:]
    pos = tap_positions(off, H, W)
    m = msk.double().abs()
    cols = []
    for k in range(9):
        f = factor(corners64(*pos[k], H, W), m[:, k])
        cols.append(sample64(x.abs(), *pos[k]) * (m[:, k] * f).unsqueeze(1))
    return contract64(cols, w.abs())


def _f16_roundings(corners, mk):
    """Roundings of one f16-blended value, in units of u s: one per non-zero corner, one more unless all four weights are f16 numbers."""
    nz = torch.zeros_like(mk)
    inexact = torch.zeros_like(mk, dtype=torch.bool)
    for _, _, wgt, ok in corners:
        w = mk * wgt
        nz = nz + (w != 0).double()
        # mk * wgt is exact in float64 when wgt fits fp32 (24 + 24 bits <= 53); only then is "w is an f16 number" a statement about the true weight
        exact = (wgt.float().double() == wgt) & (round64(w, "fp16") == w)
        inexact = inexact | ((w != 0) & ~exact)
    return nz + inexact.double()


def _sum_w(w):
    return w.double().abs().sum(dim=(1, 2, 3)).view(1, -1, 1, 1)


def _store(ref, pre, store):
    return pre + UNIT[store] * (ref.abs() + pre) + (2.0 ** -25 if store == "fp16" else 0.0)


def bound_pack16(x, off, msk, w, b, store, sigmoid_mask=False, bf16_window=False):
    """deform_pack3_kernel (both forms), deform_gather3_kernel and the routed kernel.  (ref, bound, d): d = the accumulation part in
    front of the store (rounding_model.exact_match_share's argument)."""
    ref, terms = dcn64(x, off, msk, w, b)
    n = 9 * x.shape[1] + 1
    b_blend = (U16 + 2.0 ** -22) * _blend_terms(x, off, msk, w, _f16_roundings)
    b_sub = 2.0 ** -25 * (4 + 4 * float(x.abs().max()) + (1 if bf16_window else 0)) * _sum_w(w)
    b_mask = 2.0 ** -21 * dcn64(x, off, torch.ones_like(msk), w, None)[1] if sigmoid_mask else 0.0
    d = n * U32 * terms
    pre = b_blend + b_sub + b_mask + d
    return ref, _store(ref, pre, store), d


def bound_generic16(x, off, msk, w, b, store):
    """deform_kernel<bf16 / f16>: fp32 blend, one rounding of the blended value to the storage type."""
    ref, terms = dcn64(x, off, msk, w, b)
    n = 9 * x.shape[1] + 1
    b_blend = (UNIT[store] + 2.0 ** -21) * _blend_terms(x, off, msk, w, lambda c, m: torch.ones_like(m))
    b_sub = 2.0 ** -25 * _sum_w(w) if store == "fp16" else 0.0
    d = n * U32 * terms
    return ref, _store(ref, b_blend + b_sub + d, store), d


def bound_fp32(x, off, msk, w, b):
    """deform_f32w_kernel<false> and deform_kernel<float>."""
    ref, terms = dcn64(x, off, msk, w, b)
    n = 9 * x.shape[1] + 1
    nb = terms - (b.double().abs().view(1, -1, 1, 1) if b is not None else 0.0)
    return ref, 7 * U32 * nb + 2 * n * U32 * terms, None


def bound_x3(x, off, msk, w, b):
    """deform_f32w_kernel<true>: the fp32 blend, the split's three terms (module docstring), 3 n accumulated terms."""
    ref, terms = dcn64(x, off, msk, w, b)
    n = 9 * x.shape[1] + 1
    nb = terms - (b.double().abs().view(1, -1, 1, 1) if b is not None else 0.0)
    blended = _blend_terms(x, off, msk, torch.ones_like(w), lambda c, m: torch.ones_like(m))      # sum over (tap, channel) of |blended|
    return ref, (7 * U32 + 3 * 2.0 ** -22) * nb + 3 * n * U32 * terms + 2.0 ** -25 * (_sum_w(w) + blended), None


# ------------------------------------------------------------------------------------------------------------ the lattice
def _exact(base, off):
    """every finite, moderate offset must add to its base coordinate without rounding"""
    s32 = (base.float() + off.float()).double()
    s64 = base.double() + off.double()
    ok = ~torch.isfinite(off) | (off.abs() > 2.0 ** 20) | (s32 == s64)
    assert bool(ok.all()), "a lattice offset does not add exactly in fp32"


def _grid(B, H, W):
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(B, H, W)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(B, H, W)
    return y, x


def _pick(values, sel):
    return torch.tensor(values, dtype=torch.float64)[sel % len(values)]


def edge_targets(size, eps=EPS):
    """Positions where the rule bends along one axis of extent `size`: the <= -1 / >= size rule and its neighbours, the first and last
    row themselves (lh = 0: the far corner is read against a zero weight, outside the image at size - 1), their neighbours just
    outside (one surviving corner with weight 1 - eps), and a lone corner whose weight 1/2 + 3 * 2^-11 lies beside the midpoint of two
    bf16 numbers (an f16 number: f16 weights carry it exactly, bf16 weights lose 3 * 2^-11 of it)."""
    t = [-1.0, -1.0 + eps, -1.0 - eps, size - 1.0, size - eps, float(size), 0.0, -eps, size - 1.0 + eps]
    return t + [-0.5 + 3 * 2.0 ** -11] if eps <= EPS else t      # (a coarser lattice - fp16-valued offsets - cannot carry 2^-11)


def lattice_cases(B, H, W, eps=EPS, seed=0):
    """{name: (offset [B,18,H,W], mask [B,9,H,W])} fp32 - the named edge set (module docstring of tests/test_gpu_deform_lattice.py)."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * H + W)
    y, x = _grid(B, H, W)
    yi, xi = y.long(), x.long()
    bi = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    ones = torch.ones(B, 9, H, W)
    cases = {}

    def put(name, fn, mask=None):
        off = torch.zeros(B, 18, H, W, dtype=torch.float64)
        for k in range(9):
            dy, dx = fn(k, k // 3, k % 3)
            off[:, 2 * k], off[:, 2 * k + 1] = dy, dx
            _exact(y - 1 + k // 3, off[:, 2 * k]); _exact(x - 1 + k % 3, off[:, 2 * k + 1])
        assert bool(((off.float().double() == off) | ~torch.isfinite(off)).all())
        cases[name] = (off.float(), ones.clone() if mask is None else mask)

    ints = torch.randint(-3, 4, (B, 18, H, W), generator=g).double()
    put("integers", lambda k, i, j: (ints[:, 2 * k], ints[:, 2 * k + 1]))
    quarters = torch.randint(-12, 13, (B, 18, H, W), generator=g).double() / 4
    put("half_quarter", lambda k, i, j: (quarters[:, 2 * k], quarters[:, 2 * k + 1]))
    put("half_quarter_masked", lambda k, i, j: (quarters[:, 2 * k], quarters[:, 2 * k + 1]), torch.randint(0, 5, (B, 9, H, W), generator=g).float() / 4)
    ty, tx = edge_targets(H, eps), edge_targets(W, eps)
    small = torch.randint(-1, 2, (B, 18, H, W), generator=g).double()      # the other axis stays on the lattice of integers nearby
    put("border_y", lambda k, i, j: (_pick(ty, yi + xi + bi + k) - (y - 1 + i), small[:, 2 * k + 1]))
    put("border_x", lambda k, i, j: (small[:, 2 * k], _pick(tx, yi + xi + bi + k) - (x - 1 + j)))
    put("border_corner", lambda k, i, j: (_pick(ty, yi + bi + k) - (y - 1 + i), _pick(tx, xi + 3 * k) - (x - 1 + j)))
    lone_k = (yi + 2 * xi + bi) % 9      # ONE live tap per pixel, on the lone corner beside a bf16 midpoint: nothing else hides its weight
    lone_mask = torch.stack([(lone_k == k).float() for k in range(9)], dim=1)
    put("border_lone", lambda k, i, j: (ty[-1] - (y - 1 + i), small[:, 2 * k + 1] * 0 + (1.0 - j)), lone_mask)
    # window hand-over, per pixel: tile row r, tap row i: the top-left corner's window row is r + i + 2 + floor(dy), held while in [0, 21]
    r, c = yi % TILE, xi % TILE
    axis_y = (yi + xi) % 2 == 0
    for s in range(4):
        def hand(k, i, j, s=s):
            lo_y, hi_y, lo_x, hi_x = -(r + i + 2.0), 20.0 - r - i, -(c + j + 2.0), 20.0 - c - j
            vy = torch.stack([lo_y, lo_y - eps, hi_y - eps, hi_y])[(k + s) % 4]
            vx = torch.stack([lo_x, lo_x - eps, hi_x - eps, hi_x])[(k + s) % 4]
            zero = torch.zeros_like(y)
            return torch.where(axis_y, vy, zero), torch.where(axis_y, zero, vx)
        put(f"handover_{s}", hand)
    lit = [-2.0, -2.0 - eps, 3.0 - eps, 3.0]      # the tightest of them as constants: tap row 0 on tile row 0, tap row 2 on tile row 15
    put("handover_literal", lambda k, i, j: (torch.where(axis_y, _pick(lit, yi + xi // 2 + k), torch.zeros_like(y)),
                                             torch.where(axis_y, torch.zeros_like(y), _pick(lit, yi + xi // 2 + k))))
    put("clamp", lambda k, i, j: (torch.where((yi + k) % 2 == 0, -2.0 - (y - 1 + i), H + 1.0 - (y - 1 + i)),
                                  torch.where((xi + k) % 3 == 0, -2.0 - (x - 1 + j), torch.where((xi + k) % 3 == 1, W + 1.0 - (x - 1 + j), small[:, 2 * k + 1]))))
    far = [40.0, -40.0, 1e9, -1e9, 3e38, -3e38]
    far = [float(torch.tensor(v, dtype=torch.float32)) for v in far]
    put("far", lambda k, i, j: (torch.where((yi + xi) % 3 == 0, small[:, 2 * k], _pick(far, yi + 2 * xi + k)),
                                torch.where((yi + xi) % 3 == 1, small[:, 2 * k + 1], _pick(far, xi + k + 3))))
    nonfinite = [float("inf"), float("-inf"), float("nan")]
    lone = ((yi * 3 + xi) % 5 == 0)
    put("nonfinite", lambda k, i, j: (torch.where(lone & ((yi + xi + k) % 2 == 0), _pick(nonfinite, yi + xi + k), quarters[:, 2 * k]),
                                      torch.where(lone & ((yi + xi + k) % 2 == 1), _pick(nonfinite, xi + k), quarters[:, 2 * k + 1])))
    return cases


def random_case(B, H, W, seed=0):
    """Offsets up to +-12 px on the lattice of 2^-6 px (base + offset exact in fp32), masks uniform in [0, 1)."""
    g = torch.Generator().manual_seed(2000 + seed + 7 * H + W)
    return torch.randint(-12 * 64, 12 * 64 + 1, (B, 18, H, W), generator=g).float() / 64, torch.rand(B, 9, H, W, generator=g)


# ------------------------------------------------------------------------------------------------------------ computed offsets, made exact
ON, HALF, OFF = 40.0, 0.0, -40.0     # mask logits: sigmoid = 1 to within 4e-18, exactly 1/2, 4e-18 (0 once rounded to f16)


def carrier_cases(H, W, eps=EPS, seed=0):
    """{name: (planes [n,H,W], assign [18], bias [18], logits [9])}: offset channel c = planes[assign[c]] + bias[c] (assign None: the
    bias alone), mask k = sigmoid(logits[k]).  The planes hold small integers or quarters (bf16 and f16 numbers), so ONE product
    1.0 * plane plus the fp32 bias is exact and the kernel's own offsets equal the intended ones bit for bit."""
    assert H <= 256 and W <= 256, "plane values must stay bf16 numbers"
    g = torch.Generator().manual_seed(3000 + seed + 7 * H + W)
    y, x = (t[0] for t in _grid(1, H, W))
    cases = {}
    ints = torch.randint(-3, 4, (4, H, W), generator=g).double()
    cases["integers"] = (ints, [c % 4 for c in range(18)], [0.0] * 18, [ON] * 9)
    quarters = torch.randint(-12, 13, (4, H, W), generator=g).double() / 4
    cases["half_quarter"] = (quarters, [(c * 3) % 4 for c in range(18)], [0.0] * 18, [ON, HALF, ON, ON, HALF, ON, HALF, ON, ON])
    # within +-3/4 px nothing leaves the window: the case on which the two routes must be bit-identical on an image of several tiles
    cases["sixteenths"] = (quarters / 4, [(c * 3 + 1) % 4 for c in range(18)], [0.0] * 18, [ON, ON, HALF, ON, ON, HALF, ON, ON, ON])
    rc = torch.stack([-y, -x, -(y % TILE), -(x % TILE)])
    ty, tx = edge_targets(H, eps), edge_targets(W, eps)
    for s in range(2):
        assign, bias = [], []
        for k in range(9):
            i, j = divmod(k, 3)
            if (k + s) % 2 == 0:
                assign += [0, None]; bias += [ty[(k // 2 + 5 * s) % len(ty)] + 1 - i, float((k % 3) - 1)]
            else:
                assign += [None, 1]; bias += [float((k % 3) - 1), tx[(k // 2 + 5 * s) % len(tx)] + 1 - j]
        cases[f"border_{s}"] = (rc, assign, bias, [ON] * 9)
    for s in range(4):
        assign, bias = [], []
        for k in range(9):
            i, j = divmod(k, 3)
            if k % 2 == 0:
                assign += [2, None]; bias += [[-(i + 2.0), -(i + 2.0) - eps, 20.0 - i - eps, 20.0 - i][(k // 2 + s) % 4], 0.0]
            else:
                assign += [None, 3]; bias += [0.0, [-(j + 2.0), -(j + 2.0) - eps, 20.0 - j - eps, 20.0 - j][(k // 2 + s) % 4]]
        cases[f"handover_{s}"] = (rc, assign, bias, [ON] * 9)
    lit = [-2.0, -2.0 - eps, 3.0 - eps, 3.0]
    cases["handover_literal"] = (rc, [None] * 18, [lit[(c // 2 + c) % 4] if (c // 2 + c) % 3 else 0.0 for c in range(18)], [ON] * 9)
    assign, bias = [], []
    for k in range(9):
        i, j = divmod(k, 3)
        assign += [0, 1 if k % 2 else None]
        bias += [(-2.0 if k % 2 else H + 1.0) + 1 - i, (W + 1.0 + 1 - j) if k % 2 else 0.0]
    cases["clamp"] = (rc, assign, bias, [ON] * 9)
    far = [40.0, -40.0, 1e9, -1e9, 3e38, -3e38]
    cases["far"] = (quarters, [None if c % 3 else c % 4 for c in range(18)], [0.0 if c % 3 == 0 else far[c % 6] for c in range(18)], [ON] * 9)
    nf = [float("inf"), float("-inf"), float("nan")]
    cases["nonfinite"] = (quarters, [None if c % 4 == 1 else c % 4 for c in range(18)], [nf[(c // 4) % 3] if c % 4 == 1 else 0.0 for c in range(18)], [ON] * 9)
    return cases


def carrier_tensors(case, B, C, dtype, seed=0, x_scale=1.0):
    """(x, offset_conv weight, offset_conv bias, intended offsets [B,18,H,W], intended mask [B,9,H,W]) of a carrier case.  Channels
    0..n-1 of x ARE the planes (they are image data for the DCN as well); under "amp16" the offset convolution rounds x, weight, bias
    and its result to fp16 and the mask is fp16(sigmoid)."""
    planes, assign, bias, logits = case
    n, H, W = planes.shape
    g = torch.Generator().manual_seed(4000 + seed + 7 * H + W)
    x = torch.randn(B, C, H, W, generator=g) * x_scale
    x[:, :n] = planes.float().unsqueeze(0)
    ow = torch.zeros(27, C, 3, 3)
    ob = torch.zeros(27)
    amp = dtype == "amp16"
    off = torch.zeros(B, 18, H, W)
    for c in range(18):
        raw = c if c < 9 else c + 9          # offset = cat(raw[0:9], raw[18:27]), mask = sigmoid(raw[9:18])
        b = torch.tensor(bias[c], dtype=torch.float32)
        if amp:
            b = b.half().float()
        ob[raw] = bias[c]
        v = b.expand(H, W)
        if assign[c] is not None:
            ow[raw, assign[c], 1, 1] = 1.0
            v = planes[assign[c]].float() + b
            fin = torch.isfinite(v) & (v.abs() < 6.0e4)
            assert bool((v.double() == planes[assign[c]] + b.double())[fin].all())
        if amp:
            v = v.half().float()
            if assign[c] is not None:
                assert bool((v.double() == planes[assign[c]] + b.double())[fin].all()), "not an fp16 number: choose a coarser eps"
        off[:, c] = v
    ob[9:18] = torch.tensor(logits)
    msk = torch.sigmoid(torch.tensor(logits, dtype=torch.float64)).float()
    if amp:
        msk = msk.half().float()
    return x, ow, ob, off, msk.view(1, 9, 1, 1).expand(B, 9, H, W).contiguous()


# ------------------------------------------------------------------------------------------------------------ the census, restated
def window_census(off, H, W):
    """deform_pack3_body.inl's in-window test on EXACT fp32 offsets [B,18,H,W]: (samples outside, fix-up wave-taps, all wave-taps,
    largest |offset| of the waves that flagged a sample).  A sample is outside when the top-left corner of its clamped position
    ([-2, size + 1], NaN -> -2) leaves rows / columns [0, 21] of its tile's window; a wave is 4 rows x 16 columns; fmaxf ignores NaN."""
    B = off.shape[0]
    off = off.float()
    pos = tap_positions(off, H, W)
    ty0 = (torch.arange(H) // TILE * TILE - 3).view(1, H, 1)
    tx0 = (torch.arange(W) // TILE * TILE - 3).view(1, 1, W)
    out = torch.zeros(B, 9, H, W, dtype=torch.bool)
    for k, (py, px) in enumerate(pos):
        py = torch.where(torch.isnan(py), torch.full_like(py, -2.0), py).clamp(-2.0, H + 1.0)
        px = torch.where(torch.isnan(px), torch.full_like(px, -2.0), px).clamp(-2.0, W + 1.0)
        ly, lx = torch.floor(py).long() - ty0, torch.floor(px).long() - tx0
        out[:, k] = (ly < 0) | (ly > 21) | (lx < 0) | (lx > 21)
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    pad = torch.zeros(B, 9, Hp, Wp, dtype=torch.bool)
    pad[:, :, :H, :W] = out
    groups = pad.view(B, 9, Hp // 4, 4, Wp // 16, 16).any(dim=5).any(dim=3)
    pix = groups.any(dim=1).repeat_interleave(4, dim=1).repeat_interleave(16, dim=2)[:, :H, :W]
    amax = torch.where(torch.isnan(off), torch.zeros_like(off), off.abs()).amax(dim=1)
    flagged = float(amax[pix].max()) if bool(pix.any()) else 0.0
    return int(out.sum()), int(groups.sum()), int(groups.numel()), flagged


def lattice_gate(run, bound_fn, x, w, b, cases, store, label=""):
    """Every assertion of the lattice on one kernel: run(off, msk) -> [B,O,H,W] fp32.  Returns (failures [str], stats) - no element is
    excluded anywhere.  Per case: finite everywhere; every element within bound_fn's bound; where every tap sits on an integer and the
    mask is 1 the blend is a copy, so a 16-bit result is held to rounding_model's single-layer gate (exact_match_share); and with the
    mask 1 on the dead taps only (position <= -1, >= size, far, infinite, NaN) and 0 elsewhere the output is the stored bias bit for bit."""
    from rounding_model import MISMATCH_CAP, exact_match_share, storage_round
    H, W = x.shape[2:]
    fails, stats = [], {"ratio": 0.0, "share": 0.0, "units": 0.0, "elements": 0}
    bias = torch.zeros(w.shape[0]) if b is None else b
    for name, (off, msk) in cases.items():
        got = run(off, msk)
        ref, bound, d = bound_fn(x, off, msk, w, b)
        stats["elements"] += got.numel()
        if not bool(torch.isfinite(got).all()):
            fails.append(f"{label} {name}: {int((~torch.isfinite(got)).sum())} non-finite outputs")
            continue
        ratio = float(((got.double() - ref).abs() / bound).max())
        stats["ratio"] = max(stats["ratio"], ratio)
        line = f"{label} {name}: err / bound max {ratio:.3f}"
        if ratio > 1.0:
            where = int(((got.double() - ref).abs() / bound).argmax())
            fails.append(f"{line} at flat index {where} (b, o, y, x = {tuple(int(v) for v in torch.unravel_index(torch.tensor(where), got.shape))})")
        if store != "fp32" and bool(integer_taps(off, H, W).all()) and bool((msk == 1).all()):
            share, units = exact_match_share(got, ref, store, d)
            stats["share"], stats["units"] = max(stats["share"], share), max(stats["units"], units)
            line += f", mismatch share {share:.4f} (largest {units:.0f} units)"
            if share > MISMATCH_CAP or units > 1.0:
                fails.append(f"{label} {name}: integer positions, mask 1: mismatch share {share:.4f}, largest {units:.1f} units")
        dead = dead_taps(off, H, W)
        if bool(dead.any()):
            alone = run(off, dead.float())
            want = storage_round(bias, store).view(1, -1, 1, 1).expand_as(alone)
            differ = int((alone.view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if bool(torch.isfinite(alone).all()) else -1
            line += f", dead taps alone: {differ} elements differ from the stored bias"
            if differ != 0:
                fails.append(f"{label} {name}: dead taps alone (mask 0 elsewhere) must leave the stored bias bit for bit: {differ} elements differ")
        print(line)
    return fails, stats
