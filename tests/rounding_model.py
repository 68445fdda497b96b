"""A float64 reference of the 3x3 convolution layers and the worst-case error a correct 16-bit / fp32 kernel may show against it.
Plain torch on the CPU; knows nothing of the library (tests/test_rounding_model_cpu.py tests this module with the CPU as "kernel",
tests/test_gpu_conv_rounding_model.py gates the HIP kernels with it, tests/test_gpu_mdcn.py shares storage_round).  The three-term f16
split mode (fp32x3) has its own section at the end: split22 / conv_model_x3 / chain_stats_x3 / pool_linear_model_x3, for
tests/test_gpu_fp32x3_rounding_model.py.

The model of ONE layer y = store(act(conv3x3(x, w) + b)) on operands that are already storage-rounded (they carry no error):
  * products: bf16 x bf16 (16 significant bits) and f16 x f16 (22) are exact in fp32.  n = 9 Cin + 1 terms (the bias is one) are
    added in fp32 in an order the kernel chooses: any order stays within (n - 1) 2^-24 sum|terms| of the true sum to first order;
    delta = n 2^-24 (conv(|x|, |w|) + |b|) (the term tests/test_gpu_mdcn.py::error_model calls b_acc).  In fp32 mode the products
    round too - n more roundings of values no larger than the partial sums' bound: 2 n;
  * ReLU is 1-Lipschitz: delta passes unchanged.  tanh01 = (tanh(v) + 1) / 2 is 1/2-Lipschitz: delta / 2, plus what the kernel's
    tanh is off by, TANH_TERM = 2^-21, derived from the instructions of the two epilogues that exist:
      - conv_ring_tail.inl: 1 / (1 + exp(-2 v)) as v_exp_f32 (1 ulp) of the fp32 product -2 v log2(e) (the product and the constant
        each round: the exponent moves by <= |2 v| 2^-23 -> exp by that RELATIVE amount), one fp32 add (2^-24), v_rcp_f32 (1 ulp =
        2^-23).  With s = 1 / (1 + e) in (0, 1): |ds| <= s (1 - s) (2^-23 + |2 v| 2^-23) + s (2^-24 + 2^-23), and s (1 - s) <= 1/4,
        s (1 - s) |2 v| <= 2 |v| exp(-2 |v|) <= 1 / e: |ds| <= (0.25 + 0.37 + 1.5) 2^-23 = 2.12 * 2^-23 < 2^-21;
      - conv_light.inl / conv3x3.inl: (tanhf(v) + 1.0f) / 2.0f with the device library's tanhf (OpenCL's bound for tanh is 5 ulp
        of a value <= 1: 5 * 2^-24), one add in [0, 2] (2^-24), an exact halving: 3 * 2^-24 < 2^-21;
  * the store rounds to nearest: u (|ref| + d) with u = 2^-8 (bf16), 2^-11 (f16), 0 (fp32 - also the planar head, which returns
    fp32); f16 results below 2^-14 are subnormal with spacing 2^-24: + 2^-25 absolute.

A CHAIN of layers whose intermediates are stored rounded (chain_bound): an intermediate of the kernel equals the reference's unless
the deviation of its pre-rounding value can reach a rounding boundary; see chain_bound."""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}          # unit roundoff of the storage types (half a unit in the last place)
_FORMAT = {"bf16": (8, -126), "fp16": (11, -14)}                     # (significant bits, exponent of the smallest normal number)
TANH_TERM = 2.0 ** -21
MISMATCH_CAP = 0.02   # the project's figure for "differ in rare last-place roundings only" (tests/test_gpu_parity.py, kernel against kernel)


def quantum(t, dtype):
    """Spacing of the storage type's numbers around each (float64) value: 2^(e - p + 1), e clamped to the smallest normal exponent."""
    p, emin = _FORMAT[dtype]
    a = t.double().abs()
    _, e = torch.frexp(a)                                  # a = m 2^e, m in [0.5, 1): the leading bit is 2^(e - 1)
    e = torch.where(a == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(a), e - (p - 1))


def round64(t, dtype):
    """Round-to-nearest-even of a float64 tensor to the storage type, WITHOUT passing through fp32 (no double rounding); float64 out."""
    if dtype == "fp32":
        return t.double().float().double()
    q = quantum(t, dtype)
    return torch.round(t.double() / q) * q                 # (torch.round is half-to-even; the scaling by a power of two is exact)


def storage_round(t, dtype, as_f16=False):
    """What a kernel stores of an fp32 tensor: bf16 / IEEE f16 round-to-nearest-even, fp32 = identity (`as_f16`: a bf16 model's tensor
    that is kept as f16).  A float64 tensor is rounded directly (round64)."""
    if t.dtype == torch.float64:
        return round64(t, "fp16" if (as_f16 and dtype != "fp32") else dtype)
    if dtype == "fp32":
        return t.clone()
    if dtype == "bf16" and not as_f16:
        return t.bfloat16().float()
    return t.half().float()


def conv64(x, w, b=None, stride=1):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=1)


def activation(v, act):
    if act == "none":
        return v
    if act == "relu":
        return v.relu()
    if act == "tanh01":
        return (torch.tanh(v) + 1) / 2
    raise ValueError(act)


def conv_layer(x, w, b, stride=1, act="none"):
    """float64 conv2d (pad 1) + activation on pre-rounded x, w and the fp32 bias."""
    return activation(conv64(x, w, b, stride), act)


def _accumulation(x_abs, w, b, stride, fp32_products):
    n = 9 * w.shape[1] + 1
    terms = conv64(x_abs, w.abs(), None if b is None else b.abs(), stride)
    return (2 * n if fp32_products else n) * U32 * terms


def _through_activation(d, act):
    return d / 2 + TANH_TERM if act == "tanh01" else d


def _stored(ref, d, store):
    return d + UNIT[store] * (ref.abs() + d) + (2.0 ** -25 if store == "fp16" else 0.0)


def conv_model(x, w, b, stride=1, act="none", store="fp32", fp32_products=False):
    """(ref, bound, d) of one layer: the float64 reference, the per-element worst case |kernel - ref| (module docstring) and its part
    d in front of the store (what the kernel's pre-rounding value may be off by).  `store`: the type the RESULT is rounded to;
    `fp32_products`: the operands are fp32 (fp32 mode), so the products round as well."""
    ref = conv_layer(x, w, b, stride, act)
    d = _through_activation(_accumulation(x.double().abs(), w, b, stride, fp32_products), act)
    return ref, _stored(ref, d, store), d


def conv_bound(x, w, b, stride=1, act="none", store="fp32", fp32_products=False):
    return conv_model(x, w, b, stride, act, store, fp32_products)[1]


def ulp_distance(got, want, dtype):
    """|got - want| in units of the last place of the smaller of the two (adjacent numbers across a binade are one apart)."""
    g, r = got.double(), want.double()
    return (g - r).abs() / quantum(torch.minimum(g.abs(), r.abs()), dtype)


def exact_match_share(got, ref64, dtype, d=None):
    """(share of elements with got != storage_round(ref64), largest distance of those in units of the last place).  A kernel that
    rounds to nearest differs from the rounded reference only where its fp32 sum and the float64 sum lie on two sides of a rounding
    boundary - rarely, and then by exactly one unit; a store that truncates differs in half of the elements.
    `d` (conv_model's third result): where the terms cancel, the result is small, its unit q is smaller than the accumulation error d
    of O(1) terms, and a correct kernel may be floor(d / q) + 1 units away (|round(v') - round(v)| <= |v' - v| + q).  With d given, the
    distance is reported minus floor(d / q): still "at most one" everywhere, and exactly the plain distance wherever d < q - which is
    everywhere but at such cancellations (fp32 summation of an f16 layer on the CPU: a result of 42 * 2^-24 from terms of size 1)."""
    want = round64(ref64, dtype)
    differ = got.double() != want
    if not differ.any():
        return 0.0, 0.0
    g, r = got.double()[differ], want[differ]
    units = ulp_distance(g, r, dtype)
    if d is not None:
        units = units - torch.floor(d.double().expand_as(want)[differ] / quantum(torch.minimum(g.abs(), r.abs()), dtype))
    return differ.double().mean().item(), units.max().item()


def boundary_distance(v, dtype):
    """Distance from each float64 value to the nearest rounding boundary (midpoint between two neighbouring numbers) of the storage
    type, never over-estimated.  With lo the largest number <= |v| and q the spacing of |v|'s binade the candidates are lo + q / 2
    (just below a power of two the real upper boundaries lie no nearer) and the midpoint BELOW lo, which is lo - q / 4 when lo is a
    power of two: the spacing of the binade below is half as wide."""
    a = v.double().abs()
    q = quantum(a, dtype)
    lo = torch.floor(a / q) * q
    q_low = torch.where(lo > 0, quantum((lo - q / 4).clamp_min(0), dtype), q)
    return torch.minimum((a - (lo + q / 2)).abs(), a - lo + q_low / 2)


def chain_bound(x, layers):
    """A chain of conv layers whose intermediates are stored ROUNDED.  layers: dicts with w, b, and optionally stride (1), act
    ("none"), store ("fp32"), fp32_products (False).  The float64 reference rounds every stored intermediate exactly as the
    kernel does (to nearest) and goes on from the rounded value.

    Recursion, element by element.  E_(k-1) >= 0 bounds |kernel's stored input - reference's stored input| of layer k (E_0 = 0).
    The kernel's pre-rounding value of layer k deviates from the reference's by at most
        D_k = delta_k + conv(E_(k-1), |w_k|),     delta_k = n 2^-24 (conv(|a_(k-1)| + E_(k-1), |w_k|) + |b_k|)
    (through the activation as in conv_bound).  If D_k is smaller than the distance from the float64 value to the nearest rounding
    boundary of the storage type (boundary_distance: the midpoints between neighbouring numbers), both round to the same number:
    E_k = 0.  The same holds behind a
    ReLU whose argument stays negative (pre + D_k <= 0: both store 0).  Otherwise E_k = D_k + one unit in the last place (half a unit
    for each of the two roundings, taken at |value| + D_k).  A layer stored as fp32 is not rounded: E_k = D_k.

    Returns a dict: ref (float64, the last layer's stored value), bound (per element, last layer), single (the last layer's bound
    with E = 0 in front of it: the single-layer size), touched (elements of the last layer that an upstream flipped rounding can
    reach: conv(E, |w|) > 0), flip_share (per layer: share of elements with E_k > 0)."""
    a = x.double()
    E = torch.zeros_like(a)
    out = {"flip_share": []}
    for L in layers:
        w, b = L["w"], L.get("b")
        stride, act, store, f32p = L.get("stride", 1), L.get("act", "none"), L.get("store", "fp32"), L.get("fp32_products", False)
        pre = conv64(a, w, b, stride)
        v = activation(pre, act)
        delta = _accumulation(a.abs() + E, w, b, stride, f32p)
        carried = conv64(E, w.abs(), None, stride) if bool((E > 0).any()) else torch.zeros_like(pre)
        D_pre = delta + carried
        D = _through_activation(D_pre, act)
        out["single"] = _stored(v, _through_activation(_accumulation(a.abs(), w, b, stride, f32p), act), store)
        out["bound"] = _stored(v, D, store)
        out["touched"] = carried > 0
        if store == "fp32":
            a, E = v, D
        else:
            q = quantum(v, store)
            k = torch.round(v / q)
            dist = boundary_distance(v, store)
            same = D < dist
            if act == "relu":
                same = same | (pre + D_pre <= 0)
            E = torch.where(same, torch.zeros_like(D), D + quantum(v.abs() + D, store))
            a = k * q
        out["flip_share"].append((E > 0).double().mean().item() if store != "fp32" else 1.0)
        out["ref"] = a
    return out


def sum_bound(terms_abs_sum, n):
    """fp32 sum of n fp32 terms in any order: n 2^-24 sum|terms| (the pool and the linear layer of context_encoding)."""
    return n * U32 * terms_abs_sum


def scaled_input(g, B, C, H, W):
    """x ~ N(0, 1) scaled PER INPUT CHANNEL by 2^k, k cycling over -3 .. 3: a lost or duplicated small-scale channel is not buried
    under the large ones, because the bound is per element and follows the scale."""
    scale = torch.tensor([2.0 ** ((c % 7) - 3) for c in range(C)]).view(1, C, 1, 1)
    return torch.randn(B, C, H, W, generator=g) * scale


def conv_weights(g, cout, cin):
    """w ~ N(0, 1 / (9 Cin)), b ~ 0.1 N(0, 1) (fp32)."""
    return torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, torch.randn(cout, generator=g) * 0.1


def impulse_case(cin, cout, stride, shift, g):
    """Known answer with zero tolerance (weight packing and tap geometry): integer weights in [-127, 127] (exact in bf16 and f16), x a
    field of unit impulses three apart - channel c has its single 1.0 at (3 (c // K) + 1, 3 (c % K) + 1) - so every output element is 0
    or exactly one weight w[o, c, i, j].  `shift`: the field is moved so that impulses lie on the last row and the last column (the
    image is one row and one column smaller: the former margin is gone); at stride 2 the two images put impulses on both parities.
    Returns (x [1, cin, H, W], w)."""
    K = max(1, int(cin ** 0.5 + 0.999))
    rows = (cin + K - 1) // K
    H, W = 3 * rows + (0 if shift else 1), 3 * K + (0 if shift else 1)
    x = torch.zeros(1, cin, H, W)
    for c in range(cin):
        x[0, c, 3 * (c // K) + (2 if shift else 1), 3 * (c % K) + (2 if shift else 1)] = 1.0
    w = torch.randint(-127, 128, (cout, cin, 3, 3), generator=g).float()
    return x, w


# ------------------------------------------------------------------------------------------------ the three-term f16 split (fp32x3)
# Every operand v of the split mode is carried as two IEEE f16 numbers, hi = f16(v) and lo = f16(v - hi) (the subtraction in fp32, where
# it is exact; both roundings to nearest even): the words the kernels store.  A layer contracts x_hi w_hi + x_hi w_lo + x_lo w_hi: 3 n
# exact products (n = 9 Cin) and the bias, 3 n + 1 fp32 additions in an order the kernel chooses, activation in fp32, and the result is
# split again (the planar tanh01 head returns fp32 and is not).
#   * conv_model_x3's reference ref3 is the float64 value of EXACTLY those terms through the activation, split as the kernel splits its
#     own value (carried64), so it pins all three terms and both halves of both operands.  What separates a correct kernel from it: its
#     fp32 value v' is within D = (3 n + 1) 2^-24 (sum|terms| + |b|) of the float64 value v (through the activation: _through_activation),
#     and two values D apart are split into carried values at most D plus ONE step q of lo apart (|round(v') - round(v)| <= |v' - v| + q).
#     q <= 2^-22 |v| while lo is normal (|lo| <= half a unit of hi, so lo's own unit is 2^-11 of that or less) and q = 2^-24, the
#     subnormal step, below:  bound = D + max(2^-22 (|ref3| + D), 2^-24).  (2^-25, half that step, is what separates carried(v') from
#     v' ITSELF - split_error -; against a reference that is split too, a whole step is possible.)
#   * sigma: the same terms as standard deviations, as tests/test_gpu_mdcn.py::error_model takes them - independent roundings, a random
#     walk over the partial sums.  Each of the N = 3 n + 1 additions rounds its partial sum p_k by at most 2^-24 |p_k|, uniformly:
#     standard deviation <= 2^-24 |p_k| / sqrt(3), so s_acc^2 = 2^-48 / 3 * sum_k p_k^2.  In a random order p_k is the bias, plus
#     the share k / N of the final sum v - b (the terms' common drift), plus a random walk of k terms of mean square T2 / N (T2 = sum of
#     the squared terms): sum_k p_k^2 = N (b^2 + (v - b)^2 / 3 + T2 / 2).  (error_model's shortcut "1 / n of the worst case, x 3" is
#     this with b = 0 and unbiased terms; it is too small by up to sqrt(N) where ONE term carries the partial sums - a bias of 0.1 over
#     an input of 1e-3: the CPU kernel of tests/test_rounding_model_cpu.py reached rms z = 1.1 with it at 256 -> 256 - and 3.6 times
#     too wide in the ordinary case.)  A kernel that adds blocks of exact products (an MFMA adds 16) rounds fewer partial sums.
#     The output's split turns a deviation delta = v' - v into 0 or +-q while |delta| < q (the two round across one of lo's boundaries
#     with probability |delta| / q) and into delta plus two independent roundings above.  Its mean square, q |delta|, is small, but the
#     distribution is two-valued: WHETHER an element takes the step is decided by where v lies between two boundaries, not by the
#     kernel, and one step at one of the 4 .. 36 elements of a 1 x 1 case would fill rms(z) <= 1 alone if sigma were any smaller than
#     the step.  So the split enters with its resolution, the whole step: sigma^2 = s_acc^2 + q^2 - an error of one step of lo at an
#     element says nothing about a defect; everything the mutants of tests/test_rounding_model_cpu.py do is 2^8 .. 2^10 steps.
#     What the kernel's tanh is off by is uniform inside
#     TANH_TERM: / sqrt(3).  Gates: rms(z) <= Z_RMS and max|z| <= Z_MAX with z = err / sigma (error_model's thresholds).
#   * accuracy_bound_x3: how far ref3 is from the float64 convolution of the UNSPLIT operands (tests/deform_model.py, bound_x3):
#     |v - (hi + lo)| <= 2^-22 |v| while lo is a normal f16 number and <= 2^-25 absolutely once it is subnormal (every |v| < 2^-3), and
#     w_hi x_hi + w_lo x_hi + w_hi x_lo = (w_hi + w_lo)(x_hi + x_lo) - w_lo x_lo with |w_lo x_lo| <= 2^-22 |w x|: per product
#     3 * 2^-22 |w x| + 2^-25 (|w| + |x|), to first order.  Needs |v| <= 65504 (above 65520, f16(v) is infinite).
Z_RMS, Z_MAX = 1.0, 6.0
U22 = 2.0 ** -22
F16_MAX = 65504.0


def split22(v):
    """(hi, lo) of an fp32 tensor as fp32 tensors holding f16 values: hi = f16(v), lo = f16(v - hi)."""
    v = v.float()
    hi = v.half().float()
    return hi, (v - hi).half().float()


def carried(v):
    """float64 hi + lo: the value the two halves carry (exact in fp32 as well: lo is a multiple of v's own last place)."""
    hi, lo = split22(v)
    return hi.double() + lo.double()


def split_error(v_abs):
    """|v' - carried(v')| <= max(2^-22 |v'|, 2^-25)."""
    return (U22 * v_abs).clamp_min(2.0 ** -25)


def carried64(v):
    """carried() of a float64 value without passing through fp32: hi = round64(v), lo = round64(v - hi)."""
    hi = round64(v, "fp16")
    return hi + round64(v.double() - hi, "fp16")


def terms_x3(x, w, b, stride):
    """(pre-activation float64 sum of the three terms and the bias, sum of their absolute values, sum of the products' squares)."""
    xh, xl = split22(x)
    wh, wl = split22(w)
    pre = conv64(torch.cat([xh, xh, xl], dim=1), torch.cat([wh, wl, wh], dim=1), b, stride)
    mag = conv64(torch.cat([xh, xl], dim=1).abs(), torch.cat([wh.abs() + wl.abs(), wh.abs()], dim=1), None if b is None else b.abs(), stride)
    sq = conv64(torch.cat([xh, xl], dim=1) ** 2, torch.cat([wh ** 2 + wl ** 2, wh ** 2], dim=1), None, stride)
    return pre, mag, sq


def accumulation_variance(n, start, drift, sq):
    """Variance of an fp32 sum of n terms added one at a time in a random order (the section comment above, s_acc^2): every partial sum
    rounds uniformly within 2^-24 of itself, and the partial sums are `start` (what the accumulator begins with: the bias), the share
    k / n of `drift` (the final sum less the start) and a random walk over terms whose squares add up to `sq`:
    2^-48 / 3 * n (start^2 + drift^2 / 3 + sq / 2).  THE one place this expression stands: single layers, chains, the deformable
    contraction, the pool and the Linear of context_encoding all take it from here."""
    return U32 ** 2 * (n / 3) * (start ** 2 + drift ** 2 / 3 + sq / 2)


def conv_model_x3(x, w, b, stride=1, act="none", with_truth=True):
    """(ref3, bound, sigma, truth) of one split layer on fp32 operands x, w and the fp32 bias (see the section comment above): ref3 the
    float64 value of the three terms through the activation and the output's split (the planar tanh01 head: fp32, not split), bound
    the per-element worst case |kernel - ref3| of a correct kernel, sigma the same terms as standard deviations, truth the float64
    layer on the unsplit operands."""
    n = 9 * w.shape[1]
    pre, mag, sq = terms_x3(x, w, b, stride)
    v = activation(pre, act)
    D = _through_activation((3 * n + 1) * U32 * mag, act)
    b2 = 0.0 if b is None else b.double().view(1, -1, 1, 1)
    s_acc = torch.sqrt(accumulation_variance(3 * n + 1, b2, pre - b2, sq)) * (0.5 if act == "tanh01" else 1.0)
    if act == "tanh01":      # planar fp32 head: no split behind it
        ref3, bound, sigma = v, D, torch.sqrt(s_acc ** 2 + TANH_TERM ** 2 / 3)
    else:
        ref3 = carried64(v)
        q = (U22 * (ref3.abs() + D)).clamp_min(2.0 ** -24)
        bound, sigma = D + q, torch.sqrt(s_acc ** 2 + q ** 2)
    return ref3, bound, sigma, conv_layer(x, w, b, stride, act) if with_truth else None


def chain_stats_x3(a, layers):
    """A chain of split layers whose intermediates are not visible: (ref, bound, sd) of its last layer on the fp32 input a.  The float64
    reference goes on from its own carried intermediates.
      * bound, rigorous and COARSE: every layer's worst case is carried forward, E_k = bound_k + conv(E_(k-1), |w_k|) + 2^-21 conv(|a|,
        |w_k|) (the halves of an intermediate that deviates are other halves: the dropped lo x lo term) + 2^-24 |ref_k| (the reference's
        carried value is handed on as fp32).  Worst cases of 1729 additions multiplied through two more layers: some 1e-1 .. 1 of the
        result, as the 16-bit chain bound of tests/test_gpu_conv_rounding_model.py.
      * sd, the same chain in standard deviations (conv_model_x3's terms; independent errors add in squares: V_k = s_acc^2 + q^2 +
        conv(V_(k-1), w_k^2); other halves where a lo is exactly half a unit, some 2^-12 of the elements: 2^-12 (2^-21)^2 conv(a^2,
        w^2)): what the z gates of the single layers become for a chain.
    A layer may add `pre`, (value, bound, variance) of a float64 term the accumulator starts from beside the bias (the folded context
    half).  The last layer may be `planar` (fp32 output, no split)."""
    E = V = None
    for L in layers:
        w, b, act, stride = L["w"], L["b"], L["act"], L.get("stride", 1)
        N = 3 * 9 * w.shape[1] + 1
        pre, mag, sq = terms_x3(a, w, b, stride)
        start = b.double().view(1, -1, 1, 1)
        drift = pre - start
        D, var = N * U32 * mag, 0.0
        if "pre" in L:
            pre, D, var, start = pre + L["pre"][0], D + L["pre"][1], L["pre"][2], start + L["pre"][0]
        var = var + accumulation_variance(N, start, drift, sq)
        wa, w2 = w.double().abs() * (1 + 2.0 ** -11), w.double() ** 2
        D = D + 2.0 ** -21 * conv64(a.abs(), wa, None, stride) + (conv64(E, wa, None, stride) if E is not None else 0.0)
        var = var + 2.0 ** -54 * conv64(a.double() ** 2, w2, None, stride) + (conv64(V, w2, None, stride) if V is not None else 0.0)
        v = activation(pre, act)
        D = _through_activation(D, act)
        if act == "tanh01":
            var = var / 4 + TANH_TERM ** 2 / 3
        if L.get("planar"):
            return v, D, torch.sqrt(var)
        ref = carried64(v)
        q = (U22 * (ref.abs() + D)).clamp_min(2.0 ** -24)
        E, V = D + q + U32 * ref.abs(), var + q ** 2 + (U32 * ref) ** 2 / 3
        a = ref.float()
    return ref, E, torch.sqrt(V)


POOL_REACH = 16


def pool_linear_model_x3(c2, sd_c2, lw, lb):
    """(ref, bound, sigma) of context_encoding's tail in the split mode on a given last intermediate c2 [B, C, h, w] (fp32, carried by
    its [hi | lo] halves): AdaptiveAvgPool2d(1) as fp32 sums over the pixels of the DOUBLED channels (hi and lo apart), the fold that
    adds the two sums and divides, and the fp32 Linear (FMAs on the fp32 weights lw [m, C], bias lb).  ref is float64 of carried(c2).
    `sd_c2`: the standard deviation with which the c2 the kernel pooled deviates, per element, from a float64 chain reference
    (chain_stats_x3) - the given c2 is ANOTHER correct kernel's, so the two are 2 sd_c2^2 apart.
      * bound: the pool adds 2 npix f16 values per channel and divides (sum_bound over |hi| + |lo|, one rounding more), the Linear C
        products and the bias (2 (C + 1) 2^-24 sum|terms|, as counted for rounded products), the mean's bound through |lw|, and Z_MAX
        standard deviations of the c2 difference taken through the mean with NO averaging (as if every pixel deviated alike).
      * sigma, three parts in squares.  The pool: accumulation_variance of 2 npix + 1 additions whose drift is the channel's whole sum
        (ReLU outputs: the partial sums grow with every term - a sequential sum, the widest order there is), over npix^2, and the
        division's rounding.  The Linear: accumulation_variance of C + 1 FMAs from the bias, as conv_model_x3's s_acc.  The c2
        difference: its sources are roundings of single elements of feat, c0, c1 and c2, independent of one another, and one such
        source reaches at most POOL_REACH = 16 pixels of c2 (an element of c1: the 3 x 3 around it; one of c0: 2 x 2 of c1 under
        stride 2, hence 4 x 4 of c2; one of feat: 2 x 2 of c0 in two adjacent rows and columns, which again feed 2 x 2 of c1).  With
        e_p = sum_s a_ps eps_s and at most R non-zero a_ps per source, (sum_p a_ps)^2 <= R sum_p a_ps^2 (Cauchy-Schwarz):
        var(mean_p e_p) <= min(R, npix) / npix * mean_p var(e_p).  Both enter the Linear through lw^2.
    A lo half that the pool or the fold loses is a mean of npix values of up to 2^-12 |c2| with no common sign: 2^-12 / sqrt(3 npix) of
    the channel's size, some 1e-5 of |ctx| at 162 pixels and 1e-4 at one - inside the bound and outside the z gates: rms z 5.0 at 162
    pixels, 6.4 at 45, 19 at one, where a correct pool stays below 0.1 (tests/test_rounding_model_cpu.py)."""
    hi, lo = split22(c2)
    h, l = hi.double(), lo.double()
    npix = c2.shape[2] * c2.shape[3]
    S = (h + l).sum(dim=(2, 3))
    mean = S / npix
    d_mean = sum_bound((h.abs() + l.abs()).sum(dim=(2, 3)), 2 * npix + 1) / npix + U32 * mean.abs()
    var_mean = accumulation_variance(2 * npix + 1, 0.0, S, (h ** 2 + l ** 2).sum(dim=(2, 3))) / npix ** 2 + (U32 * mean) ** 2 / 3
    var_diff = (2 * sd_c2 ** 2).mean(dim=(2, 3))
    lw, lb = lw.double(), lb.double()
    n = lw.shape[1] + 1
    ref = mean @ lw.t() + lb
    bound = 2 * n * U32 * ((mean.abs() + d_mean) @ lw.abs().t() + lb.abs()) + d_mean @ lw.abs().t() + Z_MAX * (var_diff @ (lw ** 2).t()).sqrt()
    var = accumulation_variance(n, lb, ref - lb, (mean ** 2) @ (lw ** 2).t()) + (var_mean + min(POOL_REACH, npix) / npix * var_diff) @ (lw ** 2).t()
    return ref, bound, var.sqrt()


def accuracy_bound_x3(x, w, b, stride=1, act="none"):
    """|ref3 - truth| per element: 3 * 2^-22 sum|w x| + 2^-25 (sum|w| + sum|x|) over the receptive field (the zero padding adds
    nothing), through the activation's Lipschitz constant, and the output's own split (split_error) where there is one."""
    xa, wa = x.double().abs(), w.double().abs()
    ones_x, ones_w = (xa > 0).double(), (wa > 0).double()          # an operand that is exactly zero is carried exactly
    a = 3 * U22 * conv64(xa, wa, None, stride) + 2.0 ** -25 * (conv64(ones_x, wa, None, stride) + conv64(xa, ones_w, None, stride))
    return a / 2 if act == "tanh01" else a + split_error(conv_layer(x, w, b, stride, act).abs() + a)


def z_gates(got, ref3, bound, sigma):
    """(max err / bound, rms z, max |z|) over EVERY element."""
    err = got.double() - ref3
    z = err / sigma
    return (err.abs() / bound).max().item(), z.pow(2).mean().sqrt().item(), z.abs().max().item()


def impulse_case_x3(cin, cout, stride, shift, g, scale=1.0):
    """impulse_case for the split: impulses of 1 + 3 * 2^-13 (hi = 1, lo = 3 * 2^-13, no rounding tie) and weights k + lo_w with k in
    [-7, 7] \\ {0} and lo_w = sign(k) j ulp16(k) / 2048, j = 1 + (flat index of (o, c, tap)) mod 1023 - |lo_w| < ulp16(k) / 2, so w_hi = k and
    w_lo = lo_w exactly, non-zero and different from that of every entry fewer than 1023 places away.  Every output element is 0 or
    x_hi w_hi + x_hi w_lo + x_lo w_hi of ONE weight: 22 bits at most, exact in fp32 in any order.  `scale` (a power of two >= 1 / 4:
    lo_w stays a multiple of 2^-24, the subnormal step) keeps tanh01 away from saturation.  Returns (x, w, want) with want the float64
    pre-activation value of every output element."""
    x, _ = impulse_case(cin, cout, stride, shift, g)
    x = x * (1 + 3 * 2.0 ** -13)
    k = torch.randint(1, 8, (cout, cin, 3, 3), generator=g).double() * (torch.randint(0, 2, (cout, cin, 3, 3), generator=g).double() * 2 - 1)
    idx = torch.arange(cout * cin * 9, dtype=torch.float64).view(cout, cin, 3, 3)
    low = torch.sign(k) * (1 + idx % 1023) * quantum(k, "fp16") / 2048     # away from zero: towards it, below a power of two, the unit halves
    w = ((k + low) * scale).float()
    assert torch.equal(w.double(), (k + low) * scale)
    xh, xl = split22(x)
    wh, wl = split22(w)
    assert torch.equal(wh.double(), k * scale) and torch.equal(wl.double(), low * scale) and bool((xl[x != 0] == 3 * 2.0 ** -13).all())
    want = conv64(torch.cat([xh, xh, xl], dim=1), torch.cat([wh, wl, wh], dim=1), None, stride)
    return x, w, want
