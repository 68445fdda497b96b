"""A float64 reference of the 3x3 convolution layers and the worst-case error a correct 16-bit / fp32 kernel may show against it.
Plain torch on the CPU; knows nothing of the library (tests/test_rounding_model_cpu.py tests this module with the CPU as "kernel",
tests/test_gpu_conv_rounding_model.py gates the HIP kernels with it, tests/test_gpu_mdcn.py shares storage_round).

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
