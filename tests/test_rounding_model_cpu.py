"""The rounding model (tests/rounding_model.py) tested on its own, with the CPU as the "kernel": fp32 F.conv2d on the rounded
operands, activation, storage_round - a correct kernel in one particular summation order.  For every (Cin, Cout, stride) class that
tests/test_gpu_conv_rounding_model.py runs on the GPU:
  * the clean result stays inside the gates (err / bound <= 1 for every element, mismatch share <= 2 %, mismatches one unit);
  * every defect injected into it FAILS the gate that is meant to catch it: a truncating store (the mismatch share), one output
    channel's bias 10 % wrong, one corner pixel that loses 4 of its 9 x Cin products (the bound), one single element two units off
    (the distance in units of the last place).
A gate that no injected defect can fail would be a failed test.
chain_bound: two- and three-layer chains with rounded intermediates in two summation orders (fp32 against float64 accumulation)."""
import pytest
import torch
import torch.nn.functional as F

from conv_cases import X3_PAIRS, X3_SCALES, split_sweep, x3_act, x3_layer, x3_pair_id, x3_shapes
from rounding_model import (F16_MAX, MISMATCH_CAP, U22, UNIT, Z_MAX, Z_RMS, accuracy_bound_x3, carried, chain_bound, chain_stats_x3, conv64, conv_bound, conv_layer,
                            conv_model, conv_model_x3, conv_weights, exact_match_share, impulse_case, impulse_case_x3, pool_linear_model_x3, quantum, round64,
                            scaled_input, split22, split_error, storage_round, z_gates)

# (Cin, Cout, stride, act): the classes of the GPU file's families
CLASSES = [(6, 64, 1, "relu"), (8, 8, 1, "none"), (8, 16, 2, "relu"), (11, 27, 1, "none"), (35, 32, 1, "relu"), (67, 27, 1, "none"),
           (64, 32, 1, "relu"), (64, 24, 1, "none"), (64, 2, 1, "none"), (64, 64, 1, "relu"), (64, 48, 1, "none"), (64, 33, 1, "relu"),
           (65, 64, 1, "none"), (66, 40, 1, "relu"), (67, 64, 1, "relu"), (64, 128, 2, "relu"), (64, 100, 2, "none"),
           (128, 256, 2, "relu"), (256, 256, 1, "relu"), (192, 250, 1, "none"), (160, 256, 2, "none"), (32, 3, 1, "tanh01")]


def cpu_kernel(xs, ws, b, stride, act, store, pre_hook=None, post_hook=None):
    """fp32 convolution of the rounded operands, activation, store (hooks: where the defects go in)."""
    v = F.conv2d(xs, ws, b, stride=stride, padding=1)
    if pre_hook is not None:
        v = pre_hook(v)
    v = F.relu(v) if act == "relu" else ((torch.tanh(v) + 1) / 2 if act == "tanh01" else v)
    return post_hook(v) if post_hook is not None else storage_round(v, store)


def truncating_store(v, store):
    """Drop the low 16 (bf16) / 13 (f16) mantissa bits instead of rounding to nearest."""
    bits = v.contiguous().view(torch.int32) & (-65536 if store == "bf16" else -8192)
    return bits.view(torch.float32)


def make(cin, cout, stride, dtype, H=9, W=13, seed=0):
    g = torch.Generator().manual_seed(seed + cin * 131 + cout)
    x = scaled_input(g, 2, cin, H, W)
    w, b = conv_weights(g, cout, cin)
    return storage_round(x, dtype), storage_round(w, dtype), b


def gates(got, xs, ws, b, stride, act, dtype, store):
    ref, bound, d = conv_model(xs, ws, b, stride, act, store, fp32_products=dtype == "fp32")
    ratio = ((got.double() - ref).abs() / bound).max().item()
    share, ulps = exact_match_share(got, ref, store, d) if store != "fp32" else (0.0, 0.0)
    return ratio, share, ulps


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("case", CLASSES)
def test_clean_result_is_inside_the_gates_and_every_defect_outside(case, dtype):
    """measured (this file, all classes): clean ratio up to 0.988 in the 16-bit types (the store's half unit dominates; 0.004 for the fp32
    planar head), <= 0.036 in fp32; mismatch share <= 0.43 % at these small shapes, every mismatch one unit."""
    cin, cout, stride, act = case
    store = "fp32" if (dtype == "fp32" or act == "tanh01") else dtype
    xs, ws, b = make(cin, cout, stride, dtype)
    clean = cpu_kernel(xs, ws, b, stride, act, store)
    ratio, share, ulps = gates(clean, xs, ws, b, stride, act, dtype, store)
    print(f"{case} {dtype}: clean ratio {ratio:.3f}, mismatches {100 * share:.3f} % (<= {ulps:.0f} units)")
    assert ratio <= 1.0 and share <= MISMATCH_CAP and ulps <= 1.0

    # one output channel's bias 10 % wrong (the channel with the largest bias: a 10 % error of a bias near 0 is below the rounding)
    o = int(b.abs().argmax())
    b_bad = b.clone(); b_bad[o] *= 1.1
    r_bias = gates(cpu_kernel(xs, ws, b_bad, stride, act, store), xs, ws, b, stride, act, dtype, store)[0]
    # the last pixel of sample 1 loses the products of the last four input channels at the centre tap
    Ho, Wo = clean.shape[2:]

    def lose(v):
        v = v.clone()
        yy, xx = (Ho - 1) * stride, (Wo - 1) * stride
        v[1, :, Ho - 1, Wo - 1] -= (ws[:, -4:, 1, 1] * xs[1, -4:, yy, xx]).sum(dim=1)
        return v
    r_lost = gates(cpu_kernel(xs, ws, b, stride, act, store, pre_hook=lose), xs, ws, b, stride, act, dtype, store)[0]
    print(f"    bias 10 %: ratio {r_bias:.1f}; 4 lost products at one pixel: ratio {r_lost:.1f}")
    assert r_bias > 1.0 and r_lost > 1.0
    if store == "fp32":
        return
    # the store truncates: half of the elements are one unit off - the bound alone may not see it (it is dominated by delta at large Cin)
    r_tr, s_tr, _ = gates(cpu_kernel(xs, ws, b, stride, act, store, post_hook=lambda v: truncating_store(v, store)), xs, ws, b, stride, act, dtype, store)
    # ONE element two units in the last place off - the one whose unit is coarsest against delta (where delta exceeds the unit, at
    # Cin >= 192 in f16 for the largest values, no derived gate can pin the last place: floor(d / q) units are the model's own slack)
    one = clean.clone()
    d = conv_model(xs, ws, b, stride, act, store)[2]
    idx = int((quantum(clean, store) / d).argmax())
    assert (quantum(clean, store) / d).view(-1)[idx] > 1.0
    one.view(-1)[idx] += 2 * quantum(one.view(-1)[idx], store).float()
    r_one, s_one, u_one = gates(one, xs, ws, b, stride, act, dtype, store)
    print(f"    truncating store: ratio {r_tr:.2f}, mismatches {100 * s_tr:.1f} %; one element two units off: ratio {r_one:.2f}, {u_one:.0f} units")
    assert s_tr > MISMATCH_CAP
    assert u_one > 1.0          # (the bound alone would let it pass at Cin >= 192 in f16, ratio 0.9: delta dominates it there)


def test_round64_is_the_storage_rounding():
    """round64 on fp32 values equals torch's own casts (the definition tests/test_gpu_mdcn.py uses), subnormals and ties included."""
    g = torch.Generator().manual_seed(1)
    t = torch.cat([torch.randn(4096, generator=g) * s for s in (1e-7, 1e-5, 1e-3, 1.0, 300.0)] + [torch.tensor([0.0, 1.0, 1.00390625, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25])])
    for dtype in ("bf16", "fp16"):
        assert torch.equal(round64(t.double(), dtype), storage_round(t, dtype).double())
        assert torch.equal(storage_round(t.double(), dtype), storage_round(t, dtype).double())
    assert torch.equal(storage_round(t, "bf16", as_f16=True), t.half().float()) and torch.equal(storage_round(t, "fp32"), t)


def test_impulse_fields_have_one_weight_per_output_element():
    g = torch.Generator().manual_seed(2)
    for cin, stride in ((6, 1), (64, 1), (67, 1), (64, 2), (160, 2)):
        for shift in (False, True):
            x, w = impulse_case(cin, 5, stride, shift, g)
            assert x.sum() == cin and (x.sum(dim=(0, 1)) <= 1).all()
            if shift:
                assert x[0, :, -1, :].sum() > 0 and x[0, :, :, -1].sum() > 0
            y = F.conv2d(x, w, padding=1, stride=stride)
            hits = F.conv2d(x, torch.ones_like(w), padding=1, stride=stride)
            assert hits.max() <= 1 and torch.equal(y, y.round()) and y.abs().max() <= 127
            for dtype in ("bf16", "fp16"):
                assert torch.equal(storage_round(y, dtype), y)


def chain_kernel(xs, layers, accumulate):
    a = xs
    for L in layers:
        v = F.conv2d(a.to(accumulate), L["w"].to(accumulate), L["b"].to(accumulate), stride=L.get("stride", 1), padding=1)
        v = F.relu(v) if L["act"] == "relu" else ((torch.tanh(v) + 1) / 2 if L["act"] == "tanh01" else v)
        a = storage_round(v.float(), L["store"]) if accumulate == torch.float32 else storage_round(v, L["store"]).float()
    return a


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("widths", [(67, 64, 32), (64, 64, 64), (67, 64, 32, 3), (64, 128, 256, 256)])
def test_chain_bound_holds_between_two_summation_orders(widths, dtype):
    """Two correct "kernels" - fp32 and float64 accumulation, both with intermediates rounded to the storage type - against the chain
    model: every element inside chain_bound, and the elements outside the single-layer bound are no more than the model says an
    upstream flipped rounding can reach.  (67, 64, 32, 3) is reconstruction with its fp32 tanh01 head, (64, 128, 256, 256) the
    context convolutions at strides 2, 2, 1."""
    g = torch.Generator().manual_seed(len(widths) * 7 + widths[1])
    xs = storage_round(scaled_input(g, 2, widths[0], 17, 23), dtype)
    layers = []
    for k in range(1, len(widths)):
        w, b = conv_weights(g, widths[k], widths[k - 1])
        head = widths[k] == 3
        layers.append({"w": storage_round(w * 1.4, dtype), "b": b, "stride": 2 if widths[k] > widths[k - 1] else 1,
                       "act": "tanh01" if head else "relu", "store": "fp32" if head else dtype})
    m = chain_bound(xs, layers)
    for acc in (torch.float32, torch.float64):
        got = chain_kernel(xs, layers, acc)
        err = (got.double() - m["ref"]).abs()
        ratio = (err / m["bound"]).max().item()
        outside = (err > m["single"]).double().mean().item()
        touched = m["touched"].double().mean().item()
        print(f"{widths} {dtype} {acc}: ratio {ratio:.3f}; outside the single-layer bound {100 * outside:.4f} %, reachable {100 * touched:.3f} %; "
              f"flip shares {['%.4f %%' % (100 * s) for s in m['flip_share']]}")
        assert ratio <= 1.0
        assert outside <= touched
        assert not (err > m["single"])[~m["touched"]].any()
    assert (chain_kernel(xs, layers, torch.float64).double() - m["ref"]).abs().max().item() <= 2.0 ** -24   # the float64 order IS the reference (an fp32 head: to its rounding)


def test_a_dropped_intermediate_pixel_leaves_the_chain_bound():
    """A defect in the MIDDLE of a chain - one pixel of the stored intermediate is zero in all channels, as a ring row that misses a
    column would leave it - is outside chain_bound at the nine output pixels it reaches.  (chain_bound is rigorous, not tight: with the
    worst-case delta a flipped rounding is POSSIBLE in 15 % (bf16) to 45 % (f16) of a layer's elements, so a single intermediate that is
    two units off stays inside it - ratio 0.89 here; the single layers are what pins the last place.)"""
    g = torch.Generator().manual_seed(5)
    xs = storage_round(scaled_input(g, 1, 64, 9, 11), "bf16")
    layers = []
    for cout, cin in ((64, 64), (32, 64)):
        w, b = conv_weights(g, cout, cin)
        layers.append({"w": storage_round(w, "bf16"), "b": b, "act": "relu", "store": "bf16"})
    m = chain_bound(xs, layers)
    mid = storage_round(F.relu(F.conv2d(xs, layers[0]["w"], layers[0]["b"], padding=1)), "bf16")
    clean = storage_round(F.relu(F.conv2d(mid, layers[1]["w"], layers[1]["b"], padding=1)), "bf16")
    assert ((clean.double() - m["ref"]).abs() / m["bound"]).max().item() <= 1.0
    mid[0, :, 4, 5] = 0
    got = storage_round(F.relu(F.conv2d(mid, layers[1]["w"], layers[1]["b"], padding=1)), "bf16")
    bad = (got.double() - m["ref"]).abs() / m["bound"] > 1.0
    assert bad.any() and not bad[:, :, :3].any() and not bad[:, :, :, 7:].any()
    assert UNIT["bf16"] == 2.0 ** -8


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_dropped_intermediate_pixel_leaves_the_bound_of_the_tanh01_chain(dtype):
    """The chain the GPU test holds the fused reconstruction tail to - r1 (64 -> 32, ReLU, rounded) -> r2 (32 -> 3, tanh01, fp32) from
    a given r0 -: clean inside, one pixel of the stored r1 zeroed outside, at the output pixels it reaches and nowhere else."""
    g = torch.Generator().manual_seed(9)
    r0 = storage_round(torch.randn(1, 64, 9, 11, generator=g).relu(), dtype)
    layers = []
    for cout, cin, act, store in ((32, 64, "relu", dtype), (3, 32, "tanh01", "fp32")):
        w, b = conv_weights(g, cout, cin)
        layers.append({"w": storage_round(w * 1.4, dtype), "b": b, "act": act, "store": store})
    m = chain_bound(r0, layers)
    r1 = storage_round(F.relu(F.conv2d(r0, layers[0]["w"], layers[0]["b"], padding=1)), dtype)
    head = lambda t: (torch.tanh(F.conv2d(t, layers[1]["w"], layers[1]["b"], padding=1)) + 1) / 2
    assert ((head(r1).double() - m["ref"]).abs() / m["bound"]).max().item() <= 1.0
    r1[0, :, 4, 5] = 0
    bad = (head(r1).double() - m["ref"]).abs() / m["bound"] > 1.0
    print(f"{dtype}: {int(bad.sum())} elements outside; r1 roundings that may flip {100 * m['flip_share'][0]:.1f} %")
    assert bad.any() and not bad[:, :, :3].any() and not bad[:, :, :, 7:].any()


# ---------------------------------------------------------------------------------------------------- the three-term f16 split (fp32x3)
def test_split22_properties_over_the_operand_sweep():
    """hi and lo are f16 numbers, |lo| is at most half a unit of hi, hi + lo is exact in fp32, within max(2^-22 |v|, 2^-25) of v (22 bits
    while lo is normal, an absolute 2^-25 below), exact for f16 numbers, odd in v, and splitting the carried value again carries the same
    value (the hi of a tie may move to the neighbour, the sum does not).  The header's figures as numbers: an operand of 0.02 is carried
    to 2^-25 / 0.02 = 2^-19.4, one of 1e-3 to 2^-15."""
    v = split_sweep()
    hi, lo = split22(v)
    assert torch.equal(hi, hi.half().float()) and torch.equal(lo, lo.half().float()) and torch.isfinite(hi).all()
    assert bool((lo.double().abs() <= quantum(hi, "fp16") / 2).all())
    c = carried(v)
    assert torch.equal((hi + lo).double(), c)                                                   # fp32 holds hi + lo exactly
    err = (c - v.double()).abs()
    assert bool((err <= split_error(v.double().abs())).all())
    normal_lo = lo.abs() >= 2.0 ** -14
    assert bool((err[normal_lo] <= U22 * v.double().abs()[normal_lo]).all()) and bool(normal_lo.any())
    assert not bool(normal_lo[v.abs() < 2.0 ** -3].any())                                       # below 2^-3 every lo is subnormal (or zero)
    exact = v == v.half().float()
    assert bool((lo[exact] == 0).all()) and bool(exact.any()) and bool((~exact).any())
    assert torch.equal(carried(-v), -c) and torch.equal(carried(c.float()), c)
    for x in (0.02, 1e-3):      # worst case over a binade's worth of neighbours of x
        t = torch.tensor(x) * (1 + torch.arange(4096, dtype=torch.float64) * 2.0 ** -23).float()
        rel = ((carried(t) - t.double()).abs() / t.double()).max().item()
        print(f"operand {x}: carried to 2^{torch.log2(torch.tensor(rel)).item():.1f} relative")
        assert rel <= 2.0 ** -25 / x and rel > 2.0 ** -22


X3_ACCURACY = [(6, 64, 1, "relu"), (11, 27, 1, "none"), (64, 64, 1, "none"), (67, 27, 1, "none"), (64, 128, 2, "relu"), (32, 3, 1, "tanh01")]


@pytest.mark.parametrize("case", X3_ACCURACY, ids=lambda c: f"{c[0]}to{c[1]}s{c[2]}{c[3]}")
def test_split_accuracy_statement_over_a_magnitude_sweep(case):
    """|ref3 - truth| <= 3 * 2^-22 sum|w x| + 2^-25 (sum|w| + sum|x|) per element (accuracy_bound_x3), x * 2^k and w * 2^k for k from
    -20 (every lo subnormal, most hi too) to the largest power that keeps |x| below 65504, and x scaled so that its largest magnitude IS
    65504.  Printed per k: the worst err / bound and the accuracy relative to sum|w x| in bits - the header's "22 bits" (reached: 2^-21.6 .. 2^-22
    of sum|w x| wherever both lo are normal; 2^-17 with Kaiming-scale weights at 2^-5 of theirs, 2^-14 .. 2^-17 with inputs of 1e-3,
    2^-5 .. 2^-8 at 2^-20 where only the hi halves are left) and what becomes of it below.  measured: err / bound <= 0.62 everywhere."""
    cin, cout, stride, act = case
    g = torch.Generator().manual_seed(cin * 17 + cout)
    x0 = scaled_input(g, 2, cin, 9, 13).clamp(-32, 32)
    w0, b = conv_weights(g, cout, cin)
    sweeps = [("x", k) for k in range(-20, 11, 3)] + [("w", k) for k in range(-20, 14, 3)] + [("x", "max")]
    for which, k in sweeps:
        if k == "max":
            x, w = (x0 / x0.abs().max() * F16_MAX).clamp(-F16_MAX, F16_MAX), w0
            assert x.abs().max().item() == F16_MAX
        else:
            x, w = (x0 * 2.0 ** k, w0) if which == "x" else (x0, w0 * 2.0 ** k)
        assert max(x.abs().max().item(), w.abs().max().item()) <= F16_MAX
        ref3, _, _, truth = conv_model_x3(x, w, b, stride, act)
        err = (ref3 - truth).abs()
        bound = accuracy_bound_x3(x, w, b, stride, act)
        terms = conv64(x.abs(), w.abs(), None, stride)
        ratio = (err / bound).max().item()
        bits = torch.log2((err / terms).max().clamp_min(2.0 ** -60)).item()
        print(f"{case} {which} * 2^{k}: err / bound max {ratio:.3f}; worst element at 2^{bits:.1f} of sum|w x|")
        assert torch.isfinite(ref3).all() and ratio <= 1.0


def cpu_kernel_x3(x, w, b, stride, act, mutant=None, seed=0, planar=False):
    """A correct split kernel in one particular order: the 3 n exact fp32 products of the halves in a SHUFFLED order, added to the bias
    sixteen at a time in fp32 (an MFMA's K), activation in fp32, the result split again - returned as fp32 hi + lo, which is exact.
    `mutant`: one of MUTANTS, the defects the GPU gates must be able to see."""
    xh, xl = split22(x)
    wh, wl = split22(w)
    cout, cin = w.shape[:2]
    if mutant == "x_lo zeroed in one 16-channel group":
        g0 = 16 * ((cin - 1) // 16 // 2)
        xl = xl.clone(); xl[:, g0:g0 + 16] = 0
    elif mutant == "x_hi * w_lo missing":
        wl = torch.zeros_like(wl)
    elif mutant == "x_lo of the last column from the pixel to its left":
        xl = xl.clone(); xl[..., -1] = xl[..., -2] if x.shape[3] > 1 else 0     # (one column: the pixel to the left is the zero padding)
    elif mutant == "w_lo of the centre tap from the next tap":
        wl = wl.clone(); wl[:, :, 1, 1] = wl[:, :, 1, 2]
    cols = lambda t: F.unfold(t, 3, padding=1, stride=stride)
    X = torch.cat([cols(xh), cols(xh), cols(xl)], dim=1)
    Wm = torch.cat([wh.reshape(cout, -1), wl.reshape(cout, -1), wh.reshape(cout, -1)], dim=1)
    perm = torch.randperm(Wm.shape[1], generator=torch.Generator().manual_seed(seed))
    acc = b.view(1, -1, 1).expand(x.shape[0], cout, X.shape[2]).clone()
    for i in range(0, perm.numel(), 16):
        idx = perm[i:i + 16]
        acc = acc + torch.matmul(Wm[:, idx], X[:, idx])
    Ho, Wo = (x.shape[2] + stride - 1) // stride, (x.shape[3] + stride - 1) // stride
    v = acc.view(x.shape[0], cout, Ho, Wo)
    v = F.relu(v) if act == "relu" else ((torch.tanh(v) + 1) / 2 if act == "tanh01" else v)
    if act == "tanh01" or planar:
        return v
    hi, lo = split22(v)
    return hi if mutant == "the output's lo dropped" else hi + lo


MUTANTS = ("x_lo zeroed in one 16-channel group", "x_hi * w_lo missing", "x_lo of the last column from the pixel to its left",
           "the output's lo dropped", "w_lo of the centre tap from the next tap")


X3_UNSEEN = {("64to2s1", (1, 1), -10, "x_lo zeroed in one 16-channel group")}   # and the planar head at 2^-10 and 2^10: see the test


@pytest.mark.parametrize("pair", X3_PAIRS, ids=x3_pair_id)
def test_split_gates_pass_a_correct_kernel_and_fail_every_mutant(pair):
    """For every channel pair, shape and activation tests/test_gpu_fp32x3_rounding_model.py runs (x3_layer: the same operands), at scale
    2^0 and, for the first shape, 2^-10 and 2^10: the correct kernel is inside BOTH gates (err / bound <= 1 for every element; rms z
    <= 1, max |z| <= 6) and every mutant is outside at least one of them - often NOT outside the hard bound, whose (3 n + 1) 2^-24
    sum|terms| is some 20 times a dropped term's effect at n = 577: the statistical gate is what sees them.
    Asserted in every case but those of X3_UNSEEN, where the mutant is printed only:
      * the planar head at 2^-10 and 2^10.  Its output is an fp32 number near 1/2 at 2^-10 (a pre-activation of 1e-3, of which a low
        half is 2^-12: 2e-7 of the output's own TANH_TERM) and 0 or 1 at 2^10, where the tanh is saturated whatever the convolution holds;
      * x_lo zeroed in one 16-channel group at 64 -> 2, 1 x 1, 2^-10: four output elements, each missing sixteen products x_lo w_hi of
        at most 2^-21 x 0.1 with no common sign - about ONE subnormal step of the output's lo (2^-24), which is sigma: the mutant is a
        step at three of the four elements, what a correct kernel may show at any one of them.
    Everything else at 2^-10, where every lo is subnormal and the output carries 2^-24 absolutely, is 2 .. 30 steps off at its worst
    element and outside the z gates (rms z 1.1 .. 12.6).
    measured over the 95 cases: correct kernel err / bound <= 0.57, rms z <= 0.26, max |z| <= 1.4; the mutants where they are asserted
    (cases; smallest rms z at 2^0 and where; smallest at 2^-10; largest; cases outside the hard bound):
      x_lo zeroed in one 16-channel group                  92;  14 (256 -> 256, 1 x 70);  1.1 (64 -> 128);  560;   34
      x_hi * w_lo missing                                  93;  61 (256 -> 256, 5 x 7);   1.7 (11 -> 27);   500;   64
      x_lo of the last column from the pixel to its left   93;  9.4 (256 -> 256, 1 x 70: one column of 70);  1.7 (11 -> 27);  560;   58
      the output's lo dropped                              88;  25 (64 -> 2, 1 x 1);      2.0 (11 -> 27);   530;   66 (the planar head has no lo)
      w_lo of the centre tap from the next tap             93;  34 (256 -> 256, 5 x 7);   2.3 (64 -> 2);    1350;  59"""
    cin, cout, stride, head = pair
    for i, (H, W) in enumerate(x3_shapes(stride)):
        act = x3_act(pair, i)
        for k in (X3_SCALES if i == 0 else X3_SCALES[:1]):
            x, w, b = x3_layer(pair, H, W, k)
            ref3, bound, sigma, _ = conv_model_x3(x, w, b, stride, act)
            ratio, rms, zmax = z_gates(cpu_kernel_x3(x, w, b, stride, act), ref3, bound, sigma)
            print(f"{x3_pair_id(pair)} {act} {H}x{W} 2^{k}: correct kernel err / bound {ratio:.3f}, rms z {rms:.3f}, max |z| {zmax:.2f}")
            assert ratio <= 1.0 and rms <= Z_RMS and zmax <= Z_MAX
            for m in MUTANTS:
                if head and m == "the output's lo dropped":
                    continue
                r, s, z = z_gates(cpu_kernel_x3(x, w, b, stride, act, mutant=m), ref3, bound, sigma)
                unseen = (head and k != 0) or (x3_pair_id(pair), (H, W), k, m) in X3_UNSEEN
                print(f"    {m}: err / bound {r:.2f}, rms z {s:.1f}, max |z| {z:.1f}" + (" (not asserted)" if unseen else ""))
                if not unseen:
                    assert r > 1.0 or s > Z_RMS or z > Z_MAX, (m, H, W, k)


def test_split_impulse_case_is_exact_and_sees_a_swapped_w_lo():
    """impulse_case_x3 on the CPU kernel: every output element equals carried() of the single weight's three terms bit for bit, in both
    shift variants and strides; with the centre tap's w_lo taken from the next tap it does not."""
    g = torch.Generator().manual_seed(3)
    for cin, cout, stride in ((11, 27, 1), (8, 16, 2), (67, 27, 1)):
        for shift in (False, True):
            x, w, want = impulse_case_x3(cin, cout, stride, shift, g)
            zero = torch.zeros(cout)
            assert torch.equal(cpu_kernel_x3(x, w, zero, stride, "none").double(), carried(want.float()))
            assert torch.equal(want.float().double(), want) and int((want != 0).sum()) > 0
            assert not torch.equal(cpu_kernel_x3(x, w, zero, stride, "none", mutant="w_lo of the centre tap from the next tap").double(), carried(want.float()))


def test_split_chain_statistics_pass_a_correct_chain_and_see_a_lost_low_half_in_the_middle():
    """chain_stats_x3 - what tests/test_gpu_fp32x3_rounding_model.py holds the flow to, whose intermediates no tap shows - on three
    layers (64 -> 64 ReLU, 64 -> 64 ReLU, 64 -> 2 planar) run by the CPU kernel from layer to layer: the correct chain is inside the
    rigorous chain bound and both z gates; with x_lo zeroed in one 16-channel group of the MIDDLE layer, or x_hi * w_lo missing in the
    first, it is far outside the z gates - and far INSIDE the chain bound, which is why the z gates are asserted on the GPU.
    measured: correct chain err / bound 2e-6, rms z 0.09, max |z| 0.25; the mutants rms z 28 and 59, err / bound 7e-4 and 1.2e-3."""
    g = torch.Generator().manual_seed(11)
    x = scaled_input(g, 2, 64, 9, 13)
    layers = []
    for cout, act in ((64, "relu"), (64, "relu"), (2, "none")):
        w, b = conv_weights(g, cout, 64)
        layers.append({"w": w * 1.4, "b": b, "act": act})
    layers[2]["planar"] = True
    ref, bound, sd = chain_stats_x3(x, layers)

    def run_chain(mutants):
        a = x
        for k, L in enumerate(layers):
            a = cpu_kernel_x3(a, L["w"], L["b"], 1, L["act"], mutant=mutants.get(k), seed=k, planar=k == 2)
        return a
    ratio, rms, zmax = z_gates(run_chain({}), ref, bound, sd)
    print(f"correct chain: err / chain bound {ratio:.2e}, rms z {rms:.3f}, max |z| {zmax:.2f}")
    assert ratio <= 1.0 and rms <= Z_RMS and zmax <= Z_MAX
    for mutants in ({1: "x_lo zeroed in one 16-channel group"}, {0: "x_hi * w_lo missing"}):
        r, s_, z = z_gates(run_chain(mutants), ref, bound, sd)
        print(f"{mutants}: err / chain bound {r:.2e}, rms z {s_:.1f}, max |z| {z:.1f}")
        assert r <= 1.0 and s_ > Z_RMS and z > Z_MAX


POOL_MUTANTS = ("the lo sums not added", "the hi sums added twice in place of the lo sums", "the lo sums of the neighbouring channel",
                "the last pixel of the pool missing")


def cpu_pool_linear_x3(c2, lw, lb, mutant=None):
    """A correct pool, fold and Linear in one particular order: fp32 sums of the hi and of the lo halves pixel after pixel (the doubled
    channels), the two added, one division, then FMAs from the bias (the product enters the fp32 addition unrounded).  `mutant`: one of
    POOL_MUTANTS."""
    hi, lo = split22(c2)
    B, C, H, W = c2.shape
    hi, lo = hi.reshape(B, C, -1), lo.reshape(B, C, -1)
    npix = hi.shape[2]
    a_hi, a_lo = torch.zeros(B, C), torch.zeros(B, C)
    for p in range(npix - 1 if mutant == "the last pixel of the pool missing" and npix > 1 else npix):
        a_hi, a_lo = a_hi + hi[:, :, p], a_lo + lo[:, :, p]
    if mutant == "the lo sums not added":
        a_lo = torch.zeros_like(a_lo)
    elif mutant == "the hi sums added twice in place of the lo sums":
        a_lo = a_hi
    elif mutant == "the lo sums of the neighbouring channel":
        a_lo = a_lo.roll(1, dims=1)
    mean = (a_hi + a_lo) / npix
    t = lb.view(1, -1).expand(B, -1).clone()
    for c in range(C):
        t = (t.double() + lw[:, c].double().view(1, -1) * mean[:, c:c + 1].double()).float()
    return t


@pytest.mark.parametrize("size", [(3, 4), (17, 33), (33, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_pool_and_fold_statistics_pass_a_correct_kernel_and_fail_a_lost_lo(size):
    """pool_linear_model_x3 - what tests/test_gpu_fp32x3_rounding_model.py holds the `ctx` tap to - at the three sizes it runs there (a
    feature map of 3 x 4, 17 x 33 and 33 x 70 pools 1, 45 and 162 pixels), mid_channels 64: 64 -> 128 /2 -> 256 /2 -> 256, ReLU, run
    TWICE by the CPU kernel in two summation orders - one c2 is pooled by the "kernel", the model stands on the other, as on the GPU,
    where the forward's c2 is not the stage entry's bit for bit.  The correct pool is inside the bound and both z gates; every one of
    POOL_MUTANTS is outside the z gates (one missing pixel of ONE has nothing to miss: not run) - and a lost lo is INSIDE the bound,
    at 45 and 162 pixels, which is why the z gates are asserted on the GPU.  measured (pooled pixels: correct kernel err / bound,
    rms z, max |z|; the mutants' rms z in the order of POOL_MUTANTS):
        1: 0.004, 0.06, 0.14;   19, 9.5e4, 25
       45: 0.002, 0.04, 0.09;   6.4, 1.4e5, 9.4, 2600
      162: 0.002, 0.09, 0.29;   5.0, 2.2e5, 8.1, 1100"""
    H, W = size
    g = torch.Generator().manual_seed(23 + H)
    feat = scaled_input(g, 1, 64, H, W).relu()
    layers = []
    for cin, cout, stride in ((64, 128, 2), (128, 256, 2), (256, 256, 1)):
        w, b = conv_weights(g, cout, cin)
        layers.append({"w": w * 1.4, "b": b, "act": "relu", "stride": stride})
    lw, lb = torch.randn(64, 256, generator=g) / 16, torch.randn(64, generator=g) * 0.1

    def run_chain(seed):
        a = feat
        for k, L in enumerate(layers):
            a = cpu_kernel_x3(a, L["w"], L["b"], L["stride"], "relu", seed=seed + k)
        return a
    pooled, given = run_chain(0), run_chain(100)
    _, _, sd_c2 = chain_stats_x3(feat, layers)
    ref, bound, sigma = pool_linear_model_x3(given, sd_c2, lw, lb)
    npix = given.shape[2] * given.shape[3]
    ratio, rms, zmax = z_gates(cpu_pool_linear_x3(pooled, lw, lb), ref, bound, sigma)
    print(f"{npix} pooled pixels (the two c2 differ in {100 * (pooled != given).double().mean().item():.1f} % of the elements): "
          f"correct kernel err / bound {ratio:.4f}, rms z {rms:.3f}, max |z| {zmax:.2f}; sigma / |ctx| {(sigma / ref.abs()).median().item():.1e}")
    assert ratio <= 1.0 and rms <= Z_RMS and zmax <= Z_MAX
    for m in POOL_MUTANTS:
        if m == "the last pixel of the pool missing" and npix == 1:
            continue
        r, s_, z = z_gates(cpu_pool_linear_x3(pooled, lw, lb, mutant=m), ref, bound, sigma)
        print(f"    {m}: err / bound {r:.3f}, rms z {s_:.1f}, max |z| {z:.1f}")
        assert s_ > Z_RMS and z > Z_MAX, m
