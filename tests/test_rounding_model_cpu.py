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

from rounding_model import (MISMATCH_CAP, UNIT, chain_bound, conv_bound, conv_layer, conv_model, conv_weights, exact_match_share, impulse_case, quantum,
                            round64, scaled_input, storage_round)

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
