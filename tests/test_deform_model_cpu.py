"""tests/deform_model.py tested with the CPU as kernel (no GPU): the float64 reference against the three independent statements of the
operator, the clean fp32 oracle under every bound and the mismatch cap, and a list of INJECTED DEFECTS each of which must fail the
lattice gate - with the lattice case that catches it.

The defects (variant_dcn), and the case that catches each (asserted below):
  trunc            floor replaced by truncation toward zero             border_y (positions in (-1, 0): -1 + eps, -eps)
  lt_minus1        `< -1` for `<= -1`                                   border_y (position -1 exactly)
  gt_size          `> size` for `>= size`                               border_y (position H exactly)
  swap_dydx        even offset channel read as dx                       integers
  column_major     taps enumerated column-major                        integers
  far_corner       far corner one pixel too far (floor + 2)             half_quarter
  window_drop      samples beyond the 23 x 23 window dropped            handover_* (the first value past each edge)
  window_twice     samples beyond the window added twice                handover_*
  zero_weight_nan  a corner with weight exactly 0 reads as NaN          integers (lh = 0: the far corner, outside the image in the last row)
  bf16_weights     corner weights rounded to bf16 instead of f16        border_lone (lone corner, weight 1/2 + 3 * 2^-11, f16 storage)
  mask_after_store mask applied to the blended value AFTER it was       half_quarter_masked (bf16 storage)
                   rounded to the storage type
`< -1` and `> size` are observable only in the form they take in a kernel whose corner rows are CLAMPED into the image and guarded by
the range test alone (deform_pack3's fix-up, the gather kernel): the sample at -1 then reads row 0 with weight 1.  Where every corner
carries its own validity test (the oracle, deform_warp_ref.c) the two variants are arithmetically the rule itself - at -1 the only
corner inside has weight lh = 0 - and are not defects."""
import numpy as np
import pytest
import torch

import deform_model as dm
from oracle import emavfi_oracle as oracle
from rounding_model import MISMATCH_CAP, storage_round

B, C, H, W = 1, 19, 37, 53       # three tile rows, four tile columns, ragged: every tile row and column 0..15, both hand-over sides inside the image


def operands(seed=0, c=C, h=H, w=W, b=B):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, h, w, generator=g)
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(c, generator=g) * 0.1
    return x, wt, bias


def rounded(x, wt, store):
    return storage_round(x, store), storage_round(wt, store)


# ------------------------------------------------------------------------------------------------------------ the model itself
def scalar_dcn(x, off, msk, w, b):
    """the triple loop, python floats (float64), positions added in fp32"""
    Bn, Cn, Hn, Wn = x.shape
    O = w.shape[0]
    out = np.zeros((Bn, O, Hn, Wn))
    xn, wn = x.double().numpy(), w.double().numpy()
    for bb in range(Bn):
        for y in range(Hn):
            for xx in range(Wn):
                acc = b.double().numpy().copy()
                for k in range(9):
                    i, j = divmod(k, 3)
                    py = float(np.float32(y - 1 + i) + np.float32(off[bb, 2 * k, y, xx]))
                    px = float(np.float32(xx - 1 + j) + np.float32(off[bb, 2 * k + 1, y, xx]))
                    if not (np.isfinite(py) and np.isfinite(px)) or py <= -1 or py >= Hn or px <= -1 or px >= Wn:
                        continue
                    hl, wl = int(np.floor(py)), int(np.floor(px))
                    lh, lw = py - hl, px - wl
                    v = np.zeros(Cn)
                    for r, c_, wg in ((hl, wl, (1 - lh) * (1 - lw)), (hl, wl + 1, (1 - lh) * lw), (hl + 1, wl, lh * (1 - lw)), (hl + 1, wl + 1, lh * lw)):
                        if 0 <= r <= Hn - 1 and 0 <= c_ <= Wn - 1:
                            v += wg * xn[bb, :, r, c_]
                    acc += float(msk[bb, k, y, xx]) * (wn[:, :, i, j] @ v)
                out[bb, :, y, xx] = acc
    return torch.from_numpy(out)


def finite_cases(b, h, w):
    cases = {n: c for n, c in dm.lattice_cases(b, h, w).items() if n != "nonfinite"}
    cases["random"] = dm.random_case(b, h, w)
    return cases


def test_dcn64_is_the_scalar_triple_loop():
    x, wt, bias = operands(1, c=3, h=7, w=19, b=1)
    for name, (off, msk) in dm.lattice_cases(1, 7, 19).items():       # (with the infinite and NaN offsets: the loop skips them)
        ref, _ = dm.dcn64(x, off, msk, wt, bias)
        assert (ref - scalar_dcn(x, off, msk, wt, bias)).abs().max().item() <= 1e-13, name


def test_dcn64_agrees_with_the_oracle_and_the_c_restatement(oracle_c):
    x, wt, bias = operands(2)
    for name, (off, msk) in finite_cases(B, H, W).items():
        ref, bound, _ = dm.bound_fp32(x, off, msk, wt, bias)
        got = oracle.deform_conv2d(x, off, msk, wt, bias)
        assert ((got.double() - ref).abs() <= bound).all(), f"oracle, {name}"
        got_c = torch.from_numpy(oracle_c.deform(x.numpy(), off.numpy(), msk.numpy(), wt.numpy(), bias.numpy()))
        assert ((got_c.double() - ref).abs() <= bound).all(), f"C restatement, {name}"


def test_the_fp32_oracle_leaks_nan_where_the_model_returns_zero():
    """The finding DESIGN section 2 records: oracle._dcn_bilinear multiplies the corner weights by ok = 0 instead of selecting, so an
    infinite or NaN position - weight NaN - gives NaN where the operator's early return gives 0.  The model selects."""
    x, wt, bias = operands(3)
    off, msk = dm.lattice_cases(B, H, W)["nonfinite"]
    ref, _ = dm.dcn64(x, off, msk, wt, bias)
    assert torch.isfinite(ref).all()
    got = oracle.deform_conv2d(x, off, msk, wt, bias)
    bad = ~torch.isfinite(off).all(dim=1)                                 # pixels that carry a non-finite offset
    assert torch.isnan(got).any(dim=1)[bad].all() and torch.isfinite(got).all(dim=1)[~bad].all()
    _, bound, _ = dm.bound_fp32(x, off, msk, wt, bias)
    keep = (~bad).unsqueeze(1).expand_as(got)
    assert ((got.double() - ref).abs() <= bound)[keep].all()


def test_sample64_never_multiplies_a_non_finite_position():
    x = torch.ones(1, 2, 4, 5)
    one = torch.ones(1, 4, 5)
    for v in (float("inf"), float("-inf"), float("nan"), -1.0, -1.0 - 2.0 ** -10, 5.0, 3e38, -3e38):     # (5 = W: outside on both axes)
        pos = torch.full((1, 4, 5), v)
        assert (dm.sample64(x, pos, one) == 0).all() and (dm.sample64(x, one, pos) == 0).all(), v
    assert (dm.sample64(x, torch.full((1, 4, 5), 4.0), torch.ones(1, 4, 5)) == 0).all()          # row H exactly
    assert (dm.sample64(x, torch.full((1, 4, 5), 3.0), torch.ones(1, 4, 5)) == 1).all()          # row H - 1: the far corner has weight 0
    assert (dm.sample64(x, torch.full((1, 4, 5), -1 + 2.0 ** -10), torch.ones(1, 4, 5)) == 2.0 ** -10).all()


def test_carrier_offsets_are_exact_and_cover_the_edges():
    for dtype, eps in (("bf16", dm.EPS), ("fp16", dm.EPS), ("amp16", 2.0 ** -4)):
        for name, case in dm.carrier_cases(H, W, eps).items():
            x, ow, ob, off, msk = dm.carrier_tensors(case, 2, 67, dtype)
            xs = storage_round(x, "fp16" if dtype == "amp16" else dtype)
            assert torch.equal(xs[:, :case[0].shape[0]], x[:, :case[0].shape[0]]), "a plane is not a storage number"
            if dtype == "amp16":
                continue
            raw = oracle.conv3x3(xs, ow, ob)                                # one non-zero product + the bias: any order gives this
            o1, m, o2 = torch.chunk(raw, 3, dim=1)
            got = torch.cat((o1, o2), dim=1)
            same = (got == off) | (torch.isnan(got) & torch.isnan(off))
            assert same.all(), f"{dtype} {name}"
    n_out, n_groups, _, _ = dm.window_census(dm.carrier_tensors(dm.carrier_cases(H, W)["handover_1"], 1, 67, "bf16")[3], H, W)
    assert n_out > 0 and n_groups > 0


# ------------------------------------------------------------------------------------------------------------ the gate on the clean oracle
@pytest.mark.parametrize("store", ["fp32", "bf16", "fp16"])
def test_clean_oracle_passes_every_bound_and_the_cap(store):
    """The fp32 oracle rounded to storage is a kernel with LESS error than any bound allows: it must pass the whole gate, and its
    mismatch share at integer positions must stay within MISMATCH_CAP on the inputs the GPU test uses (the reference alone)."""
    x, wt, bias = operands(4)
    xs, ws = rounded(x, wt, store)
    bound_fn = dm.bound_fp32 if store == "fp32" else (lambda *a: dm.bound_pack16(*a, store))
    cases = finite_cases(B, H, W)

    def run(off, msk):
        return storage_round(oracle.deform_conv2d(xs, off, msk, ws, bias), store)

    fails, stats = dm.lattice_gate(run, bound_fn, xs, ws, bias, cases, store, f"oracle {store}")
    assert not fails, fails
    assert stats["share"] <= MISMATCH_CAP and stats["units"] <= 1.0
    print(f"oracle as kernel, {store}: err / bound max {stats['ratio']:.3f}, mismatch share {stats['share']:.4f}")


# ------------------------------------------------------------------------------------------------------------ injected defects
def variant_dcn(x, off, msk, w, b, store, defect=None):
    """DCNv2 the way the window kernels compute it - clamped positions, clamped corner rows guarded by validity flags, the fix-up for
    samples past the window - in float64 behind the fp32 position, with ONE defect switched on.  Rounds to `store` at the end."""
    Bn, Cn, Hn, Wn = x.shape
    x64 = x.double()
    ys = torch.arange(Hn, dtype=torch.float32).view(1, Hn, 1)
    xs = torch.arange(Wn, dtype=torch.float32).view(1, 1, Wn)
    ty0 = (torch.arange(Hn) // 16 * 16 - 3).view(1, Hn, 1)
    tx0 = (torch.arange(Wn) // 16 * 16 - 3).view(1, 1, Wn)
    out = torch.zeros(Bn, w.shape[0], Hn, Wn, dtype=torch.float64)
    for k in range(9):
        i, j = divmod(k, 3)
        bi, bj = (j, i) if defect == "column_major" else (i, j)
        dy, dx = (off[:, 2 * k + 1], off[:, 2 * k]) if defect == "swap_dydx" else (off[:, 2 * k], off[:, 2 * k + 1])
        py = ((ys - 1 + bi) + dy)
        px = ((xs - 1 + bj) + dx)
        py = torch.where(torch.isnan(py), torch.full_like(py, -2.0), py).clamp(-2.0, Hn + 1.0).double()
        px = torch.where(torch.isnan(px), torch.full_like(px, -2.0), px).clamp(-2.0, Wn + 1.0).double()
        lo_ok_y = (py >= -1) if defect == "lt_minus1" else (py > -1)
        hi_ok_y = (py <= Hn) if defect == "gt_size" else (py < Hn)
        inside = lo_ok_y & hi_ok_y & (px > -1) & (px < Wn)
        fy = torch.trunc(py) if defect == "trunc" else torch.floor(py)
        fx = torch.trunc(px) if defect == "trunc" else torch.floor(px)
        lh, lw = py - fy, px - fx
        hl, wl = fy.long(), fx.long()
        step = 2 if defect == "far_corner" else 1
        col = torch.zeros_like(x64)
        for r, c_, wg in ((hl, wl, (1 - lh) * (1 - lw)), (hl, wl + step, (1 - lh) * lw), (hl + step, wl, lh * (1 - lw)), (hl + step, wl + step, lh * lw)):
            valid = (c_ >= 0) & (c_ <= Wn - 1)
            if defect not in ("lt_minus1", "gt_size"):          # (those two: the range test is the rows' only guard)
                valid = valid & (r >= 0) & (r <= Hn - 1)
            wgt = msk[:, k].double() * wg if defect != "mask_after_store" else wg
            if defect == "bf16_weights":
                wgt = wgt.float().bfloat16().double()
            v = dm._gather(x64, r.clamp(0, Hn - 1), c_.clamp(0, Wn - 1)) * torch.where(inside & valid, wgt, torch.zeros_like(wgt)).unsqueeze(1)
            if defect == "zero_weight_nan":
                v = torch.where((inside & (wg == 0)).unsqueeze(1), torch.full_like(v, float("nan")), v)
            col = col + v
        if defect == "mask_after_store":
            col = storage_round(col, store) * msk[:, k].double().unsqueeze(1)
        ly, lx = torch.floor(py).long() - ty0, torch.floor(px).long() - tx0
        outside = ((ly < 0) | (ly > 21) | (lx < 0) | (lx > 21)).unsqueeze(1)
        if defect == "window_drop":
            col = torch.where(outside, torch.zeros_like(col), col)
        if defect == "window_twice":
            col = torch.where(outside, 2 * col, col)
        out = out + torch.einsum("oc,bchw->bohw", w[:, :, i, j].double(), col)
    return storage_round(out + b.double().view(1, -1, 1, 1), store).float()


DEFECTS = {"trunc": ("fp16", "border_y"), "lt_minus1": ("fp16", "border_y"), "gt_size": ("fp16", "border_y"), "swap_dydx": ("fp16", "integers"),
           "column_major": ("fp16", "integers"), "far_corner": ("fp16", "half_quarter"), "window_drop": ("fp16", "handover_"),
           "window_twice": ("fp16", "handover_"), "zero_weight_nan": ("fp16", "integers"), "bf16_weights": ("fp16", "border_lone"),
           "mask_after_store": ("bf16", "half_quarter_masked")}


def _gate_variant(store, defect, only=None):
    x, wt, bias = operands(5)
    xs, ws = rounded(x, wt, store)
    cases = dm.lattice_cases(B, H, W)
    cases["random"] = dm.random_case(B, H, W)
    if only is not None:
        cases = {n: c for n, c in cases.items() if n.startswith(only)}
    return dm.lattice_gate(lambda off, msk: variant_dcn(xs, off, msk, ws, bias, store, defect), lambda *a: dm.bound_pack16(*a, store), xs, ws, bias, cases, store,
                           f"{defect or 'clean'} {store}")[0]


@pytest.mark.parametrize("store", ["bf16", "fp16"])
def test_the_defect_free_variant_passes(store):
    """the harness itself: the same code with no defect passes every case, the non-finite ones included"""
    fails = _gate_variant(store, None)
    assert not fails, fails


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_injected_defect_fails_the_lattice_gate(defect):
    store, catcher = DEFECTS[defect]
    fails = _gate_variant(store, defect, only=catcher)
    print("\n".join(fails))
    assert fails, f"{defect}: the lattice case {catcher} does not catch it - the lattice is incomplete"
