"""The deformable kernels pinned where the sampling rule bends: exact lattice, border and window edges (tests/deform_model.py).

Random offsets never land on an exact integer (lh = 0: the far corner is read against a zero weight), on -1 or `size` (the
`<= -1 / >= size -> 0` rule), on the window's hand-over (floor(pos) - tile0 + 3 in [0, 21]), on the clamp (-2, size + 1), on an infinity
or a NaN.  Here EVERY offset is a dyadic rational for which base + offset is exact in fp32, so kernel and float64 reference sample at
the same position: every element is held to a bound derived from the kernel's arithmetic (deform_model's docstring), NONE is excluded.

  explicit offsets  lib.deform_conv2d, bf16 / fp16 / fp32: C = O = 67 -> deform_pack3_kernel<T, false> and deform_f32w_kernel<false>;
                    C = 11, 19 -> deform_kernel (deform.inl).  Every lattice case + one random case (+-12 px on the 2^-6 lattice).
  computed offsets  lib.mdcn, routes "window" and "gather", every input form of test_gpu_pack_route.FORMS, and dtype "amp16"
                    (deform_f32w_kernel<true>): offset_conv is zero except ONE centre tap of 1.0 per offset channel from a carrier
                    plane of small integers / quarters, constants in the bias, so raw = plane + bias has one non-zero product and the
                    kernel's own offsets equal the intended ones bit for bit (deform_model.carrier_tensors; the CPU test checks it
                    against ATen).  Mask logits are +-40 / 0 in the bias.  This reaches the FUSE_OFF = true geometry, the fix-up
                    arena, the gather body and the split contraction AT the edges, and makes the census comparison exact.

Assertions (deform_model.lattice_gate): finite everywhere; every element within its bound; at integer positions with mask 1 the
blend is a copy, so 16-bit results are held to rounding_model's single-layer gate (mismatch share <= MISMATCH_CAP, one unit); with the
mask 1 on the dead taps alone (<= -1, >= size, far, infinite, NaN) the output is the stored bias bit for bit.  Census: lib.mdcn_census
EQUALS the in-window test restated (samples outside, fix-up wave-taps, largest |offset| of the flagged waves), both routes report the
same row, and the routes are bit-identical whenever the row shows no fix-up group.

Why the far, infinite and NaN cases stay inside every buffer (read from the source before the first run; they assert the documented
"NaN -> -2" contract, nothing is provoked):
  * every kernel forms its position as fminf(fmaxf(base + offset, -2.0f), size + 1) - deform.inl:57-58 (sample_tap_vals),
    deform_pack3_body.inl:269-270, deform_gather3_body.inl:216-217, deform_f32w.inl:122-123 and its fix-up :275-276.  fmaxf returns its
    non-NaN operand, so a NaN becomes -2; +-inf and +-3e38 clamp to the two ends (base + 3e38 does not overflow: |base| < 2^24).  The
    position is therefore a finite fp32 in [-2, size + 1], floorf of it is an integer in [-2, size + 1], and the int conversion is exact;
  * generic kernel (deform.inl:62-70): the four corners are min(max(., 0), size - 1) - inside the image - and the validity product zeroes
    the weight of a clamped corner;
  * window kernels (deform_pack3_body.inl:276-281, deform_f32w.inl:127-132): a sample whose top-left corner leaves window rows / columns
    [0, TR - 2] is parked (zero weights) and ITS window address is min(max(l, 0), TR - 2): always a window pixel whose +1 neighbours exist.
    The parked sample's fix-up (deform_pack3_body.inl:474-491, deform_f32w.inl:283-291) clamps all four corners into [0, size - 1] before
    the address is formed and masks the weights by validity; pack3's arena holds at most NENT records per round whatever the offsets;
  * gather kernel (deform_gather3_body.inl:231-236, :198-201): corners clamped into the image, an invalid corner's address is replaced by
    the descriptor's out-of-range constant, which a raw buffer load answers with zero."""
import math

import pytest
import torch

import deform_model as dm
from emavfi import lib
from rounding_model import MISMATCH_CAP, exact_match_share, storage_round
from test_gpu_mdcn import DEV, weight_round
from test_gpu_pack_route import forms_of

pytestmark = pytest.mark.gpu


def operands(seed, C, O=None):
    O = C if O is None else O
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(O, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(O, generator=g) * 0.1
    return g, w, b


def explicit_gate(dtype, C, shape, bound_fn, wround):
    B, H, W = shape
    g, w, b = operands(C + 3 * H + W, C)
    xs = storage_round(torch.randn(B, C, H, W, generator=g), dtype)
    ws = wround(w, dtype)
    cases = dm.lattice_cases(B, H, W)
    cases["random"] = dm.random_case(B, H, W)
    dev = [t.to(DEV) for t in (xs, ws, b)]

    def run(off, msk):
        return lib.deform_conv2d(dev[0], off.to(DEV), msk.to(DEV), dev[1], dev[2], dtype=dtype).cpu()

    fails, stats = dm.lattice_gate(run, bound_fn, xs, ws, b, cases, dtype, f"{dtype} C={C} {shape}")
    print(f"SUMMARY explicit {dtype} C={C} {shape}: err / bound max {stats['ratio']:.3f}, mismatch share max {stats['share']:.4f}, "
          f"largest {stats['units']:.0f} units, excluded 0 of {stats['elements']}")
    assert not fails, "\n".join(fails)
    assert stats["share"] <= MISMATCH_CAP


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 16, 16), (1, 5, 7), (1, 1, 40), (1, 33, 1), (1, 48, 80)])
def test_explicit_offsets_at_the_reference_width(dtype, shape):
    """C = O = 67: deform_pack3_kernel<T, FUSE_OFF = false> (bf16, fp16) and deform_f32w_kernel<false> (fp32)."""
    bound = dm.bound_fp32 if dtype == "fp32" else (lambda *a: dm.bound_pack16(*a, dtype, bf16_window=dtype == "bf16"))
    explicit_gate(dtype, 67, shape, bound, weight_round)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("C", [11, 19])
def test_explicit_offsets_on_the_generic_gather_kernel(dtype, C):
    """C = 11, 19: deform_kernel (deform.inl) in all three types - the fp32 blend, one rounding of the blended value to the type."""
    bound = dm.bound_fp32 if dtype == "fp32" else (lambda *a: dm.bound_generic16(*a, dtype))
    explicit_gate(dtype, C, (2, 23, 37), bound, storage_round)


def _census_tuple(row):
    return row["samples_outside_window"], row["fixup_wave_taps"], row["wave_taps"], row["abs_offset_px_max"]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 16, 16)])
def test_computed_exact_offsets_on_both_routes(dtype, shape):
    """lib.mdcn on the window and the gather route, every input form; census exact, routes compared."""
    B, H, W = shape
    _, dw, db = operands(67 + H, 67)
    dws = weight_round(dw, dtype)
    worst, share_max, n_identical, n_elements = 0.0, 0.0, 0, 0
    fails = []
    for name, case in dm.carrier_cases(H, W).items():
        x, ow, ob, off, msk = dm.carrier_tensors(case, B, 67, dtype)
        want_census = dm.window_census(off, H, W)
        whole_dead = dm.dead_taps(off, H, W).all(dim=3).all(dim=2).all(dim=0)                 # taps dead at every pixel
        for flags, form in forms_of(dtype):
            in_f16, out_f16 = bool(flags & lib.MDCN_IN_F16), bool(flags & lib.MDCN_OUT_F16)
            xs = storage_round(x, dtype, as_f16=in_f16)
            store = "fp16" if (dtype == "fp16" or out_f16) else "bf16"
            ref, bound, d = dm.bound_pack16(xs, off, msk, dws, db, store, sigmoid_mask=True, bf16_window=dtype == "bf16" and not in_f16)
            dev = [t.to(DEV) for t in (xs, ow, ob, dws, db)]
            got, rows = {}, {}
            for route in ("window", "gather"):
                label = f"{dtype} {shape} {name} {form} {route}"
                got[route] = lib.mdcn(*dev, dtype=dtype, flags=flags, route=route).cpu()
                rows[route] = lib.mdcn_census(B, 67, H, W, dtype=dtype, flags=flags, device=DEV)[0]
                if not bool(torch.isfinite(got[route]).all()):
                    fails.append(f"{label}: non-finite output")
                    continue
                ratio = float(((got[route].double() - ref).abs() / bound).max())
                worst, n_elements = max(worst, ratio), n_elements + got[route].numel()
                if ratio > 1.0:
                    fails.append(f"{label}: err / bound max {ratio:.3f}")
                if name == "integers":
                    share, units = exact_match_share(got[route], ref, store, d)
                    share_max = max(share_max, share)
                    if share > MISMATCH_CAP or units > 1.0:
                        fails.append(f"{label}: integer positions: mismatch share {share:.4f}, largest {units:.1f} units")
                if _census_tuple(rows[route]) != want_census:
                    fails.append(f"{label}: census {_census_tuple(rows[route])}, restated {want_census}")
            if rows["window"] != rows["gather"]:
                fails.append(f"{dtype} {shape} {name} {form}: the routes report different census rows")
            if rows["window"]["fixup_wave_taps"] == 0:
                n_identical += 1
                if not torch.equal(got["window"].view(torch.int32), got["gather"].view(torch.int32)):
                    fails.append(f"{dtype} {shape} {name} {form}: no fix-up group, yet the routes are not bit-identical")
            if bool(whole_dead.any()):
                ob0 = ob.clone()
                ob0[9:18] = torch.where(whole_dead, torch.tensor(dm.ON), torch.tensor(dm.OFF))
                for route in ("window", "gather"):
                    alone = lib.mdcn(dev[0], dev[1], ob0.to(DEV), dev[3], dev[4], dtype=dtype, flags=flags, route=route).cpu()
                    want = storage_round(db, store).view(1, -1, 1, 1).expand_as(alone).contiguous()
                    if not torch.equal(alone.view(torch.int32), want.view(torch.int32)):
                        fails.append(f"{dtype} {shape} {name} {form} {route}: dead taps alone do not leave the stored bias bit for bit")
        print(f"{dtype} {shape} {name}: restated census {want_census}, whole-dead taps {int(whole_dead.sum())}, running err / bound max {worst:.3f}")
    print(f"SUMMARY computed {dtype} {shape}: err / bound max {worst:.3f}, mismatch share max {share_max:.4f}, excluded 0 of {n_elements}, "
          f"{n_identical} (case, form) pairs without a fix-up group compared bit for bit")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 16, 16)])
def test_computed_exact_offsets_under_the_autocast_policy(shape):
    """dtype "amp16": fp16 offset_conv (offsets and masks are fp16 numbers: the lattice step is 2^-4, mask logits +-40 / 0 give exactly
    1, 1/2, 0 once rounded), then deform_f32w_kernel<true> - the three-term f16 split - on the UNROUNDED fp32 x and master weights."""
    B, H, W = shape
    _, dw, db = operands(167 + H, 67)
    worst, n_elements, fails = 0.0, 0, []
    for name, case in dm.carrier_cases(H, W, eps=2.0 ** -4).items():
        x, ow, ob, off, msk = dm.carrier_tensors(case, B, 67, "amp16")
        ref, bound, _ = dm.bound_x3(x, off, msk, dw, db)
        dev = [t.to(DEV) for t in (x, ow, ob, dw, db)]
        got = lib.mdcn(*dev, dtype="amp16").cpu()
        if not bool(torch.isfinite(got).all()):
            fails.append(f"amp16 {shape} {name}: non-finite output")
            continue
        ratio = float(((got.double() - ref).abs() / bound).max())
        worst, n_elements = max(worst, ratio), n_elements + got.numel()
        print(f"amp16 {shape} {name}: err / bound max {ratio:.3f}")
        if ratio > 1.0:
            fails.append(f"amp16 {shape} {name}: err / bound max {ratio:.3f}")
        whole_dead = dm.dead_taps(off, H, W).all(dim=3).all(dim=2).all(dim=0)
        if bool(whole_dead.any()):
            ob0 = ob.clone()
            ob0[9:18] = torch.where(whole_dead, torch.tensor(dm.ON), torch.tensor(dm.OFF))
            alone = lib.mdcn(dev[0], dev[1], ob0.to(DEV), dev[3], dev[4], dtype="amp16").cpu()
            if not torch.equal(alone.view(torch.int32), db.view(1, -1, 1, 1).expand_as(alone).contiguous().view(torch.int32)):
                fails.append(f"amp16 {shape} {name}: dead taps alone do not leave the bias bit for bit")
    print(f"SUMMARY computed amp16 {shape}: err / bound max {worst:.3f}, excluded 0 of {n_elements}")
    assert not fails, "\n".join(fails)
