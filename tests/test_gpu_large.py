"""Every single-stage entry, and the forward, run where byte offsets pass 2^31 and 2^32 - the sizes include/emavfi.h's SIZE LIMITS block
admits and no other test reaches.  The single-stage entries are held to the two references of tests/large_harness.py: the BAND reference over the whole tensor (the same entry
on row bands whose buffers stay at or below 1 GiB; equality, every element compared, none excluded) and float64 PROBES on crops around
the pixels whose offsets straddle the lines (err / bound <= 1 with the bounds rounding_model / deform_model derive, nothing tuned).
tests/test_large_harness_cpu.py shows that both see an aliased address.

Size classes, shapes the smallest that cross:  S2 = two samples, each plane just above 2 GiB (in-sample offsets have bit 31 set, sample
1 lies beyond 2^32);  S1 = one sample just under the entry's 4 GiB limit.  W is a multiple of 64, plus a ragged remainder in one case
per family.

What decides the two open questions about emavfi_conv3x3's guard (it checks the INPUT plane only, and counts an EMAVFI_F32X3 element
as 2 bytes although a pixel travels as [hi | lo]):
  * `tile 6->64 out>4GiB`: the output plane is 4.3 GB while the input plane is 1.1 GB - the tile kernel's staged-store epilogue, and
    every other kernel's output address, is 64-bit arithmetic (csrc/conv3x3.inl `orow`, conv_ring.inl `obase` + a per-row 32-bit
    offset below 2^17, conv_wreg.inl `obase`): only INPUT offsets are 32-bit (conv_dma_src, conv_wreg's doff).
  * `tile x3 over`: the real [hi | lo] plane is 4.3 GB.  EMAVFI_F32X3 always runs the tile kernel (conv_geometry), whose input
    addresses are 64-bit too, so the guard's 2-byte count admits real planes up to 8 GiB and that is addressable.
  Both run here and agree with their bands and probes: neither is a defect (MEASURED).

The warp is NOT bit-identical between a band and the whole, by definition of the operation rather than by a defect: the reference
normalises the sampling position with the image height and un-normalises it again, in fp32 (2 v / (H - 1) - 1, then ((g + 1) / 2)
(H - 1): csrc/misc_kernels.hip warp_tap, oracle.warp), so the rounded row coordinate of the same pixel differs by an ulp between a
band of 1000 rows and the image of 25900.  The warp is therefore held to the float64 model (large_harness.warp_model, the oracle's
fp32 coordinate steps reproduced exactly, float64 blend) on EVERY pixel, in chunks on the device - more than the 10^5 seeded pixels
asked of such a kernel - and on the probes.

The forward is not band-exact either (the warp; the packs add computed fp32 offsets to the row index): see its three tests.


Each test prints its figures (`LARGE ...` lines), asserts its own peak of device memory <= 48 GiB, releases everything before the
next, and skips only when the device has less free memory than it needs."""
import math
import time

import pytest
import torch

import deform_model as dm
import large_harness as lh
from emavfi import lib
from rounding_model import MISMATCH_CAP, U32, conv_model, conv_weights, exact_match_share, storage_round
from test_gpu_conv_rounding_model import ACT, NO_RING, OLD32, family_of, set_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
PEAK_CAP = 48 * GIB
BAND_BYTES = 1 * GIB
ALL_OFF = {"EMAVFI_CONV_MFMA16": "0", "EMAVFI_CONV_RING": "0", "EMAVFI_CONV_S2RING": "0", "EMAVFI_CONV_WREG": "0"}


def hw_above(pixels, W):
    """(H, W) with H * W just above `pixels`."""
    return pixels // W + 1, W


def hw_below(pixels, W):
    """(H, W) with H * W just below `pixels`."""
    return (pixels - 1) // W, W


@pytest.fixture(autouse=True)
def clean_device():
    lib.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    lib.release_workspaces()
    torch.cuda.empty_cache()


def need_memory(nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes} bytes of device memory, {free} free")


def finish(label, t0, figures):
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"LARGE {label}: {figures}; peak {peak / GIB:.1f} GiB; wall {time.time() - t0:.1f} s")
    assert peak <= PEAK_CAP, f"{label}: peak device memory {peak} above 48 GiB"


def all_finite(t):
    return all(bool(torch.isfinite(t[b]).all()) for b in range(t.shape[0]))


# ------------------------------------------------------------------------------------------------------------ convolutions
def conv_pixbytes(cin, cout, dtype):
    """(input, output) bytes per pixel of the channels-last buffers emavfi_conv3x3 carves: channels padded to 16 (fp32: 65..72 -> 72),
    2 / 4 bytes per element, [hi | lo] f16 halves under fp32x3."""
    e = 4 if dtype in ("fp32", "fp32x3") else 2
    cin_pad = 72 if (dtype == "fp32" and 64 < cin <= 72) else (cin + 15) // 16 * 16
    return cin_pad * e, (cout + 15) // 16 * 16 * e


# (id, family, env, dtype, Cin, Cout, stride, act, B, (H, W))
CONV_CASES = [
    ("tile fp32 256->256 S2", "tile", {}, "fp32", 256, 256, 1, "relu", 2, hw_above((1 << 31) // 1024, 1088)),
    ("tile fp32 256->256 S1", "tile", {}, "fp32", 256, 256, 1, "none", 1, hw_below((1 << 32) // 1024, 2085)),
    ("tile bf16 6->64 out>4GiB", "tile", {}, "bf16", 6, 64, 1, "relu", 1, hw_above((1 << 32) // 128, 5781)),
    ("tile fp32 6->64 out>4GiB", "tile", {}, "fp32", 6, 64, 1, "none", 1, hw_above((1 << 32) // 256, 4160)),
    ("tile x3 64->64 under", "tile", {}, "fp32x3", 64, 64, 1, "none", 1, hw_below((1 << 32) // 256, 4096)),
    ("tile x3 64->64 over", "tile", {}, "fp32x3", 64, 64, 1, "relu", 1, hw_above((1 << 32) // 256, 4160)),
    ("wreg fp16 256->256 s1 S2", "wreg", {}, "fp16", 256, 256, 1, "relu", 2, hw_above((1 << 31) // 512, 2112)),
    ("wreg bf16 128->256 s2 S2", "wreg", {}, "bf16", 128, 256, 2, "none", 2, hw_above((1 << 31) // 256, 2899)),
    ("s2ring fp16 64->128 s2 S2", "s2ring", {}, "fp16", 64, 128, 2, "relu", 2, hw_above((1 << 31) // 128, 4131)),
    ("ring2 bf16 64->64 S2", "ring2", {}, "bf16", 64, 64, 1, "relu", 2, hw_above((1 << 31) // 128, 4160)),
    ("ring3 fp16 67->64 S2", "ring3", {}, "fp16", 67, 64, 1, "none", 2, hw_above((1 << 31) // 160, 3661)),
    ("persist16 bf16 64->32 S2", "persist16", {}, "bf16", 64, 32, 1, "relu", 2, hw_above((1 << 31) // 128, 4160)),
    ("persist16 fp16 64->64 noring S2", "persist16", NO_RING, "fp16", 64, 64, 1, "none", 2, hw_above((1 << 31) // 128, 4131)),
    ("persist32 fp16 64->32 S2", "persist32", OLD32, "fp16", 64, 32, 1, "relu", 2, hw_above((1 << 31) // 128, 4160)),
    ("light bf16 32->3 S2", "light", {}, "bf16", 32, 3, 1, "tanh01", 2, hw_above((1 << 31) // 64, 5781)),
    ("light fp16 32->3 S1", "light", {}, "fp16", 32, 3, 1, "tanh01", 1, hw_below((1 << 32) // 64, 8192)),
]


def x3_model(crops, w, b, stride, act):
    """(ref, bound) of the three-term f16 split (conv3x3_kernel with p.x3; the derivation of deform_model.bound_x3 applied to a plain
    convolution).  Each operand v travels as hi = f16(v), lo = f16(v - hi): |v - hi - lo| <= 2^-22 |v|, or 2^-25 absolutely once lo is
    subnormal; w_hi x_hi + w_lo x_hi + w_hi x_lo drops lo x lo (2^-22 |w x|): per product 3 * 2^-22 |w x| + 2^-25 (|w| + |x|).  The three
    f16 MFMAs have exact products and add 3 n terms in fp32: 3 n 2^-24 sum|terms|.  The result is stored as [hi | lo] again and returned
    as fp32(hi) + fp32(lo): 2^-22 |v| + 2^-25, and one fp32 add 2^-24 |v|.  ReLU is 1-Lipschitz."""
    ref, _, _ = conv_model(crops, w, b, stride, act, "fp32")
    n = 9 * w.shape[1] + 1
    terms = conv_model(crops.abs(), w.abs(), b.abs(), stride, "none", "fp32")[0]
    sum_x = conv_model(crops.abs(), torch.ones_like(w), None, stride, "none", "fp32")[0]
    sum_w = w.double().abs().sum(dim=(1, 2, 3)).view(1, -1, 1, 1)
    pre = (3 * 2.0 ** -22 + 3 * n * U32) * terms + 2.0 ** -25 * (sum_w + sum_x)
    return ref, pre + (2.0 ** -22 + U32) * (ref.abs() + pre) + 2.0 ** -25


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_convolution_families_across_the_lines(case, monkeypatch):
    """lib.conv3x3 per kernel family (asserted with family_of as tests/test_gpu_conv_rounding_model.py does): x ~ N(0, 1) scaled per
    channel by 2^-3 .. 2^3, generated on the device and pre-rounded to the storage type; w ~ N(0, 1 / (9 Cin)).  Band reference:
    equality on every element.  Probes: the input-buffer and the output-buffer geometry each give a probe set; every probe's output
    pixel is held to conv_model on a 3 x 3 (stride 2: 5 x 5, starting on an even row) crop, bound and - in the 16-bit types - nearest
    rounding, the gates of the small-size file.  measured: see MEASURED."""
    label, family, env, dtype, cin, cout, stride, act, B, (H, W) = case
    set_env(monkeypatch, env)
    if dtype == "fp32x3":
        # conv_geometry() plans the split mode as an f16 layer with EVERY layout switch off - which leaves the tile or the 32x32x16
        # persistent route (restated here) - and then sets the route to CONV_TILE unconditionally (`if (x3) { ... L.route = CONV_TILE;`):
        # three weight sets exist in the tile kernel alone.  No entry reports the kernel of a stage call, so this is what can be asserted.
        assert family_of(cin, cout, stride, "fp16", ALL_OFF, act) in ("tile", "persist32")
    else:
        assert family_of(cin, cout, stride, dtype, env, act) == family
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    pin, pout = conv_pixbytes(cin, cout, dtype)
    planar = act == "tanh01"
    nbytes = B * (H * W * (4 * cin + pin) + Ho * Wo * (4 * cout + (0 if planar else pout)))
    need_memory(int(nbytes * 1.1) + 4 * GIB, label)
    L = lib.load()
    assert L.emavfi_conv3x3_workspace_bytes(B, cin, cout, H, W, stride, lib.dtype_code(dtype)) >= B * (H * W * pin + (0 if planar else Ho * Wo * pout))
    t0 = time.time()
    g = torch.Generator().manual_seed(cin * 131 + cout + 7 * H + W)
    w, b = conv_weights(g, cout, cin)
    store_in = "fp32" if dtype == "fp32x3" else dtype
    ws = storage_round(w, store_in)
    wd, bd = ws.to(DEV), b.to(DEV)
    x = lh.device_normal((B, cin, H, W), cin + 3 * cout + H, DEV, store_in, channel_scale=True)
    entry = lambda t: lib.conv3x3(t, wd, bd, stride=stride, act=ACT[act], dtype=dtype)
    big = entry(x)
    assert big.shape == (B, cout, Ho, Wo) and all_finite(big)

    rows = max(2, (BAND_BYTES // (4 * B * W * max(cin, cout)) - 2) // 2 * 2)     # (+ the two halo rows: the band's largest buffer stays <= 1 GiB)
    band = lh.band_check(entry, [x], big, lh.band_ranges(Ho, rows // stride, align=1), stride=stride, halo=1, align=stride)

    sets_in = lh.probe_pixels(B, H, W, pin, seed=cin + cout)
    print(lh.describe_probes(label + " input", sets_in, pin, H, W))
    probes = {(pb, py // stride, px // stride) for pts in sets_in.values() for pb, py, px in pts}
    if not planar:
        sets_out = lh.probe_pixels(B, Ho, Wo, pout, seed=cin + cout + 1)
        print(lh.describe_probes(label + " output", sets_out, pout, Ho, Wo))
        probes |= set(lh.merge_probes(sets_out))
    probes = sorted(probes)
    k = 3 if stride == 1 else 5
    crops = lh.gather_crops(x, probes, k, centre_of=lambda py, px: (stride * py, stride * px)).cpu()
    got = lh.gather_pixels(big, probes).cpu()
    store = "fp32" if (dtype in ("fp32", "fp32x3") or planar) else dtype
    if dtype == "fp32x3":
        ref, bound = x3_model(crops, ws, b, stride, act)
        d = None
    else:
        ref, bound, d = conv_model(crops, ws, b, stride, act, store, fp32_products=dtype == "fp32")
    ref, bound = ref[:, :, 1, 1], bound[:, :, 1, 1]
    ratio = ((got.double() - ref).abs() / bound).max().item()
    share, units = exact_match_share(got, ref, store, d[:, :, 1, 1]) if store != "fp32" else (0.0, 0.0)
    finish(label, t0, f"{B}x{cin}x{H}x{W} -> {cout} s{stride} {act}; in plane {H * W * pin / GIB:.3f} GiB, out plane {Ho * Wo * pout / GIB:.3f} GiB; "
           f"bands {math.ceil(Ho / max(1, rows // stride))}: compared {band['compared']}, excluded {band['excluded']}, differing {band['differing']}; "
           f"probes {len(probes)}: err / bound max {ratio:.3f}, mismatches {100 * share:.3f} % (<= {units:.0f} units)")
    assert band["excluded"] == 0 and band["compared"] == big.numel()
    assert band["differing"] == 0, f"{label}: band and whole differ in {band['differing']} elements, first in band {band['first']}"
    assert ratio <= 1.0, f"{label}: a probe exceeds the rounding model's worst case ({ratio:.3f}x)"
    assert share <= MISMATCH_CAP and units <= 1.0, f"{label}: not a round-to-nearest store at the probes ({share}, {units})"


# ------------------------------------------------------------------------------------------------------------ deformable convolution
DEFORM_CASES = [("deform bf16 67->67 S2", "bf16", 2, 3900, 4096), ("deform fp16 67->67 S2", "fp16", 2, 3900, 4096),
                ("deform fp32 67->67 4K B2", "fp32", 2, 2160, 3840)]
DEFORM_REACH = 4       # |offset| <= 4 px, on the 2^-6 lattice: base + offset is exact in fp32 below 2^17, so a band samples where the whole does
DEFORM_HALO = 16       # >= DEFORM_REACH + 2 (the far bilinear corner and the 3x3 tap), and the 16-row tile phase is kept


def deform_probe_model(x, off, msk, ws, b, dtype, probes, bound_fn=None):
    """deform_model's bound per probe on a crop cut CLIPPED at the image (the crop's own edges are then the image's where the probe is
    near one; elsewhere they are R = reach + 2 pixels away, beyond every corner the probe's nine taps read).  Probes are grouped by
    crop geometry and run as batches.  Returns (ref [N, O], bound [N, O]) in probe order."""
    B, C, H, W = x.shape
    R = DEFORM_REACH + 2
    groups = {}
    for i, (pb, py, px) in enumerate(probes):
        r0, r1, c0, c1 = max(0, py - R), min(H, py + R + 1), max(0, px - R), min(W, px + R + 1)
        groups.setdefault((py - r0, px - c0, r1 - r0, c1 - c0), []).append((i, pb, r0, c0))
    ref = torch.zeros(len(probes), ws.shape[0], dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for (cy, cx, h, w_), members in groups.items():
        cut = lambda t: torch.stack([t[pb, :, r0:r0 + h, c0:c0 + w_] for _, pb, r0, c0 in members]).cpu()
        xc, oc, mc = cut(x), cut(off), cut(msk)
        if bound_fn is not None:
            r, bd, _ = bound_fn(xc, oc, mc, ws, b)
        elif dtype == "fp32":
            r, bd, _ = dm.bound_fp32(xc, oc, mc, ws, b)
        else:
            r, bd, _ = dm.bound_pack16(xc, oc, mc, ws, b, dtype, bf16_window=dtype == "bf16")
        idx = torch.tensor([i for i, _, _, _ in members])
        ref[idx], bound[idx] = r[:, :, cy, cx], bd[:, :, cy, cx]
    return ref, bound


@pytest.mark.parametrize("case", DEFORM_CASES, ids=[c[0] for c in DEFORM_CASES])
def test_deform_conv2d_across_the_lines(case):
    """lib.deform_conv2d with explicit offsets at C = O = 67 (deform_pack3_kernel<T, false>; fp32: deform_f32w_kernel<false>): 160 /
    320 bytes per pixel.  Offsets are uniform on the 2^-6 lattice within +-4 px (exact positions: tests/deform_model.py), masks uniform
    in [0, 1).  Bands of multiples of 16 rows with a 16-row halo keep the kernels' 16 x 16 tile phase, so the same samples take the
    window and the same the fix-up, in the same order: equality.  The test asserts the halo covers the measured largest |offset| + 2.
    Probes: deform_model.bound_pack16 / bound_fp32 on clipped crops.  measured: see MEASURED."""
    label, dtype, B, H, W = case
    C = 67
    e = 4 if dtype == "fp32" else 2
    pix = 80 * e
    nbytes = B * H * W * (4 * C * 2 + 4 * 27 + 2 * pix + 128)
    need_memory(int(nbytes * 1.1) + 4 * GIB, label)
    t0 = time.time()
    g = torch.Generator().manual_seed(67 + 3 * H + W)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g) * 0.1
    ws = storage_round(w, dtype)
    ws = ws.half().float() if dtype == "bf16" else ws          # (a bf16 pack contracts the bf16-rounded weights stored as f16: test_gpu_mdcn.weight_round)
    wd, bd = ws.to(DEV), b.to(DEV)
    x = lh.device_normal((B, C, H, W), 670 + H, DEV, dtype)
    gd = torch.Generator(device=DEV).manual_seed(671 + W)
    off = torch.empty(B, 18, H, W, device=DEV)
    msk = torch.empty(B, 9, H, W, device=DEV)
    for s in range(B):
        off[s].copy_(torch.randint(-DEFORM_REACH * 64, DEFORM_REACH * 64 + 1, (18, H, W), device=DEV, generator=gd, dtype=torch.int32))
        off[s] /= 64
        msk[s].uniform_(generator=gd)
    reach = max(float(off[s].abs().max()) for s in range(B))
    assert reach + 2 <= DEFORM_HALO and reach > 3, reach
    entry = lambda xt, ot, mt: lib.deform_conv2d(xt, ot, mt, wd, bd, dtype=dtype)
    big = entry(x, off, msk)
    assert big.shape == (B, C, H, W) and all_finite(big)

    rows = max(16, BAND_BYTES // (4 * B * W * C) // 16 * 16 - 2 * DEFORM_HALO)
    band = lh.band_check(entry, [x, off, msk], big, lh.band_ranges(H, rows, align=16), stride=1, halo=DEFORM_HALO, align=16)

    sets = lh.probe_pixels(B, H, W, pix, seed=H)
    sets_om = lh.probe_pixels(B, H, W, 128, seed=H + 1, n_random=0)      # the offset / mask records: 32 floats per pixel
    print(lh.describe_probes(label, sets, pix, H, W))
    print(lh.describe_probes(label + " offsets", sets_om, 128, H, W))
    probes = lh.merge_probes(sets, sets_om)
    ref, bound = deform_probe_model(x, off, msk, ws, b, dtype, probes)
    got = lh.gather_pixels(big, probes).cpu()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    finish(label, t0, f"{B}x{C}x{H}x{W}; plane {H * W * pix / GIB:.3f} GiB; |offset| max {reach}; bands {len(lh.band_ranges(H, rows, align=16))}: "
           f"compared {band['compared']}, excluded {band['excluded']}, differing {band['differing']}; probes {len(probes)}: err / bound max {ratio:.3f}")
    assert band["excluded"] == 0 and band["compared"] == big.numel()
    assert band["differing"] == 0, f"{label}: band and whole differ in {band['differing']} elements, first in band {band['first']}"
    assert ratio <= 1.0, f"{label}: a probe exceeds deform_model's bound ({ratio:.3f}x)"


# ------------------------------------------------------------------------------------------------------------ the pack (lib.mdcn)
MDCN_CASES = [("mdcn bf16 window S2", "bf16", "window", 2, 3900, 4096), ("mdcn bf16 gather S2", "bf16", "gather", 2, 3900, 4096),
              ("mdcn fp16 window S2", "fp16", "window", 2, 3900, 4096), ("mdcn fp16 gather S2", "fp16", "gather", 2, 3900, 4096),
              ("mdcn fp32 4K B2", "fp32", "window", 2, 2160, 3840), ("mdcn amp16 4K B2", "amp16", "window", 2, 2160, 3840)]
MDCN_PLANES = 4
MDCN_ASSIGN = [(c * 3) % MDCN_PLANES for c in range(18)]                             # deform_model.carrier_cases' "half_quarter" assignment
MDCN_LOGITS = [dm.ON, dm.HALF, dm.ON, dm.ON, dm.HALF, dm.ON, dm.HALF, dm.ON, dm.ON]


def census_restated(off, H, W, r0, r1):
    """deform_model.window_census on the rows [r0, r1) (r0 a multiple of 16) of exact offsets that live on the device: (samples outside
    the window, fix-up wave-taps, largest |offset| of the flagged waves).  A wave is 4 rows x 16 columns of a 16 x 16 tile."""
    dev = off.device
    B = off.shape[0]
    rows = torch.arange(r0, r1, device=dev)
    cols = torch.arange(W, device=dev)
    fy, fx = rows.float().view(1, -1, 1), cols.float().view(1, 1, -1)
    ty0, tx0 = (rows // 16 * 16 - 3).view(1, -1, 1), (cols // 16 * 16 - 3).view(1, 1, -1)
    n, Hp, Wp = r1 - r0, (r1 - r0 + 3) // 4 * 4, (W + 15) // 16 * 16
    outside = fixups = 0
    any_group = torch.zeros(B, Hp // 4, Wp // 16, dtype=torch.bool, device=dev)
    for k in range(9):
        py = ((fy - 1 + k // 3) + off[:, 2 * k, r0:r1]).clamp(-2.0, H + 1.0)
        px = ((fx - 1 + k % 3) + off[:, 2 * k + 1, r0:r1]).clamp(-2.0, W + 1.0)
        ly, lx = torch.floor(py).long() - ty0, torch.floor(px).long() - tx0
        out = (ly < 0) | (ly > 21) | (lx < 0) | (lx > 21)
        outside += int(out.sum())
        pad = torch.zeros(B, Hp, Wp, dtype=torch.bool, device=dev)
        pad[:, :n, :W] = out
        groups = pad.view(B, Hp // 4, 4, Wp // 16, 16).any(dim=4).any(dim=2)
        fixups += int(groups.sum())
        any_group |= groups
    pix = any_group.repeat_interleave(4, dim=1).repeat_interleave(16, dim=2)[:, :n, :W]
    amax = off[:, :, r0:r1].abs().amax(dim=1)
    return outside, fixups, float(amax[pix].max()) if bool(pix.any()) else 0.0


@pytest.mark.parametrize("case", MDCN_CASES, ids=[c[0] for c in MDCN_CASES])
def test_mdcn_across_the_lines(case):
    """lib.mdcn (offset_conv + sigmoid + DCN as a block of the forward runs them) on both routes.  The pack computes its own offsets
    in fp32, and (y - 1 + i) + dy rounds differently at row 3000 and at row 30 of a band - so, as tests/test_gpu_deform_lattice.py does,
    the offsets are made EXACT: channels 0..3 of x carry quarters within +-4 px (numbers of every storage type), offset_conv is zero but
    for one centre tap of 1.0 per offset channel, mask logits are +-40 / 0.  Kernel and float64 model then sample at the same position,
    and a band at the same position as the whole: equality on 16-row-aligned bands with a 16-row halo (asserted to cover the census'
    largest |offset| + 2), and deform_model's bounds on the probes (bound_pack16 with the kernel's own sigmoid, bound_fp32, bound_x3
    under amp16).  The census of the big run EQUALS the in-window test restated on the device band by band (test_gpu_mdcn's exact
    count) and shows that the fix-up arena ran; the gather route reports the same row.  measured: see MEASURED."""
    label, dtype, route, B, H, W = case
    C = 67
    wide = dtype in ("fp32", "amp16")
    pix = 80 * (4 if wide else 2)
    nbytes = lib.load().emavfi_mdcn_workspace_bytes(B, C, H, W, lib.dtype_code(dtype), 0) + B * H * W * 4 * (2 * C + 18)
    need_memory(nbytes + 6 * GIB, label)
    t0 = time.time()
    g = torch.Generator().manual_seed(6700 + H)
    dw = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    db = torch.randn(C, generator=g) * 0.1
    dws = dw if wide else storage_round(dw, dtype)
    dws = dws.half().float() if dtype == "bf16" else dws
    ow = torch.zeros(27, C, 3, 3)
    ob = torch.zeros(27)
    for c in range(18):
        ow[c if c < 9 else c + 9, MDCN_ASSIGN[c], 1, 1] = 1.0
    ob[9:18] = torch.tensor(MDCN_LOGITS)
    x = lh.device_normal((B, C, H, W), 6701 + W, DEV, "fp32" if wide else dtype)
    gd = torch.Generator(device=DEV).manual_seed(6702 + H)
    for s in range(B):
        x[s, :MDCN_PLANES].copy_(torch.randint(-16, 17, (MDCN_PLANES, H, W), device=DEV, generator=gd, dtype=torch.int32))
        x[s, :MDCN_PLANES] /= 4
    dev = [t.to(DEV) for t in (ow, ob, dws, db)]
    entry = lambda xt: lib.mdcn(xt, *dev, dtype=dtype, route=route)
    big = entry(x)
    row = lib.mdcn_census(B, C, H, W, dtype=dtype, device=DEV)[0]        # (before the bands reuse the workspace)
    assert big.shape == (B, C, H, W) and all_finite(big)

    off = torch.stack([x[:, MDCN_ASSIGN[c]] for c in range(18)], dim=1)           # the intended offsets: the carrier planes themselves
    msk = torch.sigmoid(torch.tensor(MDCN_LOGITS, dtype=torch.float64)).float()
    msk = (msk.half().float() if dtype == "amp16" else msk).view(1, 9, 1, 1)
    rows = max(16, BAND_BYTES // (4 * B * W * C) // 16 * 16 - 2 * DEFORM_HALO)
    bands = lh.band_ranges(H, rows, align=16)
    census = "no one-launch pack in this mode"
    if wide:
        assert row is None
    else:
        parts = [census_restated(off, H, W, o0, o1) for o0, o1 in bands]
        want = (sum(p[0] for p in parts), sum(p[1] for p in parts), B * ((H + 15) // 16) * ((W + 15) // 16) * 36, max(p[2] for p in parts))
        got_row = (row["samples_outside_window"], row["fixup_wave_taps"], row["wave_taps"], row["abs_offset_px_max"])
        census = f"census {got_row}, restated {want}"
        assert got_row == want, f"{label}: {census}"
        assert row["samples_outside_window"] > 0 and row["fixup_wave_taps"] > 0, "the fix-up path did not run"
        assert row["abs_offset_px_max"] + 2 <= DEFORM_HALO
    band = lh.band_check(entry, [x], big, bands, stride=1, halo=DEFORM_HALO, align=16)

    sets = lh.probe_pixels(B, H, W, pix, seed=H + 2)
    print(lh.describe_probes(label, sets, pix, H, W))
    probes = lh.merge_probes(sets) if wide else lh.merge_probes(sets, lh.probe_pixels(B, H, W, 144, seed=H + 3, n_random=0))
    bound_fn = {"fp32": lambda *a: dm.bound_fp32(*a), "amp16": lambda *a: dm.bound_x3(*a)}.get(
        dtype, lambda *a: dm.bound_pack16(*a, dtype, sigmoid_mask=True, bf16_window=dtype == "bf16"))
    ref, bound = deform_probe_model(x, off, msk.to(DEV).expand(B, 9, H, W), dws, db, dtype, probes, bound_fn)
    got = lh.gather_pixels(big, probes).cpu()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    finish(label, t0, f"{B}x{C}x{H}x{W} route {route}; plane {H * W * pix / GIB:.3f} GiB; {census}; bands {len(bands)}: compared {band['compared']}, "
           f"excluded {band['excluded']}, differing {band['differing']}; probes {len(probes)}: err / bound max {ratio:.3f}")
    assert band["excluded"] == 0 and band["compared"] == big.numel()
    assert band["differing"] == 0, f"{label}: band and whole differ in {band['differing']} elements, first in band {band['first']}"
    assert ratio <= 1.0, f"{label}: a probe exceeds deform_model's bound ({ratio:.3f}x)"


# ------------------------------------------------------------------------------------------------------------ warp
WARP_CASES = [("warp tiled C3 W%4==0", 3, 25900, 25924), ("warp nchw<false> C3 W%4!=0", 3, 25900, 25925), ("warp nchw<true> C1 W%4==0", 1, 25900, 25924)]
WARP_CHUNK = 1 << 24


@pytest.mark.parametrize("case", WARP_CASES, ids=[c[0] for c in WARP_CASES])
def test_warp_across_the_lines(case):
    """lib.warp at 6.7 * 10^8 pixels: each fp32 plane is 2.7 GB (offsets inside a plane have bit 31 set), frame2 at C = 3 spans 8 GB.
    Flows ~ 6 N(0, 1): most pixels sample inside the tiled kernel's LDS window (|flow| <= 8), the rest gather from global memory -
    both asserted.  Reference: large_harness.warp_model on EVERY pixel (module docstring: why not bands), err <= bound, elements
    excluded 0; the probe set of the plane geometry is printed and reported separately.  measured: see MEASURED."""
    label, C, H, W = case
    need_memory(int(4 * H * W * (2 * C + 2) * 1.05) + 6 * GIB, label)
    t0 = time.time()
    f2 = lh.device_normal((1, C, H, W), 25 + C + W, DEV)
    flow = lh.device_normal((1, 2, H, W), 26 + C + W, DEV)
    flow *= 6.0
    got = lib.warp(f2, flow)
    assert got.shape == f2.shape
    plane = H * W
    worst, checked, outside, far, near = 0.0, 0, 0, 0, 0
    fl = flow.view(2, plane)
    gv = got.view(C, plane)
    zero = torch.zeros(1, dtype=torch.long, device=DEV)
    for p0 in range(0, plane, WARP_CHUNK):
        pix = torch.arange(p0, min(p0 + WARP_CHUNK, plane), device=DEV)
        y, x = pix // W, pix % W
        fx, fy = fl[0, p0:p0 + pix.numel()], fl[1, p0:p0 + pix.numel()]
        ref, bound = lh.warp_model(f2, fx, fy, zero.expand(pix.numel()), y, x)
        err = (gv[:, p0:p0 + pix.numel()].t().double() - ref).abs()
        assert bool(torch.isfinite(err).all())
        outside += int((err > bound).sum())
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        checked += err.numel()
        far += int(((fx.abs() > 9) | (fy.abs() > 9)).sum())
        near += int(((fx.abs() < 7) & (fy.abs() < 7)).sum())
        del ref, bound, err
    sets = lh.probe_pixels(1, H, W, 4, seed=C)
    print(lh.describe_probes(label + " (one fp32 plane)", sets, 4, H, W))
    probes = lh.merge_probes(sets)
    pb, py, px = (torch.tensor([p[i] for p in probes], device=DEV) for i in range(3))
    ref, bound = lh.warp_model(f2, flow[0, 0, py, px], flow[0, 1, py, px], pb, py, px)
    pratio = float(((got[0, :, py, px].t().double() - ref).abs() / bound.clamp_min(1e-300)).max())
    finish(label, t0, f"1x{C}x{H}x{W}; plane {4 * plane / GIB:.3f} GiB, frame2 {4 * C * plane / GIB:.3f} GiB; float64 model on {checked} elements, excluded "
           f"{got.numel() - checked}, outside the bound {outside}, err / bound max {worst:.3f}; probes {len(probes)}: err / bound max {pratio:.3f}; "
           f"flows beyond the window {far}, inside {near}")
    assert checked == got.numel()
    assert far > 0 and near > 0
    assert outside == 0 and worst <= 1.0, f"{label}: {outside} elements outside the float64 model's bound ({worst:.3f}x)"
    assert pratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ the forward
PSNR_GATE = {"bf16": 50.0, "fp16": 65.0}      # the project's gates against the fp32-accurate result (tests/test_gpu_parity.py), here PER BLOCK
BLOCK = 256


def device_frames(seed, B, H, W):
    """Natural-like frame pairs made on the device, in the model's input range: six low-frequency sinusoids per channel plus 1 % noise
    (so no two positions agree), frame2 = the same field displaced by a sub-pixel shift of up to 4 px per sample, its own noise."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ys = torch.arange(H, device=DEV, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, device=DEV, dtype=torch.float32).view(1, 1, 1, W)
    par = torch.rand(6, 5, generator=g, device=DEV)
    shift = (torch.rand(B, 2, 1, 1, 1, generator=g, device=DEV) - 0.5) * 8
    mean = torch.tensor(lib.IMAGENET_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(lib.IMAGENET_STD, device=DEV).view(1, 3, 1, 1)
    ch = torch.arange(3, device=DEV, dtype=torch.float32).view(1, 3, 1, 1)
    frames = []
    for moved in (0.0, 1.0):
        f = torch.full((B, 3, H, W), 0.5, device=DEV)
        for k in range(6):
            fx, fy = (par[k, 0] - 0.5) * 0.06, (par[k, 1] - 0.5) * 0.06
            phase = 6.2831853 * (fx * (xs + moved * shift[:, 0]) + fy * (ys + moved * shift[:, 1])) + 6.2831853 * par[k, 2] + ch * par[k, 4]
            f += (0.04 + 0.08 * par[k, 3]) * torch.sin(phase)
            del phase
        noise = torch.empty_like(f).normal_(generator=g)
        f.add_(noise, alpha=0.01).clamp_(0.0, 1.0)
        del noise
        frames.append((f - mean) / std)
    return frames[0], frames[1]


def make_model(sd, dtype, policy="window", adapt=None):
    from emavfi import EMA_VFI
    m = EMA_VFI(mid_channels=64, compute_dtype=dtype).to(DEV).eval()
    m.load_state_dict(sd, strict=True)
    m.pack_policy = policy
    m.pack_adapt = adapt
    return m


def block_psnr_min(got, ref, peak=1.0):
    """The smallest PSNR over the 256 x 256 blocks of [B, C, H, W] tensors (mean over the channels, summed one channel at a time): the
    grid from the top-left corner plus the blocks aligned to the bottom and the right edge, so every pixel lies in a block.  A wrapped
    region cannot hide in a frame average."""
    import torch.nn.functional as F
    B, C, H, W = got.shape
    sq = torch.zeros(B, 1, H, W, dtype=torch.float64, device=got.device)
    for c in range(C):
        sq[:, 0] += (got[:, c].double() - ref[:, c].double()).pow(2)
    sq /= C
    worst = 0.0
    for rows in (slice(0, H // BLOCK * BLOCK), slice(max(H - BLOCK, 0), H)):
        for cols in (slice(0, W // BLOCK * BLOCK), slice(max(W - BLOCK, 0), W)):
            part = sq[:, :, rows, cols]
            if part.numel():
                worst = max(worst, float(F.avg_pool2d(part, (min(BLOCK, part.shape[2]), min(BLOCK, part.shape[3]))).max()))
    return 99.0 if worst == 0 else 10.0 * math.log10(peak * peak / worst)


FORWARD_BATCH = [("bf16", 4, "window", None), ("fp16", 4, "window", None), ("bf16", 4, "gather", None), ("bf16", 4, "window", "1"),
                 ("fp32", 2, "window", None), ("fp32x3", 2, "window", None), ("amp16", 2, "window", None)]


@pytest.mark.parametrize("dtype,B,policy,adapt", FORWARD_BATCH, ids=[f"{d}-B{b}-{p}{'-adapt' if a else ''}" for d, b, p, a in FORWARD_BATCH])
def test_forward_4k_batch_equals_every_sample_alone(dtype, B, policy, adapt):
    """3840 x 2160 with the context path live: every sample of the batch equals the same sample run alone, bit for bit (what the suite
    asserts at B = 8 x 720p).  B = 4 in the 16-bit modes - the 2.39 GB fusion buffer of a pair lies above 2^31, the batch's above 2^32
    and sample 3 beyond 2^33 - and B = 2 in the modes that keep a 4-byte plane of 2.65 GB per sample (in-sample offsets with bit 31 set).
    A sample alone runs at small offsets.  Under pack_adapt the route state is reset before every run (load_state_dict), so every run
    starts - and, being the first forward of its state, stays - on pack_policy's window route: what that case adds over the window
    case is the entry point alone (emavfi_forward_adaptive with its device-side route state and one census per forward, as one
    sequence instead of the pipelined pieces) at a workspace above 2^32.  The gather route above 2^31 inside a sample runs in
    test_forward_at_the_largest_frame."""
    from emavfi import synth
    H, W = 2160, 3840
    label = f"forward {dtype} B{B} {policy}{' adapt' if adapt else ''} 4K"
    ws = lib.load().emavfi_workspace_bytes(3, 64, 3, B, H, W, lib.dtype_code(dtype))
    assert ws > 1 << 32
    need_memory(ws + 6 * GIB, label)
    t0 = time.time()
    sd = synth.synthetic_state_dict(seed=3)
    f1, f2 = device_frames(40 + B, B, H, W)
    model = make_model(sd, dtype, policy, adapt)
    with torch.no_grad():
        out = model(f1, f2)
        assert out.shape == (B, 3, H, W) and bool(torch.isfinite(out).all())
        differing = 0
        for b in range(B):
            if adapt:
                model.load_state_dict(sd, strict=True)
            alone = model(f1[b:b + 1], f2[b:b + 1])
            differing += int((alone[0] != out[b]).sum())
    finish(label, t0, f"workspace {ws / GIB:.1f} GiB; {B} samples compared with themselves alone: {out.numel()} elements, differing {differing}")
    assert differing == 0


def test_forward_4k_blocks_against_the_fp32_accurate_mode():
    """3840 x 2160, B = 2: the bf16 and the fp16 frame against the fp32x3 frame of the same input, PER 256 x 256 BLOCK, with the
    project's gates (bf16 >= 50 dB, fp16 >= 65 dB).  The fp32x3 run is itself held batch-versus-alone above."""
    from emavfi import synth
    B, H, W = 2, 2160, 3840
    need_memory(lib.load().emavfi_workspace_bytes(3, 64, 3, B, H, W, lib.F32X3) + 6 * GIB, "forward blocks 4K")
    t0 = time.time()
    sd = synth.synthetic_state_dict(seed=3)
    f1, f2 = device_frames(50, B, H, W)
    with torch.no_grad():
        ref = make_model(sd, "fp32x3")(f1, f2).clone()
        lib.release_workspaces()
        torch.cuda.empty_cache()
        worst = {dt: block_psnr_min(make_model(sd, dt)(f1, f2), ref) for dt in PSNR_GATE}
    finish("forward blocks 4K B2", t0, "; ".join(f"{dt} block PSNR min {v:.1f} dB (gate {PSNR_GATE[dt]:.0f})" for dt, v in worst.items()))
    for dt, v in worst.items():
        assert v >= PSNR_GATE[dt], f"{dt}: a 256 x 256 block is at {v:.1f} dB against fp32x3"


def local_state_dict():
    """synthetic weights whose motion_estimation.0 ignores the pooled context (input channels 64..127 zero): the folded bias no longer
    depends on the whole frame and the forward is a local operation."""
    from emavfi import synth
    sd = synth.synthetic_state_dict(seed=3)
    w = sd["motion_estimation.0.0.weight"].clone()
    w[:, 64:] = 0
    sd["motion_estimation.0.0.weight"] = w
    return sd


LARGEST = (4095, 4096)        # the largest frame the guard admits: 2^24 - 4096 pixels, a 2.4 GB fusion plane in the 16-bit modes
SPLIT, BAND_A, BAND_B = 2048, (0, 2200), (1896, 4095)      # two overlapping bands of < 13 421 773 pixels: 152 rows of halo each


def band_rows(t, band):
    return t[:, :, band[0]:band[1]].contiguous()


LARGEST_CASES = [("bf16", "window"), ("bf16", "gather"), ("fp16", "window")]


@pytest.mark.parametrize("dtype,policy", LARGEST_CASES, ids=[f"{d}-{p}" for d, p in LARGEST_CASES])
def test_forward_at_the_largest_frame(dtype, policy):
    """4095 x 4096, B = 1, 16-bit modes, both pack routes: the only forward whose in-sample offsets have bit 31 set (a 2.4 GB fusion
    plane), with weights that make the forward local (local_state_dict).  Stage by stage, against the SAME model run on two overlapping
    bands (152 rows of halo; needed: 7 for the feature and flow convolutions + max|flow| + 1 + 3 (max|offset| + 3) + 3 for the
    reconstruction, from the flow tap and the census of the big run - asserted):
      * `feat` and `flow` taps: convolutions only - EQUAL to the bands, every element;
      * `warped` tap: not band-exact by definition (the warp normalises with the image height, module docstring); held on EVERY pixel
        to large_harness.warp_model on frame2 and the big run's own flow tap, plus the f16 rounding of the tail buffer (both 16-bit
        models store it as f16: tests/test_gpu_parity.py) - err <= bound + 2^-11 (|ref| + bound) + 2^-25;
      * `fused_k` taps and `out`: NOT band-exact and no per-element float64 model applies - the packs compute their offsets from their
        own input in fp32 and add them to the row index, (y - 1 + i) + dy, which rounds to 2^-12 px at row 3000 and to 2^-17 at row 30
        of a band; the sample then moves by that much and the f16 blend flips last places.  The share of differing elements and the
        smallest 256 x 256 block PSNR between whole and bands are MEASURED and printed (see MEASURED: the difference is rounding noise);
        what is asserted for them is the block gate against the fp32x3 forward on the same two bands (bf16 >= 50 dB, fp16 >= 65 dB;
        fp32x3 admits 13.4 M pixels, its own addressing at full planes is covered at 4K above) - a wrapped fetch puts foreign pixels
        into a block - and, for the pack kernels alone at this size, test_mdcn_across_the_lines / test_deform_conv2d_across_the_lines
        (equality with bands on exact offsets);
      * `ctx` tap against lib.context on the feat tap, with tests/test_gpu_stages.py's tolerances (bf16 2e-3, fp16 4e-4).
    Nothing is kept on the device between the cases: the fp32x3 reference is recomputed."""
    H, W = LARGEST
    L = lib.load()
    need_memory(L.emavfi_workspace_bytes(3, 64, 3, 1, H, W, lib.dtype_code(dtype)) + H * W * 4 * (64 + 3 * 67 + 11) + 8 * GIB, f"forward {dtype} largest")
    t0 = time.time()
    sd = local_state_dict()
    f1, f2 = device_frames(60, 1, H, W)
    fa, fb = (band_rows(f1, BAND_A), band_rows(f2, BAND_A)), (band_rows(f1, BAND_B), band_rows(f2, BAND_B))
    with torch.no_grad():
        x3 = make_model(sd, "fp32x3")
        ref = torch.cat([x3(*fa)[:, :, :SPLIT], x3(*fb)[:, :, SPLIT - BAND_B[0]:]], dim=2)
        del x3
        lib.release_workspaces()
        torch.cuda.empty_cache()
        model = make_model(sd, dtype, policy)
        out, taps = model(f1, f2, return_taps=True)
        rows = model.pack_census()
        lib.release_workspaces()
        torch.cuda.empty_cache()
        assert all(r["route"] == policy for r in rows)
        flow_max = float(taps["flow"].abs().max())
        off_max = max(r["abs_offset_px_max"] for r in rows)
        assert all(r["samples_outside_window"] > 0 for r in rows), "no sample left the window: the fix-up / gather path did not run"
        halo = 7 + flow_max + 1 + 3 * (off_max + 3) + 3
        assert halo <= min(BAND_A[1] - SPLIT, SPLIT - BAND_B[0]), f"halo {halo} rows needed"
        assert out.shape == (1, 3, H, W) and bool(torch.isfinite(out).all())
        worst = block_psnr_min(out, ref)
        # ---- the warped tap against the float64 model of the warp, every pixel
        plane = H * W
        pix = torch.arange(plane, device=DEV)
        wref, wbound = lh.warp_model(f2, taps["flow"][0, 0].reshape(-1), taps["flow"][0, 1].reshape(-1), torch.zeros_like(pix), pix // W, pix % W)
        werr = (taps["warped"].reshape(3, plane).t().double() - wref).abs()
        wlimit = wbound + 2.0 ** -11 * (wref.abs() + wbound) + 2.0 ** -25
        warp_outside, warp_ratio = int((werr > wlimit).sum()), float((werr / wlimit).max())
        del pix, wref, wbound, werr, wlimit
        # ---- the same model on the two bands: feat and flow equal, the later stages measured
        keep = ("feat", "flow", "fused_0", "fused_1", "fused_2", "out")
        differing, psnr_min = {k: 0 for k in keep}, {k: 99.0 for k in keep[2:]}
        for frames, whole_rows, local_rows in ((fa, slice(0, SPLIT), slice(0, SPLIT)), (fb, slice(SPLIT, H), slice(SPLIT - BAND_B[0], H - BAND_B[0]))):
            bo, bt = model(*frames, return_taps=True)
            bt["out"] = bo
            for k in keep:
                whole, part = (out if k == "out" else taps[k])[:, :, whole_rows], bt[k][:, :, local_rows]
                assert whole.shape == part.shape
                differing[k] += int((whole != part).sum())
                if k in psnr_min:
                    psnr_min[k] = min(psnr_min[k], block_psnr_min(whole, part, peak=1.0 if k == "out" else float(taps[k].abs().max())))
            del bo, bt
        measured = {k: (differing[k] / (out if k == "out" else taps[k]).numel(), psnr_min[k]) for k in psnr_min}
        compared = taps["feat"].numel() + taps["flow"].numel()
        feat, ctx = taps["feat"], taps["ctx"].clone()
        del taps, model
        lib.release_workspaces()
        torch.cuda.empty_cache()
        names = [f"context_encoding.{k}.{p}" for k in ("0.0", "1.0", "2.0", "5") for p in ("weight", "bias")]
        again = lib.context(feat, [sd[n].to(DEV) for n in names], dtype=dtype)
        cerr = float((again - ctx).abs().max())
        ctol = {"bf16": 2e-3, "fp16": 4e-4}[dtype] * max(1.0, float(ctx.abs().max()))
    finish(f"forward {dtype} {policy} largest", t0, f"1x3x{H}x{W}; max|flow| {flow_max:.2f}, census max|offset| {off_max:.2f}: halo needed {halo:.1f} of 152 rows; "
           f"feat + flow against the bands: {compared} elements, differing {differing['feat']} + {differing['flow']}; warped against the float64 model: "
           f"{3 * plane} elements, outside {warp_outside}, err / bound max {warp_ratio:.3f}; measured against the bands (share differing, block PSNR min): "
           + ", ".join(f"{k} {v[0]:.4f} {v[1]:.1f} dB" for k, v in measured.items())
           + f"; block PSNR min against fp32x3 on two bands {worst:.1f} dB (gate {PSNR_GATE[dtype]:.0f}); ctx tap against lib.context {cerr:.2e} (tolerance {ctol:.2e})")
    assert differing["feat"] == 0 and differing["flow"] == 0, f"feat / flow differ from their bands in {differing['feat']} / {differing['flow']} elements"
    assert warp_outside == 0, f"warped tap: {warp_outside} elements outside the float64 model ({warp_ratio:.3f}x)"
    assert worst >= PSNR_GATE[dtype], f"{dtype}: a 256 x 256 block is at {worst:.1f} dB against fp32x3"
    assert cerr <= ctol


# ------------------------------------------------------------------------------------------------------------ pitched 8-bit entries
# Small frames in a large buffer: the strides pass 2^32 (or 2^31 with bit 31 set), the work is tiny.
#   "batch": B = 2 frames of 34 x 70 x 3 with padded rows in ONE allocation, batch stride 2^32 + 4096;
#   "pitch": 3 rows of 70 pixels with a row pitch of 2^31 + 64 - only what the entry's own size check demands is allocated.
FILL = 0x7B
STRIDES = {"batch": (2, 34, 70, 70 * 3 + 6, (1 << 32) + 4096), "pitch": (1, 3, 70, (1 << 31) + 64, None)}


def pitched(B, H, W, C, pitch, bstride, frames=None):
    """(buffer filled with 0x7B, [B, H, W, C] view of it with the given byte strides holding `frames`)."""
    bs = bstride if bstride else pitch * H
    buf = torch.full(((B - 1) * bs + (H - 1) * pitch + W * C,), FILL, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(buf, (B, H, W, C), (bs, pitch, C, 1))
    if frames is not None:
        view.copy_(frames)
    return buf, view


def untouched(buf, view):
    """Every byte of `buf` outside `view` still holds the fill (compared on the device; the view itself is reset first)."""
    view.fill_(FILL)
    return bool((buf == FILL).all())


def random_frames(seed, B, H, W, C=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("entry", ["resize_u8", "luma_signature_u8", "frame_diff_cells", "frame_metrics_u8"])
@pytest.mark.parametrize("kind", list(STRIDES))
def test_pitched_entries_with_strides_beyond_the_lines(entry, kind):
    """Byte for byte against the exact oracles (resize_oracle, scene_oracle, dedup_oracle, metrics_oracle), and every byte of every
    buffer outside the frames unchanged.  measured: see MEASURED."""
    import numpy as np
    import dedup_oracle
    import metrics_oracle
    import resize_oracle
    import scene_oracle
    B, H, W, pitch, bstride = STRIDES[kind]
    need_memory(3 * ((B - 1) * (bstride or 0) + H * pitch) + 2 * GIB, f"{entry} {kind}")
    t0 = time.time()
    a, b = random_frames(11, B, H, W), random_frames(12, B, H, W)
    abuf, av = pitched(B, H, W, 3, pitch, bstride, a.to(DEV))
    if entry == "resize_u8":
        Hd, Wd = (21, 45) if kind == "batch" else (3, 45)
        obuf, ov = pitched(B, Hd, Wd, 3, Wd * 3 + 6 if kind == "batch" else pitch, bstride)
        lib.resize_u8(av, (Hd, Wd), out=ov)
        assert np.array_equal(ov.cpu().numpy(), resize_oracle.resize(a.numpy(), (Hd, Wd)))
        assert untouched(obuf, ov)
    elif entry == "luma_signature_u8":
        got = lib.luma_signature_u8(av, order="bgr")
        assert np.array_equal(got.cpu().numpy().astype(np.int64), scene_oracle.signature(a.numpy(), "bgr"))
    else:
        bbuf, bv = pitched(B, H, W, 3, pitch, bstride, b.to(DEV))
        if entry == "frame_diff_cells":
            got = lib.frame_diff_cells(av, bv, order="bgr")
            assert np.array_equal(got.cpu().numpy().astype(np.int64), dedup_oracle.cells(a.numpy(), b.numpy(), "bgr"))
        else:
            got = lib.frame_metrics_u8(av, bv)
            assert np.array_equal(got.cpu().numpy(), metrics_oracle.metrics(a.numpy(), b.numpy()))
        assert torch.equal(bv.cpu(), b) and untouched(bbuf, bv)
    assert torch.equal(av.cpu(), a) and untouched(abuf, av)
    finish(f"{entry} {kind}", t0, f"{B}x{H}x{W}x3, pitch {pitch}, batch stride {bstride}; equal to the oracle, every byte outside the frames unchanged")


@pytest.mark.parametrize("kind", list(STRIDES))
def test_nv12_planes_with_strides_beyond_the_lines(kind):
    """preprocess_nv12 / postprocess_nv12 with Y and UV planes whose batch stride / row pitch pass the lines: preprocess equals
    preprocess_u8 of nv12_oracle.decode's bytes bit for bit, postprocess equals nv12_oracle.encode of postprocess_u8's bytes (their
    definitions, as tests/test_gpu_nv12.py asserts them), and every byte outside the planes is unchanged."""
    import numpy as np
    import nv12_oracle
    B, H, W, pitch, bstride = STRIDES[kind]
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    need_memory(5 * ((B - 1) * (bstride or 0) + H * pitch) + 2 * GIB, f"nv12 {kind}")
    t0 = time.time()
    g = torch.Generator().manual_seed(31)
    ynp = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    uvnp = torch.randint(0, 256, (B, H2, W2, 2), generator=g, dtype=torch.uint8)
    ypitch = W + 2 if kind == "batch" else pitch

    def planes():
        ybuf, yv = pitched(B, H, W, 1, ypitch, bstride)
        ubuf, uv = pitched(B, H2, W2, 2, ypitch, bstride)
        return ybuf, yv[..., 0], ubuf, uv
    ybuf, yv, ubuf, uv = planes()
    yv.copy_(ynp.to(DEV))
    uv.copy_(uvnp.to(DEV))
    want = lib.preprocess_u8(torch.from_numpy(nv12_oracle.decode(ynp.numpy(), uvnp.numpy())).to(DEV))
    got = lib.preprocess_nv12(yv, uv)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(yv.cpu(), ynp) and torch.equal(uv.cpu(), uvnp)
    assert untouched(ybuf, yv) and untouched(ubuf, uv)
    del ybuf, yv, ubuf, uv
    ybuf, yo, ubuf, uo = planes()
    lib.postprocess_nv12(got, out=(yo, uo))
    ywant, uvwant = nv12_oracle.encode(lib.postprocess_u8(got).cpu().numpy())
    assert np.array_equal(yo.cpu().numpy(), ywant) and np.array_equal(uo.cpu().numpy(), uvwant)
    assert untouched(ybuf, yo) and untouched(ubuf, uo)
    finish(f"nv12 {kind}", t0, f"{B}x{H}x{W}, pitch {ypitch}, batch stride {bstride}; both directions equal to their definitions, every other byte unchanged")


def pitched_plane(B, H, rowlen, tail, es, pitch, bstride):
    """(buffer of 0x7B bytes, view [B, H, rowlen, *tail] of uint8 (es = 1) or 16-bit words (es = 2)) with BYTE strides pitch / bstride."""
    bs = bstride if bstride else pitch * H
    n = 1
    for t in tail:
        n *= t
    buf = torch.full(((B - 1) * bs + (H - 1) * pitch + rowlen * n * es,), FILL, dtype=torch.uint8, device=DEV)
    base = buf if es == 1 else buf[:buf.numel() // 2 * 2].view(torch.int16)
    strides = [bs // es, pitch // es, n] + [1] * len(tail)
    return buf, torch.as_strided(base, (B, H, rowlen, *tail), strides)


def untouched_plane(buf, view):
    view.fill_(FILL if view.dtype == torch.uint8 else FILL * 257)
    return bool((buf == FILL).all())


def words_t(a):
    """numpy uint8 / uint16 -> device tensor with the same bits (uint8 / int16)"""
    import numpy as np
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).to(DEV)


def words_np(t):
    import numpy as np
    t = t.contiguous().cpu()
    return t.numpy() if t.dtype == torch.uint8 else t.numpy().view(np.uint16)


@pytest.mark.parametrize("kind", list(STRIDES))
def test_p010_planes_with_strides_beyond_the_lines(kind):
    """preprocess_p010 / postprocess_p010 (depth 10) on 16-bit Y and UV planes whose batch stride / row pitch pass the lines: bit for
    bit p010_oracle.preprocess, word for word p010_oracle.postprocess, every byte outside the planes unchanged."""
    import numpy as np
    import p010_oracle
    B, H, W, pitch, bstride = STRIDES[kind]
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    need_memory(5 * ((B - 1) * (bstride or 0) + H * pitch) + 2 * GIB, f"p010 {kind}")
    t0 = time.time()
    rng = np.random.default_rng(41)
    ynp = (rng.integers(0, 1024, (B, H, W)) << 6).astype(np.uint16)
    uvnp = (rng.integers(0, 1024, (B, H2, W2, 2)) << 6).astype(np.uint16)
    ypitch = 2 * W + 12 if kind == "batch" else pitch
    ybuf, yv = pitched_plane(B, H, W, (), 2, ypitch, bstride)
    ubuf, uv = pitched_plane(B, H2, W2, (2,), 2, ypitch, bstride)
    yv.copy_(words_t(ynp))
    uv.copy_(words_t(uvnp))
    got = lib.preprocess_p010(yv, uv, 10)
    want = p010_oracle.preprocess(ynp, uvnp, 10)
    assert np.array_equal(got.cpu().numpy().view(np.int32), np.asarray(want, dtype=np.float32).view(np.int32))
    assert np.array_equal(words_np(yv), ynp) and np.array_equal(words_np(uv), uvnp)
    assert untouched_plane(ybuf, yv) and untouched_plane(ubuf, uv)
    lib.postprocess_p010(got, 10, out=(yv, uv))                    # (the planes were reset to the fill: the same buffers take the output)
    ywant, uvwant = p010_oracle.postprocess(got.cpu().numpy(), 10)
    assert np.array_equal(words_np(yv), ywant) and np.array_equal(words_np(uv), uvwant)
    assert untouched_plane(ybuf, yv) and untouched_plane(ubuf, uv)
    finish(f"p010 {kind}", t0, f"{B}x{H}x{W}, pitch {ypitch}, batch stride {bstride}; both directions equal to p010_oracle, every other byte unchanged")


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("kind", list(STRIDES))
def test_yuv420p_planes_with_strides_beyond_the_lines(kind, depth):
    """preprocess_yuv420p / postprocess_yuv420p, bytes and 10-bit words, three planes each with strides beyond the lines: equal to the
    numpy restatement of their definition (tests/test_gpu_yuv420p.py reference_pre / reference_post on nv12_oracle / p010_oracle)."""
    import numpy as np
    from test_gpu_yuv420p import rand_planes, reference_post, reference_pre
    B, H, W, pitch, bstride = STRIDES[kind]
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    es = 1 if depth == 8 else 2
    need_memory(5 * ((B - 1) * (bstride or 0) + H * pitch) + 2 * GIB, f"yuv420p {kind}")
    t0 = time.time()
    colour = ("bt601", False, "bgr")
    ynp, unp, vnp = rand_planes(np.random.default_rng(43), B, H, W, depth)
    ypitch = es * W + 6 if kind == "batch" else pitch
    bufs = [pitched_plane(B, r, c, (), es, ypitch, bstride) for r, c in ((H, W), (H2, W2), (H2, W2))]
    for (_, view), a in zip(bufs, (ynp, unp, vnp)):
        view.copy_(words_t(a))
    views = [v for _, v in bufs]
    got = lib.preprocess_yuv420p(*views, depth=depth)
    want = reference_pre(ynp, unp, vnp, depth, colour, on_device=False)
    assert np.array_equal(got.cpu().numpy().view(np.int32), np.asarray(want, dtype=np.float32).view(np.int32))
    assert all(np.array_equal(words_np(v), a) for v, a in zip(views, (ynp, unp, vnp)))
    assert all(untouched_plane(buf, v) for buf, v in bufs)
    lib.postprocess_yuv420p(got, depth=depth, out=tuple(views))
    wants = reference_post(got.cpu().numpy(), depth, colour, True, on_device=False)
    assert all(np.array_equal(words_np(v), w) for v, w in zip(views, wants))
    assert all(untouched_plane(buf, v) for buf, v in bufs)
    finish(f"yuv420p{depth} {kind}", t0, f"{B}x{H}x{W}, pitch {ypitch}, batch stride {bstride}; both directions equal to the definition, every other byte unchanged")


@pytest.mark.parametrize("kind", list(STRIDES))
def test_resized_fusions_with_strides_beyond_the_lines(kind):
    """preprocess_nv12(size=, resized_out=) = emavfi_preprocess_nv12_resized: source planes AND the resized planes it also writes
    have strides beyond the lines; the resized planes equal resize_oracle.resize_nv12 byte for byte and the fp32 result is the plain
    entry on the oracle's resized bytes, bit for bit.  The other fusion, emavfi_preprocess_u8_resized, takes no pitch or stride at all
    (include/emavfi.h: `frames_hwc`, `out_nchw`, `resized_hwc` are dense [B][H][W][C]; lib.preprocess_u8 refuses a non-contiguous
    resized_out), so it has no case here; its resize arithmetic is the launch shared with resize_u8, run pitched above."""
    import numpy as np
    import resize_oracle
    B, H, W, pitch, bstride = STRIDES[kind]
    Hd, Wd = (21, 45) if kind == "batch" else (3, 45)
    need_memory(6 * ((B - 1) * (bstride or 0) + H * pitch) + 2 * GIB, f"resized {kind}")
    t0 = time.time()
    H2, W2, Hd2, Wd2 = (H + 1) // 2, (W + 1) // 2, (Hd + 1) // 2, (Wd + 1) // 2
    g = torch.Generator().manual_seed(52)
    ynp = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    uvnp = torch.randint(0, 256, (B, H2, W2, 2), generator=g, dtype=torch.uint8)
    spitch = W + 2 if kind == "batch" else pitch
    opitch = Wd + 3 if kind == "batch" else pitch
    ybuf, yv = pitched_plane(B, H, W, (), 1, spitch, bstride)
    ubuf, uv = pitched_plane(B, H2, W2, (2,), 1, spitch, bstride)
    yobuf, yo = pitched_plane(B, Hd, Wd, (), 1, opitch, bstride)
    uobuf, uo = pitched_plane(B, Hd2, Wd2, (2,), 1, opitch, bstride)
    yv.copy_(ynp.to(DEV))
    uv.copy_(uvnp.to(DEV))
    got = lib.preprocess_nv12(yv, uv, size=(Hd, Wd), resized_out=(yo, uo))
    ys, uvs = (np.ascontiguousarray(t) for t in resize_oracle.resize_nv12(ynp.numpy(), uvnp.numpy(), (Hd, Wd)))
    assert np.array_equal(yo.cpu().numpy(), ys) and np.array_equal(uo.cpu().numpy(), uvs)
    want = lib.preprocess_nv12(torch.from_numpy(ys).to(DEV), torch.from_numpy(uvs).to(DEV))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(yv.cpu(), ynp) and torch.equal(uv.cpu(), uvnp)
    assert all(untouched_plane(bf, vw) for bf, vw in ((ybuf, yv), (ubuf, uv), (yobuf, yo), (uobuf, uo)))
    finish(f"resized fusions {kind}", t0, f"{B}x{H}x{W} -> {Hd}x{Wd}, batch stride {bstride}; resized planes equal to resize_oracle, every other byte unchanged")


@pytest.mark.parametrize("n,stride", [(2, (1 << 32) + 4096), (3, (1 << 31) + 64)])
def test_resample_frames_with_frame_strides_beyond_the_lines(n, stride):
    """emavfi_resample_frames: dst, srcs and nodes pools of dense 34 x 70 x 3 frames whose frame strides pass the lines; copies,
    blends from both pools and a held entry, byte for byte resample_oracle.assemble; every byte between the frames unchanged."""
    import numpy as np
    import resample_oracle
    need_memory(4 * n * stride + 2 * GIB, f"resample {n} x {stride}")
    t0 = time.time()
    shape, fb = (34, 70, 3), 34 * 70 * 3
    pools = {}
    for name in ("dst", "srcs", "nodes"):
        buf = torch.full(((n - 1) * stride + fb,), FILL, dtype=torch.uint8, device=DEV)
        pools[name] = (buf, torch.as_strided(buf, (n, *shape), (stride, 210, 3, 1)))
    srcs, nodes = random_frames(61, n, 34, 70), random_frames(62, n, 34, 70)
    pools["srcs"][1].copy_(srcs.to(DEV))
    pools["nodes"][1].copy_(nodes.to(DEV))
    last = n - 1
    table = [(0, last, 0, 0, 0), (0, lib.RESAMPLE_NODES + last, 77, 0, 0), (lib.RESAMPLE_NODES + 0, last, 200, 1, last)][:n]
    if n == 2:
        table = [(0, lib.RESAMPLE_NODES + last, 77, 0, 0), (lib.RESAMPLE_NODES + 0, last, 200, 1, last)]
    flags = torch.tensor([1], dtype=torch.int32, device=DEV)
    lib.resample_frames(pools["dst"][1], pools["srcs"][1], pools["nodes"][1], table, flags=flags)
    want = resample_oracle.assemble(srcs.numpy(), nodes.numpy(), table, flags=[1])
    assert np.array_equal(pools["dst"][1].cpu().numpy(), want)
    assert torch.equal(pools["srcs"][1].cpu(), srcs) and torch.equal(pools["nodes"][1].cpu(), nodes)
    assert all(untouched(buf, view) for buf, view in pools.values())
    finish(f"resample_frames {n} frames", t0, f"frame stride {stride}; equal to resample_oracle.assemble, every other byte unchanged")


@pytest.mark.parametrize("n,stride", [(2, (1 << 32) + 4096), (3, (1 << 31) + 64)])
def test_hold_frames_with_frame_strides_beyond_the_lines(n, stride):
    """emavfi_hold_frames_u8: dense frames of 34 x 70 x 3 whose dst AND alt frame strides pass the lines; flagged pairs are copied, the
    others and every byte between the frames are left as they were."""
    need_memory(3 * n * stride + 2 * GIB, f"hold_frames {n} x {stride}")
    t0 = time.time()
    fb = 34 * 70 * 3
    d, a = random_frames(21, n, 34, 70), random_frames(22, n, 34, 70)
    dbuf = torch.full(((n - 1) * stride + fb,), FILL, dtype=torch.uint8, device=DEV)
    abuf = torch.full(((n - 1) * stride + fb,), FILL, dtype=torch.uint8, device=DEV)
    dv, avw = (torch.as_strided(t, (n, 34, 70, 3), (stride, 210, 3, 1)) for t in (dbuf, abuf))
    dv.copy_(d.to(DEV))
    avw.copy_(a.to(DEV))
    flags = torch.tensor([1, 0, 1][:n] if n == 3 else [0, 1], dtype=torch.int32, device=DEV)
    lib.hold_frames_u8(dv, avw, flags)
    want = torch.where(flags.cpu().view(n, 1, 1, 1) != 0, a, d)
    assert torch.equal(dv.cpu(), want) and torch.equal(avw.cpu(), a)
    assert untouched(dbuf, dv) and untouched(abuf, avw)
    finish(f"hold_frames_u8 {n} frames", t0, f"frame stride {stride}; flagged frames copied, every other byte unchanged")


# MEASURED (MI355X, 288 GB; this file's own `LARGE` lines; 61 passed, 0 skipped; excluded elements: 0 in every case; wall = the test's
# call phase, which includes generating the inputs on the device and the float64 models on the host):
#   case                              elements compared (bands)   differing   probes: err / bound max (mismatch share)   peak GiB   wall s
#   tile fp32 256->256 S2             1 074 003 968               0           0.002                                     19.5       0.9
#   tile fp32 256->256 S1             1 073 391 360               0           0.002                                     23.0       1.1
#   tile bf16 6->64 out>4GiB          2 147 757 120               0           0.980 (0 %)                               27.8       1.0
#   tile fp32 6->64 out>4GiB          1 073 745 920               0           0.039                                     16.4       0.1
#   tile x3 64->64 under / over       1 073 479 680 / ..745 920   0 / 0       0.003 / 0.003                             23.0       1.7 / 0.2
#   wreg fp16 256->256 s1 S2          2 147 549 184               0           0.456 (0.072 %)                           31.0       1.7
#   wreg bf16 128->256 s2 S2          1 074 252 800               0           0.887 (0.006 %)                           21.5       0.2
#   s2ring fp16 64->128 s2 S2         1 074 187 776               0           0.739 (0.023 %)                           21.5       1.7
#   ring2 bf16 64->64 S2              2 147 491 840               0           0.921 (0 %)                               31.0       0.2
#   ring3 fp16 67->64 S2              1 718 385 536               0           0.763 (0.081 %)                           25.9       1.6
#   persist16 bf16 64->32 S2          1 073 745 920               0           0.943 (0 %)                               21.5       0.1
#   persist16 fp16 64->64 noring S2   2 147 855 616               0           0.759 (0.029 %)                           31.0       1.5
#   persist32 fp16 64->32 S2          1 073 745 920               0           0.723 (0.046 %)                           21.5       0.1
#   light bf16 32->3 S2 / fp16 S1     201 352 230 / 201 302 016   0 / 0       0.001 / 0.001                             15.8 / 16.1  0.1 / 2.2
#   deform bf16 / fp16 67->67 S2      2 140 569 600               0 / 0       0.726 / 0.467                             39.5       0.6 / 0.5
#   deform fp32 67->67 4K B2          1 111 449 600               0           0.003                                     25.4       2.9
#   mdcn bf16 window / gather S2      2 140 569 600               0 / 0       0.896 / 0.896                             35.3       0.8 / 0.7
#   mdcn fp16 window / gather S2      2 140 569 600               0 / 0       0.587 / 0.587                             35.3       0.6 / 0.7
#   mdcn fp32 / amp16 4K B2           1 111 449 600               0 / 0       0.002 / 0.001                             24.3 / 29.3  2.8 / 1.8
#     (every mismatch is one unit; mdcn census, all four 16-bit cases: 8 260 676 samples outside the window, 3 187 295 fix-up wave-taps of
#      4 497 408, largest |offset| 4.0 - equal to the restatement, so the fix-up arena ran in 71 % of the wave-taps)
#   warp tiled C3 / nchw<false> C3    2 014 294 800 / 2 014 372 500 elements against the float64 model, 0 outside the bound, err / bound max
#                                     0.480 / 0.459, probes 0.278 / 0.245; 1.67 * 10^8 flows beyond the window, 3.84 * 10^8 inside; 25.3 GiB; 0.7 s
#   warp nchw<true> C1                671 431 600 elements, 0 outside, 0.483, probes 0.187; 13.9 GiB; 0.4 s
#   forward 4K, batch = alone         bf16 / fp16 / bf16 gather / bf16 adaptive at B = 4: 99 532 800 elements each, differing 0 (workspace 26.0 GiB,
#                                     peak 27.7, <= 0.8 s); fp32 / fp32x3 / amp16 at B = 2: 49 766 400 each, differing 0 (peak 25.7 / 35.6 / 24.1 GiB,
#                                     0.4 / 4.3 / 0.1 s)
#   forward 4K B2, blocks vs fp32x3   bf16 55.7 dB (gate 50), fp16 72.7 dB (gate 65): the smallest 256 x 256 block; 35.5 GiB; 0.4 s
#   forward 4095 x 4096               bf16 window / bf16 gather / fp16: max|flow| 8.1, census max|offset| 5.07: 43.3 of the 152 halo rows needed;
#     (against the same model          feat + flow: 1 107 025 920 elements, differing 0 + 0 in all three; warped against the float64 model + f16
#      on two bands)                   store: 50 319 360 elements, 0 outside, err / bound max 0.999 (a round-to-nearest store reaches its half unit);
#                                     ctx tap = lib.context on the feat tap bit for bit; smallest block against fp32x3 on the bands 55.4 / 55.4 /
#                                     72.4 dB (gates 50 / 50 / 65); peak 39.0 GiB; 0.6 .. 6.8 s.
#                                     MEASURED ONLY (not band-exact, see the docstring) - share of elements that differ from the bands and the
#                                     smallest 256 x 256 block PSNR (peak = the tap's max) against them:
#                                       bf16 (both routes)  fused_0 22.4 % 86.7 dB, fused_1 38.8 % 83.5 dB, fused_2 15.4 % 75.7 dB, out 94.0 % 63.2 dB
#                                       fp16                fused_0 22.4 % 86.7 dB, fused_1 38.8 % 83.5 dB, fused_2 51.1 % 82.5 dB, out 94.3 % 74.8 dB
#                                     i.e. last-place flips of the 16-bit stores spread over every block alike (the frame is fp32: nearly every
#                                     element moves, by ~ 1e-3 / 2e-4), 8 to 30 dB above the mode's own distance from fp32x3 - rounding noise, where
#                                     the fetch defect put foreign pixels into 16 % of the elements below the line (deform bf16 case).
#   pitched entries (resize_u8, luma_signature_u8, frame_diff_cells, frame_metrics_u8, hold_frames_u8, resample_frames, nv12, p010, yuv420p 8 / 10
#   bit, preprocess_nv12_resized)     byte-exact against the oracles, every byte outside the frames unchanged; <= 8.1 GiB (resized: 20.0 GiB);
#                                     0.01 .. 0.05 s (3 - 4 s where a process first allocates its 4.3 GB buffers)
# Before the fix in csrc/deform_pack3_body.inl (the parent commit's library, same file): `deform bf16 67->67 S2` differed from its bands in
# 55 987 048 elements, first in row 3271 of sample 0 (pixel (3276, 3277) is where the byte offset reaches 2^31), probes at 36.3 x the bound.
