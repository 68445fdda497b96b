"""tests/large_harness.py must SEE an aliased address.  No deliberately broken kernel may run on a GPU (a wrapped address is an
out-of-bounds access), so the sensitivity is shown here: a numpy stand-in for an entry - a 3x3 convolution that reads its input from a
flat channels-last byte buffer through its own address arithmetic - at toy size, with toy wrap moduli in place of 2^31 and 2^32, and
four injected defects of the kind a narrow cast produces.  Each defect must be caught by a NAMED check (band or probe), the stand-in
without a defect must pass both, and the probe-set computation is compared with hand-worked offsets."""
import numpy as np
import pytest
import torch

import large_harness as lh
from rounding_model import conv_model

# toy geometry: 4 fp32 channels = 16 bytes per pixel, 40 x 16 pixels = 10 240 bytes per sample, 2 samples = 20 480 bytes
B, C, H, W, COUT = 2, 4, 40, 16, 3
PIXBYTES = 4 * C
WRAP31, WRAP32, WRAP33 = 4096, 8192, 16384     # the in-sample line, its double, and the second total line
TOY_WRAPS = (WRAP31, WRAP32, WRAP33)
SHIFT_FROM_ROW = 24                            # the `stitch` defect: output rows from here on are written one row off


def standin(x, w, bias, defect=None):
    """y = conv3x3(x, w) + bias, pad 1, read through a flat channels-last buffer.  The address of input pixel (b, pix) is
    base(b) + off(pix) bytes; `defect` breaks one of the two as a narrow type would.  Every element is summed in the same fixed order
    (taps, then channels) whatever the shape, so a band and the whole agree bit for bit - as the kernels' per-pixel order does."""
    xb, xc, xh, xw_ = x.shape
    buf = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(-1)            # channels-last, in elements of 4 bytes
    plane_bytes = xh * xw_ * PIXBYTES
    out = np.zeros((xb, w.shape[0], xh, xw_), dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(xh), np.arange(xw_), indexing="ij")
    for b in range(xb):
        base = b * plane_bytes
        if defect == "base":                                                  # sample base truncated to the narrow type
            base %= WRAP32
        for i in range(3):
            for j in range(3):
                gy, gx = ys + i - 1, xs + j - 1
                ok = (gy >= 0) & (gy < xh) & (gx >= 0) & (gx < xw_)
                off = (np.clip(gy, 0, xh - 1) * xw_ + np.clip(gx, 0, xw_ - 1)) * PIXBYTES
                if defect == "modulo":                                        # offset taken modulo the wrap
                    off = off % WRAP31
                if defect == "sign":                                          # offset sign-extended, clamped to stay in bounds
                    off = np.where(off >= WRAP31, np.maximum(off - WRAP32, 0), off)
                for c in range(xc):
                    v = np.where(ok, buf[(base + off) // 4 + c], 0.0)
                    for o in range(w.shape[0]):
                        out[b, o] += v.astype(np.float64) * float(w[o, c, i, j])
    out += bias.reshape(1, -1, 1, 1)
    if defect == "stitch" and xh > SHIFT_FROM_ROW + 1:                         # a region of rows written one row off
        out[:, :, SHIFT_FROM_ROW:-1] = out[:, :, SHIFT_FROM_ROW + 1:].copy()
    return out.astype(np.float32)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)                   # no period: every position differs
    w = (rng.standard_normal((COUT, C, 3, 3)) / 6).astype(np.float32)
    bias = (rng.standard_normal(COUT) * 0.1).astype(np.float32)
    return x, w, bias


def run_checks(case, defect):
    """The two references exactly as tests/test_gpu_large.py applies them to a convolution: {band: differing elements, excluded,
    probe: max err / bound}."""
    x, w, bias = case
    xt, wt, bt = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias)
    big = torch.from_numpy(standin(x, w, bias, defect))
    # the bands run the same entry, defect and all: at band size no offset reaches a line, as on the device
    entry = lambda t: torch.from_numpy(standin(t.numpy(), w, bias, defect))
    band = lh.band_check(entry, [xt], big, lh.band_ranges(H, 8), stride=1, halo=1)
    sets = lh.probe_pixels(B, H, W, PIXBYTES, wraps=TOY_WRAPS, n_random=16, seed=1)
    probes = lh.merge_probes(sets)
    crops = lh.gather_crops(xt, probes, 3)
    ref, bound, _ = conv_model(crops, wt, bt, 1, "none", "fp32", fp32_products=True)
    got = lh.gather_pixels(big, probes)
    ratio = ((got.double() - ref[:, :, 1, 1]).abs() / bound[:, :, 1, 1]).max().item()
    return {"band": band["differing"], "excluded": band["excluded"], "compared": band["compared"], "probe": ratio}


def test_the_clean_standin_passes_both_references(case):
    r = run_checks(case, None)
    assert r["band"] == 0 and r["excluded"] == 0 and r["compared"] == B * COUT * H * W
    assert r["probe"] <= 1.0


@pytest.mark.parametrize("defect", ["modulo", "sign", "base", "stitch"])
def test_every_injected_defect_is_caught_by_both_named_checks(case, defect):
    """modulo: pixels at or above byte 4096 of a sample read pixel - 256; sign: they read pixel 0; base: sample 1 (base 10 240) reads
    from byte 2 048 of sample 0; stitch: rows 24.. hold their lower neighbour.  The band runs stay below every toy line (8 + 2 rows =
    2 560 bytes per sample, 5 120 in all) and never shift (10 rows), so band = whole fails; the probes sit on the lines and on the
    last pixels, so err / bound fails."""
    r = run_checks(case, defect)
    print(defect, r)
    assert r["excluded"] == 0
    assert r["band"] > 0, f"{defect}: the band reference did not see it"
    assert r["probe"] > 1.0, f"{defect}: the probes did not see it"


def test_band_check_counts_every_element_and_refuses_gaps(case):
    x, w, bias = case
    xt = torch.from_numpy(x)
    big = torch.from_numpy(standin(x, w, bias))
    entry = lambda t: torch.from_numpy(standin(t.numpy(), w, bias))
    for rows in (1, 7, 8, 40, 64):
        r = lh.band_check(entry, [xt], big, lh.band_ranges(H, rows))
        assert r == {"compared": big.numel(), "excluded": 0, "differing": 0, "first": None}
    with pytest.raises(AssertionError):
        lh.band_check(entry, [xt], big, [(0, 8), (9, 40)])
    with pytest.raises(AssertionError):
        lh.band_check(entry, [xt], big, [(0, 8), (8, 32)])
    # a halo that is too small is seen, not excused: the band's cut edge reads zeros where the image has data
    assert lh.band_check(entry, [xt], big, lh.band_ranges(H, 8), halo=0)["differing"] > 0


def test_band_rows_for_stride_two_and_tile_phase():
    assert lh.band_input_rows(0, 8, 40, 1, 1) == (0, 9, 0)
    assert lh.band_input_rows(8, 16, 40, 1, 1) == (7, 17, 1)
    assert lh.band_input_rows(32, 40, 40, 1, 1) == (31, 40, 1)
    # stride 2: output rows 4..7 read input rows 7..15; the band starts on the even row 6, where output row 3 begins
    assert lh.band_input_rows(4, 8, 37, 2, 1, align=2) == (6, 16, 1)
    assert lh.band_input_rows(16, 19, 37, 2, 1, align=2) == (30, 37, 1)
    # deformable bands keep the 16-row tile phase: halo 16, starts on multiples of 16
    assert lh.band_input_rows(32, 64, 100, 1, 16, align=16) == (16, 80, 16)
    assert lh.band_ranges(40, 8) == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 40)]
    assert lh.band_ranges(37, 20, align=16) == [(0, 16), (16, 32), (32, 37)]


def test_probe_set_against_hand_worked_offsets():
    """16 bytes per pixel, 16 pixels per row = 256 bytes per row, 10 240 per sample.  In-sample line 4 096 = pixel 256 = (16, 0) exactly,
    8 192 = pixel 512 = (32, 0).  Total offset 8 192 lies in sample 0 (pixel 512); total 16 384 = 10 240 + 6 144 = sample 1, pixel 384 =
    (24, 0)."""
    s = lh.probe_pixels(B, H, W, PIXBYTES, wraps=TOY_WRAPS, n_random=5, seed=0)
    assert s["in-sample 1"] == [(0, 15, 15), (0, 16, 0), (0, 16, 1), (1, 15, 15), (1, 16, 0), (1, 16, 1)]
    assert s["in-sample 2"] == [(0, 31, 15), (0, 32, 0), (0, 32, 1), (1, 31, 15), (1, 32, 0), (1, 32, 1)]
    assert "in-sample 3" not in s                                   # 12 288 is past the plane
    assert s[f"total {WRAP32}"] == [(0, 31, 15), (0, 32, 0), (0, 32, 1)]
    assert s[f"total {WRAP33}"] == [(1, 23, 15), (1, 24, 0), (1, 24, 1)]
    assert s["ends"] == [(0, 0, 0), (0, 39, 15), (1, 0, 0), (1, 39, 15)]
    assert s["corners"] == [(1, 0, 0), (1, 0, 15), (1, 39, 0), (1, 39, 15)]
    assert len(s["random"]) == 2 * 5 and all(0 <= b < B and 0 <= y < H and 0 <= x < W for b, y, x in s["random"])
    # a line that is no multiple of the pixel size is STRADDLED: 24 bytes per pixel, line 4 096 = 170 * 24 + 16 lies inside pixel 170
    t = lh.probe_pixels(1, 40, 16, 24, wraps=TOY_WRAPS, n_random=0)
    assert t["in-sample 1"] == [(0, 10, 9), (0, 10, 10), (0, 10, 11)] and 170 * 24 < 4096 < 171 * 24
    # a buffer shorter than a total line has no probe for it; the real lines are the defaults
    assert f"total {WRAP33}" not in lh.probe_pixels(1, 40, 16, 16, wraps=TOY_WRAPS, n_random=0)
    assert lh.WRAPS == (2 ** 31, 2 ** 32, 2 ** 33)
    big = lh.probe_pixels(2, 1928, 1088, 1024, n_random=0)          # the 256 -> 256 fp32 case: 2 148 007 936 bytes per sample
    assert big["in-sample 1"][:3] == [(0, 1927, 575), (0, 1927, 576), (0, 1927, 577)] and 2 ** 31 // 1024 == 1927 * 1088 + 576
    assert big[f"total {2 ** 32}"] == [(1, 1927, 63), (1, 1927, 64), (1, 1927, 65)] and 2 ** 32 // 1024 - 1928 * 1088 == 1927 * 1088 + 64
    assert lh.merge_probes(s) == sorted(set(p for v in s.values() for p in v))
    assert "0x1000" in lh.describe_probes("toy", s, PIXBYTES, H, W)


def test_crops_are_zero_outside_the_image_and_centred():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7) + 1
    crops = lh.gather_crops(x, [(0, 0, 0), (1, 4, 6), (1, 2, 3)], 3)
    assert crops.shape == (3, 3, 3, 3)
    assert torch.equal(crops[2], x[1, :, 1:4, 2:5])
    assert torch.equal(crops[0][:, 1:, 1:], x[0, :, :2, :2]) and crops[0][:, 0].abs().sum() == 0 and crops[0][:, :, 0].abs().sum() == 0
    assert torch.equal(crops[1][:, :2, :2], x[1, :, 3:, 5:]) and crops[1][:, 2].abs().sum() == 0
    five = lh.gather_crops(x, [(0, 1, 2)], 5, centre_of=lambda y, x: (2 * y, 2 * x))      # stride 2: centred on the input pixel (2, 4)
    assert torch.equal(five[0], x[0, :, 0:5, 2:7])
    assert torch.equal(lh.gather_pixels(x, [(1, 4, 6), (0, 0, 0)]), torch.stack([x[1, :, 4, 6], x[0, :, 0, 0]]))


def test_warp_model_matches_grid_sample():
    """The float64 restatement against the oracle (ATen's fp32 grid_sample) on every pixel of a small case with flows that leave the
    image: inside its own bound."""
    from oracle import emavfi_oracle as oracle
    g = torch.Generator().manual_seed(3)
    f2, flow = torch.randn(2, 3, 33, 44, generator=g), torch.randn(2, 2, 33, 44, generator=g) * 6
    b, y, x = (t.reshape(-1) for t in torch.meshgrid(torch.arange(2), torch.arange(33), torch.arange(44), indexing="ij"))
    ref, bound = lh.warp_model(f2, flow[b, 0, y, x], flow[b, 1, y, x], b, y, x)
    want = oracle.warp(f2, flow)[b, :, y, x]
    assert ((want.double() - ref).abs() <= bound + 1e-30).all()
    assert bound.max().item() < 1e-5 and (ref == 0).any() and (ref != 0).any()
