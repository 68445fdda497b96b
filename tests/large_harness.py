"""References for tensors that are too big for a CPU oracle: what tests/test_gpu_large.py holds the entries to where byte offsets pass
2^31 and 2^32, and what tests/test_large_harness_cpu.py shows to be sensitive to an aliased address.  Knows nothing of the library:
an `entry` is any callable tensor(s) -> tensor, so the same code runs a HIP entry on the device and a numpy stand-in on the CPU.

Two complementary references.

  BAND (band_check): every single-stage operation is local, so the same entry run on a band of input rows (with the halo the operation
  needs) must return, on the band's interior rows, what the big run returned there - bit for bit: the per-pixel accumulation order of
  the kernels does not depend on the row or the tile index.  The bands tile the full height, so EVERY output element is compared; the
  check returns the number compared and the number excluded (asserted 0 by the callers).  A band runs at small offsets - inside the
  range the rest of the suite already holds to float64 references - so a defect that needs a large offset shows as a difference.

  PROBES (probe_pixels): pixels chosen from the case's geometry where an address can go wrong - either side of every multiple of 2^31
  inside a sample, either side of a total offset of 2^32 and 2^33, the first and last pixel of every sample, the corners of the last
  sample, and 64 seeded random pixels per sample - are held to the float64 per-element models of the suite (rounding_model.conv_model,
  deform_model with sample64, and warp_model below) on a crop cut around each probe: independent of the project's kernels.

Inputs (device_normal) come from a seeded generator on the device, carry no period (a wrapped address that landed on an identical tile
would compare equal) and are pre-rounded to the storage type as tests/test_gpu_conv_rounding_model.py does.  Only crops and probe
pixels ever travel to the host."""
import numpy as np
import torch

WRAPS = (1 << 31, 1 << 32, 1 << 33)   # (in-sample line, total line, total line): the CPU self-test passes toy values instead
RANDOM_PER_SAMPLE = 64


# ------------------------------------------------------------------------------------------------------------ the probe set
def probe_pixels(B, H, W, pixbytes, wraps=WRAPS, n_random=RANDOM_PER_SAMPLE, seed=0):
    """{label: [(b, y, x)]} for one channels-last buffer of B samples of H x W pixels of `pixbytes` bytes each:
      in-sample k  the pixel whose bytes hold offset k * wraps[0] of its sample (it STRADDLES the line when the line is no multiple of
                   pixbytes, otherwise it starts on it) and its two neighbours, for every k >= 1 below the plane size, in every sample;
      total T      the pixels on either side of total offset T (from the start of sample 0) for T in wraps[1:], where the buffer is
                   that long;
      ends         the first and the last pixel of every sample; corners: the four image corners of the last sample;
      random       n_random seeded pixels per sample."""
    plane = H * W
    out = {}

    def coords(b, pix):
        return (b, pix // W, pix % W)

    k = 1
    while k * wraps[0] < plane * pixbytes:
        p = k * wraps[0] // pixbytes
        out[f"in-sample {k}"] = [coords(b, q) for b in range(B) for q in (p - 1, p, p + 1) if 0 <= q < plane]
        k += 1
    for T in wraps[1:]:
        g = T // pixbytes
        hit = [coords(q // plane, q % plane) for q in (g - 1, g, g + 1) if 0 <= q < B * plane]
        if hit and g < B * plane:
            out[f"total {T}"] = hit
    out["ends"] = [coords(b, q) for b in range(B) for q in (0, plane - 1)]
    out["corners"] = [(B - 1, y, x) for y in (0, H - 1) for x in (0, W - 1)]
    rng = np.random.default_rng(seed)
    out["random"] = [coords(b, int(q)) for b in range(B) for q in rng.integers(0, plane, n_random)]
    return out


def merge_probes(*sets):
    """The union of probe sets as a sorted list of distinct (b, y, x)."""
    return sorted({p for s in sets for pts in s.values() for p in pts})


def describe_probes(label, sets, pixbytes, H, W):
    """One line per named group with the byte offsets inside the sample: printed by every case (a fault is then read from here)."""
    lines = []
    for name, pts in sets.items():
        if name == "random":
            lines.append(f"  {name}: {len(pts)} pixels")
            continue
        lines.append(f"  {name}: " + ", ".join(f"b{b} ({y},{x}) @ {(y * W + x) * pixbytes:#x}" for b, y, x in pts))
    return f"probes {label} ({pixbytes} B per pixel):\n" + "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------ the band reference
def band_ranges(n_rows, rows_per_band, align=1):
    """[(o0, o1)] tiling [0, n_rows) with bands of at most rows_per_band rows that start on multiples of `align`."""
    step = max(align, rows_per_band // align * align)
    return [(o0, min(o0 + step, n_rows)) for o0 in range(0, n_rows, step)]


def band_input_rows(o0, o1, H_in, stride, halo, align=1):
    """Input rows [i0, i1) a band of output rows [o0, o1) needs with `halo` input rows on either side, i0 moved down to a multiple of
    `align` (stride-2 bands start on even rows; tiled kernels keep their tile phase), and the band-local index of output row o0."""
    i0 = max(0, (stride * o0 - halo) // align * align)
    i1 = min(H_in, stride * (o1 - 1) + halo + 1)
    assert i0 % stride == 0
    return i0, i1, o0 - i0 // stride


def band_check(entry, inputs, big, bands, stride=1, halo=1, align=1, row_dim=2):
    """Run `entry` on every band of `inputs` (a list of tensors cut along row_dim) and compare the interior rows with the same rows of
    `big`.  Returns {compared, excluded, differing, first}: `first` = (band, index of the first differing element inside it)."""
    H_in, H_out = inputs[0].shape[row_dim], big.shape[row_dim]
    compared = differing = 0
    first = None
    covered = 0
    for o0, o1 in bands:
        assert o0 == covered, "bands must tile the output height"
        covered = o1
        i0, i1, lo = band_input_rows(o0, o1, H_in, stride, halo, align)
        got = entry(*[t.narrow(row_dim, i0, i1 - i0).contiguous() for t in inputs])
        part = got.narrow(row_dim, lo, o1 - o0)
        want = big.narrow(row_dim, o0, o1 - o0)
        assert part.shape == want.shape, (part.shape, want.shape)
        diff = part != want
        n = int(diff.sum())
        if n and first is None:
            first = ((o0, o1), [int(v) for v in diff.nonzero()[0]])
        compared += want.numel()
        differing += n
        del got, part, diff
    assert covered == H_out, "bands must tile the output height"
    return {"compared": compared, "excluded": big.numel() - compared, "differing": differing, "first": first}


# ------------------------------------------------------------------------------------------------------------ crops around probes
def gather_crops(x, probes, k, centre_of=lambda y, x: (y, x)):
    """[N, C, k, k] crops of x [B, C, H, W] (k odd) centred on centre_of(y, x) of each probe, ZERO where the crop leaves the image - what
    a pad-1 convolution reads there.  Gathered where x lives; the result is small."""
    B, C, H, W = x.shape
    dev = x.device
    b = torch.tensor([p[0] for p in probes], device=dev)
    cy = torch.tensor([centre_of(p[1], p[2])[0] for p in probes], device=dev)
    cx = torch.tensor([centre_of(p[1], p[2])[1] for p in probes], device=dev)
    d = torch.arange(k, device=dev) - k // 2
    ys, xs = cy[:, None] + d[None], cx[:, None] + d[None]                                    # [N, k]
    ok = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :]             # [N, k, k]
    v = x[b[:, None, None], :, ys.clamp(0, H - 1)[:, :, None], xs.clamp(0, W - 1)[:, None, :]]   # [N, k, k, C]
    return (v * ok[..., None]).permute(0, 3, 1, 2).contiguous()


def gather_pixels(y, probes):
    """[N, C] values of y [B, C, H, W] at the probes."""
    dev = y.device
    b, r, c = (torch.tensor([p[i] for p in probes], device=dev) for i in range(3))
    return y[b, :, r, c]


# ------------------------------------------------------------------------------------------------------------ device inputs
def device_normal(shape, seed, device, dtype="fp32", channel_scale=False):
    """N(0, 1) of `shape` from a seeded generator ON the device, optionally scaled per channel (dim 1) by 2^-3 .. 2^3 as
    rounding_model.scaled_input does, rounded IN PLACE (one sample at a time) to the storage type."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.empty(shape, device=device, dtype=torch.float32)
    for b in range(shape[0]):
        x[b].normal_(generator=g)
    if channel_scale:
        x *= torch.tensor([2.0 ** ((c % 7) - 3) for c in range(shape[1])], device=device).view(1, -1, *([1] * (len(shape) - 2)))
    if dtype != "fp32":
        for b in range(shape[0]):
            x[b].copy_(x[b].bfloat16() if dtype == "bf16" else x[b].half())
    return x


# ------------------------------------------------------------------------------------------------------------ the warp in float64
WARP_ROUNDINGS = 8   # four rounded products and three rounded adds (or FMAs) of fp32, + 1: |kernel - ref| <= 8 * 2^-24 * sum|p w|


def _r32(t):
    """Round a float64 tensor to fp32 and widen again: after ONE +, -, * or / of fp32 numbers done in float64 this IS the correctly
    rounded fp32 result (53 >= 2 * 24 + 2 bits), wherever the tensor lives and whatever its backend's fp32 division does."""
    return t.float().double()


def warp_model(frame2, flow_x, flow_y, b, y, x):
    """oracle.warp (oracle/emavfi_oracle.py: pixel grid + flow, normalised with a true division, grid_sample bilinear / zeros /
    align_corners) restated per pixel.  The coordinate arithmetic is fp32 IN THE ORACLE'S ORDER - it is part of the operation's
    definition (sampling at x + flow directly differs by up to 5e-4 at 720p) and every step is one IEEE operation, reproduced here by
    _r32 - and the blend of the four taps is float64.  frame2 [B, C, H, W] stays where it is; b, y, x, flow_x, flow_y are [N] tensors
    on its device.  Returns (ref [N, C], bound [N, C]) with bound = WARP_ROUNDINGS * 2^-24 * sum |tap| |weight|: the taps are exact
    fp32 numbers, the weights s * e, ... are rounded once each in both, so the kernel's fp32 blend differs from this one by its own
    four products and three adds only."""
    B, C, H, W = frame2.shape
    one, two = 1.0, 2.0
    wden, hden = float(max(W - 1, 1)), float(max(H - 1, 1))
    vx, vy = _r32(x.double() + flow_x.double()), _r32(y.double() + flow_y.double())
    gx, gy = _r32(_r32(two * vx / wden) - one), _r32(_r32(two * vy / hden) - one)          # (2 v is exact)
    ix = _r32(_r32(_r32(gx + one) / two) * float(W - 1))
    iy = _r32(_r32(_r32(gy + one) / two) * float(H - 1))
    xw, yn = torch.floor(ix), torch.floor(iy)
    w, n = ix - xw, iy - yn                                                                  # exact differences
    e, s = _r32(one - w), _r32(one - n)
    flat = frame2.reshape(-1)
    plane = H * W
    ref = torch.zeros(b.numel(), C, dtype=torch.float64, device=frame2.device)
    mag = torch.zeros_like(ref)
    ch = torch.arange(C, device=frame2.device)
    for yy, xx, wt in ((yn, xw, _r32(s * e)), (yn, xw + 1, _r32(s * w)), (yn + 1, xw, _r32(n * e)), (yn + 1, xw + 1, _r32(n * w))):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (b[:, None] * C + ch[None]) * plane + (yy.clamp(0, H - 1).long() * W + xx.clamp(0, W - 1).long())[:, None]
        tap = flat[idx].double() * (wt * ok)[:, None]
        ref += tap
        mag += tap.abs()
    return ref, WARP_ROUNDINGS * 2.0 ** -24 * mag
