"""A reference of the backward warp (EMA_VFI.warp, ema_vfi.py:149-171 + ATen's grid_sampler_2d: bilinear, zeros, align_corners) that
holds a kernel PER ELEMENT, and the flow fields at which a warp kernel bends.  Plain numpy; knows nothing of the library
(tests/test_warp_model_cpu.py holds this module to ATen's CPU grid_sample, tests/test_gpu_warp_lattice.py gates the HIP kernels with it).

Coordinates: fp32, op by op, every operation one separately rounded np.float32 operation, in the reference's order -
    v = (float)x + f;  g = 2 * v / max(size - 1, 1) - 1;  i = ((g + 1) / 2) * (size - 1);  floor;  w = ix - xw, e = 1 - w
    (n, s likewise in y);  weights nw = s e, ne = s w, sw = n e, se = n w.
No multiply feeds an add, so a fused multiply-add cannot change a bit; a kernel with a correctly rounded division computes the SAME
bits.  Sampling at x + flow in float64 is not the reference (5e-4 apart at 720p).

Blend: float64.  ref = sum over the IN-RANGE corners of frame2[corner] * weight, mag = sum of |terms|.  A corner is in range iff
0 <= c <= size - 1 on the floats; an out-of-range corner contributes nothing WHATEVER the frame holds there (ATen skips it); an
in-range corner multiplies in IEEE arithmetic, a zero weight included (NaN * 0 = NaN, Inf * 0 = NaN: as ATen).  A non-finite ix or iy
(NaN / infinite flow, or one so large that 2 * v overflows) gives NaN in every channel.

Bound: the kernel forms four fp32 products and three fp32 additions, each rounded once (or fused: fewer roundings), so
|kernel - ref| <= ((1 + u)^4 - 1) * mag with u = 2^-24.  Nothing is tuned.  Where the bound is 0 - every dead sample, every zero
frame value - the result is exact.  A result stored in a 16-bit type adds the store's half unit as rounding_model._stored does."""
import numpy as np

f32 = np.float32
U32 = 2.0 ** -24
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}
REACH = 8                       # warp_tiled_kernel: the LDS window reaches 8 px past a 32 x 64 tile; beyond it a sample is gathered
CARRIER_BIAS = 16.0             # carrier planes hold flow + 16: non-negative quarters below 32 (bf16 and f16 numbers)
CONSTANTS = (1.0, 0.5, 7.75, 8.0, 8.25, 9.0, 15.75)
# the shapes of the CPU gate (model against ATen): 1-pixel axes, odd sizes, size - 1 a power of two, several tiles, a 720p-wide row
SHAPES = ((1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 17, 23), (1, 33, 64), (1, 50, 132), (1, 65, 68), (1, 40, 1280))


# ------------------------------------------------------------------------------------------------------------ the model
def taps32(flow, H, W):
    """(ix, iy, xw, yn, (nw, ne, sw, se)) of a flow [B,2,H,W]: every array fp32 [B,H,W], every operation one fp32 rounding."""
    flow = np.asarray(flow, dtype=f32)
    x = np.arange(W, dtype=f32)[None, None, :]
    y = np.arange(H, dtype=f32)[None, :, None]
    with np.errstate(all="ignore"):
        vx, vy = x + flow[:, 0], y + flow[:, 1]
        gx = f32(2) * vx / f32(max(W - 1, 1)) - f32(1)
        gy = f32(2) * vy / f32(max(H - 1, 1)) - f32(1)
        ix = ((gx + f32(1)) / f32(2)) * f32(W - 1)
        iy = ((gy + f32(1)) / f32(2)) * f32(H - 1)
        xw, yn = np.floor(ix), np.floor(iy)
        w = ix - xw
        e = f32(1) - w
        n = iy - yn
        s = f32(1) - n
        wts = (s * e, s * w, n * e, n * w)
    assert all(a.dtype == f32 for a in (ix, iy, xw, yn) + wts)
    return ix, iy, xw, yn, wts


def warp_model(f2, flow):
    """(ref, bound, copy) of warp(f2 [B,C,H,W], flow [B,2,H,W]): the float64 reference, the per-element worst case |kernel - ref| and
    the elements that are a COPY of one source pixel: one in-range corner of weight exactly 1, every other in-range corner of weight 0,
    all of them finite, so 1 * v + 0 * ... = v in any arithmetic - a kernel returns frame2's value bit for bit there."""
    f2 = np.asarray(f2, dtype=f32)
    B, C, H, W = f2.shape
    ix, iy, xw, yn, wts = taps32(flow, H, W)
    bad = ~(np.isfinite(ix) & np.isfinite(iy))
    ref, mag = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    ones, others = np.zeros((B, H, W), dtype=np.int64), np.ones((B, H, W), dtype=bool)
    bi = np.arange(B)[:, None, None]
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), wts):
        with np.errstate(all="ignore"):
            cx, cy = xw + f32(dx), yn + f32(dy)
            ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1) & ~bad
        xi, yi = np.where(ok, cx, 0).astype(np.int64), np.where(ok, cy, 0).astype(np.int64)
        ones += ok & (wt == 1)
        others &= ~ok | (wt == 1) | (wt == 0)
        w64 = wt.astype(np.float64)
        for c in range(C):
            with np.errstate(all="ignore"):
                term = np.where(ok, f2[bi, c, yi, xi].astype(np.float64) * w64, 0.0)
            ref[:, c] += term
            mag[:, c] += np.abs(term)
    ref[np.broadcast_to(bad[:, None], ref.shape)] = np.nan
    bound = ((1 + U32) ** 4 - 1) * mag
    copy = np.broadcast_to(((ones == 1) & others)[:, None], ref.shape) & np.isfinite(ref)
    return ref, bound, copy


def stored(ref, bound, store):
    """The bound behind a store that rounds to nearest (rounding_model._stored restated): d + u (|ref| + d), and 2^-25 for the
    subnormal spacing of f16."""
    with np.errstate(all="ignore"):
        return bound + UNIT[store] * (np.abs(ref) + bound) + (2.0 ** -25 if store == "fp16" else 0.0)


def gate(got, ref, bound, copy=None, want_copy=None, label=""):
    """Hold `got` to the model, EVERY element: the NaN pattern equal; an infinite reference value met exactly; finite wherever the
    model is finite; exact where the bound is 0; within the bound elsewhere; on `copy` elements (warp_model) equal to `want_copy`
    (default: the reference, which is frame2's value there).  -> (failures, largest err / bound, elements)."""
    got = np.asarray(got).astype(np.float64)
    fails = []
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        fails.append(f"{label}: NaN pattern differs in {int((np.isnan(got) != np.isnan(ref)).sum())} elements")
    inf = np.isinf(ref)
    if not np.array_equal(got[inf], ref[inf]):
        fails.append(f"{label}: {int((got[inf] != ref[inf]).sum())} infinite reference values not met")
    fin = np.isfinite(ref)
    if not np.isfinite(got[fin]).all():
        fails.append(f"{label}: {int((~np.isfinite(got[fin])).sum())} non-finite results where the model is finite")
    exact = fin & (bound == 0)
    if not np.array_equal(got[exact], ref[exact]):
        fails.append(f"{label}: {int((got[exact] != ref[exact]).sum())} of {int(exact.sum())} zero-bound elements are not exact")
    live = fin & (bound > 0) & np.isfinite(got)
    ratio = float((np.abs(got[live] - ref[live]) / bound[live]).max()) if live.any() else 0.0
    if ratio > 1.0:
        fails.append(f"{label}: err / bound max {ratio:.3f}")
    if copy is not None and copy.any():
        want = ref if want_copy is None else np.asarray(want_copy).astype(np.float64)
        if not np.array_equal(got[copy], want[copy]):
            fails.append(f"{label}: {int((got[copy] != want[copy]).sum())} of {int(copy.sum())} copied pixels are not bit-exact")
    assert int((np.isnan(ref) | inf | fin).sum()) == ref.size          # excluded: 0
    return fails, ratio, ref.size


# ------------------------------------------------------------------------------------------------------------ the cases
def _grid(H, W):
    return np.arange(W, dtype=f32)[None, None, :], np.arange(H, dtype=f32)[None, :, None]


def edge_targets(size):
    """Where a sample bends: -1 (the last dead position), 0 and size - 1 (the border pixels), size, and steps of 2^-6 / a quarter beside."""
    e = 2.0 ** -6
    return (-1.0, -1.0 - e, -1.0 + e, -0.75, 0.0, size - 1.0, size - 1.0 - e, size - 1.0 + e, size - 0.75, float(size))


def _onto(B, H, W, tx, ty):
    """The flow that sends EVERY pixel onto (tx, ty); None leaves that axis still.  t - x and x + (t - x) are exact in fp32."""
    x, y = _grid(H, W)
    fl = np.zeros((B, 2, H, W), dtype=f32)
    if tx is not None:
        fl[:, 0] = f32(tx) - x
    if ty is not None:
        fl[:, 1] = f32(ty) - y
    return fl


def flow_cases(B, H, W, seed=0):
    """{name: flow [B,2,H,W]}: whole fields, finite.  Constants (+-8 is exactly the window's reach on a tile's first / last row and
    column, 8.25 and 9 the first samples that must be gathered) in x only, y only and both; every pixel onto one edge target in x,
    in y and at mixed corners; random quarters in +-12; a Gaussian flow of sigma 5."""
    rng = np.random.default_rng(1000 * H + W + seed)
    out = {"const 0": np.zeros((B, 2, H, W), dtype=f32)}
    for a in CONSTANTS:
        for d in (a, -a):
            for axes, name in (((0,), "x"), ((1,), "y"), ((0, 1), "xy")):
                fl = np.zeros((B, 2, H, W), dtype=f32)
                fl[:, list(axes)] = d
                out[f"const {name} {d:+g}"] = fl
    tx, ty = edge_targets(W), edge_targets(H)
    for i in range(len(tx)):
        out[f"x onto {tx[i]:g}"] = _onto(B, H, W, tx[i], None)
        out[f"y onto {ty[i]:g}"] = _onto(B, H, W, None, ty[i])
        out[f"corner {tx[i]:g}, {ty[i]:g}"] = _onto(B, H, W, tx[i], ty[i])
        j = (i + 3) % len(ty)
        out[f"corner {tx[i]:g}, {ty[j]:g}"] = _onto(B, H, W, tx[i], ty[j])
    out["random quarters"] = (rng.integers(-48, 49, size=(B, 2, H, W)) / 4).astype(f32)
    out["gaussian"] = (rng.standard_normal((B, 2, H, W)) * 5).astype(f32)
    return out


def nonfinite_flow_cases(B, H, W, seed=0):
    """Far, overflowing, infinite and NaN flows scattered over a quiet field (tests/test_gpu_parity.py places six of them by hand): a
    finite coordinate far outside samples zeros, a non-finite one gives NaN.  For the NCHW entry: a forward cannot carry them."""
    rng = np.random.default_rng(2000 * H + W + seed)
    values = np.array([1e9, -300.0, np.nan, np.inf, 3e38, -np.inf, -1e9, 1e30, -3e38, 300.0], dtype=f32)
    fl = (rng.integers(-8, 9, size=(B, 2, H, W)) / 4).astype(f32)
    pick = rng.integers(0, 4 * len(values), size=fl.shape)
    hit = pick < len(values)
    fl[hit] = values[pick[hit]]
    every = np.zeros((B, 2, H, W), dtype=f32)
    every.reshape(-1)[:] = values[np.arange(every.size) % len(values)]
    return {"scattered far / inf / nan": fl, "every pixel far / inf / nan": every}


def nonfinite_frame(f2):
    """frame2 with NaN at (0, 0), +Inf at (0, W - 1), -Inf at (H - 1, 0) and NaN at one interior pixel of every plane: (0, 0) is the
    clamped address of any far-outside sample, row 0 / column 0 that of a sample just past an edge."""
    f2 = np.array(f2, dtype=f32)
    H, W = f2.shape[2:]
    f2[:, :, H // 2, W // 2] = np.nan
    f2[:, :, H - 1, 0] = -np.inf
    f2[:, :, 0, W - 1] = np.inf
    f2[:, :, 0, 0] = np.nan
    return f2


def nonfinite_frame_flows(B, H, W):
    """The flows under which a non-finite frame shows whether out-of-range corners are SKIPPED: every corner dead (far outside, onto
    `size`, onto -1 - the clamped addresses are (0, 0), the last and the first row / column) and the identity."""
    return {"far outside": np.full((B, 2, H, W), 1e6, dtype=f32), "onto size": _onto(B, H, W, float(W), float(H)),
            "onto -1": _onto(B, H, W, -1.0, -1.0), "x onto -1": _onto(B, H, W, -1.0, None), "y onto size": _onto(B, H, W, None, float(H)),
            "const 0": np.zeros((B, 2, H, W), dtype=f32)}


def frame(B, C, H, W, seed=0):
    return np.random.default_rng(3000 * H + W + seed).standard_normal((B, C, H, W)).astype(f32)


# ------------------------------------------------------------------------------------------------------------ carriers
def carrier_flow_cases(B, H, W, seed=0):
    """{name: flow}: the fields a forward can carry - quarters in (-16, 16).  Constants on both axes (and +-8, +-8.25 on one); every
    pixel within reach of an edge onto that edge's target (-1, -0.75, 0 | size - 1, size - 0.75, size), the others random quarters;
    random quarters in +-12 and in +-15.75."""
    rng = np.random.default_rng(4000 * H + W + seed)
    lim = CARRIER_BIAS - 0.25
    out = {"const 0": np.zeros((B, 2, H, W), dtype=f32)}
    for a in CONSTANTS:
        for d in (a, -a):
            out[f"const xy {d:+g}"] = np.full((B, 2, H, W), d, dtype=f32)
    for d in (8.0, -8.0, 8.25, -8.25):
        for axis, name in ((0, "x"), (1, "y")):
            fl = np.zeros((B, 2, H, W), dtype=f32)
            fl[:, axis] = d
            out[f"const {name} {d:+g}"] = fl
    x, y = _grid(H, W)
    for lo, hi in ((-1.0, 0.0), (-0.75, -0.75), (0.0, -1.0)):
        fl = (rng.integers(-48, 49, size=(B, 2, H, W)) / 4).astype(f32)
        for axis, pos, size in ((0, x, W), (1, y, H)):
            near = np.broadcast_to(pos, (B, H, W)) < size / 2
            want = np.where(near, f32(lo) - pos, f32(size + hi) - pos).astype(f32)
            fl[:, axis] = np.where(np.abs(want) <= lim, want, fl[:, axis])
        out[f"edges {lo:g} | size{hi:+g}"] = fl
    out["random quarters 12"] = (rng.integers(-48, 49, size=(B, 2, H, W)) / 4).astype(f32)
    out["random quarters 15.75"] = (rng.integers(-63, 64, size=(B, 2, H, W)) / 4).astype(f32)
    return out


def carrier_state_dict(mid, seed=1):
    """Weights under which a forward computes a PRESCRIBED flow exactly: feat_ext_* and motion_estimation.* are zero except centre taps
    of 1.0 that carry frame1's channels 0 and 1 through feature channels 0 and 1 of every layer down to motion_estimation.2, whose bias
    is -16 (the context half of motion_estimation.0 is zero with the rest).  With frame1[:, :2] = flow + 16 (carrier_frames) every
    output of every layer has ONE non-zero product, 1.0 * a quarter below 32: exact in fp32, bf16 and f16, through every ReLU and every
    storage rounding.  context_encoding, the attention blocks and the reconstruction keep synth.synthetic_state_dict's weights."""
    import torch
    from emavfi import synth
    sd = synth.synthetic_state_dict(seed=seed, mid_channels=mid)
    layers = ["feat_ext_conv1.0"] + [k[:-len(".weight")] for k in sd if k.startswith("feat_ext_blocks.") and k.endswith(".weight")]
    layers += ["motion_estimation.0.0", "motion_estimation.1.0", "motion_estimation.2"]
    for name in layers:
        sd[name + ".weight"] = torch.zeros_like(sd[name + ".weight"])
        sd[name + ".bias"] = torch.zeros_like(sd[name + ".bias"])
        sd[name + ".weight"][0, 0, 1, 1] = 1.0
        sd[name + ".weight"][1, 1, 1, 1] = 1.0
    sd["motion_estimation.2.bias"][:] = -CARRIER_BIAS
    return sd


def carrier_frames(flow, seed=0):
    """(frame1, frame2) torch tensors [B,3,H,W] for carrier_state_dict: frame1's channels 0, 1 = flow + 16, frame2 a random image."""
    import torch
    flow = np.asarray(flow, dtype=f32)
    B, _, H, W = flow.shape
    plane = flow + f32(CARRIER_BIAS)
    assert (plane >= 0).all() and (plane < 2 * CARRIER_BIAS).all() and (plane * 4 == np.round(plane * 4)).all(), "quarters in (-16, 16) only"
    f1 = np.zeros((B, 3, H, W), dtype=f32)
    f1[:, :2] = plane
    return torch.from_numpy(f1), torch.from_numpy(frame(B, 3, H, W, seed + 7))
