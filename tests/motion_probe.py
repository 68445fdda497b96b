"""motion_estimation made visible layer by layer (plain module, no fixtures; tests/test_motion_probe_cpu.py runs it with the CPU as
"kernel", tests/test_gpu_motion_layers.py on the HIP kernels).

The forward shows `feat`, `ctx` and `flow`; motion_estimation.0's output a0 and .1's output a1 exist only between launches (or, with the
fused head, only in LDS).  Exact pass-through weights bring them out through the `flow` tap:
  * motion_estimation.1.0 := the centre-tap identity, zero bias.  a0 is post-ReLU and already rounded to the storage type, so the layer
    returns it bit for bit: products with 0 and 1 are exact, sums of one value and exact zeros are that value in any order, ReLU of a
    non-negative value and re-rounding a stored value are identities (1.0 is exact in bf16, f16 and as a [hi | lo] pair with lo = 0);
  * motion_estimation.2 := a selector, w[0, 2 k, 1, 1] = w[1, 2 k + 1, 1, 1] = 1, zero bias: the two flow planes are channels 2 k and
    2 k + 1 of its input.  mid / 2 forwards assemble all mid channels (assemble).
With the real .1 weights and the same moving selector the flow planes are a1's channels.

What a0 is compared with: the single-layer model of tests/rounding_model.py on the 2 mid-channel input cat(feat, ctx broadcast over the
image) - zero padded like any input, which is what the border classes of the folded context half restate (ctx_finish_kernel,
csrc/misc_kernels.hip: R[b][cls][o], cls = ym * 4 + xm; bit 0 of ym: row y - 1 exists, bit 1: row y + 1 exists, the same for xm and
columns).  The kernels take the feat half of the weight rounded to the storage type and the context half in fp32 (pack_ctx_kernel
copies it unrounded; the table is built with fp32 FMAs): model_w0.  The products of the context half round, so the layer is counted
with rounded products throughout (fp32_products: 2 n roundings, n = 9 * 2 mid + 1).

cpu_kernel restates the fold on the CPU - the fp32 table, the class map, the fp32 convolution of feat - with a hook where MUTATIONS
plant the errors a wrong class index or a wrong table would make.  The context half of the weight is taken as it is (no power-of-two
factor on w0[:, mid:]): the synthetic context is large enough for every mutation to leave the bound at the shares the CPU file asserts."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from rounding_model import conv_model, exact_match_share, storage_round

# (B, H, W): the smallest shapes at which the class index, the per-sample table and the strip seam can go wrong.  One pixel (class 0), one
# column (xm = 0), one row of two samples (ym = 0), two rows (no interior row), and interiors; the ring list's last three lie around the
# 62-column strip pitch of conv_ring.inl (one strip exactly, one column more, two strips, two strips and one column).
RING_SHAPES = [(1, 1, 1), (1, 33, 1), (2, 1, 7), (1, 2, 62), (1, 3, 63), (2, 17, 124), (1, 17, 125)]
OTHER_SHAPES = [(1, 1, 1), (1, 33, 1), (2, 1, 7), (1, 2, 5), (2, 5, 7)]


def selector_state_dict(sd, mid, k, keep_m1):
    """sd with motion_estimation.2 := the selector of channels (2 k, 2 k + 1) and, unless keep_m1, motion_estimation.1.0 := identity."""
    out = OrderedDict(sd)
    if not keep_m1:
        w1 = torch.zeros(mid, mid, 3, 3)
        w1[torch.arange(mid), torch.arange(mid), 1, 1] = 1.0
        out["motion_estimation.1.0.weight"], out["motion_estimation.1.0.bias"] = w1, torch.zeros(mid)
    w2 = torch.zeros(2, mid, 3, 3)
    w2[0, 2 * k, 1, 1] = w2[1, 2 * k + 1, 1, 1] = 1.0
    out["motion_estimation.2.weight"], out["motion_estimation.2.bias"] = w2, torch.zeros(2)
    return out


def assemble(run_forward, sd, mid, keep_m1, ks=None):
    """run_forward(state_dict) -> flow [B, 2, H, W] (fp32, CPU), once per selector position k in `ks` (default: all mid / 2).  Returns
    [B, mid, H, W]: channels (2 k, 2 k + 1) are the flow planes of position k; channels of positions not in `ks` are NaN."""
    out = None
    for k in (range(mid // 2) if ks is None else ks):
        flow = run_forward(selector_state_dict(sd, mid, k, keep_m1))
        if out is None:
            out = torch.full((flow.shape[0], mid) + tuple(flow.shape[2:]), float("nan"))
        out[:, 2 * k:2 * k + 2] = flow
    return out


def border_class(H, W):
    """[H, W] int64 map of ym * 4 + xm (ctx_finish_kernel's header comment)."""
    y, x = torch.arange(H), torch.arange(W)
    ym = (y >= 1).long() | ((y <= H - 2).long() << 1)
    xm = (x >= 1).long() | ((x <= W - 2).long() << 1)
    return ym.view(H, 1) * 4 + xm.view(1, W)


def class_taps():
    """[16, 3, 3] 0 / 1: the taps inside the image for each border class."""
    t = torch.ones(16, 3, 3)
    for cls in range(16):
        ym, xm = cls >> 2, cls & 3
        if not ym & 1:
            t[cls, 0, :] = 0
        if not ym & 2:
            t[cls, 2, :] = 0
        if not xm & 1:
            t[cls, :, 0] = 0
        if not xm & 2:
            t[cls, :, 2] = 0
    return t


def model_w0(w0, mid, dtype):
    """motion_estimation.0's weight as the kernels take it: the feat half rounded to the storage type, the context half fp32."""
    return torch.cat([storage_round(w0[:, :mid], dtype), w0[:, mid:]], dim=1)


def a0_model(feat, ctx, w0m, b0, store):
    """(ref, bound, d) of motion_estimation.0 as ONE 2 mid-channel layer on cat(feat, ctx broadcast), rounded products, ReLU, `store`."""
    B, mid, H, W = feat.shape
    x = torch.cat([feat, ctx.view(B, mid, 1, 1).expand(B, mid, H, W)], dim=1)
    return conv_model(x, w0m, b0, 1, "relu", store, fp32_products=True)


def gate_figures(got, ref, bound, d, store):
    """(err / bound per element, mismatch share, largest mismatch in units) - the three gates' figures (mismatches: 16-bit stores only)."""
    ratio = (got.double() - ref).abs() / bound
    share, units = exact_match_share(got, ref, store, d) if store != "fp32" else (0.0, 0.0)
    return ratio, share, units


def cpu_kernel(feat, ctx, w0m, b0, store, hook=None):
    """The fold restated in fp32: tsum[b][o][tap] = sum_c w9[o, mid + c, tap] ctx[b][c]; R[b][cls][o] = b9[o] + sum of tsum over the
    class's in-image taps; a0 = storage_round(relu(fp32 conv of feat with w0[:, :mid] + R[b][cls(y, x)])).
    hook(cls [B, H, W], taps [16, 3, 3], sample [B]) -> the same three, altered: the class every pixel takes, the taps every class
    counts, and the sample whose table every sample reads.  Returns (a0, touched [B, H, W]: pixels whose table row the hook changed)."""
    B, mid, H, W = feat.shape
    cls0 = border_class(H, W).unsqueeze(0).expand(B, H, W)
    taps0, sample0 = class_taps(), torch.arange(B)
    cls, taps, sample = (cls0, taps0, sample0) if hook is None else hook(cls0.clone(), taps0.clone(), sample0.clone())
    tsum = torch.einsum("ocyx,bc->boyx", w0m[:, mid:].float(), ctx.float())              # [B, mid, 3, 3]
    R = b0.float().view(1, 1, mid) + torch.einsum("kyx,boyx->bko", taps, tsum)              # [B, 16, mid]
    rows = R[sample][torch.arange(B).view(B, 1, 1), cls]                                     # [B, H, W, mid]
    v = F.conv2d(feat.float(), w0m[:, :mid].float(), None, padding=1) + rows.permute(0, 3, 1, 2)
    touched = (taps[cls] != taps0[cls0]).flatten(3).any(dim=3) | (sample != sample0).view(B, 1, 1)
    return storage_round(v.relu(), store), touched


def _ym_xm(cls):
    return cls >> 2, cls & 3


def _interior(cls, taps, sample):
    return torch.full_like(cls, 15), taps, sample


def _last_row_ym3(cls, taps, sample):
    cls[:, -1, :] = 12 + (cls[:, -1, :] & 3)
    return cls, taps, sample


def _last_col_xm3(cls, taps, sample):
    cls[:, :, -1] = (cls[:, :, -1] & 12) + 3
    return cls, taps, sample


def _corners_take_edge(cls, taps, sample):
    ym, xm = _ym_xm(cls)
    return torch.where((ym != 3) & (xm != 3), ym * 4 + 3, cls), taps, sample


def _xm_ym_exchanged(cls, taps, sample):
    ym, xm = _ym_xm(cls)
    return xm * 4 + ym, taps, sample


def _ym_bits_exchanged(cls, taps, sample):
    ym, xm = _ym_xm(cls)
    return (((ym & 1) << 1) | (ym >> 1)) * 4 + xm, taps, sample


def _sample0_table(cls, taps, sample):
    return cls, taps, torch.zeros_like(sample)


def _tap22_never(cls, taps, sample):
    taps[:, 2, 2] = 0
    return cls, taps, sample


MUTATIONS = OrderedDict([("interior class everywhere", _interior), ("last row takes ym = 3", _last_row_ym3), ("last column takes xm = 3", _last_col_xm3),
                         ("corners take their edge's class", _corners_take_edge), ("xm and ym exchanged", _xm_ym_exchanged),
                         ("the two bits of ym exchanged", _ym_bits_exchanged), ("sample 0's table for every sample", _sample0_table),
                         ("tap (2, 2) never counted", _tap22_never)])
