"""Cases shared by the convolution gates (plain module, no fixtures): the tile-remainder shapes and the layout switches of
tests/test_gpu_conv_rounding_model.py, and what tests/test_rounding_model_cpu.py (the CPU as "kernel") and
tests/test_gpu_fp32x3_rounding_model.py (the HIP kernels) both run of the three-term f16 split mode - the same channel pairs, shapes,
scales and operands, so that what the CPU file shows about the gates' discriminating power holds for the cases the GPU file runs."""
import torch

from rounding_model import F16_MAX, conv_weights, scaled_input

ALL_SWITCHES = ("EMAVFI_CONV_MFMA16", "EMAVFI_CONV_RING", "EMAVFI_CONV_S2RING", "EMAVFI_CONV_WREG")
TILE_SHAPES = [(1, 1), (1, 70), (70, 1), (5, 7), (33, 47)]                                                           # tile remainders in both directions
S2_SHAPES = [(37, 53), (36, 52)]                                                                                     # odd and even sizes under stride 2


def set_env(monkeypatch, env):
    for name in ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


# (Cin, Cout, stride, planar tanh01 head): every channel pair the fp32x3 forward runs at mid_channels 64, and three of the narrow models
X3_PAIRS = [(6, 64, 1, False), (64, 64, 1, False), (64, 128, 2, False), (128, 256, 2, False), (256, 256, 1, False), (64, 2, 1, False), (67, 27, 1, False),
            (67, 64, 1, False), (64, 32, 1, False), (32, 3, 1, True), (8, 8, 1, False), (11, 27, 1, False), (16, 16, 1, False)]
X3_SCALES = (0, -10, 10)   # the whole input times 2^k, on top of scaled_input's per-channel 2^-3 .. 2^3


def x3_pair_id(pair):
    return f"{pair[0]}to{pair[1]}s{pair[2]}" + ("tanh01" if pair[3] else "")


def x3_shapes(stride):
    return TILE_SHAPES + (S2_SHAPES if stride == 2 else [])


def x3_act(pair, i):
    """`none` and `relu` alternate over a pair's shapes (1 x 1, whose few elements a ReLU could all clear, has none); the planar head is tanh01."""
    return "tanh01" if pair[3] else ("none", "relu")[i % 2]


def x3_layer(pair, H, W, k, B=2):
    """(x, w, b), all fp32: scaled_input times 2^k, conv_weights with the bias times 2^k as well (a bias of 0.1 beside an input of 1e-3
    would leave its own rounding as the only error to see).  At 2^10 the largest |x| is some 3e4, inside f16's range."""
    cin, cout = pair[:2]
    g = torch.Generator().manual_seed(cin * 131 + cout + 7 * H + W + 1000 * (k + 10))
    x = scaled_input(g, B, cin, H, W) * 2.0 ** k
    w, b = conv_weights(g, cout, cin)
    assert x.abs().max().item() < F16_MAX
    return x, w, b * 2.0 ** k


def split_sweep():
    """The deterministic operand sweep of the split's equality tests, fp32 [N]: every binade from 2^-30 to 2^15 at mantissas that are
    exact f16 numbers, half-way ties between two of them (even and odd side), just beside a tie, just below the next binade, and with
    all 24 bits set; values on both sides of 65504 / 2; the largest fp32 below 65504 and 65504 itself; +-0; every value with both
    signs.  Below 2^-3 every lo is subnormal, below 2^-14 hi is too, below 2^-25 both halves are zero."""
    frac = [0.0, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11, 2.0 ** -11 + 2.0 ** -23, 2.0 ** -11 - 2.0 ** -23, 0.5 + 2.0 ** -12, 0.7071067811865476,
            1 - 2.0 ** -10, 1 - 2.0 ** -12, 1 - 2.0 ** -23, 1023 * 2.0 ** -21]
    vals = [(1 + f) * 2.0 ** e for e in range(-30, 16) for f in frac]
    half = torch.tensor(F16_MAX / 2)
    top = torch.tensor(F16_MAX)
    vals += [half.item(), torch.nextafter(half, torch.tensor(0.0)).item(), torch.nextafter(half, top).item(), top.item(), torch.nextafter(top, torch.tensor(0.0)).item()]
    v = torch.tensor(vals, dtype=torch.float64).float()
    v = v[v.abs() <= F16_MAX]
    return torch.cat([v, -v, torch.tensor([0.0, -0.0])])
