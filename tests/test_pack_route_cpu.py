"""CPU side of the per-block pack route (include/emavfi.h, EMAVFI_ROUTE_*; emavfi_forward_launches_routed, EMA_VFI.pack_policy): the routed
launch list, its refusals, the policy values, and the code object of the window-free kernel."""
import os
import subprocess
import sys

import pytest

from emavfi import lib, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -2   # include/emavfi.h


def test_error_codes_are_the_header_ones():
    hdr = open(os.path.join(ROOT, "include", "emavfi.h")).read()
    assert f"#define EMAVFI_E_ARG ({E_ARG})" in hdr and f"#define EMAVFI_E_UNSUPPORTED ({E_UNSUPPORTED})" in hdr


def _routed(dtype, mask, B=2, H=256, W=448):
    L = lib.load()
    return L.emavfi_forward_launches_routed(3, 64, 3, B, H, W, lib.dtype_code(dtype), mask, None, 0, None, None, 0)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mask_zero_is_the_plain_launch_list(dtype):
    assert lib.forward_launches(3, 64, 3, 2, 256, 448, dtype, gather_blocks=0) == lib.forward_launches(3, 64, 3, 2, 256, 448, dtype)
    L = lib.load()
    assert _routed(dtype, 0) == L.emavfi_forward_launches(3, 64, 3, 2, 256, 448, lib.dtype_code(dtype), None, 0, None, None, 0)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mask", [1, 2, 4, 5, 7])
def test_masked_blocks_name_the_gather_kernel(dtype, mask):
    plain = lib.forward_launches(3, 64, 3, 2, 256, 448, dtype)
    routed = lib.forward_launches(3, 64, 3, 2, 256, 448, dtype, gather_blocks=mask)
    assert len(routed) == len(plain)
    packs = [i for i, (n, _, _) in enumerate(plain) if "offset_conv+dcn_v2" in n]
    assert len(packs) == 3
    for b, i in enumerate(packs):
        if (mask >> b) & 1:
            assert routed[i][0].startswith("deform_gather<") and routed[i][0].endswith("offset_conv+dcn_v2"), routed[i]
        else:
            assert routed[i] == plain[i]
    assert [r for i, r in enumerate(routed) if i not in packs] == [p for i, p in enumerate(plain) if i not in packs]


@pytest.mark.parametrize("dtype", ["fp32", "amp16", "fp32x3"])
def test_modes_without_a_one_launch_pack_refuse_the_gather_route(dtype):
    assert _routed(dtype, 0) > 0
    for mask in (1, 2, 4, 7):
        assert _routed(dtype, mask) == E_UNSUPPORTED
        assert "no gather route" in lib.last_error()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mask_bits_beyond_the_blocks_are_argument_errors(dtype):
    for mask in (8, 9, 1 << 31):
        assert _routed(dtype, mask) == E_ARG
        assert "num_blocks" in lib.last_error()


def test_pack_policy_values(monkeypatch):
    m = model.EMA_VFI(compute_dtype="bf16")
    assert m.pack_policy == "window"
    for v in model.PACK_POLICIES:
        m.pack_policy = v
        assert m.pack_policy == v
    for bad in ("fast", "auto"):   # (no census-driven policy: profiles/r07_gather_route_kill.md)
        with pytest.raises(ValueError):
            m.pack_policy = bad
    monkeypatch.setenv("EMAVFI_PACK_POLICY", "gather")
    assert model.EMA_VFI(compute_dtype="bf16").pack_policy == "gather"


def test_gather_kernel_code_object():
    """No scratch; LDS within what two workgroups per CU need (its launch bounds); pack3's layout constants unchanged."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "gather3_kernel"], capture_output=True, text=True,
                         check=True).stdout
    rows = [line.split() for line in out.splitlines() if "deform_gather3_kernel" in line]
    assert len(rows) == 2, out
    for r in rows:
        vgpr, agpr, sgpr, lds, scratch, spill, waves = (int(v) for v in r[-7:])
        assert scratch == 0 and spill == 0, r
        assert vgpr + agpr <= 256 and waves >= 2, r
    src = open(os.path.join(ROOT, "video-frame-interpolation_amd", "csrc", "deform_gather3.inl")).read()
    assert "LDS_BYTES = W3_OFF + W3_BYTES" in src and "__launch_bounds__(256, 2)" in src
    # 46 656 B window + 4 608 B table = 51 264 B dynamic LDS: two workgroups per CU fit in 160 KiB with room to spare
    assert 2 * (18 * 18 * 144 + 9 * 4 * 4 * 2 * 16) <= 160 * 1024
