"""CPU side of the adaptive per-block pack route (include/emavfi.h, emavfi_forward_adaptive; EMA_VFI.pack_adapt): the exported entries,
the argument refusals that need no device, the adaptive launch list, the pack_adapt values and the routed kernel's code objects."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from emavfi import lib, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1   # include/emavfi.h
NEW = ("emavfi_route_state_bytes", "emavfi_route_state_init", "emavfi_forward_adaptive", "emavfi_forward_launches_adaptive")


def test_new_symbols_are_exported_and_declared():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "emavfi.h")).read()
    for name in NEW:
        assert name in lib.SYMBOLS and hasattr(L, name) and re.search(rf"\b{name}\(", hdr), name
    assert 0 < L.emavfi_route_state_bytes() <= 256
    assert L.emavfi_route_state_bytes() % 16 == 0


def _adaptive(state, enter, leave, num_blocks=3):
    L = lib.load()
    return L.emavfi_forward_adaptive(3, 64, num_blocks, None, 0, None, None, None, None, 0, 1, 32, 32, lib.BF16, None, None, None, 0,
                                     state, enter, leave, None)


@pytest.mark.parametrize("enter,leave", [(0.5, 0.5), (0.6, 0.7), (1.5, 0.2), (0.75, -0.1), (float("nan"), 0.1), (0.5, float("nan"))])
def test_bad_thresholds_are_argument_errors(enter, leave):
    assert _adaptive(None, enter, leave) == E_ARG
    assert "thresholds" in lib.last_error()


def test_null_or_foreign_state_is_an_argument_error():
    assert _adaptive(None, 0.75, 0.65) == E_ARG
    assert "null route state" in lib.last_error()
    fake = (ctypes.c_uint * 64)()   # never written by emavfi_route_state_init
    assert _adaptive(ctypes.addressof(fake), 0.75, 0.65) == E_ARG
    assert "magic" in lib.last_error()


def test_state_init_refusals():
    L = lib.load()
    buf = (ctypes.c_uint * 80)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    assert L.emavfi_route_state_init(None, 3, 0, None) == E_ARG and "null" in lib.last_error()
    assert L.emavfi_route_state_init(a16 + 4, 3, 0, None) == E_ARG and "aligned" in lib.last_error()
    for nb in (0, 9):
        assert L.emavfi_route_state_init(a16, nb, 0, None) == E_ARG and "num_blocks" in lib.last_error()
    for mask in (8, 1 << 31):
        assert L.emavfi_route_state_init(a16, 3, mask, None) == E_ARG and "start_gather_mask" in lib.last_error()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 256, 448), (1, 37, 53)])
def test_adaptive_launch_list_names_the_routed_pack_and_one_selector(dtype, shape):
    plain = lib.forward_launches(3, 64, 3, *shape, dtype)
    adapt = lib.forward_launches(3, 64, 3, *shape, dtype, adaptive=True)
    packs = [i for i, (n, _, _) in enumerate(plain) if "offset_conv+dcn_v2" in n]
    assert len(packs) == 3
    sel = [i for i, (n, _, _) in enumerate(adapt) if n == "route_select"]
    assert len(sel) == 1 and len(adapt) == len(plain) + 1
    # the selector right behind the last attention block; everything else as in the plain forward
    assert sel[0] == packs[-1] + 1
    rest = adapt[:sel[0]] + adapt[sel[0] + 1:]
    for i, (p, a) in enumerate(zip(plain, rest)):
        if i in packs:
            assert a[0].startswith("deform_routed<") and a[0].endswith("offset_conv+dcn_v2"), a
            assert a[1:] == p[1:]
        else:
            assert a == p


@pytest.mark.parametrize("dtype", ["fp32", "amp16", "fp32x3"])
def test_adaptive_launch_list_is_the_plain_one_without_a_one_launch_pack(dtype):
    assert lib.forward_launches(3, 64, 3, 2, 256, 448, dtype, adaptive=True) == lib.forward_launches(3, 64, 3, 2, 256, 448, dtype)
    # other widths have no one-launch pack either
    assert lib.forward_launches(3, 32, 2, 1, 64, 64, "bf16", adaptive=True) == lib.forward_launches(3, 32, 2, 1, 64, 64, "bf16")


def test_adaptive_and_gather_mask_exclude_each_other():
    with pytest.raises(ValueError):
        lib.forward_launches(3, 64, 3, 1, 64, 64, "bf16", gather_blocks=1, adaptive=True)


def test_pack_adapt_values(monkeypatch):
    monkeypatch.delenv("EMAVFI_PACK_ADAPT", raising=False)
    m = model.EMA_VFI(compute_dtype="bf16")
    assert m.pack_adapt is None
    m.pack_adapt = (0.8, 0.5)
    assert m.pack_adapt == (0.8, 0.5)
    m.pack_adapt = [0.3, 0.0]
    assert m.pack_adapt == (0.3, 0.0)
    m.pack_adapt = None
    assert m.pack_adapt is None
    for bad in ((0.5, 0.5), (0.4, 0.6), (1.2, 0.5), (0.5, -0.1), (0.5,), "fast", 3, (float("nan"), 0.1)):
        with pytest.raises(ValueError):
            m.pack_adapt = bad
    assert m.pack_adapt is None
    for env, want in (("1", model.PACK_ADAPT_DEFAULT), ("0.9,0.4", (0.9, 0.4)), (" 0.7 , 0.2 ", (0.7, 0.2)), ("0", None), ("", None)):
        monkeypatch.setenv("EMAVFI_PACK_ADAPT", env)
        assert model.EMA_VFI(compute_dtype="bf16").pack_adapt == want, env
    for env in ("yes", "0.5,0.6", "0.5", "0.5,0.4,0.3", "a,b"):
        monkeypatch.setenv("EMAVFI_PACK_ADAPT", env)
        with pytest.raises(ValueError):
            model.EMA_VFI(compute_dtype="bf16")
    assert model.PACK_ADAPT_DEFAULT == (0.75, 0.65)


def test_auto_is_still_not_a_pack_policy():
    m = model.EMA_VFI(compute_dtype="bf16")
    assert "auto" not in model.PACK_POLICIES
    with pytest.raises(ValueError):
        m.pack_policy = "auto"


def test_pack_routes_needs_an_adaptive_forward():
    m = model.EMA_VFI(compute_dtype="bf16")
    with pytest.raises(RuntimeError):
        m.pack_routes()


def _resources(pattern):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), pattern], capture_output=True, text=True,
                         check=True).stdout
    return [line.split() for line in out.splitlines() if line.startswith("_Z")]


def test_routed_pack_code_objects():
    """Two routed instantiations, in the pack's family (deform_pack3_kernel<Route3<T>, true>); LDS within two workgroups per CU, at
    least two waves per SIMD.  Scratch: none for f16; the bf16 one holds one census flag (4 bytes per lane, written once, read only
    by waves that had a sample beyond the window) in scratch - the gather body alone already uses all 256 VGPRs."""
    rows = _resources("Route3")
    names = sorted(r[0] for r in rows)
    assert len(rows) == 2 and all(re.match(r"_Z19deform_pack3_kernelI6Route3I", n) for n in names), names
    for r in rows:
        vgpr, agpr, sgpr, lds, scratch, spill, waves = (int(v) for v in r[-7:])
        assert vgpr + agpr <= 256 and waves >= 2, r
        if "DF16_" in r[0]:
            assert scratch == 0 and spill == 0, r
        else:
            assert scratch <= 8 and spill <= 1, r
    src = open(os.path.join(ROOT, "video-frame-interpolation_amd", "csrc", "deform_route3.inl")).read()
    assert "C::LDS_BYTES" in src and "__launch_bounds__(256, 2)" in src
    assert 2 * 81312 <= 160 * 1024


def test_route_select_has_no_lds_dma():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import code_objects, LLVM
    import tempfile
    so = os.path.join(ROOT, "video-frame-interpolation_amd", "emavfi", "lib", "libemavfi.so")
    found = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so, tmp):
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
            for name, body in re.findall(r"<(\w+)>:\n(.*?)(?=\n\n|\Z)", dis, re.S):
                if "route_select" in name and "s_endpgm" in body:
                    found += 1
                    assert "global_load_lds" not in body and not re.search(r"buffer_load\w*[^\n]* lds", body), name
    assert found >= 1
