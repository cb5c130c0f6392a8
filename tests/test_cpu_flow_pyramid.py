"""The dispatch rules of the pyramids' two resizes are safe (flow_kernels.hip: resize_linear_f32_tiled, resize_cubic_f32c2_tiled), without
a GPU: the launcher's own answer, asked through the report-only mode of the test taps (include/s360_debug_flow_pyramid.h) of the
emulated library, against the box / window the tiled kernels form, restated in numpy from resize_coord's definition
(tests/flow_pyramid_cases.py: linear_box, cubic_window). The kernels trust the launcher: a shape it admits whose box does not fit
76 x 20 floats (72 x 24 for the cubic window) would write beyond the kernel's LDS arrays. Nothing is launched here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_pyramid_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 320  # source and destination sizes 1 .. N on the swept axis


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so"])
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    lib.s360_debug_resize_linear_f32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.s360_debug_resize_cubic_flow.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    return lib


def _linear(lib, sw, sh, dw, dh, cn=1):
    t = C.c_int(-1)
    assert lib.s360_debug_resize_linear_f32(None, None, sw, sh, cn, 1, dw, dh, 1.0, 0, None, C.byref(t)) == 0
    assert t.value in (0, 1)
    return bool(t.value)


def _cubic(lib, sw, sh, dw, dh, table=0):
    t = C.c_int(-1)
    assert lib.s360_debug_resize_cubic_flow(None, None, sw, sh, 1, dw, dh, 1.0, table, None, C.byref(t)) == 0
    assert t.value in (0, 1)
    return bool(t.value)


@pytest.mark.parametrize("axis", ["x", "y"])
def test_every_shape_the_linear_rule_admits_fits_the_box(emu, axis):
    """All source and destination sizes 1 .. 320 on one axis, the other fixed at a fitting 18 -> 16: wherever the launcher answers
    "tiled", every tile's box — first tap of the first column / row to last tap of the last, the kernel's clamps, on x the rounding
    to 16-byte pieces — fits. No shape is skipped; the count of admitted shapes is asserted so that an empty sweep cannot pass."""
    cap = S.RL_BW if axis == "x" else S.RL_BH
    admitted, largest, misfits = 0, 0, []
    for sn in range(1, N + 1):
        for dn in range(1, N + 1):
            tiled = _linear(emu, sn, 18, dn, 16) if axis == "x" else _linear(emu, 18, sn, 16, dn)
            if not tiled:
                continue
            admitted += 1
            extent = max(b[1] for b in S.linear_box(sn, dn, axis))
            largest = max(largest, extent)
            if extent > cap:
                misfits.append((sn, dn, extent))
    assert not misfits, "%d shapes admitted whose box does not fit %d: %s" % (len(misfits), cap, misfits[:10])
    assert admitted > 40000 and largest == cap, (admitted, largest)   # the rule is exercised up to the full box
    assert not _linear(emu, 18, 18, 16, 16, cn=2)                     # two channels never go tiled


@pytest.mark.parametrize("axis", ["x", "y"])
def test_every_shape_the_cubic_rule_admits_fits_the_window(emu, axis):
    """The same sweep for the flow upscale: "ratios <= 1" must imply a window of at most 72 x 24; a downscale on the swept axis with an
    upscale on the other must not go tiled, and neither may anything through the pointer table."""
    cap = S.UC_SW if axis == "x" else S.UC_SH
    admitted, largest, misfits = 0, 0, []
    for sn in range(1, N + 1):
        for dn in range(1, N + 1):
            tiled = _cubic(emu, sn, 16, dn, 16) if axis == "x" else _cubic(emu, 16, sn, 16, dn)
            assert tiled == (sn <= dn), (sn, dn)
            if not tiled:
                continue
            admitted += 1
            extent = max(e for _, e in S.cubic_window(sn, dn, axis))
            largest = max(largest, extent)
            if extent > cap:
                misfits.append((sn, dn, extent))
    assert not misfits, "%d shapes admitted whose window does not fit %d: %s" % (len(misfits), cap, misfits[:10])
    assert admitted == N * (N + 1) // 2 and largest <= cap, (admitted, largest)
    assert not _cubic(emu, 16, 16, 32, 32, table=1) and _cubic(emu, 16, 16, 32, 32)


def test_the_dispatch_literals_of_the_gpu_cases(emu):
    """tests/flow_pyramid_cases.py's expected kernels are what the launcher answers (the GPU tests assert the same on *tiled)."""
    for sw, sh, dw, dh, tiled, why in S.LINEAR_DISPATCH + S.LINEAR_SHAPES:
        assert _linear(emu, sw, sh, dw, dh) == tiled, (sw, sh, dw, dh, why)
    for sw, sh, dw, dh, _ in S.CUBIC_TILED:
        assert _cubic(emu, sw, sh, dw, dh)
    for sw, sh, dw, dh, _ in S.CUBIC_GENERIC:
        assert not _cubic(emu, sw, sh, dw, dh)


def test_no_pyramid_level_leaves_the_tiled_kernels(emu, oracle):
    """Every x0.9 step from 25 to 3000 pixels passes the linear rule and, upwards, the cubic one: the generic one-channel linear kernel
    and the generic cubic kernel without a table run in no flow of the product — only the GPU tests of this part launch them."""
    for n in range(25, 3001):
        m = int(np.float32(n) * np.float32(0.9) + np.float32(0.5))
        if m <= 24:
            continue
        assert _linear(emu, n, n, m, m) and _cubic(emu, m, m, n, n), n
        assert max(e for _, e in S.cubic_window(m, n, "x")) <= S.TW, n   # ... and the cubic window's columns beyond 64 are never needed
