"""tests/test_gpu_final_flow.py without a GPU: the same cases on tools/libflow_emu.so, the flow sources compiled for the CPU with
the kernels run wave by wave (tools/flow_emulate.cpp: emu_upscale_blur, emu_upscale_blur_generic)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import final_flow_cases as S
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libflow_emu.so"])
    lib = C.CDLL(os.path.join(ROOT, "tools", "libflow_emu.so"))
    for f in (lib.emu_upscale_blur, lib.emu_upscale_blur_generic):
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    O.lib()
    return lib


def _run(lib):
    def run(f, dw, dh, post, generic):
        f = np.ascontiguousarray(f, np.float32)
        b, sh, sw = f.shape[:3]
        out = np.full((b, dh, dw, 2), 7.0, np.float32)
        took = (lib.emu_upscale_blur_generic if generic else lib.emu_upscale_blur)(f.ctypes.data_as(C.c_void_p), sw, sh, b, dw, dh, post,
                                                                                  out.ctypes.data_as(C.c_void_p))
        assert took in (0, 1)
        return out, bool(took)
    return run


@pytest.mark.parametrize("w,h,src,tiled,why", S.SHAPES, ids=S.IDS)
def test_final_flow_shape(emu, w, h, src, tiled, why):
    S.check_shape(_run(emu), O, w, h, src, tiled)
