"""A finished frame as a JPEG file encoded on the device (include/s360_frame_jpeg.h, host/TestRenderStereoPanorama --device_jpeg)
without a GPU: the entry points in header, binding and emulated library; tests/test_gpu_frame_jpeg.py — the cases of
tests/frame_jpeg_cases.py, all but the 8K one — in a process whose binding points at tools/libs360_emu.so, under two lane orders (a
missing barrier around an LDS hand-over shows as a byte mismatch there); and the host program's .jpg outputs, on the host threads
and on the emulated device, from tests/test_gpu_zz_frame_jpeg_host.py on tools/emu/TestRenderStereoPanorama. What the emulation
covers and what it cannot: tests/test_cpu_library_emulation.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import jpeg_cases as JC
import test_gpu_zz_frame_jpeg_host as ZF

ROOT = JC.ROOT


@pytest.fixture(scope="module")
def emu(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    JC.host_tool()
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_libraries_agree_on_the_entry_points(emu, s360lib):
    from surround360_amd import _capi
    assert declared("s360_frame_jpeg.h") == sorted(_capi.FRAME_JPEG_SYMBOLS) and len(_capi.FRAME_JPEG_SYMBOLS) == 7
    assert declared("s360_debug_frame_jpeg.h") == sorted(_capi.DEBUG_FRAME_JPEG_SYMBOLS) == ["s360_debug_frame_jpeg"]
    s360 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360.h")).read(), flags=re.S)
    assert '#include "s360_frame_jpeg.h"' in s360 and "s360_debug_frame_jpeg.h" not in s360
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in _capi.FRAME_JPEG_SYMBOLS + _capi.DEBUG_FRAME_JPEG_SYMBOLS:
        assert hasattr(lib, n) and hasattr(s360lib, n), n
        assert getattr(s360lib, n).argtypes is not None and getattr(s360lib, n).restype is not None, n
        assert '"%s"' % n in src
    for hdr in ("s360_frame_jpeg.h", "s360_debug_frame_jpeg.h"):
        code = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", hdr)], capture_output=True, text=True)
        assert code.returncode == 0, code.stderr
    from surround360_amd import render as R
    for name in ("set_jpeg_encode", "jpeg_bound", "cubemap_jpeg_bound", "download_jpeg", "download_jpeg_slot", "download_cubemap_jpeg",
                 "download_cubemap_jpeg_slot"):
        assert callable(getattr(R.Context, name)), name


def test_the_slot_capacity_is_the_one_the_tests_assume():
    import frame_jpeg_cases as FJ
    src = open(os.path.join(ROOT, "surround360_amd", "csrc", "jpeg.hpp")).read()
    assert "JPEG_FRAME_MCU_BYTES = 16 * 16 * 3;" in src and FJ.MCU_BYTES == 16 * 16 * 3 and "JPEG_HEADER_BYTES = %d;" % FJ.HEADER in src


@pytest.mark.parametrize("order", ["fwd", "shuffle"])
def test_gpu_cases_pass_on_the_emulated_library(emu, order):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", EMU_LANE_ORDER=order)
    e.pop("S360_TEST_EMULATED_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_frame_jpeg.py"), "-q", "-m", "gpu and not fullsize", "-p",
                        "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=1800, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 7 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


def test_emulated_program_one_frame(tmp_path, emu):
    """The .jpg host path (and the device path of the emulated library) of one frame against the oracle."""
    ZF.check_one_frame(emu, tmp_path)


def test_emulated_program_environment_switch(tmp_path, emu):
    ZF.check_environment_switch(emu, tmp_path)


def test_emulated_program_num_streams_2(tmp_path, emu):
    ZF.check_stream(emu, tmp_path, 4, ["--num_streams", "2"])
