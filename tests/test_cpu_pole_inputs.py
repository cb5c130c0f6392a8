"""Pole removal on the device input paths, the pole masks resident per context (include/s360_pole_inputs.h), without a GPU: the entry
points in header, binding, libs360.so and the emulated library; tests/test_gpu_pole_inputs.py in processes whose binding points at
tools/libs360_emu.so (two lane orders); and the host cases of tests/test_gpu_zz_pole_inputs_host.py on the programs of tools/emu.
What the emulation covers and what it cannot: tests/test_cpu_library_emulation.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import pole_inputs_cases as PC

ROOT = PC.ROOT
GPU_CASES = 20  # the test cases of tests/test_gpu_pole_inputs.py


@pytest.fixture(scope="module")
def emu(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "Unpacker"), os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


@pytest.fixture
def emulated_encoder(emu, tmp_path):
    """B,G,R image -> the banded PNG file of the device encoder, on the emulated library (the binding of this process points at it
    for the duration of the test)."""
    from surround360_amd import _capi
    from surround360_amd import render as R
    saved = _capi.LIB_PATH, _capi._lib
    _capi.LIB_PATH, _capi._lib = os.path.join(ROOT, "tools", "libs360_emu.so"), None
    c = None
    try:
        c = R.Context(R.RigDescription(PC.small_rig(tmp_path)), R.make_params(**PC.FLAGS))
        yield lambda a: bytes(c.encode_png(a))
    finally:
        if c is not None:
            c.close()
        _capi.LIB_PATH, _capi._lib = saved


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_libraries_agree_on_the_entry_points(emu):
    from surround360_amd import _capi
    assert declared("s360_pole_inputs.h") == sorted(_capi.POLE_INPUTS_SYMBOLS) and len(_capi.POLE_INPUTS_SYMBOLS) == 2
    assert isinstance(_capi.POLE_INPUTS_SYMBOLS, tuple)
    others = set(_capi.SYMBOLS) | set(_capi.INPUT_PNG_SYMBOLS) | set(_capi.INPUT_JPEG_SYMBOLS) | set(_capi.DEBUG_IMAGES_SYMBOLS)
    assert not set(_capi.POLE_INPUTS_SYMBOLS) & others
    header = open(os.path.join(ROOT, "include", "s360_pole_inputs.h")).read()
    assert re.search(r"#define S360_CAMERA_BOTTOM2 \(-3\)", header) and _capi.S360_CAMERA_BOTTOM2 == -3 == PC.BOTTOM2
    from surround360_amd import render as R
    assert R.S360_CAMERA_BOTTOM2 == -3 and callable(R.Context.set_pole_masks) and callable(R.Context.upload_bottom2)
    s360 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360.h")).read(), flags=re.S)
    assert s360.rstrip().endswith("#endif") and '#include "s360_pole_inputs.h"' in s360[s360.index('#include "s360_cubemap.h"'):]
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for path in (os.path.join(ROOT, "surround360_amd", "libs360.so"), os.path.join(ROOT, "tools", "libs360_emu.so")):
        lib = C.CDLL(path)
        for n in _capi.POLE_INPUTS_SYMBOLS:
            assert hasattr(lib, n), (path, n)
    for n in _capi.POLE_INPUTS_SYMBOLS:
        assert "L.%s.argtypes" % n in src and "L.%s.restype" % n in src, n
    code = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "s360_pole_inputs.h")],
                          capture_output=True, text=True)
    assert code.returncode == 0, code.stderr


# ---- the GPU test file on the emulation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["fwd", "shuffle"])
def test_gpu_cases_pass_on_the_emulated_library(emu, order):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", EMU_LANE_ORDER=order)
    e.pop("S360_TEST_EMULATED_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_pole_inputs.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == GPU_CASES and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


# ---- the host program on the emulation ------------------------------------------------------------------------------------
def test_emulated_bin_list_with_pole_removal(tmp_path, emu):
    PC.check_bin_list_pole_removal(emu[0], emu[1], tmp_path)


def test_emulated_device_input_png(tmp_path, emu, emulated_encoder):
    PC.check_device_input_png(emu[1], tmp_path, emulated_encoder)


def test_emulated_device_input_jpeg(tmp_path, emu):
    PC.check_device_input_jpeg(emu[1], tmp_path)


def test_emulated_secondary_file_on_the_host_path(tmp_path, emu, emulated_encoder):
    PC.check_secondary_on_the_host_path(emu[1], tmp_path, emulated_encoder)
