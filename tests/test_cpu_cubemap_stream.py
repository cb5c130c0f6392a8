"""The cubemap of every frame (s360_set_cubemap_output, host/TestRenderStereoPanorama --output_cubemap_path in the stream modes)
without a GPU: tests/test_gpu_cubemap_stream.py in a process whose binding points at tools/libs360_emu.so, and the host cases
of tests/test_gpu_zz_cubemap_host.py on tools/emu/TestRenderStereoPanorama, against the same golden digests of the reference's
own program. What the emulation covers and what it cannot: tests/test_cpu_library_emulation.py."""
import os
import re
import subprocess
import sys

import pytest

import refprog
import test_gpu_zz_cubemap_host as H

ROOT = refprog.ROOT


@pytest.fixture(scope="module")
def emu_exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def test_header_binding_and_emulated_library_agree_on_the_cubemap_entry_points(emu_exe):
    """include/s360_cubemap.h (which include/s360.h includes) declares them, surround360_amd/_capi.py lists them, the emulated
    library exports them."""
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    hdr = strip(open(os.path.join(ROOT, "include", "s360_cubemap.h")).read())
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.CUBEMAP_SYMBOLS) and len(names) == 7
    assert not set(names) & set(_capi.SYMBOLS)
    assert '#include "s360_cubemap.h"' in strip(open(os.path.join(ROOT, "include", "s360.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in names:
        assert hasattr(lib, n), n


def test_header_binding_and_emulated_library_agree_on_the_cubemap_test_taps(emu_exe):
    """include/s360_debug_cubemap.h (NOT included by include/s360.h) declares them, surround360_amd/_capi.py lists them, the
    emulated library exports them."""
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    hdr = strip(open(os.path.join(ROOT, "include", "s360_debug_cubemap.h")).read())
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_CUBEMAP_SYMBOLS) and len(names) == 2
    assert not set(names) & (set(_capi.SYMBOLS) | set(_capi.CUBEMAP_SYMBOLS))
    assert "s360_debug_cubemap" not in strip(open(os.path.join(ROOT, "include", "s360.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in names:
        assert hasattr(lib, n), n


def test_library_cases_pass_on_the_emulated_library(emu_exe):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_cubemap_stream.py"), "-q", "-m",
                        "gpu and not fullsize", "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 17 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("device_png", [False, True], ids=["save_png", "device_png"])
def test_emulated_two_frames_as_a_stream(tmp_path, emu_exe, device_png):
    H.check_stream_cubemaps(emu_exe, tmp_path, "two_frames", ["--device_png"] if device_png else [])


def test_emulated_pole_removal_photo_as_a_stream(tmp_path, emu_exe):
    H.check_stream_cubemaps(emu_exe, tmp_path, "pole_removal")


def test_emulated_two_streams(tmp_path, emu_exe):
    H.check_two_streams_cubemaps(emu_exe, tmp_path)


def test_emulated_cubemap_path_without_placeholder(tmp_path, emu_exe):
    H.check_bad_command_line(emu_exe, tmp_path)
