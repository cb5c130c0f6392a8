"""16-bit PNG encode and the ISP's result as a finished file (include/s360_isp_png.h, host/Unpacker --device_png, host/Raw2Rgb
--device_png) without a GPU: tests/test_gpu_png16.py in a process whose binding points at tools/libs360_emu.so, and the program
cases of tests/test_gpu_zz_unpacker_png.py on tools/emu/*. What the emulation covers and what it cannot:
tests/test_cpu_library_emulation.py."""
import os
import re
import subprocess
import sys

import pytest

import refprog
import test_gpu_zz_unpacker_png as H

ROOT = refprog.ROOT


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu")


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu):
    """include/s360_isp_png.h (which include/s360.h includes) declares them, surround360_amd/_capi.py lists them with argtypes and
    restype, the emulated library exports them; the other lists are what they were."""
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    hdr = strip(open(os.path.join(ROOT, "include", "s360_isp_png.h")).read())
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.ISP_PNG_SYMBOLS) and len(names) == 5
    assert not set(names) & (set(_capi.SYMBOLS) | set(_capi.STATE_PNG_SYMBOLS) | set(_capi.CUBEMAP_SYMBOLS) | set(_capi.PNG_DECODE_SYMBOLS))
    assert '#include "s360_isp_png.h"' in strip(open(os.path.join(ROOT, "include", "s360.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in names:
        assert hasattr(lib, n), n
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in names:
        assert "L.%s.restype" % n in src and "L.%s.argtypes" % n in src, n


def test_library_cases_pass_on_the_emulated_library(emu):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    reader = "test_gpu_zz_unpacker_png.py::test_our_file_reader_reads_a_device_encoded_16_bit_file"  # (the one library case of that file)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_png16.py"), os.path.join(ROOT, "tests", reader),
                        "-q", "-m", "gpu", "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 33 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("bits,soft", [(12, False), (8, False), (12, True), (8, True)], ids=["12-pipe", "8-pipe", "12-soft_isp", "8-soft_isp"])
def test_emulated_unpacker_device_png(tmp_path, emu, bits, soft):
    H.check_unpacker_png(os.path.join(emu, "Unpacker"), tmp_path, bits, soft)


def test_emulated_unpacker_device_png_by_environment(tmp_path, emu):
    H.check_unpacker_png(os.path.join(emu, "Unpacker"), tmp_path, 12, False, by_environment=True)


def test_emulated_renderer_reads_an_imgs_dir_unpacked_on_the_device(tmp_path, emu):
    H.check_renderer_reads_device_pngs(os.path.join(emu, "Unpacker"), os.path.join(emu, "TestRenderStereoPanorama"), tmp_path)


@pytest.mark.parametrize("accelerate", [False, True], ids=["soft", "accelerate"])
@pytest.mark.parametrize("bpp", [8, 16])
def test_emulated_raw2rgb_device_png(tmp_path, emu, bpp, accelerate):
    H.check_raw2rgb_png(os.path.join(emu, "Raw2Rgb"), tmp_path, bpp, accelerate)
