"""RGBA and batched PNG encode (include/s360_state_png.h, host/TestRenderStereoPanorama --device_state_png) without a GPU:
tests/test_gpu_state_png.py in a process whose binding points at tools/libs360_emu.so, and the host cases of
tests/test_gpu_zz_state_png_host.py on tools/emu/TestRenderStereoPanorama, against the same golden digests of the reference's own
program. What the emulation covers and what it cannot: tests/test_cpu_library_emulation.py."""
import os
import re
import subprocess
import sys

import pytest

import refprog
import test_gpu_zz_state_png_host as H

ROOT = refprog.ROOT


@pytest.fixture(scope="module")
def emu_exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu_exe):
    """include/s360_state_png.h (which include/s360.h includes) declares them, surround360_amd/_capi.py lists them, the emulated
    library exports them."""
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    hdr = strip(open(os.path.join(ROOT, "include", "s360_state_png.h")).read())
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.STATE_PNG_SYMBOLS) and len(names) == 6
    assert not set(names) & set(_capi.SYMBOLS)
    assert '#include "s360_state_png.h"' in strip(open(os.path.join(ROOT, "include", "s360.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in names:
        assert hasattr(lib, n), n


def test_library_cases_pass_on_the_emulated_library(emu_exe):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_state_png.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 19 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("name", ["two_frames", "pole_removal"])
def test_emulated_chained_processes(tmp_path, emu_exe, name):
    H.check_chained_case(emu_exe, tmp_path, name, H.FLAG)


@pytest.mark.parametrize("mode", ["num_frames", "num_streams"])
def test_emulated_state_behind_a_streams_last_frame(tmp_path, emu_exe, mode):
    H.check_stream_state(emu_exe, tmp_path, ["--num_streams", "2"] if mode == "num_streams" else [])


def test_emulated_environment_switch(tmp_path, emu_exe):
    H.check_environment_switch(emu_exe, tmp_path)


def test_emulated_two_gpus_keep_the_state_on_its_owner_rank(tmp_path, emu_exe):
    """--num_gpus 2 on two emulated devices: every pair is encoded on the rank of its partition, every pole unit on its owner — a
    rank asked for an image it does not hold would refuse — and the files are the reference program's."""
    H.check_chained_case(emu_exe, tmp_path, "two_frames", H.FLAG + ["--num_gpus", "2"], env={"EMU_DEVICES": "2"})
