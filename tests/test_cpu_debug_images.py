"""--save_debug_images and TestPoleRemoval without a GPU (include/s360_debug_images.h, include/s360_debug_views.h): the entry points in
headers, binding and emulated library; tests/test_gpu_debug_views.py and tests/test_gpu_debug_images.py in a process whose binding
points at tools/libs360_emu.so; the host programs' checks of tests/test_gpu_zz_debug_images_host.py on tools/emu/
TestRenderStereoPanorama and tools/emu/TestPoleRemoval; the tap's sizes on the sanitised emulation (tools/fuzz/debug_views_sweep, a
stand-alone program); and, where the reference's program has been built (oracle/_ref), the golden script's comparison again. What the
emulation covers and what it cannot: tests/test_cpu_library_emulation.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import debug_images_cases as D
import refprog
import test_gpu_zz_debug_images_host as ZH

ROOT = D.ROOT


@pytest.fixture(scope="module")
def emu(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text)))


def test_headers_binding_and_libraries_agree_on_the_entry_points(emu, s360lib):
    from surround360_amd import _capi, debug_images as DI
    assert declared("s360_debug_images.h") == sorted(_capi.DEBUG_IMAGES_SYMBOLS) and len(_capi.DEBUG_IMAGES_SYMBOLS) == 8
    assert declared("s360_debug_views.h") == sorted(_capi.DEBUG_VIEWS_SYMBOLS) == ["s360_debug_views"]
    s360 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360.h")).read(), flags=re.S)
    assert s360.rstrip().endswith('#include "s360_debug_images.h" \n#endif') and "s360_debug_views.h" not in s360
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in _capi.DEBUG_IMAGES_SYMBOLS + _capi.DEBUG_VIEWS_SYMBOLS:
        assert hasattr(lib, n) and hasattr(s360lib, n), n
        assert getattr(s360lib, n).argtypes is not None and getattr(s360lib, n).restype is not None, n
    for hdr in ("s360_debug_images.h", "s360_debug_views.h"):
        for cmd in (["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]):
            r = subprocess.run(cmd[:2] + ["-Wall", "-Werror", "-fsyntax-only"] + cmd[2:] + [os.path.join(ROOT, "include", hdr)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
    for name in ("set_debug_images", "debug_image_list", "get_debug_image", "encode_debug_pngs", "debug_png_bound", "download_debug_png",
                 "pole_removal_combine", "debug_views"):
        assert callable(getattr(DI, name)), name
    assert C.sizeof(_capi.DebugView) == 56  # s360_debug_view: two 64-bit offsets, ten 32-bit fields


def test_without_a_device_the_entry_points_fail_loudly(s360lib):
    """No context can exist without a HIP device; a NULL context is an argument error, never a crash or a silent success."""
    n = C.c_size_t(0)
    assert s360lib.s360_set_debug_images(None, 1) < 0 and s360lib.s360_frame_debug_image_count(None) < 0
    assert s360lib.s360_frame_encode_debug_pngs(None) < 0 and s360lib.s360_frame_debug_png_bound(None, 0) == 0
    assert s360lib.s360_frame_download_debug_png(None, 0, None, 0, C.byref(n)) < 0
    assert s360lib.s360_debug_views(None, 0, None, None, 0, None, 0) < 0
    assert s360lib.s360_pole_removal_combine(None, None, None, None, None, 8, 8, 1.0, 1.0, 0, 31, b"pixflow_low", None, None, None, None, None) < 0


def run_gpu_tests_on_the_emulation(files, order, expect):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", EMU_LANE_ORDER=order)
    e.pop("S360_TEST_EMULATED_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(ROOT, "tests", f) for f in files] + ["-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=1800, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == expect and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("order", ["fwd", "shuffle"])
def test_debug_views_on_the_emulated_library(emu, order):
    run_gpu_tests_on_the_emulation(["test_gpu_debug_views.py"], order, 3)


def test_library_tests_on_the_emulated_library(emu):
    run_gpu_tests_on_the_emulation(["test_gpu_debug_images.py"], "fwd", 7)


def test_debug_views_sizes_on_the_sanitised_emulation():
    """tools/fuzz/debug_views_sweep: every view of tests/debug_views_cases.py alone on heap blocks of exactly its bytes, then all in
    one call, AddressSanitizer + UndefinedBehaviorSanitizer on library and program (CPU only, a stand-alone program)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/libs360_asan.so", "fuzz/debug_views_sweep"])
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "debug_views_sweep"), os.path.join(ROOT, "tests", "golden", "rig_17cam.json")],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "all calls returned S360_OK" in r.stdout and "canaries intact" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name", list(D.CASES))
def test_emulated_program_writes_the_reference_programs_debug_images(tmp_path, emu, name):
    ZH.check_case(emu, tmp_path, name)


def test_emulated_program_device_png_batch(tmp_path, emu):
    ZH.check_device_batch(emu, tmp_path)


def test_emulated_program_stream_of_two_frames(tmp_path, emu):
    ZH.check_stream(emu, tmp_path)


def test_emulated_program_refuses_several_streams_or_gpus(tmp_path, emu):
    ZH.check_refused_with_streams(emu, tmp_path)


def test_emulated_program_missing_directory(tmp_path, emu):
    ZH.check_missing_directory_is_a_write_error(emu, tmp_path)


def test_emulated_pole_removal_program(tmp_path, emu):
    ZH.check_pole_removal_program(os.path.join(ROOT, "tools", "emu", "TestPoleRemoval"), tmp_path)


def test_golden_is_what_the_reference_program_writes():
    """Where oracle/_ref exists: the golden script's run of the reference's own program again, against the committed digests, with
    its two assertions (the flag changes nothing else; the pole-removal debug images are the state images of the same name)."""
    if not os.path.exists(refprog.REF_EXE):
        pytest.skip("oracle/_ref/TestRenderStereoPanorama not built (needs the reference's sources)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_debug_images_golden.py"), "--check"], capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0 and "up to date" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_golden_covers_what_the_issue_asks_of_it():
    g = D.golden()
    assert set(g) == set(D.CASES)
    odd = g["odd_490x245"]
    assert odd["000007/sphericalImg_offsetwrapL.png"]["shape"] == [105, 490, 4] and odd["000007/_topSpherical.png"]["shape"] == [125, 490, 4]
    assert odd["000007/eqr_sideL.png"]["shape"] == [245, 490, 3] and 490 // 3 == 163 and 490 * 4 % 16 and 490 * 3 % 16
    assert "000000/_eqr_sideL_sharpened.png" in g["sharpen_cubemap_search"] and not any("sharpened" in k or "top" in k for k in g["pole_removal"])
    assert {k.split("/")[0] for k in g["pole_removal"]} == {"000000", "000001"} and "000001/_bottomCombined.png" in g["pole_removal"]
