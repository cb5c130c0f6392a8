"""The device JPEG encoder without a GPU: the preconditions of tests/jpeg_cases.py on the host writer's files alone, the entry
points of include/s360_jpeg.h and include/s360_debug_jpeg.h in header, binding and emulated library, tests/test_gpu_jpeg.py on the
CPU emulation of the HIP sources (tools/libs360_emu.so; what the emulation covers: tests/test_cpu_library_emulation.py) under three
lane orders — a missing S360_WAVE_SYNC() or barrier around an LDS hand-over shows as a byte mismatch there —, the size sweep of
tools/fuzz/jpeg_device_sweep on the sanitised emulated library, and the emulated program with and without --device_jpeg."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpeg_cases as JC
import test_gpu_jpeg as GJ

ROOT = JC.ROOT


# ---- preconditions, on the host writer's files alone --------------------------------------------------------------------
def test_host_writer_is_pil_over_all_cases():
    """The second oracle: PIL's save(quality=q, subsampling=2) writes the host writer's file, the whole file, for every case."""
    for case in JC.cases():
        assert JC.host_case(case)[0] == JC.pil_encode(JC.case_image(case), case[3]), case


def test_cases_reach_the_hard_places():
    """Stuffed bytes in every noise and checker case from 70 x 37 pixels up; two stuffed bytes in a row; all-EOB blocks of 6 and 4
    bits; a Y dummy column and a Y dummy row; a last byte that is 0xFF (padded, in one case at least); scans longer than the scan
    and stuffing kernels' per-workgroup share, by a non-multiple."""
    stuffed = {}
    for case in JC.cases():
        w, h, kind, q, _ = case
        scan = JC.scan_of(JC.host_case(case)[0])
        stuffed[case] = scan.count(b"\xff\x00")
        assert b"\xff" not in scan.replace(b"\xff\x00", b"")  # (no marker inside the scan)
        if w * h >= 70 * 37 and kind in ("noise", "checker1", "checker3"):
            assert stuffed[case] > 0, case
    print("stuffed bytes: 400 x 304 noise %d, checker1 %d" % (stuffed[(400, 304, "noise", 95, 1)], stuffed[(400, 304, "checker1", 95, 1)]))
    assert stuffed[(400, 304, "noise", 95, 1)] > 100 and stuffed[(400, 304, "checker1", 95, 1)] > 1000
    assert JC.scan_of(JC.host_case((64, 64, "checker3", 100, 1))[0]).count(b"\xff\x00\xff\x00") >= 1
    for w, h in JC.SIZES:  # a constant image: after the first MCU every block is DC difference 0 + EOB, 2 + 4 and 2 + 2 bits
        _, coef, bits = JC.host_case((w, h, "constant", 95, 1))
        assert not coef[:, 1:].any()
        tail = bits[6:].reshape(-1, 6)
        assert (tail[:, :4] == 6).all() and (tail[:, 4:] == 4).all()
    assert any(((w + 7) // 8) % 2 == 1 for w, h in JC.SIZES) and any(((h + 7) // 8) % 2 == 1 for w, h in JC.SIZES)  # Y dummy column / row
    assert any(((w + 7) // 8) % 2 == 1 and ((h + 7) // 8) % 2 == 0 for w, h in JC.SIZES)  # ... on one edge only
    assert any(((w + 7) // 8) % 2 == 0 and ((h + 7) // 8) % 2 == 1 for w, h in JC.SIZES)
    padded = 0
    for w, h, seed in JC.LAST_FF:
        f, _, bits = JC.host_case((w, h, "noise", 100, seed))
        assert f[-4:] == b"\xff\x00\xff\xd9", (w, h, seed)
        padded += int(bits.astype(np.int64).sum() % 8 != 0)
    assert padded >= 1
    assert any(JC.n_blocks(w, h) > JC.SCAN_ITEMS and JC.n_blocks(w, h) % JC.SCAN_ITEMS for w, h in JC.SIZES)
    for size in ((400, 304), (1030, 70)):
        bits = JC.host_case(size + ("noise", 95, 1))[2]
        nbytes = (int(bits.astype(np.int64).sum()) + 7) // 8
        assert nbytes > 2 * JC.STUFF_TILE and nbytes % JC.STUFF_TILE
    src = open(os.path.join(ROOT, "surround360_amd", "csrc", "jpeg.hpp")).read()
    assert "JPEG_SCAN_ITEMS = %d;" % JC.SCAN_ITEMS in src and "JPEG_STUFF_TILE = %d;" % JC.STUFF_TILE in src


# ---- the emulated library -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestHyperPreview")


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu_exe):
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for hdr, names in (("s360_jpeg.h", _capi.JPEG_SYMBOLS), ("s360_debug_jpeg.h", _capi.DEBUG_JPEG_SYMBOLS)):
        text = strip(open(os.path.join(ROOT, "include", hdr)).read())
        assert sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text))) == sorted(names)
        for n in names:
            assert hasattr(lib, n), n
        code = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", hdr)], capture_output=True, text=True)
        assert code.returncode == 0, code.stderr
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in _capi.JPEG_SYMBOLS + _capi.DEBUG_JPEG_SYMBOLS + ["s360_preview_set_jpeg", "s360_preview_jpeg_bound", "s360_preview_fetch_jpeg",
                                                            "s360_preview_last_jpeg_time"]:
        assert "L.%s.argtypes" % n in src and "L.%s.restype" % n in src, n


@pytest.mark.parametrize("order", ["fwd", "rev", "shuffle"])
def test_gpu_cases_pass_on_the_emulated_library(emu_exe, order):
    """tests/test_gpu_jpeg.py, the whole file, in a process whose binding points at the emulated library."""
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", EMU_LANE_ORDER=order)
    e.pop("S360_TEST_EMULATED_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_jpeg.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 7 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


def test_size_sweep_on_the_sanitised_library():
    """tools/fuzz/jpeg_device_sweep: every (w, h) of 1..34 x 1..34 and the larger sizes through s360_jpeg_encode of the emulated
    library under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded) against
    jpegio::encode, byte for byte."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/jpeg_device_sweep"])
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "jpeg_device_sweep")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and not r.stderr and "1177 files, 0 mismatches" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_emulated_program(tmp_path, emu_exe):
    GJ.check_program(emu_exe, tmp_path)
