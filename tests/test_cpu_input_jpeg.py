"""Camera images as baseline JPEG files decoded on the device (include/s360_input_jpeg.h, host/TestRenderStereoPanorama
--device_input_jpeg) without a GPU: preconditions on the two byte oracles and on the case set, the entry points in header, binding
and emulated library, s360_input_jpeg_decodable on the CPU, tests/test_gpu_input_jpeg.py in processes whose binding points at
tools/libs360_emu.so (three lane orders, and once with a small subsequence length), tools/fuzz/jpeg_decode_sweep on the sanitised
emulation build (a stand-alone program; nothing is preloaded), and the host cases of tests/test_gpu_zz_input_jpeg_host.py on
tools/emu/TestRenderStereoPanorama. What the emulation covers and what it cannot: tests/test_cpu_library_emulation.py."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import input_jpeg_cases as IJ
import jpeg_cases as JC
import test_gpu_zz_input_jpeg_host as ZJ

ROOT = IJ.ROOT
NOT_MSG = b"not a JPEG file of this decoder"


# ---- preconditions on the oracles alone ----------------------------------------------------------------------------------
def test_host_decoder_is_pil_over_all_cases():
    """jpegio::decode_any equals PIL's Image.open(...).convert("RGB") for every PIL-written case, and for the host writer's files."""
    for (k, f), px in zip(IJ.pil_cases(), IJ.pil_case_pixels()):
        assert px.shape == (k[1], k[0], 3) and np.array_equal(px, IJ.pil_decode(f)), k
    cases = IJ.host_writer_cases()
    files = [JC.host_case(c)[0] for c in cases]
    for c, f, px in zip(cases, files, IJ.host_decode(files)):
        assert np.array_equal(px, IJ.pil_decode(f)), c


def test_cases_reach_the_hard_places():
    files = dict(IJ.pil_cases())
    scans = {k: IJ.scan_of(f)[1] for k, f in files.items()}
    assert any(b"\xff\x00" in s for s in scans.values())
    assert any(b"\xff\x00\xff\x00" in s for s in scans.values())  # two stuffed bytes in a row
    assert any(s.endswith(b"\xff\x00") for s in scans.values()) or any(
        IJ.scan_of(JC.host_case((w, h, "noise", 100, s))[0])[1].endswith(b"\xff\x00") for w, h, s in JC.LAST_FF)  # the last scan byte is 0xFF
    import test_gpu_input_jpeg as G
    G.constant_case()  # (asserts: a constant 4:2:0 image of at least 8 subsequences)
    # a scan longer than one synchronisation workgroup's share, and than one unstuffing workgroup's, by non-multiples
    share = IJ.SUB_BITS * IJ.SYNC_THREADS
    longest = max(IJ.unstuffed_bits(f) for f in files.values())
    assert longest > share and longest % share and (longest // 8) % IJ.UNSTUFF_SEG
    assert max(len(s) for s in scans.values()) > IJ.UNSTUFF_SEG
    assert any(k[5] for k in files) and any(not k[5] for k in files)  # optimised Huffman tables, and the standard ones
    assert any(k[0] % 16 in range(1, 9) and k[4] == 2 for k in files) and any(k[1] % 16 in range(1, 9) and k[4] == 2 for k in files)  # dummy luma column / row
    assert {k[4] for k in files} == {0, 1, 2} and {k[3] for k in files} == set(IJ.QUALITIES)
    src = open(os.path.join(ROOT, "surround360_amd", "csrc", "jpeg_decode.hpp")).read()
    assert "kJpegSubBits = %d;" % IJ.SUB_BITS in src and "kJpegSyncThreads = %d;" % IJ.SYNC_THREADS in src and "kJpegUnstuffSeg = %d;" % IJ.UNSTUFF_SEG in src


# ---- header, binding, emulated library ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu):
    import ctypes as C
    from surround360_amd import _capi
    assert declared("s360_input_jpeg.h") == sorted(_capi.INPUT_JPEG_SYMBOLS) and len(_capi.INPUT_JPEG_SYMBOLS) == 5
    assert declared("s360_debug_input_jpeg.h") == sorted(_capi.DEBUG_INPUT_JPEG_SYMBOLS) and len(_capi.DEBUG_INPUT_JPEG_SYMBOLS) == 1
    assert isinstance(_capi.INPUT_JPEG_SYMBOLS, tuple) and isinstance(_capi.DEBUG_INPUT_JPEG_SYMBOLS, tuple)
    assert not set(_capi.INPUT_JPEG_SYMBOLS) & (set(_capi.SYMBOLS) | set(_capi.JPEG_SYMBOLS) | set(_capi.INPUT_PNG_SYMBOLS))
    assert declared("s360_jpeg.h") == sorted(_capi.JPEG_SYMBOLS)  # (the encoder's header is what it was)
    s360 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360.h")).read(), flags=re.S)
    assert '#include "s360_input_jpeg.h"' in s360 and "s360_debug_input_jpeg.h" not in s360
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in _capi.INPUT_JPEG_SYMBOLS + _capi.DEBUG_INPUT_JPEG_SYMBOLS:
        assert hasattr(lib, n), n
        assert "L.%s.argtypes" % n in src and "L.%s.restype" % n in src, n
    for hdr in ("s360_input_jpeg.h", "s360_debug_input_jpeg.h"):
        code = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", hdr)], capture_output=True, text=True)
        assert code.returncode == 0, code.stderr
    for f in ("jpeg_decode.hip", "jpeg_decode.hpp", "api_jpeg_in.hip"):  # the library includes nothing from oracle/
        text = open(os.path.join(ROOT, "surround360_amd", "csrc", f)).read()
        assert not [ln for ln in text.splitlines() if ln.startswith("#include") and "oracle" in ln]


def pil_file(img, fmt="JPEG", **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, fmt, **kw)
    return b.getvalue()


def sof1_12bit(f):
    """A baseline file relabelled as a 12-bit extended-sequential one (SOF1, precision 12): not a valid image, but what a header
    parser sees of one."""
    at = f.index(b"\xff\xc0")
    return f[:at] + b"\xff\xc1" + f[at + 2:at + 4] + bytes([12]) + f[at + 5:]


def test_decodable_needs_no_device(emu):
    """s360_input_jpeg_decodable on the CPU: PIL's files of the three samplings, the host writer's and (the same bytes) the device
    encoder's; and what it refuses, each with the stated message."""
    from surround360_amd import _capi
    from surround360_amd import render as R
    saved = _capi.LIB_PATH, _capi._lib
    _capi.LIB_PATH, _capi._lib = os.path.join(ROOT, "tools", "libs360_emu.so"), None
    try:
        a = IJ.image(37, 53, "photo")
        for s, (hs, vs) in ((2, (2, 2)), (1, (2, 1)), (0, (1, 1))):
            for opt in (False, True):
                f = IJ.pil_encode(a, 95, s, opt)
                assert R.input_jpeg_decodable(f) == (37, 53, 3, hs, vs, len(IJ.scan_of(f)[1]))
        f = JC.host_case((33, 15, "noise", 95, 1))[0]  # (the device encoder writes this file byte for byte: tests/test_gpu_jpeg.py)
        assert R.input_jpeg_decodable(f) == (33, 15, 3, 2, 2, len(IJ.scan_of(f)[1]))
        rgb = np.ascontiguousarray(a[..., ::-1])
        good = IJ.pil_encode(a, 95, 2, False)
        ex = Image.Exif()
        ex[0x0112] = 6
        refused = {"progressive": pil_file(rgb, progressive=True), "greyscale": pil_file(rgb[..., 0]), "restart markers": pil_file(rgb, restart_marker_blocks=3),
                   "12-bit SOF1": sof1_12bit(good), "orientation 6": pil_file(rgb, exif=ex), "png": pil_file(rgb, "PNG"), "empty": b"", "SOI only": good[:2]}
        for cut in (3, 20, 100, 200, IJ.scan_of(good)[0] - 1):
            refused["truncated header %d" % cut] = good[:cut]
        for name, bad in refused.items():
            assert R.input_jpeg_decodable(bad) is None, name
            assert NOT_MSG in R.lib().s360_last_error(None), name
        ex[0x0112] = 1
        assert R.input_jpeg_decodable(pil_file(rgb, exif=ex)) is not None  # orientation 1 is fine
    finally:
        _capi.LIB_PATH, _capi._lib = saved


# ---- the GPU test file on the emulation ----------------------------------------------------------------------------------
def replay(order, sub_bits=None):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1", EMU_LANE_ORDER=order)
    e.pop("S360_TEST_EMULATED_LIB_PATH", None)
    e.pop("S360_JPEG_SUB_BITS", None)
    if sub_bits:
        e["S360_JPEG_SUB_BITS"] = str(sub_bits)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_input_jpeg.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == 8 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("order", ["fwd", "rev", "shuffle"])
def test_gpu_cases_pass_on_the_emulated_library(emu, order):
    replay(order)


def test_gpu_cases_pass_with_short_subsequences(emu):
    """The library's developer switch S360_JPEG_SUB_BITS=640: every file of a few hundred bytes spans several subsequences, the larger
    ones many workgroups and launches — the propagation paths carry far more of the cases than at the default length."""
    replay("shuffle", 640)


# ---- the stand-alone sweep under sanitizers -------------------------------------------------------------------------------
def test_sweep_and_damaged_files_on_the_sanitised_library(tmp_path):
    """tools/fuzz/jpeg_decode_sweep: sizes 1..40 x 1..40 and the case sizes at the three samplings, and damaged copies (scan bytes
    changed, the scan cut at every byte of a small file, DHT bytes changed) through s360_decode_input_jpeg_batch of the emulated
    library under AddressSanitizer and UndefinedBehaviorSanitizer, against jpegio::decode_any."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/libs360_asan.so", "fuzz/jpeg_decode_sweep"])
    d = tmp_path / "cases"
    d.mkdir()
    n = 0
    for w in range(1, 41):
        for h in range(1, 41):
            a = IJ.image(w, h, ("noise", "ramps", "photo")[(w + h) % 3], seed=w * 41 + h)
            for s in IJ.SAMPLINGS:
                (d / ("base_%02d_%02d_%d.jpg" % (w, h, s))).write_bytes(IJ.pil_encode(a, IJ.QUALITIES[(w + 2 * h + s) % 4], s, bool((w ^ h) & 1)))
                n += 1
    for (w, h) in IJ.SIZES[6:]:
        for s in IJ.SAMPLINGS:
            (d / ("base_big_%d_%d_%d.jpg" % (w, h, s))).write_bytes(IJ.pil_encode(IJ.image(w, h, "noise" if w < 1000 else "photo"), 95, s, False))
            n += 1
    for i, (w, h, kind, s, opt) in enumerate([(16, 8, "noise", 2, False), (33, 17, "photo", 2, True), (24, 24, "noise", 0, False), (40, 9, "ramps", 1, True)]):
        (d / ("mut_%d.jpg" % i)).write_bytes(IJ.pil_encode(IJ.image(w, h, kind), 90, s, opt))
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "jpeg_decode_sweep"), os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(d)],
                       capture_output=True, text=True, timeout=3000)
    print(r.stdout[-600:])
    assert r.returncode == 0 and not r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    m = re.search(r"(\d+) undamaged files, (\d+) accepted; (\d+) damaged files, (\d+) accepted, (\d+) refused; 0 violations", r.stdout)
    assert m and int(m.group(1)) == n == int(m.group(2)) and int(m.group(3)) >= 4 * 64 + 50 and int(m.group(5)) > 100, r.stdout[-600:]


# ---- the host program on the emulation ------------------------------------------------------------------------------------
def test_emulated_single_frame(tmp_path, emu):
    ZJ.check_single_frame(emu, tmp_path)


def test_emulated_fallback_is_per_file(tmp_path, emu):
    ZJ.check_fallback_per_file(emu, tmp_path)


def test_emulated_num_frames_2(tmp_path, emu):
    ZJ.check_stream(emu, tmp_path, [])


def test_emulated_num_streams_2(tmp_path, emu):
    ZJ.check_stream(emu, tmp_path, ["--num_streams", "2"])
