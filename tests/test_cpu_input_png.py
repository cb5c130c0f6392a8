"""Camera images as banded PNG files decoded on the device (include/s360_input_png.h, host/TestRenderStereoPanorama
--device_input_png) without a GPU: tests/test_gpu_input_png.py in a process whose binding points at tools/libs360_emu.so, and the
host cases of tests/test_gpu_zz_input_png_host.py on tools/emu/Unpacker and tools/emu/TestRenderStereoPanorama. What the emulation
covers and what it cannot: tests/test_cpu_library_emulation.py."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import refprog
import test_gpu_png16 as P16
import test_gpu_png_decode as D
import test_gpu_zz_input_png_host as Z

ROOT = refprog.ROOT


@pytest.fixture(scope="module")
def emu(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "Unpacker"), os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu):
    """include/s360_input_png.h (which include/s360.h includes) declares them, surround360_amd/_capi.py lists them in a tuple of their
    own with argtypes and restype, the emulated library exports them; the other PNG headers' lists are what they were."""
    import ctypes as C
    from surround360_amd import _capi
    names = declared("s360_input_png.h")
    assert names == sorted(_capi.INPUT_PNG_SYMBOLS) and len(names) == 3
    assert isinstance(_capi.INPUT_PNG_SYMBOLS, tuple)
    others = set(_capi.SYMBOLS) | set(_capi.STATE_PNG_SYMBOLS) | set(_capi.CUBEMAP_SYMBOLS) | set(_capi.PNG_DECODE_SYMBOLS) | set(_capi.ISP_PNG_SYMBOLS)
    assert not set(names) & others
    assert declared("s360_png_decode.h") == sorted(_capi.PNG_DECODE_SYMBOLS) and len(_capi.PNG_DECODE_SYMBOLS) == 7
    assert declared("s360_isp_png.h") == sorted(_capi.ISP_PNG_SYMBOLS) and len(_capi.ISP_PNG_SYMBOLS) == 5
    assert declared("s360_state_png.h") == sorted(_capi.STATE_PNG_SYMBOLS) and len(_capi.STATE_PNG_SYMBOLS) == 6
    assert declared("s360_cubemap.h") == sorted(_capi.CUBEMAP_SYMBOLS) and len(_capi.CUBEMAP_SYMBOLS) == 7
    s360 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360.h")).read(), flags=re.S)
    for h in ("s360_input_png.h", "s360_png_decode.h", "s360_isp_png.h", "s360_state_png.h", "s360_cubemap.h"):
        assert '#include "%s"' % h in s360
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in names:
        assert hasattr(lib, n), n
        assert "L.%s.argtypes" % n in src and "L.%s.restype" % n in src, n


def test_decodable_needs_no_device(emu):
    """s360_input_png_decodable on the CPU: zlib-made banded files of both depths, and files it does not take; s360_png_decodable
    still refuses the 16-bit one."""
    import test_gpu_input_png as IP
    from surround360_amd import _capi
    from surround360_amd import render as R
    saved = _capi.LIB_PATH, _capi._lib
    _capi.LIB_PATH, _capi._lib = os.path.join(ROOT, "tools", "libs360_emu.so"), None
    try:
        a8, a16 = D.repeated_image(), IP.repeated16()
        f8, f16 = D.zlib_banded(a8, 5, 1, zlib.Z_RLE), IP.zlib_banded16(a16, 7, 1, zlib.Z_RLE)
        assert R.input_png_decodable(f8) == (93, 40, 4, 8, 5)
        assert R.input_png_decodable(f16) == (93, 40, 3, 16, 7)
        assert np.array_equal(P16.decode16(f16)[0], a16)
        assert R.png_decodable(f8) == (93, 40, 4, 5) and R.png_decodable(f16) is None
        for bad in (IP.with_ihdr(f16, ctype=6), IP.with_ihdr(f16, ctype=0), IP.with_ihdr(f16, interlace=1), D.pil_file(a8[..., [2, 1, 0, 3]]), b""):
            assert R.input_png_decodable(bad) is None
            assert b"not a banded PNG file of this decoder" in R.lib().s360_last_error(None)
    finally:
        _capi.LIB_PATH, _capi._lib = saved


def test_library_cases_pass_on_the_emulated_library(emu):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_input_png.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 31 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("depth", [16, 8])
def test_emulated_single_frame(tmp_path, emu, depth):
    Z.check_single_frame(emu[0], emu[1], tmp_path, depth)


def test_emulated_fallback_is_per_file(tmp_path, emu):
    Z.check_fallback_per_file(emu[0], emu[1], tmp_path)


def test_emulated_chained_processes(tmp_path, emu):
    Z.check_chained_processes(emu[0], emu[1], tmp_path)


def test_emulated_num_frames_3(tmp_path, emu):
    Z.check_stream(emu[0], emu[1], tmp_path, [])


def test_emulated_num_streams_2(tmp_path, emu):
    Z.check_stream(emu[0], emu[1], tmp_path, ["--num_streams", "2"], frames=4)


# ---- fuzz: corrupted and truncated 16-bit band data on the sanitised emulation build (a stand-alone program) -----------------
def zlib_says16(png):
    """What Python's zlib makes of a 16-bit banded file: its B,G,R uint16 pixels, or None if the container is not the banded one,
    a band does not inflate to exactly its rows, a filter type is not 0 or 1, or the Adler-32 differs."""
    import test_cpu_png_decode as CD
    ch = [c for c in CD.container(png) if c[0] != b"IEND"]
    if len(ch) < 5 or [t for t, _ in ch[:3]] != [b"IHDR", b"sbNd", b"IDAT"] or len(ch[-1][1]) != 4 or any(t != b"IDAT" for t, _ in ch[2:]):
        return None
    w, h = int.from_bytes(ch[0][1][:4], "big"), int.from_bytes(ch[0][1][4:8], "big")
    rows, line = int.from_bytes(ch[1][1], "big"), 1 + 6 * w
    if len(ch[3:-1]) != -(-h // rows):
        return None
    scan = b""
    for i, (_, data) in enumerate(ch[3:-1]):
        n = min(rows, h - i * rows) * line
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(data, n + 1)
        except zlib.error:
            return None
        if len(out) != n:
            return None
        scan += out
    if zlib.adler32(scan) != int.from_bytes(ch[-1][1], "big"):
        return None
    f = np.frombuffer(scan, np.uint8).reshape(h, line)
    if (f[:, 0] > 1).any():
        return None
    b = f[:, 1:].reshape(h, w, 6).astype(np.int64)
    b = np.where((f[:, 0] == 1)[:, None, None], np.cumsum(b, axis=1) & 255, b).astype(np.uint16)
    return np.ascontiguousarray(((b[..., 0::2] << 8) | b[..., 1::2])[..., ::-1])


def test_fuzz_of_16_bit_band_data_on_the_sanitised_emulation(tmp_path):
    """tools/fuzz/fuzz_png_decode calls s360_decode_input_png_batch on every 16-bit file with output buffers of exactly the image's
    size, for uint16 samples and for high bytes: every call returns, no sanitizer report, and what is accepted is what zlib gives."""
    import test_gpu_input_png as IP
    import test_gpu_png as T
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/libs360_asan.so", "fuzz/fuzz_png_decode"])
    rng = np.random.default_rng(2025)
    a = np.repeat(rng.integers(0, 65536, (17, 8, 3), dtype=np.uint16), 3, axis=1)  # 17 x 24
    s = P16.smooth16(17, 33, rng, 3.0)
    bases = [IP.zlib_banded16(a, 5, 1, zlib.Z_RLE), IP.zlib_banded16(a, 6, 9, zlib.Z_DEFAULT_STRATEGY), IP.zlib_banded16(a, 5, 0, zlib.Z_DEFAULT_STRATEGY),
             IP.zlib_banded16(s, 7, 6, zlib.Z_DEFAULT_STRATEGY, pieces=2), IP.zlib_banded16(s, 3, 1, zlib.Z_RLE, ftype=0),
             IP.zlib_banded16(s, 17, 6, zlib.Z_HUFFMAN_ONLY)]
    files = {"base_%02d.png" % k: b for k, b in enumerate(bases)}
    for k in range(120):  # one byte replaced or one bit flipped inside a band's data, or a band cut short
        ch = T.chunks(bases[k % len(bases)])
        bi = 3 + int(rng.integers(0, len(ch) - 5))
        d = bytearray(ch[bi][1])
        at = int(rng.integers(0, len(d)))
        if k % 3 == 0:
            d[at] ^= 1 << int(rng.integers(0, 8))
        elif k % 3 == 1:
            d[at] = (d[at] + int(rng.integers(1, 256))) & 255
        else:
            d = d[:at]
        ch[bi] = (b"IDAT", bytes(d))
        files["corrupt_%03d.png" % k] = D.SIG + b"".join(D.chunk(t, x) for t, x in ch)
    d = tmp_path / "cases"
    d.mkdir()
    for nm, b in files.items():
        (d / nm).write_bytes(b)
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "fuzz_png_decode"), os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(d)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])  # every call returned; no sanitizer report
    rc = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.splitlines() if ".png " in ln)
    assert sorted(rc) == sorted(files)
    accepted = 0
    for nm, b in files.items():
        want = zlib_says16(b)
        if rc[nm] == 0:
            accepted += 1
            assert want is not None, "%s: accepted, but zlib refuses these bytes" % nm
            assert np.array_equal(np.fromfile(str(d / (nm + ".out")), np.uint16).reshape(want.shape), want), nm
            assert np.array_equal(np.fromfile(str(d / (nm + ".out8")), np.uint8).reshape(want.shape), (want >> 8).astype(np.uint8)), nm
    print("fuzz: %d of %d 16-bit files accepted" % (accepted, len(files)))
    assert all(rc[nm] == 0 for nm in files if nm.startswith("base_"))
