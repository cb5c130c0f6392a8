"""The device PNG decoder (include/s360_png_decode.h, host/TestRenderStereoPanorama --device_state_read) without a GPU:
tests/test_gpu_png_decode.py in a process whose binding points at tools/libs360_emu.so, the host cases of
tests/test_gpu_zz_png_decode_host.py on tools/emu/TestRenderStereoPanorama, and — only here — a seeded fuzz of corrupted and
truncated band data on the sanitised emulation build (tools/fuzz/libs360_asan.so: device buffers are heap blocks with red zones,
a kernel's access outside them aborts the run). What the emulation covers and what it cannot:
tests/test_cpu_library_emulation.py."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import refprog
import test_gpu_png as T
import test_gpu_png_decode as D
import test_gpu_zz_png_decode_host as Z
import test_gpu_zz_state_png_host as H

ROOT = refprog.ROOT


@pytest.fixture(scope="module")
def emu_exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestRenderStereoPanorama")


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu_exe):
    """include/s360_png_decode.h (which include/s360.h includes) declares them, surround360_amd/_capi.py lists them with argtypes
    and restype, the emulated library exports them; s360_state_png.h and s360.h's own list are what they were."""
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    hdr = strip(open(os.path.join(ROOT, "include", "s360_png_decode.h")).read())
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.PNG_DECODE_SYMBOLS) and len(names) == 7
    assert not set(names) & (set(_capi.SYMBOLS) | set(_capi.STATE_PNG_SYMBOLS) | set(_capi.CUBEMAP_SYMBOLS))
    state = strip(open(os.path.join(ROOT, "include", "s360_state_png.h")).read())
    assert sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", state))) == sorted(_capi.STATE_PNG_SYMBOLS)
    assert '#include "s360_png_decode.h"' in strip(open(os.path.join(ROOT, "include", "s360.h")).read())
    lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
    for n in names:
        assert hasattr(lib, n), n
    src = open(os.path.join(ROOT, "surround360_amd", "_capi.py")).read()
    for n in names:
        assert "L.%s.argtypes" % n in src and "L.%s.restype" % n in src, n


def test_decodable_needs_no_device():
    """s360_png_decodable on the CPU: a zlib-made banded file, and files it does not take."""
    from surround360_amd import _capi
    from surround360_amd import render as R
    saved = _capi.LIB_PATH, _capi._lib
    _capi.LIB_PATH, _capi._lib = os.path.join(ROOT, "tools", "libs360_emu.so"), None
    try:
        a = D.repeated_image()
        assert R.png_decodable(D.zlib_banded(a, 5, 1, zlib.Z_RLE)) == (93, 40, 4, 5)
        assert R.png_decodable(D.pil_file(a[..., [2, 1, 0, 3]])) is None
        assert R.png_decodable(b"") is None
    finally:
        _capi.LIB_PATH, _capi._lib = saved


def test_library_cases_pass_on_the_emulated_library(emu_exe):
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_png_decode.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=e, timeout=3000, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 60 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("name", ["two_frames", "pole_removal"])
def test_emulated_chained_processes(tmp_path, emu_exe, name):
    H.check_chained_case(emu_exe, tmp_path, name, H.FLAG + Z.READ)


def test_emulated_host_written_files(tmp_path, emu_exe):
    Z.check_host_written_files(emu_exe, tmp_path)


def test_emulated_files_of_another_writer(tmp_path, emu_exe):
    Z.check_other_writers_files(emu_exe, tmp_path)


def test_emulated_environment_switch(tmp_path, emu_exe):
    Z.check_read_environment_switch(emu_exe, tmp_path)


def test_emulated_damaged_file(tmp_path, emu_exe):
    Z.check_a_damaged_file_dies_like_the_host_reader(emu_exe, tmp_path)


def test_emulated_mismatched_pole_removal_flow(tmp_path, emu_exe):
    Z.check_a_mismatched_pole_removal_flow_dies_like_the_host_path(emu_exe, tmp_path)


def test_emulated_stream_segments_resume_on_the_device(tmp_path, emu_exe):
    """--num_streams 2 over a range that starts from --prev_frame_data_dir: frame 1 and 2 of three_frames_sharpened as two
    streams behind frame 0's files, with and without the flag: the same equirects."""
    rig = H._rig(tmp_path)
    name = "three_frames_sharpened"
    frames, extra = refprog.CASES[name]
    outs = {}
    for tag, more in (("off", H.FLAG), ("on", H.FLAG + Z.READ)):
        work = str(tmp_path / tag)
        imgs, out, _ = refprog.write_inputs(work, rig, frames)
        base = [emu_exe, "--rig_json_file", rig, "--imgs_dir", imgs, "--output_data_dir", out, "--eqr_width", str(refprog.EQR_W),
                "--eqr_height", str(refprog.EQR_H), "--final_eqr_width", str(refprog.FINAL), "--final_eqr_height", str(refprog.FINAL)] + extra
        env = dict(os.environ, EMU_DEVICES="2")
        r = subprocess.run(base + ["--frame_number", frames[0], "--prev_frame_data_dir", "NONE", "--output_equirect_path",
                                   os.path.join(out, "eqr_%s.png" % frames[0])] + H.FLAG, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["--frame_number", frames[1], "--num_frames", "2", "--num_streams", "2", "--prev_frame_data_dir", frames[0],
                                   "--output_equirect_path", os.path.join(out, "eqr_%s.png"), "--v", "1"] + more,
                           capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        if tag == "on":
            assert Z.decoded_where(r.stderr)[0] >= 30
        outs[tag] = out
    for f in frames[1:]:
        assert refprog._digest_png(os.path.join(outs["on"], "eqr_%s.png" % f)) == refprog._digest_png(os.path.join(outs["off"], "eqr_%s.png" % f)), f


def test_emulated_two_gpus_decode_the_state_on_its_owner_rank(tmp_path, emu_exe):
    """--num_gpus 2 on two emulated devices: every pair is decoded on the rank of its partition, every pole unit on its owner — a
    rank handed an image it does not hold would refuse — and the files are the reference program's."""
    H.check_chained_case(emu_exe, tmp_path, "two_frames", H.FLAG + Z.READ + ["--num_gpus", "2"], env={"EMU_DEVICES": "2"})


# ---- fuzz: corrupted and truncated band data on the sanitised emulation build --------------------------------------------------
def container(png):
    """The chunks of a file as the library's parser walks them: up to IEND or the first chunk that is not whole."""
    out, pos = [], 8
    while pos + 12 <= len(png):
        n = int.from_bytes(png[pos:pos + 4], "big")
        if pos + 12 + n > len(png):
            break
        out.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        if out[-1][0] == b"IEND":
            break
        pos += 12 + n
    return out


def inflated_bands(png):
    """The scanlines of a banded file if every band inflates under zlib to exactly its rows, else None."""
    ch = [c for c in container(png) if c[0] != b"IEND"]
    w, h = int.from_bytes(ch[0][1][:4], "big"), int.from_bytes(ch[0][1][4:8], "big")
    rows, line = int.from_bytes(ch[1][1], "big"), 1 + (4 if ch[0][1][9] == 6 else 3) * w
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
    return scan


def zlib_says(png):
    """What Python's zlib makes of a banded file's bytes: its B,G,R(,A) pixels, or None if the container is not the banded one, a
    band does not inflate to exactly its rows, a filter type is not 0 or 1, or the Adler-32 differs."""
    ch = [c for c in container(png) if c[0] != b"IEND"]
    if len(ch) < 5 or [t for t, _ in ch[:3]] != [b"IHDR", b"sbNd", b"IDAT"] or len(ch[-1][1]) != 4 or any(t != b"IDAT" for t, _ in ch[2:]):
        return None
    w, h = int.from_bytes(ch[0][1][:4], "big"), int.from_bytes(ch[0][1][4:8], "big")
    c = 4 if ch[0][1][9] == 6 else 3
    rows = int.from_bytes(ch[1][1], "big")
    line = 1 + c * w
    bands = ch[3:-1]
    if len(bands) != -(-h // rows):
        return None
    scan = inflated_bands(png)
    if scan is None or zlib.adler32(scan) != int.from_bytes(ch[-1][1], "big"):
        return None
    f = np.frombuffer(scan, np.uint8).reshape(h, line)
    if (f[:, 0] > 1).any():
        return None
    px = f[:, 1:].reshape(h, w, c).astype(np.int64)
    px = np.where((f[:, 0] == 1)[:, None, None], np.cumsum(px, axis=1) & 255, px).astype(np.uint8)
    return np.ascontiguousarray(px[..., [2, 1, 0, 3] if c == 4 else [2, 1, 0]])


def rebuild(ch):
    return D.SIG + b"".join(D.chunk(t, d) for t, d in ch)


def test_fuzz_of_band_data_on_the_sanitised_emulation(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/libs360_asan.so", "fuzz/fuzz_png_decode"])
    rng = np.random.default_rng(2024)
    a4 = np.repeat(rng.integers(0, 256, (17, 8, 4), dtype=np.uint8), 3, axis=1)  # 17 x 24
    a3 = np.ascontiguousarray(D.smooth_image(3)[:17, :33])
    bases = [D.zlib_banded(a4, 5, 1, zlib.Z_RLE), D.zlib_banded(a4, 4, 6, zlib.Z_FIXED), D.zlib_banded(a4, 6, 9, zlib.Z_DEFAULT_STRATEGY),
             D.zlib_banded(a4, 5, 0, zlib.Z_DEFAULT_STRATEGY), D.zlib_banded(a3, 7, 6, zlib.Z_DEFAULT_STRATEGY, pieces=2),
             D.zlib_banded(a3, 3, 1, zlib.Z_RLE, ftype=0), D.zlib_banded(a3, 17, 6, zlib.Z_HUFFMAN_ONLY)]
    files = {}
    for k, b in enumerate(bases):
        assert zlib_says(b) is not None
        files["base_%02d.png" % k] = b
    for k in range(200):  # one byte replaced or one bit flipped inside a band's data
        ch = T.chunks(bases[k % len(bases)])
        bi = 3 + int(rng.integers(0, len(ch) - 5))
        d = bytearray(ch[bi][1])
        at = int(rng.integers(0, len(d)))
        if k % 2:
            d[at] ^= 1 << int(rng.integers(0, 8))
        else:
            d[at] = (d[at] + int(rng.integers(1, 256))) & 255
        ch[bi] = (b"IDAT", bytes(d))
        files["corrupt_%03d.png" % k] = rebuild(ch)
        scan = inflated_bands(rebuild(ch))
        if scan is not None:  # the bands still inflate: the same file with the Adler-32 of what they now hold
            ch[-2] = (b"IDAT", zlib.adler32(scan).to_bytes(4, "big"))
            files["corrupt_%03d_adler.png" % k] = rebuild(ch)
    for k in range(20):  # a band's segment cut short (the container stays whole), or the file itself
        b = bases[k % len(bases)]
        if k % 2:
            files["truncated_%03d.png" % k] = b[:int(rng.integers(60, len(b)))]
        else:
            ch = T.chunks(b)
            bi = 3 + int(rng.integers(0, len(ch) - 5))
            ch[bi] = (b"IDAT", ch[bi][1][:int(rng.integers(0, len(ch[bi][1])))])
            files["truncated_%03d.png" % k] = rebuild(ch)
    d = tmp_path / "cases"
    d.mkdir()
    for nm, b in files.items():
        (d / nm).write_bytes(b)
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "fuzz_png_decode"), os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(d)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])  # every call returned; no sanitizer report
    rc = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.splitlines() if ln.endswith(tuple("0123456789")) and ".png " in ln)
    assert sorted(rc) == sorted(files)
    accepted, stricter = 0, []
    for nm, b in files.items():
        want = zlib_says(b)
        if rc[nm] == 0:
            accepted += 1
            assert want is not None, "%s: accepted, but zlib refuses these bytes" % nm
            got = np.fromfile(str(d / (nm + ".out")), np.uint8).reshape(want.shape)
            assert np.array_equal(got, want), nm
        elif want is not None:
            # zlib hands out a band's bytes as soon as it has them; the device decoder also wants the segment complete (the end of
            # the block, the sync flush's empty stored block): damage behind the last literal is refused here and unseen there
            stricter.append(nm)
    print("fuzz: %d of %d files accepted; refused although zlib gives the band's bytes: %s" % (accepted, len(files), stricter))
    assert all(rc[nm] == 0 for nm in files if nm.startswith("base_"))
