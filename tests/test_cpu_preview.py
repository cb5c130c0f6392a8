"""The preview path without a GPU: the numpy restatement of the reference's TestHyperPreview (tests/preview_oracle.py) against the
recorded outputs of the reference's own functions (tests/golden/preview_golden.npz, tests/golden/make_preview_golden.py), the JPEG
writer of host/jpeg_io.hpp against PIL, the device's expf sequence over its extended range (tools/expf_check.c), the command-line
errors of TestHyperPreview, and the library and the program on the CPU emulation of the HIP sources (tools/libs360_emu.so,
tools/emu/TestHyperPreview; what the emulation covers: tests/test_cpu_library_emulation.py)."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import preview_cases as PC
import preview_oracle as PO
import test_gpu_preview as G

ROOT = PC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "preview_golden.npz")
CHAINS = [("landscape", "spread", 12, 1.0), ("portrait", "checker", 8, 1.0), ("portrait", "dark", 12, 2.2)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape,content,bits,gamma", CHAINS)
def test_restatement_against_the_reference(shape, content, bits, gamma):
    """Cameras (createRescaledCamera), maps (projectEquirectToCam), developed layers (simpleDemosaic with its XOR constants, both
    fades), a remapped layer, flattenLayersAlphaSoftmax's floats (NaNs included) and the final bytes: bit for bit what the
    reference's own code returned when the golden file was written."""
    g = np.load(GOLDEN)
    key = "%s/%s/%d/%g/" % (shape, content, bits, gamma)
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    poles = PC.pole_cameras(PC.small_rig(shape))
    frames = PC.frames(shape, content, bits)
    cams = [PO.rescaled_camera_json(c) for c in poles]
    for l in range(3):
        assert list(g[key + "cams"][l]) == cams[l]["resolution"] + cams[l]["principal"] + cams[l]["focal"]
    maps = G.oracle_maps(shape)[0]
    if gamma == 1.0:
        for l in range(3):
            assert same(maps[l], g[key + "map%d" % l]), "map of layer %d" % l
    dev = [PO.develop(frames[l], bits, raw_w, raw_h, l, gamma) for l in range(3)]
    for l in range(3):
        assert same(dev[l], g[key + "developed%d" % l]), "developed layer %d" % l
    rem = [PO.remap(d, m) for d, m in zip(dev, maps)]
    assert same(rem[1], g[key + "remapped1"])
    flat = PO.flatten_layers_alpha_softmax(rem, 30.0)
    assert same(flat, g[key + "flat"])
    assert np.isnan(flat).any() == (shape == "portrait")
    assert same(PO.to_u8(flat), g[key + "bytes"])
    assert not PO.to_u8(flat)[np.isnan(flat)].any()
    r = PO.Renderer(poles, raw_w, raw_h, W, H, gamma, maps=maps)
    assert same(r.render(*frames, bits), g[key + "bytes"])


def test_demosaic_constants_are_xor_expressions():
    """`2^16-1` and `2^32-1` are 13 and 29: a full-scale sample comes out as 65535 / 13 * 29, far above 65535."""
    d = PO.simple_demosaic(np.full((2, 2), 65535, np.uint16))
    assert d.shape == (1, 1, 3) and (d == np.float32(65535.0) / np.float32(13.0) * np.float32(29.0)).all() and d[0, 0, 0] > 146000


@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_tie_window_of_the_oracle_maps(shape):
    """The allowance of test_whole_object_on_its_own_maps, looked at on the CPU: how many pixels of the chosen shapes have an oracle
    map entry x 32 within 0.032 of a rounding tie. The window covers 6.4 % of the line per coordinate, so with two coordinates and up
    to three layers this is far more than the 1 % the GPU test allows to be LEFT OUT — which is why that test leaves a pixel out only
    where the device's entry actually quantises differently, and counts those against the cap. Here: the window is what the
    arithmetic says (each layer between 5 % and 25 % of its seen pixels), i.e. no map sits on ties systematically."""
    maps, _, seen = G.oracle_maps(shape)
    for l in range(3):
        frac = G.near_tie(maps[l])[seen[l]].mean()
        print("%s layer %d: %.1f %% of the seen pixels within the window" % (shape, l, 100 * frac))
        assert 0.05 <= frac <= 0.25


# ---- the JPEG writer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpeg_encode():
    """tools/fuzz/jpeg_encode: host/jpeg_io.hpp's writer behind a main() of its own, built with AddressSanitizer and
    UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "fuzz/jpeg_encode"])
    return os.path.join(ROOT, "tools", "fuzz", "jpeg_encode")


def jpeg_image(w, h, kind):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "spread":  # PC.content's skewed spread, another seed per channel
        return np.stack([PC.content("spread", w, h, 8, seed=c) for c in range(3)], axis=-1).astype(np.uint8)
    if kind == "checker":
        return np.repeat(PC.content("checker", w, h, 8)[..., None], 3, axis=-1).astype(np.uint8)
    return np.full((h, w, 3), (31, 200, 90), np.uint8)


def segments(data):
    """(marker, payload) of every segment up to SOS."""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out


@pytest.mark.parametrize("kind", ["spread", "checker", "constant"])
@pytest.mark.parametrize("w,h", [(16, 16), (17, 9), (48, 32), (70, 37)])
def test_jpeg_writer_against_pil(tmp_path, jpeg_encode, w, h, kind):
    """The file decodes in PIL to exactly the pixels PIL decodes from its own save(quality=95, subsampling=2) of the same image —
    equal decodes mean equal quantised coefficients — and is a baseline JFIF file with 2 x 2 luma sampling, libjpeg's tables and
    marker order."""
    bgr = jpeg_image(w, h, kind)
    src, dst = tmp_path / "in.bgr", tmp_path / "out.jpg"
    bgr.tofile(str(src))
    r = subprocess.run([jpeg_encode, str(src), str(w), str(h), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    mine = open(str(dst), "rb").read()
    im = Image.open(io.BytesIO(mine))
    assert im.format == "JPEG" and im.size == (w, h) and im.mode == "RGB"
    assert np.array_equal(np.array(im), G.pil_roundtrip(bgr))
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=95, subsampling=2)
    segs, pil = segments(mine), segments(b.getvalue())
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]  # APP0, DQT x 2, SOF0, DHT x 4, SOS
    assert segs[0][1] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    sof = segs[3][1]
    assert sof[0] == 8 and int.from_bytes(sof[1:3], "big") == h and int.from_bytes(sof[3:5], "big") == w
    assert sof[5:] == bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for marker in (0xDB, 0xC4):  # quantisation and Huffman tables: what libjpeg writes at quality 95
        assert [p for m, p in segs if m == marker] == [p for m, p in pil if m == marker]
    assert mine[-2:] == b"\xff\xd9"


def test_jpeg_writer_sweep_under_sanitizers(jpeg_encode):
    """Every size from 1 x 1 to 40 x 40 and a few larger ones, encoded and decoded again by the reader of the same header."""
    r = subprocess.run([jpeg_encode, "--sweep"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and "4815 files" in r.stdout, r.stderr[-2000:]


# ---- expf ---------------------------------------------------------------------------------------------------------------
def test_expf_sequence_over_the_positive_range(tmp_path):
    """tools/expf_check.c, `pos` mode: the device's expf sequence (expf_glibc.hpp, restated in C there) against the host's expf for
    every 61st float of [0, 88) and EVERY float of [88, 88.8], where the overflow branch decides. (All 1 118 935 451 floats of
    [0, 88.8], and all floats <= 0, take a minute: run the tool without arguments.)"""
    exe = str(tmp_path / "expf_check")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "expf_check.c"), "-lm"])
    r = subprocess.run([exe, "pos", "61"], capture_output=True, text=True)
    m = re.search(r"(\d+) floats in \[0, 88.8\] checked, (\d+) mismatches", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) > 18_000_000 and int(m.group(2)) == 0, r.stdout
    src = open(os.path.join(ROOT, "surround360_amd", "csrc", "expf_glibc.hpp")).read()
    assert "0x1.62e42ep6f" in src and "expf_glibc" in open(os.path.join(ROOT, "surround360_amd", "csrc", "isp_kernels.hip")).read()


# ---- the emulated library and program --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
    return os.path.join(ROOT, "tools", "emu", "TestHyperPreview")


def test_header_binding_and_emulated_library_agree_on_the_entry_points(emu_exe):
    import ctypes as C
    from surround360_amd import _capi
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    for hdr, names in (("s360_preview.h", _capi.PREVIEW_SYMBOLS), ("s360_debug_preview.h", _capi.DEBUG_PREVIEW_SYMBOLS)):
        text = strip(open(os.path.join(ROOT, "include", hdr)).read())
        assert sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", text))) == sorted(names)
        lib = C.CDLL(os.path.join(ROOT, "tools", "libs360_emu.so"))
        for n in names:
            assert hasattr(lib, n), n
    code = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "s360_debug_preview.h")],
                          capture_output=True, text=True)
    assert code.returncode == 0, code.stderr


def test_library_cases_pass_on_the_emulated_library(emu_exe):
    """tests/test_gpu_preview.py's 128 x 96 cases (and the shape-independent ones) in a process whose binding points at the
    emulated library."""
    e = dict(os.environ, S360_TEST_EMULATED_LIB="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_preview.py"), "-q", "-m", "gpu",
                        "-k", "landscape or persistence or submit", "-p", "no:cacheprovider"], capture_output=True, text=True, env=e,
                       timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 28 and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


def test_emulated_program(tmp_path, emu_exe):
    G.check_program(emu_exe, tmp_path)


def run(exe, args):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)


def test_program_command_line_errors(tmp_path, emu_exe):
    """Missing required flags, an unknown flag, bad magic, a wrong file count, a file index that is not the file's name, a camera
    index past the list: the reference's messages, a failing exit status, nothing written."""
    cap = tmp_path / "capture"
    cap.mkdir()
    PC.write_capture(str(cap), "landscape", 8)
    rig = PC.write_rig(PC.small_rig("landscape"), str(tmp_path / "rig.json"))
    dest = str(tmp_path / "out")
    good = ["--rig_json_file", rig, "--binary_prefix", str(cap), "--preview_dest", dest, "--eqr_width", "96", "--eqr_height", "48"]
    for k in ("rig_json_file", "binary_prefix", "preview_dest"):
        i = good.index("--" + k)
        r = run(emu_exe, good[:i] + good[i + 2:])
        assert r.returncode != 0 and "missing required command line argument: " + k in r.stderr
    r = run(emu_exe, good + ["--no_such_flag", "1"])
    assert r.returncode == 1 and "unknown command line flag 'no_such_flag'" in r.stderr
    r = run(emu_exe, good + ["--file_count", "3"])
    assert r.returncode != 0 and "error opening binary file" in r.stderr and "2.bin" in r.stderr
    r = run(emu_exe, good + ["--file_count", "1"])
    assert r.returncode != 0 and "binary file count in metadata != num .bin files" in r.stderr
    r = run(emu_exe, good + ["--bottom_cam2_index", "17"])
    assert r.returncode != 0 and "bottom_cam2_index" in r.stderr
    r = run(emu_exe, good + ["--preview_ext", "gif"])
    assert r.returncode != 0 and "preview_ext" in r.stderr
    bad = tmp_path / "bad_magic"
    bad.mkdir()
    PC.write_capture(str(bad), "landscape", 8, magic=0xfaceb00d)
    r = run(emu_exe, good[:2] + ["--binary_prefix", str(bad)] + good[4:])
    assert r.returncode != 0 and "binary file not tagged" in r.stderr
    swapped = tmp_path / "swapped"
    swapped.mkdir()
    PC.write_capture(str(swapped), "landscape", 8)
    os.rename(str(swapped / "0.bin"), str(swapped / "t.bin"))
    os.rename(str(swapped / "1.bin"), str(swapped / "0.bin"))
    os.rename(str(swapped / "t.bin"), str(swapped / "1.bin"))
    r = run(emu_exe, good[:2] + ["--binary_prefix", str(swapped)] + good[4:])
    assert r.returncode != 0 and "binary file name in metadata != loaded .bin file" in r.stderr
    assert not os.path.exists(dest) or not os.listdir(dest)
    r = run(emu_exe, good + ["--enable_pole_removal", "false", "--image_width", "7", "--logbuflevel", "-1", "--frame_count", "1"])
    assert r.returncode == 0 and os.listdir(dest) == ["000000.jpg"], r.stderr[-1000:]
