"""The device JPEG encoder (include/s360_jpeg.h, surround360_amd/jpeg.py; the preview object's .jpg output, include/s360_preview.h;
host/TestHyperPreview --device_jpeg) against its two byte oracles: host/jpeg_io.hpp's writer (tools/jpeg_host_encode) and PIL's
save(quality=q, subsampling=2). Everything is byte equality; there is no tolerance anywhere. The test tap of
include/s360_debug_jpeg.h places a mismatch in the block stage or in the bitstream stage. Cases: tests/jpeg_cases.py.

The file also runs on the CPU emulation of the library (S360_TEST_EMULATED_LIB=1, tests/test_cpu_jpeg_device.py); test_program then
takes tools/emu/TestHyperPreview, the same source linked against the emulated library."""
import io
import os
import random
import subprocess

import numpy as np
import pytest

import jpeg_cases as JC
import preview_cases as PC
import test_gpu_preview as G

pytestmark = pytest.mark.gpu

ROOT = JC.ROOT
EMULATED = os.environ.get("S360_TEST_EMULATED_LIB") == "1"


@pytest.fixture(scope="module")
def encoders():
    """One encoder object of 1030 x 304 per quality; each serves every size."""
    from surround360_amd.jpeg import JpegEncoder
    made = {}

    def get(quality):
        if quality not in made:
            made[quality] = JpegEncoder(JC.MAX_W, JC.MAX_H, quality)
        return made[quality]
    return get


def shuffled_cases():
    cs = JC.cases()
    random.Random(360).shuffle(cs)  # a small image after a large one: stale scratch of the larger one would show
    return cs


def first_difference(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def test_blocks(encoders):
    """The tap's quantised coefficients (emission order, dummy blocks included) and bit lengths before stuffing against the two
    halves of the host writer, for every size at quality 95, the quality sweep and the last-byte cases."""
    for case in shuffled_cases():
        _, coef, bits = JC.host_case(case)
        got_coef, got_bits = encoders(case[3]).debug_blocks(JC.case_image(case))
        assert got_coef.shape == coef.shape and got_bits.shape == bits.shape, case
        bad = np.flatnonzero((got_coef != coef).any(axis=1))
        assert bad.size == 0, "%s: %d of %d blocks differ, the first is block %d (block %d of its MCU)" % (case, bad.size, len(coef), bad[0], bad[0] % 6)
        bad = np.flatnonzero(got_bits != bits)
        assert bad.size == 0, "%s: %d bit lengths differ, the first at block %d: %d, not %d" % (case, bad.size, bad[0], got_bits[bad[0]], bits[bad[0]])


def test_file_bytes(encoders):
    """JpegEncoder.encode is the host writer's file and PIL's file, over all cases, from one object per quality in shuffled order;
    a second encode of the same image returns the same bytes."""
    for case in shuffled_cases():
        bgr = JC.case_image(case)
        want = JC.host_case(case)[0]
        got = encoders(case[3]).encode(bgr)
        assert got == want, "%s: %d bytes, the host writer's file has %d; the first difference is at byte %d" % (case, len(got), len(want), first_difference(got, want))
        assert got == JC.pil_encode(bgr, case[3]), "%s: differs from PIL's file" % (case,)
        assert len(got) <= JC_bound(bgr)
        assert encoders(case[3]).encode(bgr) == got, "%s: the second encode differs" % (case,)


def JC_bound(bgr):
    from surround360_amd import jpeg
    return jpeg.bound(bgr.shape[1], bgr.shape[0])


def test_arguments(encoders):
    """cap one byte short: S360_ERR_INVALID_ARG and the size needed; an image wider or taller than the object's maximum is refused;
    qualities outside 1..100 are clamped as the host writer clamps them; the file decodes in PIL to what PIL decodes from its own."""
    from surround360_amd import _capi, jpeg
    from PIL import Image
    bgr = JC.image(70, 37, "spread")
    enc = encoders(95)
    want = JC.host_encode(bgr, 95)[0]
    with pytest.raises(_capi.S360Error) as e:
        enc.encode(bgr, cap=len(want) - 1)
    assert e.value.code == _capi.ERR_INVALID_ARG and enc.needed == len(want)
    assert enc.encode(bgr, cap=len(want)) == want
    for w, h in ((JC.MAX_W + 1, 8), (8, JC.MAX_H + 1)):
        with pytest.raises(_capi.S360Error) as e:
            enc.encode(np.zeros((h, w, 3), np.uint8))
        assert e.value.code == _capi.ERR_INVALID_ARG
    for q, same_as in ((0, 1), (101, 100), (-7, 1)):
        got = jpeg.JpegEncoder(70, 37, q).encode(bgr)
        assert got == JC.host_encode(bgr, q)[0] == JC.host_encode(bgr, same_as)[0]
    assert jpeg.bound(0, 5) == 0 and jpeg.bound(70000, 5) == 0 and jpeg.bound(70, 37) >= len(want)
    with pytest.raises(_capi.S360Error) as e:
        jpeg.JpegEncoder(0, 5)
    assert e.value.code == _capi.ERR_INVALID_ARG
    im = Image.open(io.BytesIO(want))
    assert im.format == "JPEG" and im.size == (70, 37)
    assert np.array_equal(np.array(im.convert("RGB")), G.pil_roundtrip(bgr))
    assert enc.last_time() >= 0


def test_more_than_256_scan_groups():
    """3360 x 3344: 43 890 MCUs, 263 340 blocks, 258 groups of JPEG_SCAN_ITEMS — the kernel that scans the group totals takes 256 a
    round and carries into a second one (every size up to 8192 x 8192 must work: 1536 groups). Ramps: every block differs."""
    from surround360_amd.jpeg import JpegEncoder
    w, h = 3360, 3344
    assert JC.n_blocks(w, h) > 256 * JC.SCAN_ITEMS and JC.n_blocks(w, h) % JC.SCAN_ITEMS
    bgr = JC.image(w, h, "ramps")
    enc = JpegEncoder(w, h, 95)
    got, want = enc.encode(bgr), JC.pil_encode(bgr, 95)  # (PIL's file is the host writer's: test_cpu_jpeg_device.py)
    assert got == want, "%d bytes, PIL's file has %d; the first difference is at byte %d" % (len(got), len(want), first_difference(got, want))
    host = JC.host_encode(bgr, 95)
    assert got == host[0]
    coef, bits = enc.debug_blocks(bgr)
    assert np.array_equal(coef, host[1]) and np.array_equal(bits, host[2])
    enc.close()


@pytest.mark.parametrize("shape", list(PC.SHAPES))
def test_preview_fetch_jpeg(shape):
    """The preview object with the encoder on: two frames in flight come back as the host writer's files of render_packed's pixels,
    in order; fetch() on an encoded frame still returns the pixels; fetch_jpeg on a frame submitted with the encoder off is refused
    and leaves the frame to fetch(); a third submit is still refused."""
    from surround360_amd import _capi
    pv, _ = G.make_preview(shape)
    a, b = PC.frames(shape, "spread", 12), PC.frames(shape, "checker", 12)
    wa, wb = pv.render_packed(*a, 12), pv.render_packed(*b, 12)
    fa, fb = JC.host_encode(wa, 95)[0], JC.host_encode(wb, 95)[0]
    assert fa != fb
    with pytest.raises(_capi.S360Error) as e:
        pv.last_jpeg_time()
    assert e.value.code == _capi.ERR_STATE
    pv.set_jpeg(True, 95)
    assert pv.jpeg_bound() >= max(len(fa), len(fb))
    pv.submit_packed(*a, 12)
    pv.submit_packed(*b, 12)
    with pytest.raises(_capi.S360Error) as e:
        pv.submit_packed(*a, 12)
    assert e.value.code == _capi.ERR_STATE
    with pytest.raises(_capi.S360Error) as e:  # too small a buffer: the size needed, and the frame stays queued
        pv.fetch_jpeg(cap=len(fa) - 1)
    assert e.value.code == _capi.ERR_INVALID_ARG
    got_a, got_b = pv.fetch_jpeg(), pv.fetch_jpeg()
    assert got_a == fa, "first frame: first difference at byte %d" % first_difference(got_a, fa)
    assert got_b == fb, "second frame: first difference at byte %d" % first_difference(got_b, fb)
    with pytest.raises(_capi.S360Error) as e:
        pv.fetch_jpeg()
    assert e.value.code == _capi.ERR_STATE
    assert pv.last_jpeg_time() >= 0
    pv.submit_packed(*a, 12)  # an encoded frame, taken as pixels
    assert np.array_equal(pv.fetch(), wa)
    assert pv.render_packed_jpeg(*b, 12) == fb
    assert np.array_equal(pv.render_packed(*a, 12), wa)
    pv.set_jpeg(False)
    pv.submit_packed(*b, 12)
    with pytest.raises(_capi.S360Error) as e:
        pv.fetch_jpeg()
    assert e.value.code == _capi.ERR_STATE and "encoder off" in str(e.value)
    assert np.array_equal(pv.fetch(), wb)
    pv.set_jpeg(True, 50)  # another quality on the same object
    assert pv.render_packed_jpeg(*a, 12) == JC.host_encode(wa, 50)[0]
    # the quality changed while a frame is queued: that frame keeps the quality it was submitted with, header and scan
    pv.submit_packed(*b, 12)
    pv.set_jpeg(True, 95)
    pv.submit_packed(*a, 12)
    pv.set_jpeg(True, 1)
    got_b, got_a = pv.fetch_jpeg(), pv.fetch_jpeg()
    assert got_b == JC.host_encode(wb, 50)[0], "queued at 50: first difference at byte %d" % first_difference(got_b, JC.host_encode(wb, 50)[0])
    assert got_a == fa, "queued at 95: first difference at byte %d" % first_difference(got_a, fa)
    assert pv.render_packed_jpeg(*a, 12) == JC.host_encode(wa, 1)[0]


# ---- the program ----------------------------------------------------------------------------------------------------------
def program():
    if EMULATED:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libs360_emu.so", "emu_programs"])
        return os.path.join(ROOT, "tools", "emu", "TestHyperPreview")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "TestHyperPreview")


def run_program(exe, tmp_path, name, more=(), env=None, shape="landscape", bits=12):
    cap, dest = tmp_path / "capture", tmp_path / name
    if not cap.exists():
        cap.mkdir()
        PC.write_capture(str(cap), shape, bits)
    _, _, W, H, _, _ = PC.SHAPES[shape]
    rig = PC.write_rig(PC.small_rig(shape), str(tmp_path / "rig.json"))
    cmd = [exe, "--logbuflevel", "-1", "--stderrthreshold", "0", "--v", "0", "--log_dir", str(tmp_path / "logs"), "--rig_json_file", rig,
           "--binary_prefix", str(cap), "--preview_dest", str(dest), "--eqr_width", str(W), "--eqr_height", str(H), "--gamma", "1.0",
           "--file_count", "2"] + list(more)
    e = {k: v for k, v in os.environ.items() if k != "S360_PREVIEW_DEVICE_JPEG"}
    e.update(env or {})
    return dest, subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e)


def check_program(exe, tmp_path):
    """TestHyperPreview on the two-file capture of preview_cases.write_capture: with --device_jpeg, and with
    S360_PREVIEW_DEVICE_JPEG=1 and no flag, the same file names and byte for byte the same files as without; --device_jpeg
    together with --preview_ext png is refused with a message that names both."""
    base, r = run_program(exe, tmp_path, "host")
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(base))
    assert names == ["%06d.jpg" % f for f in range(PC.CAPTURE_FRAMES)]
    files = [open(os.path.join(base, n), "rb").read() for n in names]
    assert len(set(files)) == len(files)
    for name, more, env in (("flag", ["--device_jpeg"], None), ("flag_eq", ["--device_jpeg=true", "--jpeg_threads", "1"], None),
                            ("env", [], {"S360_PREVIEW_DEVICE_JPEG": "1"})):
        dest, r = run_program(exe, tmp_path, name, more, env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert all("Rendering frame %d..." % f in r.stderr for f in range(PC.CAPTURE_FRAMES))
        assert sorted(os.listdir(dest)) == names, name
        for n, want in zip(names, files):
            got = open(os.path.join(dest, n), "rb").read()
            assert got == want, "%s, %s: first difference at byte %d" % (name, n, first_difference(got, want))
    # a flag on the command line wins over the environment; with --preview_ext png the environment switch is ignored
    dest, r = run_program(exe, tmp_path, "flag_off", ["--device_jpeg=false"], {"S360_PREVIEW_DEVICE_JPEG": "1"})
    assert r.returncode == 0 and [open(os.path.join(dest, n), "rb").read() for n in names] == files, r.stderr[-2000:]
    dest, r = run_program(exe, tmp_path, "env_png", ["--preview_ext", "png"], {"S360_PREVIEW_DEVICE_JPEG": "1"})
    assert r.returncode == 0 and sorted(os.listdir(dest)) == [n.replace(".jpg", ".png") for n in names], r.stderr[-2000:]
    dest, r = run_program(exe, tmp_path, "refused", ["--device_jpeg", "--preview_ext", "png"])
    assert r.returncode != 0 and "--device_jpeg" in r.stderr and "--preview_ext png" in r.stderr
    assert not os.path.exists(dest) or not os.listdir(dest)


def test_program(tmp_path):
    check_program(program(), tmp_path)
