"""host/TestRenderStereoPanorama --device_input_png: the camera files of imgs_dir are read as bytes and decoded on the device
straight into the frame's source slots (s360_frame_upload_png, include/s360_input_png.h) instead of being inflated on host threads
and uploaded as pixels. The imgs_dir is what host/Unpacker --device_png writes from a small capture (16-bit banded files); the
8-bit variant holds those images' high bytes in the banded layout host/png_io.hpp writes (Z_RLE, level 1) — host/Unpacker has no
8-bit output. The oracle is the same program without the flag: the equirect's bytes, the state images' pixels and the flow files
must be equal, and the --v 1 line says how many files took which path. The check functions take the programs' paths:
tests/test_cpu_input_png.py runs them on the programs linked against the emulated library."""
import hashlib
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import isputil
import refprog
import rigutil
import test_gpu_input_png as IP
import test_gpu_png_decode as D
from test_gpu_zz_unpacker_png import run_unpacker

pytestmark = pytest.mark.gpu

ROOT = refprog.ROOT
FLAG = ["--device_input_png"]
COMMON = ["--enable_top", "--enable_bottom", "--sharpening", "0.25", "--v", "1"]


def prepare(unpacker_exe, tmp_path, nframes, depth=16):
    """(rig, imgs_dir, camera ids, frame names): a capture of the small rig's 17 cameras unpacked with --device_png."""
    cam = refprog.CAM
    rig = rigutil.scaled_rig_json(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"), cam / 2048.0)
    n = len(json.load(open(rig))["cameras"])
    serials = [40000 + 7 * k for k in range(n)]
    configs = [isputil.CONFIG_GRBG_NOSHARP if k % 3 else isputil.CONFIG_FULL for k in range(n)]
    pats = ["GRBG" if k % 3 else "RGGB" for k in range(n)]
    frames = [[isputil.bayer_frame(cam, cam, seed=100 * f + k, pattern=pats[k]) for k in range(n)] for f in range(nframes)]
    binp, ispd = tmp_path / "0.bin", tmp_path / "isp"
    isputil.footage_file(str(binp), frames, 12, serials)
    ispd.mkdir()
    for s, js in zip(serials, configs):
        (ispd / ("%d.json" % s)).write_text(js)
    imgs, _, _ = run_unpacker(unpacker_exe, tmp_path, "dev", binp, ispd, ["--device_png"], raw=False)
    ids = sorted(os.listdir(str(imgs)))
    names = ["%06d" % f for f in range(nframes)]
    assert len(ids) == n
    for cid in ids:
        for f in names:
            p = imgs / cid / (f + ".png")
            b = p.read_bytes()
            assert IP.T.chunks(b)[0][1][8:10] == bytes([16, 2]) and IP.T.chunks(b)[1][0] == b"sbNd"
            if depth == 8:
                p.write_bytes(D.zlib_banded((IP.decode16_quick(b) >> 8).astype(np.uint8), 16, 1, zlib.Z_RLE))
    return rig, str(imgs), ids, names


def used(rig):
    """The camera files a frame reads: the side cameras, the top camera, the primary bottom camera."""
    return len(refprog.rig_ids(rig)[0]) + 2


def render(exe, rig, imgs, out, frame, more=(), env=None, prev="NONE", num_frames=None):
    """One process of the renderer; returns its stderr."""
    for d in [out, os.path.join(out, "flow"), os.path.join(out, "debug")]:
        os.makedirs(d, exist_ok=True)
    n = num_frames or 1
    for k in range(n):
        f = "%06d" % (int(frame) + k)
        os.makedirs(os.path.join(out, "flow", f), exist_ok=True)
        os.makedirs(os.path.join(out, "debug", f, "flow_images"), exist_ok=True)
    cmd = [exe, "--rig_json_file", rig, "--eqr_width", str(refprog.EQR_W), "--eqr_height", str(refprog.EQR_H), "--final_eqr_width",
           str(refprog.FINAL), "--final_eqr_height", str(refprog.FINAL), "--imgs_dir", imgs, "--frame_number", frame, "--output_data_dir", out,
           "--prev_frame_data_dir", prev, "--output_equirect_path", os.path.join(out, "eqr_%s.png" if num_frames else "eqr_%s.png" % frame)] + COMMON
    if num_frames:
        cmd += ["--num_frames", str(num_frames)]
    r = subprocess.run(cmd + list(more), capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-2000:])
    return r.stderr


def results(out):
    """Every file under the output directory: the equirects by their bytes, the state images by their pixels, the flows by
    their bytes."""
    d = {}
    for dp, _, fs in os.walk(out):
        for fn in fs:
            p = os.path.join(dp, fn)
            rel = os.path.relpath(p, out)
            if fn.endswith(".png") and not fn.startswith("eqr_"):
                d[rel] = refprog._digest_png(p)
            elif fn.endswith((".png", ".bin")):
                d[rel] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return d


def assert_same(a, b, at_least):
    ra, rb = results(a), results(b)
    assert len(ra) >= at_least and sorted(ra) == sorted(rb)
    differing = sorted(k for k in ra if ra[k] != rb[k])
    assert not differing, "%d of %d files differ: %s" % (len(differing), len(ra), differing[:12])


def decoded_where(log):
    """(camera files decoded on the device, on the host) from the --v 1 line "camera images"."""
    m = re.findall(r"camera images:\s+(\d+) files decoded on the device, (\d+) on the host", log)
    assert m, log[-1500:]
    return int(m[-1][0]), int(m[-1][1])  # (the counters are the process's: with one job per GPU the last line has them all)


def check_single_frame(unpacker_exe, exe, tmp_path, depth):
    """One frame with and without the flag; with depth 8 also with the environment switch in the flag's place."""
    rig, imgs, ids, names = prepare(unpacker_exe, tmp_path, 1, depth)
    off = render(exe, rig, imgs, str(tmp_path / "off"), names[0])
    assert "camera images:" not in off
    on = render(exe, rig, imgs, str(tmp_path / "on"), names[0], FLAG)
    assert decoded_where(on) == (used(rig), 0)
    assert refprog.png_pixels_bgr(str(tmp_path / "off" / "eqr_000000.png")).std() > 5
    assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60)
    if depth == 8:
        env = render(exe, rig, imgs, str(tmp_path / "env"), names[0], env={"S360_DEVICE_INPUT_PNG": "1"})
        assert decoded_where(env) == (used(rig), 0)
        assert_same(str(tmp_path / "off"), str(tmp_path / "env"), 60)


def check_fallback_per_file(unpacker_exe, exe, tmp_path):
    """One camera's file rewritten by PIL (one zlib stream, no bands), one as RGBA: those two take the host decoder, the other
    fifteen the device, and nothing in the output changes."""
    rig, imgs, ids, names = prepare(unpacker_exe, tmp_path, 1, 8)
    side, top, _ = refprog.rig_ids(rig)
    for cid in (side[3], top):
        p = os.path.join(imgs, cid, names[0] + ".png")
        a = np.asarray(Image.open(p))
        assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8
        Image.fromarray(a if cid == top else np.dstack([a, np.full(a.shape[:2], 255, np.uint8)])).save(p)
    off = render(exe, rig, imgs, str(tmp_path / "off"), names[0])
    on = render(exe, rig, imgs, str(tmp_path / "on"), names[0], FLAG)
    assert "camera images:" not in off and decoded_where(on) == (used(rig) - 2, 2)
    assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60)


def check_chained_processes(unpacker_exe, exe, tmp_path):
    """Two single-frame processes chained with --prev_frame_data_dir, both with the flag, against both without."""
    rig, imgs, ids, names = prepare(unpacker_exe, tmp_path, 2)
    for tag, more in (("off", []), ("on", FLAG)):
        out = str(tmp_path / tag)
        render(exe, rig, imgs, out, names[0], more)
        log = render(exe, rig, imgs, out, names[1], more, prev=names[0])
        if more:
            assert decoded_where(log) == (used(rig), 0)
    assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 120)
    a = refprog.png_pixels_bgr(str(tmp_path / "on" / "eqr_000000.png"))
    assert not np.array_equal(a, refprog.png_pixels_bgr(str(tmp_path / "on" / "eqr_000001.png")))


def check_stream(unpacker_exe, exe, tmp_path, more, frames=3):
    """--num_frames 3 in one process (more: e.g. --num_streams), with and without the flag."""
    rig, imgs, ids, names = prepare(unpacker_exe, tmp_path, frames)
    for tag, flag in (("off", []), ("on", FLAG)):
        log = render(exe, rig, imgs, str(tmp_path / tag), names[0], list(more) + flag, num_frames=frames)
        if flag:
            assert decoded_where(log) == (frames * used(rig), 0)
    for f in names:
        assert os.path.exists(str(tmp_path / "on" / ("eqr_%s.png" % f)))
    assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60 + frames)


@pytest.fixture(scope="module")
def programs(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "Unpacker"), os.path.join(ROOT, "host", "TestRenderStereoPanorama")


@pytest.mark.parametrize("depth", [16, 8])
def test_single_frame(tmp_path, programs, depth):
    check_single_frame(programs[0], programs[1], tmp_path, depth)


def test_fallback_is_per_file(tmp_path, programs):
    check_fallback_per_file(programs[0], programs[1], tmp_path)


def test_chained_processes(tmp_path, programs):
    check_chained_processes(programs[0], programs[1], tmp_path)


def test_num_frames_3(tmp_path, programs):
    check_stream(programs[0], programs[1], tmp_path, [])


def test_num_streams_2(tmp_path, programs):
    check_stream(programs[0], programs[1], tmp_path, ["--num_streams", "2"], frames=4)
