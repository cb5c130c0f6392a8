"""host/TestRenderStereoPanorama with .jpg output paths: the extension decides the codec, as it does for cv::imwrite behind the
reference's imwriteExceptionOnFail. Without a flag the file is written by jpegio::encode on the host threads at quality 95; with
--device_jpeg (or S360_DEVICE_JPEG=1) it is encoded on the device (include/s360_frame_jpeg.h) and must be the same file. The
oracles: tools/jpeg_host_encode on the pixels decoded from the .png the same command line writes, and the program against itself.
The rig is the tests' small one at the frame size of tests/frame_jpeg_cases.py (an output of 250 x 214 and a cubemap of 100 x 96
faces: dummy blocks on both edges). The check functions take the program's path: tests/test_cpu_frame_jpeg.py runs the one-frame
case on the program linked against the emulated library."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import frame_jpeg_cases as FJ
import jpeg_cases as JC
import refprog
import rigutil

pytestmark = pytest.mark.gpu

ROOT = refprog.ROOT
FINAL_W, FINAL_H = FJ.SHAPES["odd"]["final"]
FACE_W, FACE_H, CUBE_FMT = FJ.SHAPES["odd"]["cube"]
COMMON = ["--enable_top", "--enable_bottom", "--sharpening", "0.25", "--v", "1", "--cubemap_width", str(FACE_W), "--cubemap_height", str(FACE_H),
          "--cubemap_format", CUBE_FMT, "--write_state=false"]
ON_HOST, ON_DEVICE = "JPEG encoded on the host", "JPEG encoded on the device"


def prepare(tmp_path, nframes):
    """(rig, imgs_dir, frame names): the small rig's cameras as PNG files."""
    rig = rigutil.scaled_rig_json(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"), FJ.CAM / 2048.0)
    names = ["%06d" % f for f in range(nframes)]
    for f, name in enumerate(names):
        for cid, img in refprog.frame_images(rig, f, FJ.CAM).items():
            os.makedirs(str(tmp_path / "rgb" / cid), exist_ok=True)
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(str(tmp_path / "rgb" / cid / (name + ".png")))
    return rig, str(tmp_path / "rgb"), names


def render(exe, rig, imgs, out, names, eq_ext, cube_ext, more=(), env=None):
    """One process of the renderer over the frames `names`; returns its stderr. One frame: the paths name the files themselves."""
    os.makedirs(out, exist_ok=True)
    stream = len(names) > 1
    cmd = [exe, "--rig_json_file", rig, "--eqr_width", str(FJ.EQR_W), "--eqr_height", str(FJ.EQR_H), "--final_eqr_width", str(FINAL_W),
           "--final_eqr_height", str(FINAL_H), "--imgs_dir", imgs, "--frame_number", names[0], "--output_data_dir", out,
           "--output_equirect_path", os.path.join(out, "eqr_%s" + eq_ext if stream else "eqr_" + names[0] + eq_ext),
           "--output_cubemap_path", os.path.join(out, "cube_%s" + cube_ext if stream else "cube_" + names[0] + cube_ext)] + COMMON
    if stream:
        cmd += ["--num_frames", str(len(names))]
    e = dict(os.environ, **(env or {}))
    if env is None:
        e.pop("S360_DEVICE_JPEG", None)
    r = subprocess.run(cmd + list(more), capture_output=True, text=True, timeout=900, env=e)
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-2000:])
    return r.stderr


def outputs(out, names, eq_ext, cube_ext):
    return {stem + n + ext: open(os.path.join(out, stem + n + ext), "rb").read() for n in names for stem, ext in (("eqr_", eq_ext), ("cube_", cube_ext))}


def path_line(log):
    lines = [ln for ln in log.splitlines() if ln.startswith("output files:")]
    assert lines, log[-1500:]
    return lines[-1]


def assert_jpeg_of_png(jpg, png_path, what):
    """jpg == jpegio::encode (and PIL's file) of the pixels in the PNG; PIL opens it as a baseline 4:2:0 JPEG of that size."""
    px = refprog.png_pixels_bgr(png_path)
    assert px.std() > 5
    FJ.same(jpg, FJ.oracle(px, 95), what)
    assert jpg[:2] == b"\xff\xd8" and jpg[-2:] == b"\xff\xd9"
    im = Image.open(io.BytesIO(jpg))
    assert im.format == "JPEG" and im.size == (px.shape[1], px.shape[0]) and im.mode == "RGB"
    im.load()


def check_one_frame(exe, tmp_path):
    """.png outputs, .jpg outputs on the host, .jpg outputs on the device: each .jpg is the oracle's file of the .png's pixels, the
    device path's files are the host path's, and --v 1 names the path taken."""
    rig, imgs, names = prepare(tmp_path, 1)
    n = names[0]
    log = render(exe, rig, imgs, str(tmp_path / "png"), names, ".png", ".png")
    assert "JPEG" not in path_line(log)
    log = render(exe, rig, imgs, str(tmp_path / "host"), names, ".jpg", ".JPEG")  # (the extension in either case)
    assert path_line(log).count(ON_HOST) == 2 and ON_DEVICE not in log
    host = outputs(str(tmp_path / "host"), names, ".jpg", ".JPEG")
    assert_jpeg_of_png(host["eqr_%s.jpg" % n], str(tmp_path / "png" / ("eqr_%s.png" % n)), "equirect on the host")
    assert_jpeg_of_png(host["cube_%s.JPEG" % n], str(tmp_path / "png" / ("cube_%s.png" % n)), "cubemap on the host")
    log = render(exe, rig, imgs, str(tmp_path / "dev"), names, ".jpg", ".JPEG", ["--device_jpeg"])
    assert path_line(log).count(ON_DEVICE) == 2 and ON_HOST not in log
    dev = outputs(str(tmp_path / "dev"), names, ".jpg", ".JPEG")
    for k in host:
        FJ.same(dev[k], host[k], k + " on the device")


def check_environment_switch(exe, tmp_path):
    """S360_DEVICE_JPEG=1 switches the device path on; --device_jpeg=false on the command line wins; PNG outputs ignore both."""
    rig, imgs, names = prepare(tmp_path, 1)
    log = render(exe, rig, imgs, str(tmp_path / "env"), names, ".jpe", ".png", env={"S360_DEVICE_JPEG": "1"})
    assert path_line(log).count(ON_DEVICE) == 1 and "cubemap PNG" in path_line(log)
    log = render(exe, rig, imgs, str(tmp_path / "no"), names, ".jpe", ".png", ["--device_jpeg=false"], env={"S360_DEVICE_JPEG": "1"})
    assert path_line(log).count(ON_HOST) == 1 and ON_DEVICE not in log
    a, b = outputs(str(tmp_path / "env"), names, ".jpe", ".png"), outputs(str(tmp_path / "no"), names, ".jpe", ".png")
    assert a == b and a["eqr_%s.jpe" % names[0]][:2] == b"\xff\xd8" and a["cube_%s.png" % names[0]][:4] == b"\x89PNG"


def check_stream(exe, tmp_path, frames, more):
    """--num_frames (more: e.g. --num_streams) with a cubemap beside every frame: --device_jpeg on against off, all files identical."""
    rig, imgs, names = prepare(tmp_path, frames)
    render(exe, rig, imgs, str(tmp_path / "off"), names, ".jpg", ".jpg", more)
    log = render(exe, rig, imgs, str(tmp_path / "on"), names, ".jpg", ".jpg", list(more) + ["--device_jpeg"])
    assert path_line(log).count(ON_DEVICE) == 2
    off, on = outputs(str(tmp_path / "off"), names, ".jpg", ".jpg"), outputs(str(tmp_path / "on"), names, ".jpg", ".jpg")
    assert len(on) == 2 * frames and len(set(on.values())) == 2 * frames
    for k in off:
        FJ.same(on[k], off[k], k)


def check_mixed_outputs(exe, tmp_path):
    """.png equirect beside .jpg cubemap, both device flags, two frames: each file against its own oracle — the PNG's pixels are
    those of the host-encoded PNG, the JPEG is the oracle's file of the cubemap's pixels (a run with .png cubemaps)."""
    rig, imgs, names = prepare(tmp_path, 2)
    log = render(exe, rig, imgs, str(tmp_path / "mixed"), names, ".png", ".jpg", ["--device_png", "--device_jpeg"])
    assert "equirect PNG encoded on the device" in path_line(log) and "cubemap " + ON_DEVICE in path_line(log)
    render(exe, rig, imgs, str(tmp_path / "host"), names, ".png", ".png", ["--device_png=false"])
    for n in names:
        a = refprog.png_pixels_bgr(str(tmp_path / "mixed" / ("eqr_%s.png" % n)))
        assert np.array_equal(a, refprog.png_pixels_bgr(str(tmp_path / "host" / ("eqr_%s.png" % n))))
        assert_jpeg_of_png(open(str(tmp_path / "mixed" / ("cube_%s.jpg" % n)), "rb").read(), str(tmp_path / "host" / ("cube_%s.png" % n)), "cubemap " + n)


@pytest.fixture(scope="module")
def program(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    JC.host_tool()
    return os.path.join(ROOT, "host", "TestRenderStereoPanorama")


def test_one_frame_host_and_device(tmp_path, program):
    check_one_frame(program, tmp_path)


def test_environment_switch(tmp_path, program):
    check_environment_switch(program, tmp_path)


def test_num_frames_3(tmp_path, program):
    check_stream(program, tmp_path, 3, [])


def test_num_streams_2(tmp_path, program):
    check_stream(program, tmp_path, 4, ["--num_streams", "2"])


def test_mixed_outputs(tmp_path, program):
    check_mixed_outputs(program, tmp_path)
