"""host/TestRenderStereoPanorama --device_input_jpeg: the camera files of a .jpg imgs_dir are read as bytes and decoded on the device
straight into the frame's source slots (s360_frame_upload_jpeg, include/s360_input_jpeg.h) instead of being decoded on host threads
(host/jpeg_io.hpp) and uploaded as pixels. The imgs_dir is PIL's: the side cameras' files are <frame>.jpg, the pole cameras' files
keep the name <frame>.png the program asks for and hold JPEG bytes (the decoder is chosen by the signature, as imread does). The
oracle is the same program without the flag: every file it writes must be equal (the equirect's bytes, the state images' pixels,
the flow files), and the --v 1 line says how many files took which path. The check functions take the program's path:
tests/test_cpu_input_jpeg.py runs them on the program linked against the emulated library."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import input_jpeg_cases as IJ
import refprog
import rigutil
import test_gpu_zz_input_png_host as Z

pytestmark = pytest.mark.gpu

ROOT = refprog.ROOT
FLAG = ["--device_input_jpeg"]


def prepare(tmp_path, nframes, sampling=2, host_camera=None):
    """(rig, imgs_dir, frame names): the small rig's 17 cameras as JPEG files, quality 95. host_camera: the index of a side camera
    whose file is written with restart markers: not the device decoder's, and one the host decoder reads. (A progressive file is
    refused by s360_input_jpeg_decodable just the same — tests/test_cpu_input_jpeg.py — but host/jpeg_io.hpp does not read it, so a
    directory that holds one cannot be rendered with or without the flag.)"""
    rig = rigutil.scaled_rig_json(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"), refprog.CAM / 2048.0)
    side_ids, _, _ = refprog.rig_ids(rig)
    idir = tmp_path / "rgb"
    names = ["%06d" % f for f in range(nframes)]
    for f, name in enumerate(names):
        for cid, img in refprog.frame_images(rig, f).items():
            os.makedirs(str(idir / cid), exist_ok=True)
            if cid in side_ids and host_camera is not None and side_ids.index(cid) == host_camera:
                Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(str(idir / cid / (name + ".jpg")), quality=95, subsampling=sampling, restart_marker_blocks=5)
            else:
                (idir / cid / (name + (".jpg" if cid in side_ids else ".png"))).write_bytes(IJ.pil_encode(img, 95, sampling, False))
    return rig, str(idir), names


def check_single_frame(exe, tmp_path):
    """One frame of a 4:2:0 directory with the flag, without it, with the environment switch, and with the switch overruled by the
    flag: all camera files on the device path, the same files written."""
    rig, imgs, names = prepare(tmp_path, 1)
    off = Z.render(exe, rig, imgs, str(tmp_path / "off"), names[0])
    assert "camera images:" not in off
    on = Z.render(exe, rig, imgs, str(tmp_path / "on"), names[0], FLAG)
    assert "--device_input_jpeg" in on and Z.decoded_where(on) == (Z.used(rig), 0)
    assert refprog.png_pixels_bgr(str(tmp_path / "off" / "eqr_000000.png")).std() > 5
    Z.assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60)
    env = Z.render(exe, rig, imgs, str(tmp_path / "env"), names[0], env={"S360_DEVICE_INPUT_JPEG": "1"})
    assert Z.decoded_where(env) == (Z.used(rig), 0)
    Z.assert_same(str(tmp_path / "off"), str(tmp_path / "env"), 60)
    both = Z.render(exe, rig, imgs, str(tmp_path / "both"), names[0], FLAG + ["--device_input_png"])  # a directory may hold either kind
    assert Z.decoded_where(both) == (Z.used(rig), 0)
    Z.assert_same(str(tmp_path / "off"), str(tmp_path / "both"), 60)
    overruled = Z.render(exe, rig, imgs, str(tmp_path / "no"), names[0], ["--device_input_jpeg=false"], env={"S360_DEVICE_INPUT_JPEG": "1"})
    assert "camera images:" not in overruled


def check_fallback_per_file(exe, tmp_path):
    """One side camera's file has restart markers: it takes the host decoder, the other sixteen the device, and nothing in the
    output changes. 4:4:4 files here."""
    rig, imgs, names = prepare(tmp_path, 1, sampling=0, host_camera=3)
    off = Z.render(exe, rig, imgs, str(tmp_path / "off"), names[0])
    on = Z.render(exe, rig, imgs, str(tmp_path / "on"), names[0], FLAG)
    assert "camera images:" not in off and Z.decoded_where(on) == (Z.used(rig) - 1, 1)
    Z.assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60)


def check_stream(exe, tmp_path, more, frames=2):
    """--num_frames in one process (more: e.g. --num_streams), with and without the flag."""
    rig, imgs, names = prepare(tmp_path, frames, sampling=1)
    for tag, flag in (("off", []), ("on", FLAG)):
        log = Z.render(exe, rig, imgs, str(tmp_path / tag), names[0], list(more) + flag, num_frames=frames)
        if flag:
            assert Z.decoded_where(log) == (frames * Z.used(rig), 0)
    for f in names:
        assert os.path.exists(str(tmp_path / "on" / ("eqr_%s.png" % f)))
    Z.assert_same(str(tmp_path / "off"), str(tmp_path / "on"), 60 + frames)


@pytest.fixture(scope="module")
def program(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    return os.path.join(ROOT, "host", "TestRenderStereoPanorama")


def test_single_frame(tmp_path, program):
    check_single_frame(program, tmp_path)


def test_fallback_is_per_file(tmp_path, program):
    check_fallback_per_file(program, tmp_path)


def test_num_frames_2(tmp_path, program):
    check_stream(program, tmp_path, [])


def test_num_streams_2(tmp_path, program):
    check_stream(program, tmp_path, ["--num_streams", "2"])
