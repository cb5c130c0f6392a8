"""host/TestRenderStereoPanorama --output_cubemap_path with --num_frames N > 1 and --num_streams: the cubemap of EVERY frame, as the
reference's per-frame caller asks for it (scripts/batch_process_video.py:40-47), from one process. The files must be what the
REFERENCE'S OWN PROGRAM wrote in chained single-frame processes (tests/golden/refprogram_golden.json, cases of tests/refprog.py).
The check functions take the program, so that tests/test_cpu_cubemap_stream.py runs them on tools/emu/TestRenderStereoPanorama."""
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import refprog
import rigutil

pytestmark = pytest.mark.gpu


def _rig(tmp_path):
    return rigutil.scaled_rig_json(os.path.join(refprog.ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"),
                                   refprog.CAM / 2048.0)


def run_stream_with_cubemaps(exe, work, rig, name, more_args=(), cube_pattern="cube_%s.png", expect_ok=True):
    """The frames of a refprog case as --num_frames N in one process with a cubemap path; returns (output directory, process)."""
    frames, extra = refprog.CASES[name]
    imgs, out, mdir = refprog.write_inputs(work, rig, frames, masks="--enable_pole_removal" in extra)
    cmd = [exe, "--rig_json_file", rig, "--imgs_dir", imgs, "--frame_number", frames[0], "--num_frames", str(len(frames)),
           "--output_data_dir", out, "--output_equirect_path", os.path.join(out, "eqr_%s.png"),
           "--output_cubemap_path", os.path.join(out, cube_pattern),
           "--eqr_width", str(refprog.EQR_W), "--eqr_height", str(refprog.EQR_H), "--final_eqr_width", str(refprog.FINAL),
           "--final_eqr_height", str(refprog.FINAL)] + extra + list(more_args)
    if "--logbuflevel" in extra:
        cmd += ["--log_dir", os.path.join(out, "logs")]
    if mdir:
        cmd += ["--bottom_pole_masks_dir", mdir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    if expect_ok:
        assert r.returncode == 0, "%s as a stream with cubemaps: rc %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    return out, r


def check_stream_cubemaps(exe, tmp_path, name, more_args=()):
    """cube_<frame>.png (and eqr_<frame>.png) of every frame of the stream: the reference program's digests."""
    out, _ = run_stream_with_cubemaps(exe, str(tmp_path), _rig(tmp_path), name, more_args)
    golden = json.load(open(refprog.GOLDEN))[name]
    for f in refprog.CASES[name][0]:
        assert refprog._digest_png(os.path.join(out, "cube_%s.png" % f)) == golden["cube_%s" % f], "cube " + f
        assert refprog._digest_png(os.path.join(out, "eqr_%s.png" % f)) == golden["eqr_%s" % f], "eqr " + f


def check_two_streams_cubemaps(exe, tmp_path, more_args=()):
    """--num_streams 2 --num_frames 2: two streams of one frame each. cube_000000 is the reference program's; cube_000001 is the
    oracle's cubemap of that frame rendered WITHOUT a predecessor (a stream's first frame has none)."""
    import oracle_lib as O
    name = "two_frames"
    rig = _rig(tmp_path)
    out, _ = run_stream_with_cubemaps(exe, str(tmp_path), rig, name, ["--num_streams", "2"] + list(more_args))
    golden = json.load(open(refprog.GOLDEN))[name]
    assert refprog._digest_png(os.path.join(out, "cube_000000.png")) == golden["cube_000000"]
    cams, _ = O.load_rig(rig)
    of = O.Frame(cams, O.make_params(eqr_width=refprog.EQR_W, eqr_height=refprog.EQR_H, final_eqr_width=refprog.FINAL,
                                     final_eqr_height=refprog.FINAL, enable_top=1, enable_bottom=1, sharpening=0.0))
    side_ids, top_id, bottoms = refprog.rig_ids(rig)
    imgs = refprog.frame_images(rig, 1)
    want_eq, _ = of.render([imgs[c] for c in side_ids], imgs[top_id], imgs[bottoms[0]])
    got = np.asarray(Image.open(os.path.join(out, "cube_000001.png")))[:, :, ::-1]
    assert np.array_equal(got, of.cubemap(96, 96, "video"))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "eqr_000001.png")))[:, :, ::-1], want_eq)
    assert refprog._digest_png(os.path.join(out, "cube_000001.png")) != golden["cube_000001"]  # (the chained frame differs)


def check_bad_command_line(exe, tmp_path):
    """A cubemap path without a placeholder and N > 1: every frame would be written to one name."""
    out, r = run_stream_with_cubemaps(exe, str(tmp_path), _rig(tmp_path), "two_frames", cube_pattern="cube.png", expect_ok=False)
    assert r.returncode != 0
    assert "--output_cubemap_path" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(os.path.join(out, "cube.png"))


@pytest.fixture(scope="module")
def host_exe(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(refprog.ROOT, "host"), "-s"])
    return refprog.HOST_EXE


@pytest.mark.parametrize("device_png", [False, True], ids=["save_png", "device_png"])
def test_two_frames_as_a_stream(tmp_path, host_exe, device_png):
    check_stream_cubemaps(host_exe, tmp_path, "two_frames", ["--device_png"] if device_png else [])


def test_pole_removal_photo_as_a_stream(tmp_path, host_exe):
    check_stream_cubemaps(host_exe, tmp_path, "pole_removal")


def test_two_streams(tmp_path, host_exe):
    check_two_streams_cubemaps(host_exe, tmp_path)


def test_cubemap_path_without_placeholder(tmp_path, host_exe):
    check_bad_command_line(host_exe, tmp_path)
