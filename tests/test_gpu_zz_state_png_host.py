"""host/TestRenderStereoPanorama --device_state_png: the state images a frame leaves for the next one (overlap_<i>_{L,R}.png,
extendedSideSpherical_*, extendedFisheyeSpherical_*, bottomImage{,2}.png) are encoded on the device by one batched launch
sequence per context (s360_frame_encode_state_pngs) and the program only writes the bytes. Every file of the chained
single-frame processes must still be what the REFERENCE'S OWN PROGRAM wrote (tests/golden/refprogram_golden.json, cases of
tests/refprog.py) — state PNGs compared by decoded pixels, and frame 1 has been resumed from frame 0's device-encoded files
through the banded reader of host/png_io.hpp. The check functions take the program, so that tests/test_cpu_state_png.py runs
them on tools/emu/TestRenderStereoPanorama."""
import glob
import hashlib
import json
import os
import subprocess

import pytest

import refprog
import rigutil
import test_gpu_png as T

pytestmark = pytest.mark.gpu

FLAG = ["--device_state_png"]


def _rig(tmp_path):
    return rigutil.scaled_rig_json(os.path.join(refprog.ROOT, "tests", "golden", "rig_17cam.json"), str(tmp_path / "rig_small.json"),
                                   refprog.CAM / 2048.0)


def state_pngs(out, frame):
    return sorted(glob.glob(os.path.join(out, "debug", frame, "flow_images", "*.png")))


def assert_device_encoded(out, frame, at_least=30):
    """Every state PNG of the frame carries the band chunk "sbNd" and colour type 6."""
    files = state_pngs(out, frame)
    assert len(files) >= at_least
    for p in files:
        ch = T.chunks(open(p, "rb").read())
        assert ch[0][0] == b"IHDR" and ch[0][1][8:10] == bytes([8, 6]) and ch[1][0] == b"sbNd", p


def check_chained_case(exe, tmp_path, name, more_args=(), env=None):
    """The case's frames as chained single-frame processes with the device encoder: the reference program's digests, file for file."""
    out = refprog.run_case(exe, str(tmp_path), _rig(tmp_path), name, more_args=list(more_args), env=env)
    got = refprog.digests(out, name)
    golden = json.load(open(refprog.GOLDEN))[name]
    assert sorted(got) == sorted(golden)
    differing = sorted(k for k in golden if got[k] != golden[k])
    assert not differing, "%d of %d files differ from the reference program's: %s" % (len(differing), len(golden), differing[:12])
    for f in refprog.CASES[name][0]:
        assert_device_encoded(out, f)
    return out


def state_digests(out, frame):
    d = {}
    for folder in (os.path.join(out, "flow", frame), os.path.join(out, "debug", frame, "flow_images")):
        for fn in sorted(os.listdir(folder)):
            p = os.path.join(folder, fn)
            d[fn] = refprog._digest_png(p) if fn.endswith(".png") else hashlib.sha256(open(p, "rb").read()).hexdigest()
    return d


def check_stream_state(exe, tmp_path, more_args=()):
    """two_frames as one process (--num_frames 2, or with more_args --num_streams 2): the state files behind each last frame are
    digest-equal with and without the flag, and with the flag they are the device's files."""
    rig = _rig(tmp_path)
    name = "two_frames"
    frames = refprog.CASES[name][0]
    on = refprog.run_stream(exe, str(tmp_path / "on"), rig, name, more_args=list(more_args) + FLAG)
    off = refprog.run_stream(exe, str(tmp_path / "off"), rig, name, more_args=list(more_args))
    last = frames if "--num_streams" in more_args else frames[-1:]
    for f in last:
        a, b = state_digests(on, f), state_digests(off, f)
        assert len(a) > 60 and a == b, "frame %s: %s" % (f, sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))[:8])
        assert_device_encoded(on, f)
    for f in frames:
        assert refprog._digest_png(os.path.join(on, "eqr_%s.png" % f)) == refprog._digest_png(os.path.join(off, "eqr_%s.png" % f)), f


def check_environment_switch(exe, tmp_path):
    """S360_DEVICE_STATE_PNG=1 without the flag writes the same FILES (bytes) as the flag."""
    rig = _rig(tmp_path)
    name = "two_frames"
    a = refprog.run_stream(exe, str(tmp_path / "flag"), rig, name, more_args=FLAG)
    b = refprog.run_stream(exe, str(tmp_path / "env"), rig, name, env=dict(os.environ, S360_DEVICE_STATE_PNG="1"))
    f = refprog.CASES[name][0][-1]
    fa, fb = state_pngs(a, f), state_pngs(b, f)
    assert len(fa) >= 30 and [os.path.basename(p) for p in fa] == [os.path.basename(p) for p in fb]
    for pa, pb in zip(fa, fb):
        assert open(pa, "rb").read() == open(pb, "rb").read(), pa
    assert_device_encoded(b, f)


@pytest.fixture(scope="module")
def host_exe(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(refprog.ROOT, "host"), "-s"])
    return refprog.HOST_EXE


@pytest.mark.parametrize("name", ["two_frames", "pole_removal"])
def test_chained_processes_write_the_reference_programs_files(tmp_path, host_exe, name):
    check_chained_case(host_exe, tmp_path, name, FLAG)


@pytest.mark.parametrize("mode", ["num_frames", "num_streams"])
def test_state_behind_a_streams_last_frame(tmp_path, host_exe, mode):
    check_stream_state(host_exe, tmp_path, ["--num_streams", "2"] if mode == "num_streams" else [])


def test_environment_switch(tmp_path, host_exe):
    check_environment_switch(host_exe, tmp_path)
