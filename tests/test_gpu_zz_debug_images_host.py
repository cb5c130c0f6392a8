"""host/TestRenderStereoPanorama --save_debug_images and host/TestPoleRemoval against the REFERENCE'S OWN PROGRAM:
tests/golden/debug_images_golden.json holds the digests of every file oracle/_ref/TestRenderStereoPanorama writes under
debug/<frame>/ (outside flow_images/) with --save_debug_images for the cases of tests/debug_images_cases.py. The HIP program gets
the same integer-generated inputs and flags and must write exactly those files — every one present, none beside them, pixels and
shapes equal — while its equirect, cubemap, flows and state images stay those of tests/golden/refprogram_golden.json; the same
through the device PNG batch (--device_state_png), as a --num_frames stream, and refused for several streams. The check functions
take the program, so that tests/test_cpu_debug_images.py runs them on the emulation. (No reference involved at run time.)"""
import os
import subprocess

import pytest

import debug_images_cases as D
import refprog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(s360lib):
    subprocess.check_call(["make", "-C", os.path.join(D.ROOT, "host"), "-s"])
    return refprog.HOST_EXE


def check_case(exe, tmp_path, name, more_args=(), env=None):
    out = D.run_case(exe, str(tmp_path / "run"), D.small_rig(tmp_path), name, more_args=more_args, env=env)
    D.check_against_golden(out, name)
    if D.CASES[name][4]:
        D.check_other_outputs(out, name)
    return out


def check_device_batch(exe, tmp_path):
    """The odd-sized case with the files encoded on the device (flag, then environment switch): same digests; --v 1 names the path."""
    name = "odd_490x245"
    rig = D.small_rig(tmp_path)
    imgs, out, mdir = D.write_inputs(str(tmp_path / "flag"), rig, name)
    f = D.CASES[name][0][0]
    r = subprocess.run(D.command(exe, rig, name, imgs, out, mdir, f) + ["--device_state_png", "--v", "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    D.check_against_golden(out, name)
    n = len(D.golden()[name])
    assert "debug images:            %d files" % n in r.stderr and "encoded on the device in one batch" in r.stderr, r.stderr[-1500:]
    r = subprocess.run(D.command(exe, rig, name, imgs, out, mdir, f) + ["--v", "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "debug images:            %d files" % n in r.stderr and "encoded by the writers" in r.stderr, r.stderr[-1500:]
    D.check_against_golden(out, name)  # (over the first run's files: old projections are removed, the rest overwritten)
    check_case(exe, tmp_path / "env", name, env={"S360_DEVICE_STATE_PNG": "1"})


def check_stream(exe, tmp_path, more_args=()):
    """pole_removal as --num_frames 2: both frames' debug images are the chained reference runs'."""
    name = "pole_removal"
    out, _ = D.run_stream(exe, str(tmp_path / "stream"), D.small_rig(tmp_path), name, more_args=more_args)
    D.check_against_golden(out, name)
    want = __import__("json").load(open(refprog.GOLDEN))[name]
    for f in D.CASES[name][0]:
        assert refprog._digest_png(os.path.join(out, "eqr_%s.png" % f)) == want["eqr_%s" % f], f


def check_refused_with_streams(exe, tmp_path):
    name = "pole_removal"
    for more in (["--num_streams", "2"], ["--num_gpus", "2"]):
        out, r = D.run_stream(exe, str(tmp_path / more[0][2:]), D.small_rig(tmp_path), name, more_args=more, check=False)
        assert r.returncode not in (0, -6, 134), (r.returncode, r.stderr[-500:])
        lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
        assert len(lines) == 1 and "--save_debug_images" in lines[0] and "several contexts" in lines[0], r.stderr[-500:]
        for f in D.CASES[name][0]:
            assert D.debug_files(out, f) == [] and not os.path.exists(os.path.join(out, "eqr_%s.png" % f))
            assert os.listdir(os.path.join(out, "flow", f)) == [] and os.listdir(os.path.join(out, "debug", f, "flow_images")) == []


def check_missing_directory_is_a_write_error(exe, tmp_path):
    """The program makes no directories: without debug/<frame>/projections the first crop is the write error it is in the reference."""
    name = "odd_490x245"
    rig = D.small_rig(tmp_path)
    imgs, out, mdir = D.write_inputs(str(tmp_path / "nodir"), rig, name)
    f = D.CASES[name][0][0]
    os.rmdir(os.path.join(out, "debug", f, "projections"))
    r = subprocess.run(D.command(exe, rig, name, imgs, out, mdir, f), capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "projections/crop_" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not os.path.exists(os.path.join(out, "debug", f, "projections"))


def check_pole_removal_program(exe_pr, tmp_path):
    """TestPoleRemoval on the inputs of case pole_removal, frame 000000: its four files are that case's golden entries (the frame has
    no predecessor, like the program), in a directory it made itself; nothing else is written."""
    name = "pole_removal"
    rig = D.small_rig(tmp_path)
    imgs, _, mdir = D.write_inputs(str(tmp_path / "in"), rig, name)
    f = D.CASES[name][0][0]
    out = str(tmp_path / "pr_out")
    r = subprocess.run([exe_pr, "--src_images_dir", imgs, "--frame_number", f, "--pole_masks_dir", mdir, "--output_dir", out,
                        "--rig_json_file", rig, "--flow_alg", "pixflow_low", "--alpha_feather_size", "31", "--logbuflevel", "-1",
                        "--stderrthreshold", "0"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = ["_bottomCombined.png", "bottomImage.png", "bottomImage2.png", "bottomWarp2.png"]
    assert sorted(os.listdir(os.path.join(out, "debug", f))) == names and os.listdir(out) == ["debug"]
    want = D.golden()[name]
    for fn in names:
        assert refprog._digest_png(os.path.join(out, "debug", f, fn)) == want["%s/%s" % (f, fn)]["sha256"], fn
    r = subprocess.run([exe_pr, "--src_images_dir", imgs, "--frame_number", f], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "missing required command line argument: pole_masks_dir" in r.stderr


@pytest.mark.parametrize("name", list(D.CASES))
def test_debug_images_are_the_reference_programs(exe, tmp_path, name):
    check_case(exe, tmp_path, name)


def test_device_png_batch_writes_the_same_pixels(exe, tmp_path):
    check_device_batch(exe, tmp_path)


def test_stream_of_two_frames(exe, tmp_path):
    check_stream(exe, tmp_path)


def test_refused_with_several_streams_or_gpus(exe, tmp_path):
    check_refused_with_streams(exe, tmp_path)


def test_missing_directory_is_a_write_error(exe, tmp_path):
    check_missing_directory_is_a_write_error(exe, tmp_path)


def test_pole_removal_program(exe, tmp_path):
    check_pole_removal_program(D.HOST_POLE_REMOVAL, tmp_path)
