"""Shared by tests/golden/make_debug_images_golden.py, tests/test_gpu_zz_debug_images_host.py, tests/test_gpu_debug_images.py and
tests/test_cpu_debug_images.py: the cases of --save_debug_images, how a TestRenderStereoPanorama program is run over them, and
the digests of what it leaves under <output_data_dir>/debug/<frame>/ outside flow_images/.

tests/golden/debug_images_golden.json holds, per case and file, what the REFERENCE'S OWN PROGRAM (oracle/_ref/
TestRenderStereoPanorama) writes with --save_debug_images for the integer-generated inputs of tests/refprog.py: the SHA-256 of the
decoded pixels (refprog._digest_png) and their shape. Cases:
  sharpen_cubemap_search   refprog's: top + bottom, sharpening 0.25 (hence the _sharpened files)
  pole_removal             refprog's, both chained frames: the four pole-removal images, no top_* files, no _sharpened files
  odd_490x245              one frame with the flags of refprog's three_frames_sharpened at --eqr_width 490 --eqr_height 245: rows of
                           1960 (B,G,R,A) and 1470 (B,G,R) bytes, wrap shift 163, panoramas of 105 rows, pole images of 125 rows —
                           nothing is a multiple of 16 bytes"""
import json
import os
import subprocess

import numpy as np
from PIL import Image

import refprog

ROOT = refprog.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "debug_images_golden.json")
HOST_POLE_REMOVAL = os.path.join(ROOT, "host", "TestPoleRemoval")
# name -> (frames, flags, eqr_width, eqr_height, the case of refprogram_golden.json its other files are in or None)
CASES = {
    "sharpen_cubemap_search": (refprog.CASES["sharpen_cubemap_search"][0], refprog.CASES["sharpen_cubemap_search"][1], refprog.EQR_W, refprog.EQR_H,
                               "sharpen_cubemap_search"),
    "pole_removal": (refprog.CASES["pole_removal"][0], refprog.CASES["pole_removal"][1], refprog.EQR_W, refprog.EQR_H, "pole_removal"),
    "odd_490x245": (["000007"], refprog.CASES["three_frames_sharpened"][1], 490, 245, None),
}


def golden():
    return json.load(open(GOLDEN))


def small_rig(tmp):
    import rigutil
    os.makedirs(str(tmp), exist_ok=True)
    return rigutil.scaled_rig_json(os.path.join(ROOT, "tests", "golden", "rig_17cam.json"), os.path.join(str(tmp), "rig_small.json"),
                                   refprog.CAM / 2048.0)


def write_inputs(work, rig_path, name):
    """refprog.write_inputs, and debug/<frame>/projections: the caller of the program makes it (batch_process_video.py:132-135)."""
    frames, extra = CASES[name][:2]
    imgs, out, mdir = refprog.write_inputs(work, rig_path, frames, masks="--enable_pole_removal" in extra)
    for f in frames:
        os.makedirs(os.path.join(out, "debug", f, "projections"), exist_ok=True)
    return imgs, out, mdir


def command(exe, rig_path, name, imgs, out, mdir, frame, prev="NONE", equirect=None):
    frames, extra, w, h, _ = CASES[name]
    cmd = [exe, "--rig_json_file", rig_path, "--imgs_dir", imgs, "--frame_number", frame, "--output_data_dir", out,
           "--prev_frame_data_dir", prev, "--output_equirect_path", equirect or os.path.join(out, "eqr_%s.png" % frame),
           "--eqr_width", str(w), "--eqr_height", str(h), "--final_eqr_width", str(refprog.FINAL),
           "--final_eqr_height", str(refprog.FINAL), "--save_debug_images"] + extra
    if "--cubemap_width" in extra:
        cmd += ["--output_cubemap_path", os.path.join(out, "cube_%s.png" % (frame if equirect is None else "%s"))]
    if mdir:
        cmd += ["--bottom_pole_masks_dir", mdir]
    return cmd


def run_case(exe, work, rig_path, name, more_args=(), env=None, timeout=900):
    """The frames of a case, one process per frame, chained with --prev_frame_data_dir; returns the output directory."""
    imgs, out, mdir = write_inputs(work, rig_path, name)
    prev = "NONE"
    for f in CASES[name][0]:
        r = subprocess.run(command(exe, rig_path, name, imgs, out, mdir, f, prev) + list(more_args), capture_output=True, text=True,
                           timeout=timeout, env=dict(os.environ, **(env or {})))
        assert r.returncode == 0, "%s frame %s: rc %d\n%s" % (name, f, r.returncode, r.stderr[-2000:])
        prev = f
    return out


def run_stream(exe, work, rig_path, name, more_args=(), env=None, timeout=900, check=True):
    """The frames of a case as one --num_frames stream of host/TestRenderStereoPanorama; returns (output directory, the process)."""
    imgs, out, mdir = write_inputs(work, rig_path, name)
    frames = CASES[name][0]
    cmd = command(exe, rig_path, name, imgs, out, mdir, frames[0], equirect=os.path.join(out, "eqr_%s.png"))
    r = subprocess.run(cmd + ["--num_frames", str(len(frames))] + list(more_args), capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    if check:
        assert r.returncode == 0, "%s as a stream: rc %d\n%s" % (name, r.returncode, r.stderr[-2000:])
    return out, r


def debug_files(out, frame):
    """Paths relative to debug/<frame>/ of every file there outside flow_images/."""
    base = os.path.join(out, "debug", frame)
    found = []
    for dp, dn, fn in os.walk(base):
        rel = os.path.relpath(dp, base)
        if rel == "flow_images" or rel.startswith("flow_images" + os.sep):
            continue
        found += [os.path.normpath(os.path.join(rel, f)) for f in fn]
    return sorted(found)


def pixels_digest(a):
    """refprog._digest_png of an image already in memory, in the file's channel order (R,G,B[,A])."""
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()


def digests(out, name):
    """{"<frame>/<path under debug/<frame>/>": {"sha256": ..., "shape": [h, w, c]}} of a case's debug images."""
    d = {}
    for f in CASES[name][0]:
        for rel in debug_files(out, f):
            p = os.path.join(out, "debug", f, rel)
            d["%s/%s" % (f, rel)] = {"sha256": refprog._digest_png(p), "shape": list(np.asarray(Image.open(p)).shape)}
    return d


def check_against_golden(out, name, frames=None):
    """Every golden file present and equal; nothing under debug/<frame>/ outside flow_images/ that the golden does not list."""
    want = {k: v for k, v in golden()[name].items() if frames is None or k.split("/")[0] in frames}
    assert want
    got = {k: v for k, v in digests(out, name).items() if frames is None or k.split("/")[0] in frames}
    missing = sorted(set(want) - set(got))
    assert not missing, "%s: files the reference writes and this program does not: %s" % (name, missing)
    extra = sorted(set(got) - set(want))
    assert not extra, "%s: files the reference does not write: %s" % (name, extra)
    differing = sorted(k for k in want if got[k] != want[k])
    assert not differing, "%s: %d of %d debug images differ from the reference's: %s" % (name, len(differing), len(want), [
        (k, got[k]["shape"], want[k]["shape"]) for k in differing[:10]])


def check_other_outputs(out, name):
    """The equirect, cubemap, flows and state images of a case still equal tests/golden/refprogram_golden.json."""
    ref_name = CASES[name][4]
    want = json.load(open(refprog.GOLDEN))[ref_name]
    got = refprog.digests(out, ref_name)
    bad = sorted(k for k in want if got.get(k) != want[k])
    assert not bad, "%s: %d of %d outputs differ from the reference program's: %s" % (name, len(bad), len(want), bad[:10])

