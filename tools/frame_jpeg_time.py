#!/usr/bin/env python
"""What the finished frame costs as a JPEG file (include/s360_frame_jpeg.h, host/TestRenderStereoPanorama --device_jpeg) at the 8K
preset (8400 x 4096 eyes -> an 8192 x 8192 stereo frame), on one MI355X:
  1. device time per frame of the JPEG encode and of the PNG encode of the SAME frames (both switches on, the profile families
     "jpeg_encode" and "png_encode": hipEvents on the stream that renders), warm, median of `--reps`; beside them one host thread's
     jpegio::encode of the same pixels (tools/jpeg_host_time), and the sizes of the three files.
  2. peak device memory of one context with the JPEG switch off and on (hipMemGetInfo around a context that renders two frames).
  3. host/TestRenderStereoPanorama --num_streams 8 from a capture's .bin container, `--rounds` alternating rounds of: .png outputs
     with --device_png (what existed), .jpg outputs with --device_jpeg, .jpg outputs encoded on the host: the program's "steady
     state" frames per second (files written) and the bytes written per frame.
The camera images are the synthetic ones of the other timing tools (surround360_amd.synth). Every run of the program keeps a time
limit of its own (--timeout).
usage: python tools/frame_jpeg_time.py [--rounds 3] [--reps 12] [--out profiles/frame_jpeg.txt] [--skip-streams]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--streams", type=int, default=8)
ap.add_argument("--frames-per-stream", type=int, default=4)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_jpeg.txt"))
ap.add_argument("--skip-streams", action="store_true")
ap.add_argument("--timeout", type=int, default=240)
ap.add_argument("--program", default=os.path.join(ROOT, "host", "TestRenderStereoPanorama"))
ap.add_argument("--torch-device", default="cuda")  # (where the synthetic camera images are made)
args = ap.parse_args()

W, H = (int(v) for v in args.eqr.split("x"))
flags = dict(eqr_width=W, eqr_height=H, enable_top=1, enable_bottom=1, final_eqr_width=args.final, final_eqr_height=args.final, sharpening=0.25)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def save():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def spread(v, fmt="%.3f"):
    return (fmt + " (" + fmt + ".." + fmt + ")") % (statistics.median(v), min(v), max(v))


cuda = args.torch_device == "cuda"
dev = torch.device("cuda", 0) if cuda else torch.device(args.torch_device)
rr = synth.RigRenderer(args.rig, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
nf = args.streams * args.frames_per_stream
frames = [rr.frame_numpy(yaw_deg=1.5 * k, disc_deg=10.0) for k in range(2 if args.skip_streams else nf)]
del rr
if cuda:
    torch.cuda.empty_cache()
subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "jpeg_host_time"])
work = tempfile.mkdtemp(prefix="s360_frame_jpeg_")
say("# the finished frame as a JPEG file: eyes %d x %d -> %d x %d stereo frame, quality 95, sharpening 0.25" % (W, H, args.final, args.final))


def free_bytes():
    return torch.cuda.mem_get_info(0)[0] if cuda else 0


try:
    # ---- 2. memory (first: nothing of this process is on the device yet but torch's own) ------------------------------------------
    say("## 2. device memory of one context (one slot, two frames rendered, PNG encoder on in both), hipMemGetInfo before / after")
    used = {}
    for form in ("off", "on", "off", "on"):
        before = free_bytes()
        c = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
        c.set_png_encode(True)
        c.set_jpeg_encode(form == "on", 95)
        for k in range(2):
            c.upload_frame(*frames[k])
            c.render(k > 0)
        c.synchronize()
        used.setdefault(form, []).append((before - free_bytes()) / 1e6)
        c.close()
        del c
    for form in ("off", "on"):
        say("JPEG switch %-3s: %s MB" % (form, " ".join("%.1f" % v for v in used[form])))
    say("the switch adds %.1f MB (second round): the encoder's scratch 201 + 326 + 13 MB and one scan buffer of 201 MB" % (used["on"][1] - used["off"][1]))
    save()

    # ---- 1. device time ---------------------------------------------------------------------------------------------------------------
    ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
    ctx.set_png_encode(True)
    ctx.set_jpeg_encode(True, 95)
    for k in range(2):  # warm-up: buffers, maps, code objects
        ctx.upload_frame(*frames[k])
        ctx.render(k > 0)
    ctx.synchronize()
    tj, tp = [], []
    for rep in range(args.reps):
        ctx.upload_frame(*frames[rep & 1])
        ctx.profile_enable(True)
        ctx.render(True)
        ctx.synchronize()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        assert prof["jpeg_encode"][1] == 1 and prof["png_encode"][1] == 1
        tj.append(prof["jpeg_encode"][0])
        tp.append(prof["png_encode"][0])
    px = ctx.download_equirect()
    jpg = ctx.download_jpeg().tobytes()
    png = ctx.download_png().tobytes()
    raw = os.path.join(work, "frame.bgr")
    px.tofile(raw)
    r = subprocess.run([os.path.join(ROOT, "tools", "jpeg_host_time"), raw, str(px.shape[1]), str(px.shape[0]), "3", "95"], capture_output=True, text=True,
                       timeout=args.timeout, check=True)
    th = [float(ln.split()[0]) for ln in r.stdout.splitlines()]
    host_bytes = int(r.stdout.split()[1])
    say("## 1. per %d x %d frame, the same %d frames through both device encoders (ms, median (min..max))" % (px.shape[1], px.shape[0], args.reps))
    say("JPEG encode on the device (profile family jpeg_encode):  %s   file %d bytes" % (spread(tj), len(jpg)))
    say("PNG encode on the device (profile family png_encode):    %s   file %d bytes" % (spread(tp), len(png)))
    say("jpegio::encode on one host thread, %d encodes:            %s   file %d bytes (%s the device's)" % (
        len(th), spread(th, "%.0f"), host_bytes, "the same size as" if host_bytes == len(jpg) else "NOT the size of"))
    say("JPEG encode below the PNG encode in every repetition: %s" % ("yes" if all(a < b for a, b in zip(tj, tp)) else "NO"))
    save()
    ctx.close()
    del ctx
    if cuda:
        torch.cuda.empty_cache()

    # ---- 3. the program ---------------------------------------------------------------------------------------------------------------
    if not args.skip_streams:
        from bench import write_capture_container
        cams = json.load(open(args.rig))["cameras"]
        side_ids = [c["id"] for c in cams if "side" in c.get("group", "")]
        other = [c for c in cams if "side" not in c.get("group", "")]
        ids = side_ids + [max(other, key=lambda c: c["forward"][2])["id"], min(other, key=lambda c: c["forward"][2])["id"]]
        by_id = [dict(zip(ids, list(side) + [top, bottom])) for side, top, bottom in frames]
        binp, ispd = os.path.join(work, "0.bin"), os.path.join(work, "isp")
        write_capture_container(binp, ispd, ids, by_id)
        del by_id, frames

        def run(form):
            ext, more = {"png_device": (".png", ["--device_png"]), "jpg_device": (".jpg", ["--device_jpeg"]), "jpg_host": (".jpg", ["--device_jpeg=false"])}[form]
            out = os.path.join(work, "out_" + form)
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out)
            cmd = [args.program, "--rig_json_file", args.rig, "--bin_list", binp, "--isp_dir", ispd, "--frame_number", "000000", "--num_frames", str(nf),
                   "--num_streams", str(args.streams), "--stream_gpus", "1", "--output_data_dir", out, "--prev_frame_data_dir", "NONE",
                   "--output_equirect_path", os.path.join(out, "eqr_%s" + ext), "--sharpening", "0.25", "--enable_top", "--enable_bottom",
                   "--write_state=false", "--v", "1"] + more
            for k in ("eqr_width", "eqr_height", "final_eqr_width", "final_eqr_height"):
                cmd += ["--" + k, str(flags[k])]
            env = dict(os.environ)
            env.pop("S360_DEVICE_JPEG", None)
            t = time.perf_counter()
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout, env=env)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
            m = re.search(r"^steady state:\s+(.*\(([0-9.]+) frames per second.*)$", r.stderr, re.M)
            files = [os.path.join(out, f) for f in sorted(os.listdir(out)) if f.startswith("eqr_")]
            assert len(files) == nf
            return wall, float(m.group(2)) if m else float("nan"), sum(os.path.getsize(f) for f in files) // nf, files

        say("## 3. --num_streams %d from a .bin container, %d frames, %d alternating rounds" % (args.streams, nf, args.rounds))
        say("%-5s %-11s %8s %10s %16s" % ("round", "outputs", "wall s", "frames/s", "bytes per frame"))
        fps = {}
        last = {}
        for rnd in range(args.rounds):
            for form in ("png_device", "jpg_device", "jpg_host"):
                wall, f, nbytes, files = run(form)
                fps.setdefault(form, []).append(f)
                say("%-5d %-11s %8.2f %10.2f %16d" % (rnd, form, wall, f, nbytes))
                if form != "png_device":
                    last[form] = [open(p, "rb").read() for p in (files[0], files[-1])]
                save()
        say("the .jpg files of the device path and of the host path are the same bytes (first and last frame): %s" % (
            "yes" if last["jpg_device"] == last["jpg_host"] else "NO"))
        for a, b in (("jpg_device", "png_device"), ("jpg_device", "jpg_host")):
            say("%s above %s in every round: %s (%.2f..%.2f against %.2f..%.2f frames/s)" % (
                a, b, "yes" if all(x > y for x, y in zip(fps[a], fps[b])) else "NO", min(fps[a]), max(fps[a]), min(fps[b]), max(fps[b])))
        save()
finally:
    shutil.rmtree(work, ignore_errors=True)
save()
