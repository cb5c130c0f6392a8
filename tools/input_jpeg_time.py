#!/usr/bin/env python
"""What reading the camera images of one 8K frame (14 side, top, bottom: 16 files of 2048 x 2048, baseline JPEG files written by PIL at
quality 95, 4:2:0 and 4:4:4) costs with the device decoder (include/s360_input_jpeg.h), on an MI355X:
  1. device time of the 16-file batch (s360_decode_input_jpeg_batch): the entropy stage's and the pixel stage's times from
     s360_jpeg_decode_stats (hipEvents; the entropy stage's time includes the host's round trips between the synchronisation
     launches), warm, median of `--reps`, with the launches and the decode passes per file; the same for other subsequence lengths
     (the library's developer switch S360_JPEG_SUB_BITS); and the wall time of s360_frame_upload_jpeg for the same files.
  2. host/TestRenderStereoPanorama, one process per frame, without and with --device_input_jpeg, alternating, `--rounds` rounds:
     the "load + decode + upload" line of its --v 1 breakdown and the process's wall time.
  3. --num_streams 8 over `--stream-frames` frames, without and with the flag, alternating, `--rounds` rounds: the "steady state"
     frames per second (files written).
The comparison is the same binary with the flag off. The camera images are the synthetic ones of tools/input_png_time.py
(surround360_amd.synth). Every run of the program keeps a time limit of its own (--timeout).
usage: python tools/input_jpeg_time.py [--rounds 3] [--out profiles/input_jpeg.txt] [--skip-host] [--skip-streams]"""
import argparse
import io
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
from PIL import Image  # noqa: E402
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--quality", type=int, default=95)
ap.add_argument("--stream-frames", type=int, default=32)
ap.add_argument("--sub-bits", default="1024,4096,8192,16384,65536")
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_jpeg.txt"))
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--skip-streams", action="store_true")
ap.add_argument("--timeout", type=int, default=240)
ap.add_argument("--program", default=os.path.join(ROOT, "host", "TestRenderStereoPanorama"))
ap.add_argument("--torch-device", default="cuda")  # (where the synthetic camera images are made)
args = ap.parse_args()

W, H = (int(v) for v in args.eqr.split("x"))
flags = dict(eqr_width=W, eqr_height=H, enable_top=1, enable_bottom=1, final_eqr_width=args.final, final_eqr_height=args.final, sharpening=0.25)
SAMPLINGS = (("4:2:0", 2), ("4:4:4", 0))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def save():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def jpeg(bgr, sampling):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=args.quality, subsampling=sampling)
    return b.getvalue()


dev = torch.device(args.torch_device, 0) if args.torch_device == "cuda" else torch.device(args.torch_device)
rr = synth.RigRenderer(args.rig, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
frames = [rr.frame_numpy(yaw_deg=1.5 * k, disc_deg=10.0) for k in range(2)]
del rr
if args.torch_device == "cuda":
    torch.cuda.empty_cache()

# ---- the files ------------------------------------------------------------------------------------------------------------------
n_side = len(frames[0][0])
cams = list(range(n_side)) + [-1, -2]
files = {}  # per sampling, per frame: the files
for name, s in SAMPLINGS:
    files[name] = [[jpeg(np.ascontiguousarray(a[..., :3]), s) for a in list(side) + [top, bottom]] for side, top, bottom in frames]
say("# camera images of one frame from baseline JPEG files (PIL, quality %d): %d files of %d x %d (eyes %d x %d)" % (
    args.quality, len(cams), args.cam, args.cam, W, H))

# ---- 1. device time ---------------------------------------------------------------------------------------------------------------
ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
say("## 1. device time of the %d-file batch (s360_decode_input_jpeg_batch), warm, median of %d" % (len(cams), args.reps))
say("%-6s %8s %10s %8s %9s %12s %14s %10s %10s  %s" % ("sampl.", "S bits", "files MB", "subseq.", "launches", "entropy ms", "(min..max)", "pixels ms", "call ms",
                                                       "decode passes per file"))
for name, s in SAMPLINGS:
    fs = files[name][0]
    want = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(fs[3])).convert("RGB"))[..., ::-1])
    for sub in ["default"] + [v for v in args.sub_bits.split(",") if v]:
        if sub == "default":
            os.environ.pop("S360_JPEG_SUB_BITS", None)
        else:
            os.environ["S360_JPEG_SUB_BITS"] = sub
        got = ctx.decode_input_jpeg_batch(fs)  # (first call: buffers are allocated)
        assert np.array_equal(got[3], want)
        te, tp, tw = [], [], []
        for rep in range(args.reps):
            t = time.perf_counter()
            ctx.decode_input_jpeg_batch(fs)
            tw.append((time.perf_counter() - t) * 1e3)
            st = ctx.jpeg_decode_stats()
            te.append(st["ms_entropy"])
            tp.append(st["ms_pixels"])
        say("%-6s %8s %10.1f %8d %9d %12.3f %14s %10.3f %10.1f  %s" % (
            name, sub, sum(len(f) for f in fs) / 1e6, st["subsequences"], st["rounds"], statistics.median(te), "%.3f..%.3f" % (min(te), max(te)),
            statistics.median(tp), statistics.median(tw), " ".join(str(v) for v in st["file_rounds"])))
        save()
    os.environ.pop("S360_JPEG_SUB_BITS", None)
    ctx.upload_jpeg(cams, fs)  # (first call: the slots are allocated)
    tw = []
    for rep in range(5):
        t = time.perf_counter()
        ctx.upload_jpeg(cams, files[name][rep & 1])
        tw.append((time.perf_counter() - t) * 1e3)
    say("       s360_frame_upload_jpeg of the same files (copy, decode into the source slots, wait): %.1f ms median of 5 (%.1f..%.1f)" % (
        statistics.median(tw), min(tw), max(tw)))
    save()
ctx.close()
del ctx
if args.torch_device == "cuda":
    torch.cuda.empty_cache()

# ---- 2. and 3. the host program --------------------------------------------------------------------------------------------------
if not args.skip_host:
    rig_cams = json.load(open(args.rig))["cameras"]
    side_ids = [c["id"] for c in rig_cams if "side" in c.get("group", "")]
    other = [c for c in rig_cams if "side" not in c.get("group", "")]
    top_id = max(other, key=lambda c: c["forward"][2])["id"]
    bot_id = min(other, key=lambda c: c["forward"][2])["id"]
    ids = side_ids + [top_id, bot_id]
    work = tempfile.mkdtemp(prefix="s360_input_jpeg_")
    try:
        imgs = {}
        for name, _ in SAMPLINGS:
            imgs[name] = os.path.join(work, "rgb" + name.replace(":", ""))
            for cid_i, cid in enumerate(ids):
                os.makedirs(os.path.join(imgs[name], cid), exist_ok=True)
                ext = ".jpg" if cid in side_ids else ".png"  # (the program asks for the pole cameras' files by that name; JPEG bytes inside)
                for k in range(2):
                    with open(os.path.join(imgs[name], cid, "%06d%s" % (k, ext)), "wb") as f:
                        f.write(files[name][k][cid_i])
                for k in range(2, args.stream_frames):  # a stream's later frames are the first two again
                    os.symlink("%06d%s" % (k & 1, ext), os.path.join(imgs[name], cid, "%06d%s" % (k, ext)))

        def run(out, name, more, num_frames=None):
            for k in range(num_frames or 1):
                os.makedirs(os.path.join(out, "debug", "%06d" % k, "flow_images"), exist_ok=True)
                os.makedirs(os.path.join(out, "flow", "%06d" % k), exist_ok=True)
            cmd = [args.program, "--rig_json_file", args.rig, "--imgs_dir", imgs[name], "--frame_number", "000000", "--output_data_dir", out,
                   "--prev_frame_data_dir", "NONE", "--output_equirect_path", os.path.join(out, "eqr_%s.png"),
                   "--sharpening", "0.25", "--enable_top", "--enable_bottom", "--v", "1"]
            for k in ("eqr_width", "eqr_height", "final_eqr_width", "final_eqr_height"):
                cmd += ["--" + k, str(flags[k])]
            if num_frames:
                cmd += ["--num_frames", str(num_frames)]
            t = time.perf_counter()
            r = subprocess.run(cmd + more, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
            return wall, r.stderr

        say("## 2. one process per frame, --device_input_jpeg off and on, %d alternating rounds (seconds)" % args.rounds)
        say("%-6s %-5s %-5s %8s %24s  %s" % ("sampl.", "round", "flag", "wall", "load + decode + upload", "split"))
        for name, _ in SAMPLINGS:
            rows = {"off": [], "on": []}
            for rnd in range(args.rounds):
                for form, more in (("off", []), ("on", ["--device_input_jpeg"])):
                    out = os.path.join(work, "out_%s_%s" % (name.replace(":", ""), form))
                    wall, log = run(out, name, more)
                    m = re.search(r"^load \+ decode \+ upload:\s+([0-9.]+)\s*(.*)$", log, re.M)
                    rows[form].append((wall, float(m.group(1))))
                    say("%-6s %-5d %-5s %8.3f %24.3f  %s" % (name, rnd, form, wall, float(m.group(1)), m.group(2)))
                    save()
            for what, col in (("load + decode + upload", 1), ("wall time", 0)):
                a, b = [r[col] for r in rows["on"]], [r[col] for r in rows["off"]]
                say("%s: %s with the flag below without it in every round: %s (%.3f..%.3f s against %.3f..%.3f s)" % (
                    name, what, "yes" if all(x < y for x, y in zip(a, b)) else "NO", min(a), max(a), min(b), max(b)))
            same = open(os.path.join(work, "out_%s_on" % name.replace(":", ""), "eqr_000000.png"), "rb").read() == \
                open(os.path.join(work, "out_%s_off" % name.replace(":", ""), "eqr_000000.png"), "rb").read()
            say("%s: the equirect files of the two forms are the same bytes: %s" % (name, "yes" if same else "NO"))
            save()

        if not args.skip_streams:
            say("## 3. --num_streams 8, %d frames, flag off and on, %d alternating rounds" % (args.stream_frames, args.rounds))
            say("%-6s %-5s %-5s %8s %10s  %s" % ("sampl.", "round", "flag", "wall", "frames/s", "steady state"))
            for name, _ in SAMPLINGS:
                fps = {"off": [], "on": []}
                for rnd in range(args.rounds):
                    for form, more in (("off", []), ("on", ["--device_input_jpeg"])):
                        out = os.path.join(work, "stream_%s" % form)
                        wall, log = run(out, name, ["--num_streams", "8", "--write_state", "false"] + more, num_frames=args.stream_frames)
                        m = re.search(r"^steady state:\s+(.*\(([0-9.]+) frames per second.*)$", log, re.M)
                        fps[form].append(float(m.group(2)) if m else float("nan"))
                        say("%-6s %-5d %-5s %8.3f %10.2f  %s" % (name, rnd, form, wall, fps[form][-1], m.group(1) if m else "(no steady-state line)"))
                        save()
                say("%s: frames per second with the flag above without it in every round: %s (%.2f..%.2f against %.2f..%.2f)" % (
                    name, "yes" if all(x > y for x, y in zip(fps["on"], fps["off"])) else "NO", min(fps["on"]), max(fps["on"]), min(fps["off"]),
                    max(fps["off"])))
                save()
    finally:
        shutil.rmtree(work, ignore_errors=True)
save()
