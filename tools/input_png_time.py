#!/usr/bin/env python
"""What reading the camera images of one 8K frame (14 side, top, bottom: 16 files of 2048 x 2048, banded PNG files of the device encoder, 16-bit as
host/Unpacker --device_png writes them and 8-bit) costs with the device decoder (include/s360_input_png.h), on an MI355X:
  1. device time of the 16-file batch (s360_decode_input_png_batch, 16-bit files to their high bytes; 8-bit files): the two
     kernels' times from the library's profiler (hipEvents), warm, median of `--reps`, with the per-call counters and the histogram
     of speculation rounds; and the wall time of s360_frame_upload_png for the same files. Nothing else runs on the GPU.
  2. host/TestRenderStereoPanorama, one process per frame, without and with --device_input_png, alternating, `--rounds` rounds:
     the "load + decode + upload" line of its --v 1 breakdown and the process's wall time.
  3. --num_streams 8 over `--stream-frames` frames from the 16-bit files, without and with the flag, alternating, `--rounds` rounds:
     the "steady state" frames per second (files written).
The camera images are synthetic (surround360_amd.synth); a 16-bit sample is the 8-bit image's value with random bits below it, as a
developed sensor image has noise in its low byte.
usage: python tools/input_png_time.py [--rounds 3] [--out profiles/input_png.txt] [--skip-host] [--skip-streams]"""
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
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--stream-frames", type=int, default=32)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_png.txt"))
ap.add_argument("--skip-host", action="store_true")
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


dev = torch.device(args.torch_device, 0) if args.torch_device == "cuda" else torch.device(args.torch_device)
rr = synth.RigRenderer(args.rig, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
frames = [rr.frame_numpy(yaw_deg=1.5 * k, disc_deg=10.0) for k in range(2)]
del rr
if args.torch_device == "cuda":
    torch.cuda.empty_cache()

# ---- the files ------------------------------------------------------------------------------------------------------------------
ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
rng = np.random.default_rng(17)
n_side = len(frames[0][0])
cams = list(range(n_side)) + [-1, -2]
files = {16: [], 8: []}  # per depth, per frame: the files
for side, top, bottom in frames:
    imgs8 = [np.ascontiguousarray(a[..., :3]) for a in list(side) + [top, bottom]]
    files[8].append([bytes(ctx.encode_png(a)) for a in imgs8])
    files[16].append([bytes(ctx.encode_png16((a.astype(np.uint16) << 8) | rng.integers(0, 256, a.shape).astype(np.uint16))) for a in imgs8])
pixels = sum(a.shape[0] * a.shape[1] for a in list(frames[0][0]) + [frames[0][1], frames[0][2]])
say("# camera images of one frame from banded PNG files: %d files of %d x %d (eyes %d x %d)" % (len(cams), args.cam, args.cam, W, H))

# ---- 1. device time ---------------------------------------------------------------------------------------------------------------
say("## 1. device time of the %d-file batch (s360_decode_input_png_batch; 16-bit files to their high bytes), warm, median of %d" % (len(cams), args.reps))
say("%-6s %10s %12s %12s %14s %14s %10s" % ("depth", "files MB", "scanlines MB", "inflate ms", "(min..max)", "unfilter ms", "call ms"))
for depth in (16, 8):
    fs = files[depth][0]
    in_bytes = sum(len(f) for f in fs)
    scan = pixels * (6 if depth == 16 else 3)
    got = ctx.decode_input_png_batch(fs)  # (first call: buffers are allocated)
    assert np.array_equal(got[3], np.ascontiguousarray(frames[0][0][3][..., :3]))
    ti, tu, tw = [], [], []
    for rep in range(args.reps):
        ctx.profile_enable(True)
        t = time.perf_counter()
        ctx.decode_input_png_batch(fs)
        tw.append((time.perf_counter() - t) * 1e3)
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        ti.append(prof["png_inflate"][0])
        tu.append(prof["png_unfilter"][0])
    say("%-6d %10.1f %12.1f %12.3f %14s %14.3f %10.1f" % (depth, in_bytes / 1e6, scan / 1e6, statistics.median(ti),
                                                       "%.3f..%.3f" % (min(ti), max(ti)), statistics.median(tu), statistics.median(tw)))
    fast, general, stored, rounds = ctx.png_decode_stats()
    hist = ctx.png_decode_round_histogram()
    say("       bands: %d on the fast path, %d on the general path, %d of stored blocks only; most speculation rounds in a band: %d" % (
        fast, general, stored, rounds))
    say("       speculation rounds (the slowest window of each fast-path band): " + ", ".join("%d: %d" % (r, n) for r, n in enumerate(hist) if n))
    ctx.upload_frame_png(cams, fs)  # (first call: the slots are allocated)
    tw = []
    for rep in range(5):
        t = time.perf_counter()
        ctx.upload_frame_png(cams, files[depth][rep & 1])
        tw.append((time.perf_counter() - t) * 1e3)
    say("       s360_frame_upload_png of the same files (copy, inflate, unfilter into the source slots, wait): %.1f ms median of 5 (%.1f..%.1f)" % (
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
    work = tempfile.mkdtemp(prefix="s360_input_png_")
    try:
        imgs = {}
        for depth in (16, 8):
            imgs[depth] = os.path.join(work, "rgb%d" % depth)
            for cid_i, cid in enumerate(ids):
                os.makedirs(os.path.join(imgs[depth], cid), exist_ok=True)
                for k in range(2):
                    with open(os.path.join(imgs[depth], cid, "%06d.png" % k), "wb") as f:
                        f.write(files[depth][k][cid_i])
                for k in range(2, args.stream_frames):  # a stream's later frames are the first two again
                    os.symlink("%06d.png" % (k & 1), os.path.join(imgs[depth], cid, "%06d.png" % k))

        def run(out, depth, more, num_frames=None):
            for k in range(num_frames or 1):
                os.makedirs(os.path.join(out, "debug", "%06d" % k, "flow_images"), exist_ok=True)
                os.makedirs(os.path.join(out, "flow", "%06d" % k), exist_ok=True)
            cmd = [args.program, "--rig_json_file", args.rig, "--imgs_dir", imgs[depth], "--frame_number", "000000", "--output_data_dir", out,
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

        say("## 2. one process per frame, --device_input_png off and on, %d alternating rounds (seconds)" % args.rounds)
        say("%-6s %-5s %-5s %8s %24s  %s" % ("depth", "round", "flag", "wall", "load + decode + upload", "split"))
        for depth in (16, 8):
            rows = {"off": [], "on": []}
            for rnd in range(args.rounds):
                for form, more in (("off", []), ("on", ["--device_input_png"])):
                    out = os.path.join(work, "out_%d_%s" % (depth, form))
                    wall, log = run(out, depth, more)
                    m = re.search(r"^load \+ decode \+ upload:\s+([0-9.]+)\s*(.*)$", log, re.M)
                    rows[form].append((wall, float(m.group(1))))
                    say("%-6d %-5d %-5s %8.3f %24.3f  %s" % (depth, rnd, form, wall, float(m.group(1)), m.group(2)))
                    save()
            for what, col in (("load + decode + upload", 1), ("wall time", 0)):
                a, b = [r[col] for r in rows["on"]], [r[col] for r in rows["off"]]
                say("depth %d: %s with the flag below without it in every round: %s (%.3f..%.3f s against %.3f..%.3f s)" % (
                    depth, what, "yes" if all(x < y for x, y in zip(a, b)) else "NO", min(a), max(a), min(b), max(b)))
            same = open(os.path.join(work, "out_%d_on" % depth, "eqr_000000.png"), "rb").read() == \
                open(os.path.join(work, "out_%d_off" % depth, "eqr_000000.png"), "rb").read()
            say("depth %d: the equirect files of the two forms are the same bytes: %s" % (depth, "yes" if same else "NO"))
            save()

        if not args.skip_streams:
            say("## 3. --num_streams 8, %d frames from the 16-bit files, flag off and on, %d alternating rounds" % (args.stream_frames, args.rounds))
            say("%-5s %-5s %8s %10s  %s" % ("round", "flag", "wall", "frames/s", "steady state"))
            fps = {"off": [], "on": []}
            for rnd in range(args.rounds):
                for form, more in (("off", []), ("on", ["--device_input_png"])):
                    out = os.path.join(work, "stream_%s" % form)
                    wall, log = run(out, 16, ["--num_streams", "8", "--write_state", "false"] + more, num_frames=args.stream_frames)
                    m = re.search(r"^steady state:\s+(.*\(([0-9.]+) frames per second.*)$", log, re.M)
                    fps[form].append(float(m.group(2)) if m else float("nan"))
                    say("%-5d %-5s %8.3f %10.2f  %s" % (rnd, form, wall, fps[form][-1], m.group(1) if m else "(no steady-state line)"))
                    save()
            say("frames per second with the flag above without it in every round: %s (%.2f..%.2f against %.2f..%.2f)" % (
                "yes" if all(x > y for x, y in zip(fps["on"], fps["off"])) else "NO", min(fps["on"]), max(fps["on"]), min(fps["off"]), max(fps["off"])))
    finally:
        shutil.rmtree(work, ignore_errors=True)
save()
