#!/usr/bin/env python
"""What the state images of one 8K frame (28 overlaps + 8 extended pole images, B,G,R,A, 0.92 GB) cost as PNG files, on an MI355X:
  1. the batched encode (s360_frame_encode_state_pngs: one launch sequence for all 36) against the same 36 images as 36
     single-image launch sequences, HIP events on the library's stream, `--rounds` alternating rounds: ms and GB/s of input;
  2. host/TestRenderStereoPanorama one process per frame — frame 0, then frame 1 with --prev_frame_data_dir — with
     --device_state_png off and on, alternating on the same box and build, `--rounds` rounds: frame 1's wall time and the
     "state files" lines of its --v 1 breakdown.
usage: python tools/state_png_time.py [--rounds 3] [--out profiles/state_png.txt] [--skip-host]"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_png.txt"))
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--timeout", type=int, default=300)
args = ap.parse_args()

W, H = (int(v) for v in args.eqr.split("x"))
flags = dict(eqr_width=W, eqr_height=H, enable_top=1, enable_bottom=1, final_eqr_width=args.final, final_eqr_height=args.final, sharpening=0.25)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda", 0)
rr = synth.RigRenderer(args.rig, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
frames = [rr.frame_numpy(yaw_deg=1.5 * k, disc_deg=10.0) for k in range(2)]
del rr
torch.cuda.empty_cache()

# ---- 1. the encode alone ----------------------------------------------------------------------------------------------------
ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
ctx.upload_frame(*frames[0])
ctx.render(False)
n_side = len(frames[0][0])
names = [(n, p) for p in range(n_side) for n in ("overlap_l", "overlap_r")] + \
        [("extended_side", i) for i in range(4)] + [("extended_fisheye", i) for i in range(4)]
in_bytes = sum(int(np.prod(ctx.get_u8(n, i).shape)) for n, i in names)
stream = torch.cuda.ExternalStream(R.lib().s360_stream(ctx.h), device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def batched():
    ctx.encode_state_pngs(names)


def singles():
    for nm in names:
        ctx.encode_state_pngs([nm])


batched()
file_bytes = sum(ctx.download_state_png(i).size for i in range(len(names)))
singles()
say("# state images of one frame as PNG files: %d images, %.1f MB of B,G,R,A in, %.1f MB of files out (eyes %d x %d)" % (
    len(names), in_bytes / 1e6, file_bytes / 1e6, W, H))
say("## 1. encode alone (HIP events on the library's stream), %d alternating rounds" % args.rounds)
say("%-5s %14s %10s %18s %10s" % ("round", "batched ms", "GB/s", "36 single ms", "GB/s"))
enc = []
for rnd in range(args.rounds):
    tb, ts = timed(batched), timed(singles)
    enc.append((tb, ts))
    say("%-5d %14.3f %10.1f %18.3f %10.1f" % (rnd, tb, in_bytes / tb / 1e6, ts, in_bytes / ts / 1e6))
say("batched below the single launches in every round: %s (batched %.3f..%.3f ms, singles %.3f..%.3f ms)" % (
    "yes" if all(b < s for b, s in enc) else "NO", min(b for b, _ in enc), max(b for b, _ in enc), min(s for _, s in enc), max(s for _, s in enc)))
ctx.close()
del ctx
torch.cuda.empty_cache()

# ---- 2. the host program, one process per frame -----------------------------------------------------------------------------
program = os.path.join(ROOT, "host", "TestRenderStereoPanorama")
if not args.skip_host:
    import json
    cams = json.load(open(args.rig))["cameras"]
    side_ids = [c["id"] for c in cams if "side" in c.get("group", "")]
    other = [c for c in cams if "side" not in c.get("group", "")]
    top_id = max(other, key=lambda c: c["forward"][2])["id"]
    bot_id = min(other, key=lambda c: c["forward"][2])["id"]
    work = tempfile.mkdtemp(prefix="s360_state_png_")
    try:
        imgs = os.path.join(work, "rgb")
        jobs = []
        for k, (side, top, bottom) in enumerate(frames):
            for cid, img in list(zip(side_ids, side)) + [(top_id, top), (bot_id, bottom)]:
                os.makedirs(os.path.join(imgs, cid), exist_ok=True)
                jobs.append((np.asarray(img), os.path.join(imgs, cid, "%06d.png" % k)))
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda j: Image.fromarray(np.ascontiguousarray(j[0][:, :, ::-1])).save(j[1], compress_level=1), jobs))

        def one(out, frame, prev, on):
            os.makedirs(os.path.join(out, "debug", frame, "flow_images"), exist_ok=True)
            os.makedirs(os.path.join(out, "flow", frame), exist_ok=True)
            cmd = [program, "--rig_json_file", args.rig, "--imgs_dir", imgs, "--frame_number", frame, "--output_data_dir", out,
                   "--prev_frame_data_dir", prev, "--output_equirect_path", os.path.join(out, "eqr_%s.png" % frame),
                   "--sharpening", "0.25", "--enable_top", "--enable_bottom", "--v", "1"]
            for k in ("eqr_width", "eqr_height", "final_eqr_width", "final_eqr_height"):
                cmd += ["--" + k, str(flags[k])]
            if on:
                cmd += ["--device_state_png"]
            t = time.perf_counter()
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
            got = {}
            for ln in r.stderr.splitlines():
                m = re.match(r"^state files(, \w+)?:\s+([0-9.]+)", ln.strip())
                if m:
                    got[(m.group(1) or ", all")[2:]] = float(m.group(2))
            return wall, got

        say("## 2. host program, one process per frame: frame 1 with --prev_frame_data_dir, %d alternating rounds (seconds)" % args.rounds)
        say("%-5s %-4s %8s %12s %8s %8s %8s" % ("round", "flag", "wall", "state files", "images", "flows", "writers"))
        rows = []
        for rnd in range(args.rounds):
            for on in (False, True):
                out = os.path.join(work, "out_%d_%d" % (rnd, on))
                one(out, "000000", "NONE", on)
                wall, g = one(out, "000001", "000000", on)
                rows.append((rnd, on, wall, g))
                say("%-5d %-4s %8.3f %12.3f %8.3f %8.3f %8.3f" % (rnd, "on" if on else "off", wall, g.get("all", -1), g.get("images", -1),
                                                                    g.get("flows", -1), g.get("writers", -1)))
                shutil.rmtree(out, ignore_errors=True)
        off = [r[3].get("all", 0) for r in rows if not r[1]]
        onn = [r[3].get("all", 0) for r in rows if r[1]]
        say("\"state files\" with the flag below without it in every round: %s (off %.3f..%.3f s, on %.3f..%.3f s)" % (
            "yes" if all(a < b for a, b in zip(onn, off)) else "NO", min(off), max(off), min(onn), max(onn)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
