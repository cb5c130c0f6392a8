#!/usr/bin/env python
"""What --save_debug_images costs for one 8K frame of the synthetic footage, on one MI355X (recorded, not gated):
  1. on the device: k_debug_views (the frame's one launch, the library's own "debug_views" profile scope) and the debug PNG batch
     (s360_frame_encode_debug_pngs, HIP events on the library's stream), `--rounds` alternating rounds; the device memory a
     context holds after a frame with the switch on against off; the bytes of the images and of their files;
  2. host/TestRenderStereoPanorama one process per frame (no previous frame), alternating on the same box and build: without the
     flag, with it (host threads encode the files), and both again with --device_state_png (the device encodes the state images
     and, with the flag, the debug images): wall time, and the "debug images:" line of --v 1 (files, MB written, seconds).
usage: python tools/debug_images_time.py [--rounds 3] [--out profiles/debug_images.txt] [--skip-host]"""
import argparse
import json
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
from surround360_amd import debug_images as DI, render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debug_images.txt"))
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
frame = rr.frame_numpy(yaw_deg=0.0, disc_deg=10.0)
del rr
torch.cuda.empty_cache()


def held(on):
    """Device memory a context holds after one rendered frame (bytes), and the context."""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
    if on:
        DI.set_debug_images(ctx, True)
    ctx.upload_frame(*frame)
    ctx.render(False)
    ctx.synchronize()
    return free0 - torch.cuda.mem_get_info()[0], ctx


# ---- 1. on the device -------------------------------------------------------------------------------------------------------
mem_off, ctx = held(False)
ctx.close()
del ctx
mem_on, ctx = held(True)
lst = DI.debug_image_list(ctx)
in_bytes = sum(w * h * c for _, w, h, c in lst)
DI.encode_debug_pngs(ctx)
file_bytes = sum(DI.download_debug_png(ctx, i).size for i in range(len(lst)))
view_names = [n for n, _, _, _ in lst if n.startswith(("croppedSideSpherical_", "sphericalImg_offsetwrap", "eqr_side", "_eqr_side"))]
view_bytes = sum(w * h * c for n, w, h, c in lst if n in view_names)
say("# debug images of one frame (eyes %d x %d, top + bottom, sharpening 0.25): %d images, %.1f MB of pixels, %.1f MB as PNG files" % (
    W, H, len(lst), in_bytes / 1e6, file_bytes / 1e6))
say("device memory a context holds after one frame: switch off %.1f MB, on %.1f MB (+%.1f MB: panoramas before the composite, eyes "
    "before the sharpen, the %d views; the PNG batch's buffers come on top when it is used)" % (mem_off / 1e6, mem_on / 1e6, (mem_on - mem_off) / 1e6, len(view_names)))
stream = torch.cuda.ExternalStream(R.lib().s360_stream(ctx.h), device=dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


say("## 1. on the device, %d rounds: k_debug_views (%d views, %.1f MB written; the frame's \"debug_views\" profile scope, table upload included), "
    "the debug PNG batch (HIP events on the library's stream)" % (args.rounds, len(view_names), view_bytes / 1e6))
say("%-5s %18s %10s %18s %10s" % ("round", "k_debug_views ms", "GB/s out", "PNG batch ms", "GB/s in"))
ctx.profile_enable(True)
for rnd in range(args.rounds):
    ctx.upload_frame(*frame)
    ctx.render(False)
    tv = ctx.profile_get()["debug_views"][0]
    tb = timed(lambda: DI.encode_debug_pngs(ctx))
    say("%-5d %18.3f %10.1f %18.3f %10.1f" % (rnd, tv, view_bytes / tv / 1e6, tb, in_bytes / tb / 1e6))
ctx.profile_enable(False)
ctx.close()
del ctx
torch.cuda.empty_cache()

# ---- 2. the host program, one process per frame -----------------------------------------------------------------------------
program = os.path.join(ROOT, "host", "TestRenderStereoPanorama")
if not args.skip_host:
    cams = json.load(open(args.rig))["cameras"]
    side_ids = [c["id"] for c in cams if "side" in c.get("group", "")]
    other = [c for c in cams if "side" not in c.get("group", "")]
    top_id = max(other, key=lambda c: c["forward"][2])["id"]
    bot_id = min(other, key=lambda c: c["forward"][2])["id"]
    work = tempfile.mkdtemp(prefix="s360_debug_images_")
    try:
        imgs = os.path.join(work, "rgb")
        jobs = []
        side, top, bottom = frame
        for cid, img in list(zip(side_ids, side)) + [(top_id, top), (bot_id, bottom)]:
            os.makedirs(os.path.join(imgs, cid), exist_ok=True)
            jobs.append((np.asarray(img), os.path.join(imgs, cid, "000000.png")))
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda j: Image.fromarray(np.ascontiguousarray(j[0][:, :, ::-1])).save(j[1], compress_level=1), jobs))

        def one(out, more):
            for d in (os.path.join(out, "debug", "000000", "flow_images"), os.path.join(out, "debug", "000000", "projections"), os.path.join(out, "flow", "000000")):
                os.makedirs(d, exist_ok=True)
            cmd = [program, "--rig_json_file", args.rig, "--imgs_dir", imgs, "--frame_number", "000000", "--output_data_dir", out,
                   "--prev_frame_data_dir", "NONE", "--output_equirect_path", os.path.join(out, "eqr_000000.png"),
                   "--sharpening", "0.25", "--enable_top", "--enable_bottom", "--v", "1"] + more
            for k in ("eqr_width", "eqr_height", "final_eqr_width", "final_eqr_height"):
                cmd += ["--" + k, str(flags[k])]
            t = time.perf_counter()
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout)
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
            m = re.search(r"^debug images:\s+(\d+) files, ([0-9.]+) MB, ([0-9.]+)", r.stderr, re.M)
            return wall, (int(m.group(1)), float(m.group(2)), float(m.group(3))) if m else (0, 0.0, 0.0)

        variants = [("off", []), ("host", ["--save_debug_images"]), ("off+dev", ["--device_state_png"]),
                    ("device", ["--save_debug_images", "--device_state_png"])]
        say("## 2. host program, one process per frame (no previous frame), %d alternating rounds (seconds). off: no flag; host: "
            "--save_debug_images, files encoded by host threads; off+dev: --device_state_png alone (the state images encoded on the device); "
            "device: --save_debug_images --device_state_png (state and debug images encoded on the device)" % args.rounds)
        say("%-5s %-7s %8s %7s %12s %16s" % ("round", "variant", "wall", "files", "MB written", "debug images s"))
        walls = {v: [] for v, _ in variants}
        for rnd in range(args.rounds):
            for v, more in variants:
                out = os.path.join(work, "out_%d_%s" % (rnd, v))
                wall, (n, mb, sec) = one(out, more)
                walls[v].append(wall)
                say("%-5d %-7s %8.3f %7d %12.1f %16.3f" % (rnd, v, wall, n, mb, sec))
                shutil.rmtree(out, ignore_errors=True)
        say("wall time: off %.3f..%.3f s, host %.3f..%.3f s (+%.3f s over off, mean); off+dev %.3f..%.3f s, device %.3f..%.3f s (+%.3f s over off+dev, mean); "
            "device below host in every round: %s" % (
                min(walls["off"]), max(walls["off"]), min(walls["host"]), max(walls["host"]), (sum(walls["host"]) - sum(walls["off"])) / args.rounds,
                min(walls["off+dev"]), max(walls["off+dev"]), min(walls["device"]), max(walls["device"]),
                (sum(walls["device"]) - sum(walls["off+dev"])) / args.rounds,
                "yes" if all(d < h for d, h in zip(walls["device"], walls["host"])) else "NO"))
    finally:
        shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
