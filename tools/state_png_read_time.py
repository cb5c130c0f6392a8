#!/usr/bin/env python
"""What reading back the state images of one 8K frame (28 overlaps + 8 extended pole images, B,G,R,A, 0.92 GB, as banded PNG files)
costs with the device decoder, on an MI355X:
  a. the batched decode of the frame's 36 device-encoded files straight into the previous-state buffers
     (s360_frame_set_prev_images_png: one upload of the files' bytes, one inflate launch over all bands, one unfilter launch):
     wall time of the call and the two kernels' device times (the library's profiler), `--rounds` rounds, with input and output
     GB/s of the kernels, the per-call counters and the histogram of speculation rounds;
  b. host/TestRenderStereoPanorama, frame 1 of a chain as a process of its own, in four forms — no flag, --device_state_png alone,
     --device_state_png + --device_state_read with the decode overlapped with reading the flow files (the default order), and
     with all images decoded behind the file reads (S360_STATE_READ_ORDER=batch) — `--rounds` alternating rounds on the same box
     and build: the process's wall time and the "previous-frame state" line of its --v 1 breakdown;
  c. once: --device_state_read on the files the HOST writer left (bands of 2 MB: few, and several blocks each, so every band is
     inflated serially by one lane).
usage: python tools/state_png_read_time.py [--rounds 3] [--out profiles/state_png_read.txt] [--skip-host]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_png_read.txt"))
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--timeout", type=int, default=300)
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

# ---- a. the decode alone ------------------------------------------------------------------------------------------------------
ctx = R.Context(R.RigDescription(args.rig), R.make_params(**flags))
ctx.upload_frame(*frames[0])
ctx.render(False)
n_side = len(frames[0][0])
names = [(n, p) for p in range(n_side) for n in ("overlap_l", "overlap_r")] + \
        [("extended_side", i) for i in range(4)] + [("extended_fisheye", i) for i in range(4)]
out_bytes = sum(int(np.prod(ctx.get_u8(n, i).shape)) for n, i in names)
ctx.encode_state_pngs(names)
files = [ctx.download_state_png(i).tobytes() for i in range(len(names))]
in_bytes = sum(len(f) for f in files)
want = ctx.get_u8("overlap_r", 3).copy()
ctx.set_prev_images_png(names, files)  # (first call: buffers are allocated)
assert np.array_equal(ctx.get_u8("overlap_r", 3), want)
say("# state images of one frame read back from PNG files: %d files, %.1f MB of files in, %.1f MB of B,G,R,A out (eyes %d x %d)" % (
    len(names), in_bytes / 1e6, out_bytes / 1e6, W, H))
say("## a. batched decode into the previous-state buffers (s360_frame_set_prev_images_png), %d rounds" % args.rounds)
say("%-5s %10s %12s %8s %8s %12s %8s %8s" % ("round", "call ms", "inflate ms", "in GB/s", "out GB/s", "unfilter ms", "in GB/s", "out GB/s"))
for rnd in range(args.rounds):
    ctx.profile_enable(True)
    t = time.perf_counter()
    ctx.set_prev_images_png(names, files)
    wall = (time.perf_counter() - t) * 1e3
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    ms = {k: v[0] for k, v in prof.items()}
    ti, tu = ms.get("png_inflate", float("nan")), ms.get("png_unfilter", float("nan"))
    gbs = lambda b, t: b / t / 1e6 if t > 0 else float("nan")  # noqa: E731
    say("%-5d %10.2f %12.3f %8.1f %8.1f %12.3f %8.1f %8.1f" % (rnd, wall, ti, gbs(in_bytes, ti), gbs(out_bytes, ti), tu, gbs(out_bytes, tu),
                                                                gbs(out_bytes, tu)))
fast, general, stored, rounds = ctx.png_decode_stats()
hist = ctx.png_decode_round_histogram()
say("bands: %d on the fast path, %d on the general path, %d of stored blocks only; most speculation rounds in a band: %d" % (fast, general, stored, rounds))
say("speculation rounds (the slowest window of each fast-path band): " + ", ".join("%d rounds: %d bands" % (r, n) for r, n in enumerate(hist) if n))
ctx.close()
del ctx
if args.torch_device == "cuda":
    torch.cuda.empty_cache()
save()

# ---- b. the host program, one process per frame ----------------------------------------------------------------------------------
program = args.program
if not args.skip_host:
    import json
    cams = json.load(open(args.rig))["cameras"]
    side_ids = [c["id"] for c in cams if "side" in c.get("group", "")]
    other = [c for c in cams if "side" not in c.get("group", "")]
    top_id = max(other, key=lambda c: c["forward"][2])["id"]
    bot_id = min(other, key=lambda c: c["forward"][2])["id"]
    work = tempfile.mkdtemp(prefix="s360_state_png_read_")
    try:
        imgs = os.path.join(work, "rgb")
        jobs = []
        for k, (side, top, bottom) in enumerate(frames):
            for cid, img in list(zip(side_ids, side)) + [(top_id, top), (bot_id, bottom)]:
                os.makedirs(os.path.join(imgs, cid), exist_ok=True)
                jobs.append((np.asarray(img), os.path.join(imgs, cid, "%06d.png" % k)))
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda j: Image.fromarray(np.ascontiguousarray(j[0][:, :, ::-1])).save(j[1], compress_level=1), jobs))

        def one(out, frame, prev, more, env=None):
            os.makedirs(os.path.join(out, "debug", frame, "flow_images"), exist_ok=True)
            os.makedirs(os.path.join(out, "flow", frame), exist_ok=True)
            cmd = [program, "--rig_json_file", args.rig, "--imgs_dir", imgs, "--frame_number", frame, "--output_data_dir", out,
                   "--prev_frame_data_dir", prev, "--output_equirect_path", os.path.join(out, "eqr_%s.png" % frame),
                   "--sharpening", "0.25", "--enable_top", "--enable_bottom", "--v", "1"]
            for k in ("eqr_width", "eqr_height", "final_eqr_width", "final_eqr_height"):
                cmd += ["--" + k, str(flags[k])]
            t = time.perf_counter()
            r = subprocess.run(cmd + more, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout,
                               env=dict(os.environ, **(env or {})))
            wall = time.perf_counter() - t
            if r.returncode != 0:
                raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
            m = re.search(r"^previous-frame state:\s+([0-9.]+)(.*)$", r.stderr, re.M)
            return wall, float(m.group(1)) if m else -1.0, (m.group(2).strip() if m else "")

        # frame 0 once per writer; every form of frame 1 resumes from one of the two
        outs = {"host": os.path.join(work, "out_host"), "dev": os.path.join(work, "out_dev")}
        one(outs["host"], "000000", "NONE", [])
        one(outs["dev"], "000000", "NONE", ["--device_state_png"])
        forms = [("no flag", "host", [], None),
                 ("state_png", "dev", ["--device_state_png"], None),
                 ("png+read overlap", "dev", ["--device_state_png", "--device_state_read"], None),
                 ("png+read batch", "dev", ["--device_state_png", "--device_state_read"], {"S360_STATE_READ_ORDER": "batch"})]
        say("## b. host program, frame 1 as a process of its own (--prev_frame_data_dir), %d alternating rounds (seconds)" % args.rounds)
        say("%-5s %-18s %8s %16s  %s" % ("round", "form", "wall", "previous state", "split"))
        rows = []
        for rnd in range(args.rounds):
            for form, src, more, env in forms:
                wall, prev_s, split = one(outs[src], "000001", "000000", more, env)
                rows.append((rnd, form, wall, prev_s))
                say("%-5d %-18s %8.3f %16.3f  %s" % (rnd, form, wall, prev_s, split))
                save()
        by = lambda form: [r[3] for r in rows if r[1] == form]  # noqa: E731
        for form in ("png+read overlap", "png+read batch"):
            say("\"previous-frame state\" with %s below --device_state_png alone in every round: %s (%.3f..%.3f s against %.3f..%.3f s)" % (
                form, "yes" if all(a < b for a, b in zip(by(form), by("state_png"))) else "NO", min(by(form)), max(by(form)),
                min(by("state_png")), max(by("state_png"))))
        say("overlap below batch in every round: %s" % ("yes" if all(a < b for a, b in zip(by("png+read overlap"), by("png+read batch"))) else "NO"))
        save()
        say("## c. --device_state_read on the HOST writer's files (2 MB bands, several blocks each: every band serial on one lane), once")
        wall, prev_s, split = one(outs["host"], "000001", "000000", ["--device_state_read"], None)
        say("wall %.3f s, previous-frame state %.3f s  %s" % (wall, prev_s, split))
    finally:
        shutil.rmtree(work, ignore_errors=True)
save()
