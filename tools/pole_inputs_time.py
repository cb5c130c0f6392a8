#!/usr/bin/env python
"""What pole removal's alpha work costs per frame with the masks handed in per frame against resident per context
(include/s360_pole_inputs.h), on one MI355X (recorded, not gated):
  device time of the library's profile scopes pole_removal_prepare + pole_removal_merge for one frame of the synthetic footage with
  bottom cameras of --cam x --cam, per-frame path (s360_frame_upload_pole_removal) against resident path (s360_set_pole_masks +
  s360_frame_upload_bottom2) on two contexts of the same build, `--rounds` alternating rounds, the median of `--frames` warm frames
  each; the host-to-device bytes a frame's pole-removal inputs take on either path (computed from the sizes); the one-time cost of
  s360_set_pole_masks (host clock around the call, which waits for the device); and that both paths left the same equirect.
The program half of the measurement (8K preset, --num_streams 8, .bin containers against --device_input_png files) is not part of
this tool.
usage: python tools/pole_inputs_time.py [--rounds 3] [--frames 20] [--cam 2048] [--out profiles/pole_inputs.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pole_inputs.txt"))
args = ap.parse_args()

W, H = (int(v) for v in args.eqr.split("x"))
flags = dict(eqr_width=W, eqr_height=H, enable_top=1, enable_bottom=1, enable_pole_removal=1, final_eqr_width=args.final,
             final_eqr_height=args.final, sharpening=0.25)
SCOPES = ("pole_removal_prepare", "pole_removal_merge")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


if not torch.cuda.is_available():
    sys.exit("pole_inputs_time: no GPU (a time is measured on the device or not at all)")
dev = torch.device("cuda", 0)
rig = R.RigDescription(args.rig)
rr = synth.RigRenderer(args.rig, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
every = rr.frame_all_numpy(yaw_deg=0.0, disc_deg=10.0)
side, top, bottom = [every[i] for i in rr.side], every[rr.top], every[rr.bottom]
ids = [c["id"] for c in rr.cams]
bottom2 = every[ids.index(rig.get_bottom_camera2_id())]
del rr
torch.cuda.empty_cache()
n = args.cam
yy, xx = np.mgrid[0:n, 0:n]


def mask(cx, half_w):  # (the wedge of tests/rigutil.py)
    m = np.full((n, n, 3), 255, np.uint8)
    m[(np.abs(xx - cx) < half_w + (yy * 0.04)) & (yy > n * 0.35)] = (0, 0, 255)
    return m


m1, m2 = mask(n * 0.5, n * 0.04), mask(n * 0.45, n * 0.05)
per_frame, resident = R.Context(rig, R.make_params(**flags)), R.Context(rig, R.make_params(**flags))
t0 = time.perf_counter()
resident.set_pole_masks(m1, m2)
t_masks = time.perf_counter() - t0


def feed(ctx):
    ctx.upload_frame(side, top, bottom)
    if ctx is resident:
        ctx.upload_bottom2(bottom2)
    else:
        ctx.upload_pole_removal(bottom2, m1, m2)


def frames_of(ctx, k, timed):
    """k frames, each uploaded and rendered on its own; the scopes' device times of every frame (ms)."""
    out = []
    for _ in range(k):
        feed(ctx)
        ctx.render(False)
        ctx.synchronize()
        if timed:
            p = ctx.profile_get()
            out.append(tuple(p[s][0] for s in SCOPES))
    return out


px = n * n
say("# pole removal's inputs and alpha work per frame: bottom cameras %d x %d, eyes %d x %d, golden rig (the secondary image is flipped)" % (n, n, W, H))
say("host-to-device bytes per frame for pole removal's inputs: per-frame path 3 x %.1f MB (secondary image, two masks), resident path "
    "1 x %.1f MB (the secondary image; 0 for the masks; 0 in all when the secondary camera comes through a device input path)" % (px * 3 / 1e6, px * 3 / 1e6))
say("s360_set_pole_masks, once per context: %.1f ms (host clock; two mask uploads, three alpha planes, waits for the device)" % (t_masks * 1e3))
for ctx in (per_frame, resident):
    frames_of(ctx, args.warmup, False)
    ctx.profile_enable(True)
    frames_of(ctx, 1, True)
say("## device time of the profile scopes %s, %d alternating rounds, median of %d warm frames (ms)" % (" + ".join(SCOPES), args.rounds, args.frames))
say("%-5s %-10s %10s %10s %10s" % ("round", "path", "prepare", "merge", "sum"))
lower = []
for rnd in range(args.rounds):
    sums = {}
    for name, ctx in (("per-frame", per_frame), ("resident", resident)):
        t = frames_of(ctx, args.frames, True)
        med = [statistics.median(v[i] for v in t) for i in range(2)]
        sums[name] = statistics.median(v[0] + v[1] for v in t)
        say("%-5d %-10s %10.3f %10.3f %10.3f" % (rnd, name, med[0], med[1], sums[name]))
    lower.append(sums["resident"] < sums["per-frame"])
same = np.array_equal(per_frame.download_equirect(), resident.download_equirect())
say("resident below per-frame in every round: %s; both contexts' last equirects equal byte for byte: %s" % ("yes" if all(lower) else "no", "yes" if same else "NO"))
per_frame.close()
resident.close()
open(args.out, "w").write("\n".join(lines) + "\n")
sys.exit(0 if same else 1)
