#!/usr/bin/env python
"""What the cubemap of every frame costs at the presets' size (8400 x 4096 eyes -> 1536^2 faces), alternating the old and the
new way inside one process, `--rounds` rounds:
  1. kernels (HIP events of the profile families): k_cubemap through the on-demand s360_frame_cubemap ("cubemap") against
     k_cubemap_tiles ("cubemap_stream") for one slot and for all slots of a batch in one launch, video and photo; the fraction of
     8 TB/s against the algorithmic bytes (3 B per output pixel + 4 B per pixel of prepared map + both eyes once);
  2. in the batch (host clock around work that ends in the fetches): ms per frame of render_batch with the cubemap off, on,
     on + PNG (the equirect's PNG is encoded in both PNG configurations), and the only thing that existed before: render_batch,
     then s360_frame_cubemap into a page-locked buffer per slot.
usage: python tools/cubemap_time.py [--slots 8] [--rounds 3] [--out profiles/cubemap_stream.txt]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--face", type=int, default=1536)
ap.add_argument("--eqr", default="8400x4096")
ap.add_argument("--final", type=int, default=8192)
ap.add_argument("--cam", type=int, default=2048)
ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
ap.add_argument("--out", default="")
args = ap.parse_args()

HBM = 8.0e12
W, H = (int(v) for v in args.eqr.split("x"))
FW = FH = args.face
S = args.slots
RIG = args.rig
flags = dict(eqr_width=W, eqr_height=H, enable_top=1, enable_bottom=1, final_eqr_width=args.final, final_eqr_height=args.final,
             sharpening=0.25)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda", 0)
rr = synth.RigRenderer(RIG, synth.World(4 * args.cam, seed=360, device=dev), args.cam)
frames = [rr.frame_numpy(yaw_deg=1.5 * k, disc_deg=10.0) for k in range(min(S, 3))]
del rr
torch.cuda.empty_cache()
ctx = R.Context(R.RigDescription(RIG), R.make_params(**flags))
ctx.set_frame_slots(S)
ctx.set_sweep_mode("throughput")
for k in range(S):
    ctx.select_frame_slot(k)
    ctx.upload_frame(*frames[k % len(frames)])
ctx.select_frame_slot(0)
lib = R.lib()


def dims(fmt):
    return (3 * FW, 4 * FH) if fmt == "video" else (FW, 12 * FH)


cube_buf = {fmt: R.pinned_empty((dims(fmt)[1], dims(fmt)[0], 3)) for fmt in ("video", "photo")}


def profiled(fn, family):
    ctx.profile_enable(True)
    fn()
    ctx.synchronize()
    ms, launches = ctx.profile_get()[family]
    ctx.profile_enable(False)
    return ms, launches


def on_demand(fmt, slot=0):
    ctx.select_frame_slot(slot)
    whc = (C.c_int * 3)()
    ctx._ck(lib.s360_frame_cubemap(ctx.h, FW, FH, fmt.encode(), whc, cube_buf[fmt].ctypes.data_as(C.c_void_p)))
    return cube_buf[fmt]


# ---- 1. kernels -----------------------------------------------------------------------------------------------------
say("# cubemap of every frame: %d x %d eyes -> %d^2 faces, %d slots, %d rounds (alternating in one process)" % (W, H, FW, S, args.rounds))
say("## 1. kernels (HIP events), ms per frame")
say("%-6s %-5s %12s %14s %14s %10s %10s" % ("format", "round", "k_cubemap", "tiles 1 slot", "tiles %d slots" % S, "ratio 1", "ratio %d" % S))
kernel_rows = []
for fmt in ("video", "photo"):
    ow, oh = dims(fmt)
    ctx.set_cubemap_output(FW, FH, fmt)
    ctx.render_batch()  # warm-up of every shape: buffers, code objects
    want = [on_demand(fmt, k).copy() for k in range(min(S, 2))]
    for k in range(min(S, 2)):
        assert np.array_equal(ctx.download_cubemap(slot=k), want[k]), "the two kernels differ"
    ctx.render_slots([0])
    for rnd in range(args.rounds):
        old_ms, n_old = profiled(lambda: on_demand(fmt), "cubemap")
        one_ms, n_one = profiled(lambda: ctx.render_slots([0]), "cubemap_stream")
        all_ms, n_all = profiled(lambda: ctx.render_batch(), "cubemap_stream")
        assert n_old == 1 and n_one == 1 and n_all == 1
        all_ms /= S
        kernel_rows.append(dict(format=fmt, round=rnd, k_cubemap_ms=old_ms, tiles_one_slot_ms=one_ms, tiles_batch_ms_per_frame=all_ms))
        say("%-6s %-5d %12.4f %14.4f %14.4f %10.2f %10.2f" % (fmt, rnd, old_ms, one_ms, all_ms, old_ms / max(one_ms, 1e-9), old_ms / max(all_ms, 1e-9)))
    nbytes = 3 * ow * oh + 4 * ow * (oh // 2) + 2 * 4 * W * H
    best = min(r["tiles_batch_ms_per_frame"] for r in kernel_rows if r["format"] == fmt)
    one = min(r["tiles_one_slot_ms"] for r in kernel_rows if r["format"] == fmt)
    say("%s: algorithmic bytes %d per frame; of 8 TB/s: one slot %.3f, in the batch %.3f (best round)" % (
        fmt, nbytes, nbytes / (max(one, 1e-9) * 1e-3) / HBM, nbytes / (max(best, 1e-9) * 1e-3) / HBM))
ok1 = all(r["tiles_one_slot_ms"] <= r["k_cubemap_ms"] and r["tiles_batch_ms_per_frame"] <= r["k_cubemap_ms"] for r in kernel_rows)
say("condition (new kernel not slower than k_cubemap per frame in any round): %s" % ("met" if ok1 else "NOT met"))

# ---- 2. in the batch ------------------------------------------------------------------------------------------------
say("## 2. in the batch: ms per frame of render_batch + fetches, %d slots, sharpening 0.25, video" % S)
fmt = "video"


def cfg_off():
    ctx.set_cubemap_output(0, 0, fmt)
    ctx.set_png_encode(False)
    ctx.render_batch()
    ctx.synchronize()


def cfg_on():
    ctx.set_cubemap_output(FW, FH, fmt)
    ctx.set_png_encode(False)
    ctx.render_batch()
    for k in range(S):
        ctx.download_cubemap(slot=k, out=cube_buf[fmt])


def cfg_off_png():
    ctx.set_cubemap_output(0, 0, fmt)
    ctx.set_png_encode(True)
    ctx.render_batch()
    ctx.synchronize()


def cfg_on_png():
    ctx.set_cubemap_output(FW, FH, fmt)
    ctx.set_png_encode(True)
    ctx.render_batch()
    for k in range(S):
        ctx.download_cubemap_png(slot=k, out=png_buf)


def cfg_parent():
    ctx.set_cubemap_output(0, 0, fmt)
    ctx.set_png_encode(False)
    ctx.render_batch()
    for k in range(S):
        on_demand(fmt, k)


ctx.set_cubemap_output(FW, FH, fmt)
png_buf = R.pinned_empty((int(lib.s360_frame_cubemap_png_bound(ctx.h)),))
configs = [("cubemap off", cfg_off), ("on + fetch", cfg_on), ("off, PNG encoder on", cfg_off_png), ("on + PNG fetch", cfg_on_png),
           ("parent: on-demand per slot", cfg_parent)]
for _, fn in configs:
    fn()  # warm-up
say("%-5s " % "round" + " ".join("%28s" % n for n, _ in configs))
batch_rows = []
for rnd in range(args.rounds):
    row = {}
    for name, fn in configs:  # alternating
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        row[name] = 1e3 * (time.perf_counter() - t) / S
    batch_rows.append(row)
    say("%-5d " % rnd + " ".join("%28.3f" % row[n] for n, _ in configs))
ok2 = all(r["on + fetch"] < r["parent: on-demand per slot"] for r in batch_rows)
say("condition (render + fetch of all %d cubemaps the new way takes less time per frame than the parent's way in every round): %s" % (
    S, "met" if ok2 else "NOT met"))
say(json.dumps({"eyes": [W, H], "face": FW, "slots": S, "kernels": kernel_rows, "batch": batch_rows, "conditions_met": [ok1, ok2]}))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
ctx.close()
