#!/usr/bin/env python
"""What k_morph_views (generateNovelView on the device, s360_generate_novel_views) costs per launch on a 2048 x 2048 pair:
1 and 11 views, merged only and with both warped images written, for the two ways of mapping shifts to the grid — one view per
grid.z slice (S360_MORPH_VPB=1) and all views as a loop inside the workgroup (S360_MORPH_VPB=n). HIP events of the "morph_views"
profile family around the launch; the variants alternate call by call inside one process, after warm-up calls of every shape.
Algorithmic bytes: two BGRA images and two flow fields read once per launch (24 B per pixel), 4 or 12 B written per pixel and
view; the fraction is of 8 TB/s.   usage: python tools/morph_time.py [--size 2048] [--reps 12]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from surround360_amd import render as R, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

HBM = 8.0e12
w = h = args.size
ctx = R.Context(R.RigDescription(os.path.join(ROOT, "tests", "golden", "rig_17cam.json")), R.make_params(eqr_width=1008, eqr_height=504))
il, ir = synth.flow_pair(w, h, seed=11)
_, f_lr, f_rl = ctx.interpolate_views(il, ir, 0.5, want_flows=True)


def timed(shifts, sides, vpb):
    os.environ["S360_MORPH_VPB"] = str(vpb)
    ctx.profile_enable(True)
    out = ctx.generate_novel_views(il, ir, f_lr, f_rl, shifts, want_sides=sides)
    ctx.synchronize()
    ms, launches = ctx.profile_get()["morph_views"]
    ctx.profile_enable(False)
    assert launches == 1
    return ms, out


rows = []
print("%-6s %-6s %-10s %10s %10s %10s %12s %10s" % ("views", "sides", "mapping", "median ms", "min ms", "max ms", "bytes", "of 8 TB/s"))
for n in (1, 11):
    shifts = [float(v) / float(max(n - 1, 1)) if n > 1 else 0.5 for v in range(n)]
    for sides in (False, True):
        variants = [("grid.z", 1), ("loop", n)] if n > 1 else [("grid.z", 1)]
        ts = {name: [] for name, _ in variants}
        ref = None
        for it in range(args.warmup + args.reps):
            for name, vpb in variants:  # alternating
                ms, out = timed(shifts, sides, vpb)
                d = [hash(a.tobytes()) for a in (out if sides else (out,))]
                ref = ref or d
                assert d == ref, "the two mappings differ"
                if it >= args.warmup:
                    ts[name].append(ms)
        nbytes = w * h * (24 + (12 if sides else 4) * n)
        for name, _ in variants:
            t = np.array(ts[name])
            med = float(np.median(t))
            rows.append(dict(views=n, sides=sides, mapping=name, ms_median=med, ms_min=float(t.min()), ms_max=float(t.max()),
                             bytes=nbytes, hbm_frac=nbytes / (med * 1e-3) / HBM))
            print("%-6d %-6s %-10s %10.4f %10.4f %10.4f %12d %10.3f" % (n, "yes" if sides else "no", name, med, t.min(), t.max(), nbytes,
                                                                        rows[-1]["hbm_frac"]))
print(json.dumps({"size": [w, h], "reps": args.reps, "rows": rows}))
