#!/usr/bin/env python3
"""How much of the 15x15 flow blurs' work has a known result (flow_kernels.hip, k_sepblur): the share of
32x32 tiles, over every pyramid level of every flow of one frame and weighted by tile area, on which

  * `1.0f - a0 * a1 == 0.0f` for every pixel  — lowAlphaFlowDiffusion returns the flow it was given, and
  * no pixel has `a0 > 0.9f && a1 > 0.9f`      — the sweeps read only the NaN mark of the tile's records (EPI 2 / 3 leave).

The alphas depend on the rig and the flags, not on the pictures, so one frame of any content answers for a preset. Counted
on the CPU with the oracle (tests/oracle_lib.py): the frame rendered by Frame.render, the alphas of the side flows' inputs
(overlap_l / overlap_r [0..13]) and the pole flows' (extended_side / extended_fisheye [0..3]) taken through pixflow_entry
(the x0.5 entry downscale), the x0.9 pyramids built with resize_linear_f32, tiles cut as the kernels cut them.

  python tools/tile_classes.py                       # the 8k preset on the 17-camera test rig (minutes of CPU time)
  python tools/tile_classes.py --eqr_width 1008 --eqr_height 504 --cam 512   # a scaled-down rig, seconds
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = 32


def tile_areas(mask_any):
    """mask_any: per-pixel bool. Returns (area of the tiles that hold no True pixel, whole area)."""
    h, w = mask_any.shape
    free = 0
    for y in range(0, h, T):
        for x in range(0, w, T):
            t = mask_any[y:y + T, x:x + T]
            if not t.any():
                free += t.size
    return free, h * w


def flow_shares(O, img0, img1):
    """One flow: (identity area, masked area, whole area) summed over its pyramid levels."""
    a0, a1 = O.pixflow_entry(img0)[2], O.pixflow_entry(img1)[2]
    h, w = img0.shape[:2]
    ident = masked = total = 0
    for lw, lh in O.pixflow_levels(w, h):  # finest first
        if a0.shape != (lh, lw):
            a0, a1 = O.resize_linear_f32(a0, lw, lh), O.resize_linear_f32(a1, lw, lh)
        cc = np.float32(1.0) - a0 * a1
        upd = (a0 > np.float32(0.9)) & (a1 > np.float32(0.9))
        i, n = tile_areas(cc != 0)
        m, _ = tile_areas(upd)
        ident += i
        masked += m
        total += n
    return ident, masked, total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rig", default=os.path.join(ROOT, "tests", "golden", "rig_17cam.json"))
    ap.add_argument("--eqr_width", type=int, default=8400)
    ap.add_argument("--eqr_height", type=int, default=4096)
    ap.add_argument("--cam", type=int, default=2048, help="camera image size; below 2048 the rig is scaled to it")
    a = ap.parse_args()
    import oracle_lib as O
    import rigutil
    from surround360_amd import synth
    rig = a.rig
    if a.cam != 2048:
        import tempfile
        rig = rigutil.scaled_rig_json(a.rig, os.path.join(tempfile.mkdtemp(), "rig_scaled.json"), a.cam / 2048.0)
    side, top, bottom = synth.rig_frame(rig, size=a.cam, world_h=max(256, a.cam // 2))
    cams, _ = O.load_rig(rig)
    of = O.Frame(cams, O.make_params(eqr_width=a.eqr_width, eqr_height=a.eqr_height, enable_top=1, enable_bottom=1))
    of.render(side, top, bottom, threaded=True)
    rows = {}
    s = np.zeros(3, np.int64)
    for i in range(len(side)):
        s += flow_shares(O, of.get_u8("overlap_l", i), of.get_u8("overlap_r", i))
    rows["side"] = s
    p = np.zeros(3, np.int64)
    for u in range(4):
        p += flow_shares(O, of.get_u8("extended_side", u), of.get_u8("extended_fisheye", u))
    rows["pole"] = p
    # every side pair is matched in both directions over the same two alphas
    rows["side"] = rows["side"] * 2
    rows["all"] = rows["side"] + rows["pole"]
    whole = rows["all"][2]
    print("%-6s %12s %28s %30s" % ("flows", "tile area", "diffusion is the identity", "tiles without an updated pixel"))
    for k in ("side", "pole", "all"):
        i, m, n = rows[k]
        print("%-6s %11.0f%% %28.2f %30.2f" % (k, 100.0 * n / whole, i / n, m / n))


if __name__ == "__main__":
    main()
