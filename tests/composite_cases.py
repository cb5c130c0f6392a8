"""The cases tests/test_gpu_composite_poles.py (on the GPU) and tests/test_cpu_composite_poles.py (the same kernels on the CPU
emulation of the library) share: the pole layers, which the frame path stores without their transparent padding rows, and their
composite onto the eyes in one pass (render_kernels.hip: k_composite_poles_v4), against the oracle's frame byte for byte and
against the launch-per-layer path (S360_COMPOSITE_FUSED=0, a developer switch read once per process: results do not depend on
it, which is what case (c) checks)."""
import json
import os
import subprocess
import sys

import numpy as np

import rigutil
from surround360_amd import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = 128
# the eye size: tests/sharpen_shapes_cases.py's; S360_COMPOSITE_CASES_EQR=WxH is how tests/test_cpu_composite_poles.py asks for
# its quarter-size frames (the emulation takes half a minute per 1008x504 frame)
EQR_W, EQR_H = [int(v) for v in os.environ.get("S360_COMPOSITE_CASES_EQR", "1008x504").split("x")]
P = 14  # side cameras of tests/golden/rig_17cam.json: the eye width is a multiple of it
MASKS = (1, 2, 4, 8, 5, 10, 15)  # pole units: 1 top_left, 2 top_right, 4 bottom_left, 8 bottom_right


def same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    d = got.astype(np.int32) - want.astype(np.int32)
    assert not d.any(), "%s: %d mismatching bytes, max |d| %d" % (name, int((d != 0).sum()), int(np.abs(d).max()))


def make_rig(rig_json, tmpdir, pole_fov=None):
    """The 17-camera rig with 128-pixel cameras; pole_fov: the `fov` of the top and bottom cameras in the copy (radians)."""
    path = rigutil.scaled_rig_json(rig_json, str(tmpdir / ("rig_%d%s.json" % (CAM, "" if pole_fov is None else "_fov"))), CAM / 2048.0)
    if pole_fov is not None:
        rig = json.load(open(path))
        n = 0
        for c in rig["cameras"]:
            if "fov" in c:
                c["fov"] = pole_fov
                n += 1
        assert n == 3  # top, bottom, second bottom
        json.dump(rig, open(path, "w"))
    return path


def flags(**over):
    f = dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=0, final_eqr_height=0)
    f.update(over)
    return f


def frame(path, yaw_deg=0.0):
    return rigutil.frame_inputs(path, CAM, yaw_deg=yaw_deg)


def check_against_oracle(path, oracle, fl, yaws=(0.0,), expect_rows=None):
    """Frames of different content one after the other in one context (no temporal state): eyes, equirect and pole layers against
    the oracle's; from the second frame on the layers' padding rows are rows the frame path did not write for this frame."""
    cams, _ = oracle.load_rig(path)
    of = oracle.Frame(cams, oracle.make_params(**fl))
    ctx = R.Context(R.RigDescription(path), R.make_params(**fl))
    try:
        g = ctx.geometry
        if expect_rows is not None:
            expect_rows(g.top_rows, g.bottom_rows, fl["eqr_height"])
        prev = None
        for k, yaw in enumerate(yaws):
            f = frame(path, yaw)
            want, _ = of.render(*f)
            ctx.upload_frame(*f)
            ctx.render()
            got = ctx.download_equirect()
            if prev is not None:
                assert not np.array_equal(prev, got)  # (different content)
            prev = got
            for u in range(4):
                if not fl["enable_top" if u < 2 else "enable_bottom"]:
                    continue
                rows = g.top_rows if u < 2 else g.bottom_rows
                layer = ctx.get_u8("pole_warped", u)
                assert layer.shape == (fl["eqr_height"], fl["eqr_width"], 4)
                assert not layer[rows:].any(), "frame %d, pole unit %d: the padding rows are not all zero" % (k, u)
                assert layer[:rows].any()
                same("frame %d pole_warped %d" % (k, u), layer, of.get_u8("pole_warped", u))
            same("frame %d eye_l" % k, ctx.get_u8("eye_l"), of.get_u8("eye_l"))
            same("frame %d eye_r" % k, ctx.get_u8("eye_r"), of.get_u8("eye_r"))
            same("frame %d equirect" % k, got, want)
    finally:
        ctx.close()


def render_masks(path, fl, masks=MASKS):
    """One frame's side stage, then s360_frame_pole_units(mask) + s360_frame_composite(mask) per mask: the equirects and eyes."""
    ctx = R.Context(R.RigDescription(path), R.make_params(**fl))
    out = []
    try:
        ctx.upload_frame(*frame(path))
        ctx.render_pairs(0, P)
        for m in masks:
            ctx.pole_units(m)
            ctx.composite(m)
            out.append(np.concatenate([ctx.get_u8("eye_l")[..., :3].reshape(-1), ctx.get_u8("eye_r")[..., :3].reshape(-1),
                                       ctx.download_equirect().reshape(-1)]))
    finally:
        ctx.close()
    return np.stack(out)


_CHILD = r"""
import os, sys
root, path, out = sys.argv[1:4]
sys.path[:0] = [root, os.path.join(root, "tests")]
import torch  # (its HIP runtime first, as in tests/conftest.py)
from surround360_amd import _capi
if os.environ.get("S360_TEST_EMULATED_LIB") == "1":
    _capi.LIB_PATH = os.environ.get("S360_TEST_EMULATED_LIB_PATH") or os.path.join(root, "tools", "libs360_emu.so")
import numpy as np
import composite_cases as S
np.save(out, S.render_masks(path, S.flags()))
"""


def check_masks_against_per_layer_path(path, tmpdir):
    """Every mask with the fused composite (this process) and with one launch per layer (a child process with the switch off)."""
    assert os.environ.get("S360_COMPOSITE_FUSED") is None, "these tests run with the fused composite on"
    out = str(tmpdir / "per_layer.npy")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, out], check=True, timeout=900, cwd=ROOT,
                   env=dict(os.environ, S360_COMPOSITE_FUSED="0"))
    want = np.load(out)
    got = render_masks(path, flags())
    assert got.shape == want.shape and got.shape[0] == len(MASKS)
    for i, m in enumerate(MASKS):
        same("mask %d, fused against per layer" % m, got[i], want[i])
    for i in range(1, len(MASKS)):
        assert not np.array_equal(got[i], got[0])  # (the masks give different frames)
    # mask 15 is the whole frame
    ctx = R.Context(R.RigDescription(path), R.make_params(**flags()))
    try:
        ctx.upload_frame(*frame(path))
        ctx.render()
        same("mask 15 against s360_frame_render", got[-1][-ctx.download_equirect().size:], ctx.download_equirect().reshape(-1))
    finally:
        ctx.close()


def check_batch(path, nslots=3):
    """Three slots (three different frames) in one render_batch: the layers of all slots go through one set of scratch buffers."""
    fl = flags()
    rig = R.RigDescription(path)
    frames = [frame(path, y) for y in (0.0, 1.1, 2.3)]
    cb = R.Context(rig, R.make_params(**fl))
    c1 = R.Context(rig, R.make_params(**fl))
    try:
        cb.set_frame_slots(nslots)
        cb.set_sweep_mode("throughput")
        for k in range(nslots):
            cb.select_frame_slot(k)
            cb.upload_frame(*frames[k % 3])
        cb.render_batch()
        alone = []
        for f in frames:
            c1.upload_frame(*f)
            c1.render()
            alone.append(c1.download_equirect())
        assert not np.array_equal(alone[0], alone[1])
        for k in range(nslots):
            cb.select_frame_slot(k)
            same("batched slot %d of %d" % (k, nslots), cb.download_equirect(), alone[k % 3])
    finally:
        cb.close()
        c1.close()
