"""GPU parity where the known-result short cuts act (flow_kernels.hip: the tile exit of the 15x15 blur into the sweeps'
records, the horizontal-only final resize), against the oracle, bit for bit: flows whose alphas make whole 32x32 tiles masked
(no updated pixel: the record blur leaves), opaque or neither; frames whose final
resize keeps the eyes' height, with even and odd output widths, and one whose vertical scale is not 1; and one 8K frame
rendered by a child process with S360_KNOWN_RESULT=0 (the switch is read once per process) equal to the same frame with the
short cuts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import content as K
import rigutil
from surround360_amd import render as R, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (331, 271)  # x0.5: 165 x 135 — 6 x 5 tiles at the finest level, partial at both edges
MODES = ("throughput", "latency")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    if got.dtype == np.float32:
        bad = bits(got) != bits(want)
    else:
        bad = got != want
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (name, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _noise(w, h):
    return synth.flow_pair(w, h, seed=3)


def _pole_mask(w, h):
    """The pole flows' shape: everything above a third of the height below the update threshold in one image."""
    a = np.full((h, w), 255, np.uint8)
    a[: h // 3] = 0
    return a


def _stripes_4(w, h):
    """Bands of alpha 229 / 230 (around PixFlow's 0.9f threshold), 254 (1 - a0 * a1 just above 0) and 255, 48 input px wide
    and high in turn: tiles of every class, and class edges inside tiles."""
    lv = np.array([229, 230, 254, 255], np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return lv[((yy // 48) + (xx // 48)) % 4]


FLOW_CASES = {
    "opaque": lambda w, h: K.with_alpha(_noise(w, h), 255),
    "generator_alpha": lambda w, h: _noise(w, h),  # synth.flow_pair's own feathered border
    "pole_mask_i1": lambda w, h: K.with_alpha(_noise(w, h), 255, _pole_mask(w, h)),
    "pole_mask_both": lambda w, h: K.with_alpha(_noise(w, h), _pole_mask(w, h)),
    "hole_rows_31": lambda w, h: K.with_alpha(_noise(w, h), K.alpha_hole_rows(w, h, 31)),
    "hole_rows_32": lambda w, h: K.with_alpha(_noise(w, h), K.alpha_hole_rows(w, h, 32)),
    "stripes_229_230_254_255": lambda w, h: K.with_alpha(_noise(w, h), _stripes_4(w, h)),
    "stripes_i0_only": lambda w, h: K.with_alpha(_noise(w, h), _stripes_4(w, h), 255),
}


@pytest.fixture(scope="module")
def ctxs(gpu_rig):
    out = {}
    for mode in MODES:
        c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
        c.set_sweep_mode(mode)
        out[mode] = c
    yield out
    for c in out.values():
        c.close()


def _tile_shares(oracle, i0, i1):
    """Of the finest level's 32x32 tiles: the share where the diffusion is the identity, and the share without an updated pixel."""
    a0, a1 = oracle.pixflow_entry(i0)[2], oracle.pixflow_entry(i1)[2]
    cc = np.float32(1.0) - a0 * a1
    upd = (a0 > np.float32(0.9)) & (a1 > np.float32(0.9))
    h, w = a0.shape
    tiles = [(x, y) for y in range(0, h, 32) for x in range(0, w, 32)]
    ident = sum(not (cc[y:y + 32, x:x + 32] != 0).any() for x, y in tiles)
    masked = sum(not upd[y:y + 32, x:x + 32].any() for x, y in tiles)
    return ident / len(tiles), masked / len(tiles)


@pytest.mark.parametrize("name", sorted(FLOW_CASES))
def test_flows_on_tiles_of_every_class(ctxs, oracle, name):
    """Both sweep kernels (half and full records), hints LEFT and RIGHT, every pyramid level; then the same pair chained
    to itself as the previous frame."""
    i0, i1 = FLOW_CASES[name](*SIZE)
    ident, masked = _tile_shares(oracle, i0, i1)
    print("%s: finest level, identity tiles %.2f, tiles without an updated pixel %.2f" % (name, ident, masked))
    if name == "opaque":
        assert ident == 1.0 and masked == 0.0
    if name.startswith("pole_mask"):
        assert 0 < masked < 1 and 0 < ident < 1
    if name.startswith("stripes"):
        assert ident < 1
    for hint in ("LEFT", "RIGHT"):
        final, levels = oracle.compute_optical_flow(i0, i1, "pixflow_low", hint, want_levels=True)
        prev_flow = np.ascontiguousarray(final * np.float32(0.5) + np.float32(0.25))
        chained = oracle.compute_optical_flow(i0, i1, "pixflow_low", hint, prev_flow=prev_flow, prev_i0=i0,
                                              prev_i1=np.ascontiguousarray(np.roll(i1, 1, axis=0)))
        for mode, ctx in ctxs.items():
            tag = "%s %s %s" % (name, mode, hint)
            _same(tag, ctx.compute_optical_flow(i0, i1, "pixflow_low", hint), final)
            buf, n = ctx.debug_flow_levels(i0, i1, "pixflow_low", hint)
            assert n == len(levels), tag
            off = 0
            for li, wl in enumerate(levels):
                _same("%s level %d (coarsest first)" % (tag, li), buf[off:off + wl.size].reshape(wl.shape), wl)
                off += wl.size
            _same(tag + " chained", ctx.compute_optical_flow(i0, i1, "pixflow_low", hint, prev_flow=prev_flow, prev_i0=i0,
                                                             prev_i1=np.ascontiguousarray(np.roll(i1, 1, axis=0))), chained)


# ---- the final resize ---------------------------------------------------------------------------------------------------------
EQR_W, EQR_H, CAM, WORLD_H = 1008, 504, 512, 1024


@pytest.fixture(scope="module")
def rig_small(tmp_path_factory, rig_json):
    d = tmp_path_factory.mktemp("rig_known_result")
    return rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)


@pytest.fixture(scope="module")
def small_frame(rig_small):
    return synth.rig_frame(rig_small, size=CAM, world=K.world_cartoon(WORLD_H), nearest=True)


@pytest.mark.parametrize("final_w,final_h", [(984, 2 * EQR_H), (983, 2 * EQR_H), (1100, 2 * EQR_H), (700, 2 * EQR_H),
                                             (984, 2 * EQR_H - 48)],
                         ids=["same_height_even", "same_height_odd_tail_column", "same_height_upscale",
                              "same_height_scale_1.44_general_kernel", "other_height_general_kernel"])
def test_final_resize(rig_small, small_frame, oracle, s360lib, final_w, final_h):
    """final_eqr_height == 2 * eqr_height: the eyes keep their height and the resize reads one source row per output row; an
    odd width ends on the column the reference's SSE2 loop leaves to its scalar tail. Horizontal scales beyond the tile's
    source box and any other height take the general kernel."""
    flags = dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=final_w,
                 final_eqr_height=final_h, sharpening=0.25)
    cams, _ = oracle.load_rig(rig_small)
    of = oracle.Frame(cams, oracle.make_params(**flags))
    want, _ = of.render(*small_frame)
    ctx = R.Context(R.RigDescription(rig_small), R.make_params(**flags))
    try:
        ctx.upload_frame(*small_frame)
        ctx.render()
        got = ctx.download_equirect()
    finally:
        ctx.close()
    assert got.shape == (final_h, final_w, 3)
    _same("equirect %dx%d" % (final_w, final_h), got, want)


# ---- 8K, switch off against switch on --------------------------------------------------------------------------------------
FLAGS_8K = dict(eqr_width=8400, eqr_height=4096, enable_top=1, enable_bottom=1, final_eqr_width=8192, final_eqr_height=8192)

_CHILD_8K = r"""
import os, sys
import numpy as np
root, out, rig = sys.argv[1:4]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch  # (its HIP runtime first, as in tests/conftest.py)
from surround360_amd import render as R, synth
import test_gpu_known_result as T
side, top, bottom = T.frame_8k(rig)
ctx = R.Context(R.RigDescription(rig), R.make_params(**T.FLAGS_8K))
ctx.upload_frame(side, top, bottom)
ctx.render()
first = ctx.download_equirect()
ctx.upload_frame(side, top, bottom)
ctx.render(use_prev=True)
np.save(out, np.stack([first, ctx.download_equirect()]))
ctx.close()
"""


def frame_8k(rig_json):
    world = synth.World(4096, seed=360, device="cuda")
    rr = synth.RigRenderer(rig_json, world, 2048)
    return rr.frame_numpy(yaw_deg=0.2, disc_deg=10.5)


@pytest.mark.fullsize
def test_8k_frame_switch_off_equals_switch_on(rig_json, s360lib, gpu_rig, tmp_path):
    """The 8k preset, a frame and its chained successor, each process with its own setting of the switch."""
    outs = {}
    for tag, val in (("on", None), ("off", "0")):
        env = {k: v for k, v in os.environ.items() if k != "S360_KNOWN_RESULT"}
        if val is not None:
            env["S360_KNOWN_RESULT"] = val
        out = str(tmp_path / ("eq_%s.npy" % tag))
        subprocess.run([sys.executable, "-c", _CHILD_8K, ROOT, out, rig_json], check=True, env=env, timeout=900, cwd=ROOT)
        outs[tag] = np.load(out, mmap_mode="r")
    assert outs["on"].shape == (2, 8192, 8192, 3)
    assert np.array_equal(outs["on"], outs["off"])
