"""The stereo cubemap as an output of every frame (s360_set_cubemap_output): what a stream or a batch leaves per frame and per
slot — pixels and the device-encoded PNG — against the oracle's convertSphericalToCubemapBicubicRemap +
stackOutputCubemapFaces (OracleFrame.cubemap) and against the on-demand s360_frame_cubemap, byte for byte. Sizes are those of
tests/refprog.py (504 x 252 eyes), so that the file also runs on the emulated library (S360_TEST_EMULATED_LIB=1,
tests/test_cpu_cubemap_stream.py)."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import rigutil
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQR_W, EQR_H, CAM, FINAL = 504, 252, 256, 480
S360_ERR_INVALID_ARG, S360_ERR_STATE = -1, -6
FLAGS = dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=FINAL, final_eqr_height=FINAL)


def _cmp(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    d = got.astype(np.int32) - want.astype(np.int32)
    assert not d.any(), "%s: %d mismatching bytes, max |d| %d" % (name, int((d != 0).sum()), int(np.abs(d).max()))


@pytest.fixture(scope="module")
def env(tmp_path_factory, rig_json, oracle, s360lib):
    d = tmp_path_factory.mktemp("rig")
    path = rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)
    a = rigutil.frame_inputs(path, CAM)
    b = rigutil.frame_inputs(path, CAM, yaw_deg=1.5)
    c = ([np.ascontiguousarray(s[:, ::-1]) for s in a[0]], a[2], a[1])
    cams, _ = oracle.load_rig(path)
    return dict(path=path, rig=R.RigDescription(path), inputs=dict(a=a, b=b, c=c), cams=cams, oracle=oracle)


def _ctx(env, slots=1, **flags):
    ctx = R.Context(env["rig"], R.make_params(**dict(FLAGS, **flags)))
    if slots > 1:
        ctx.set_frame_slots(slots)
    return ctx


def _oracle_frame(env, **flags):
    O = env["oracle"]
    return O.Frame(env["cams"], O.make_params(**dict(FLAGS, **flags)))


def _upload(ctx, env, names):
    for k, n in enumerate(names):
        if len(names) > 1:
            ctx.select_frame_slot(k)
        ctx.upload_frame(*env["inputs"][n])


# ---- single frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharpening", [0.0, 0.25])
@pytest.mark.parametrize("fmt,fw,fh", [("video", 96, 80), ("photo", 64, 64), ("photo", 50, 38)])
def test_single_frame(env, fmt, fw, fh, sharpening):
    """The cubemap rendered with the frame == the oracle's == the on-demand call's (k_cubemap), from the sharpened eyes; a face
    width that is no multiple of 4 takes the kernel's scalar stores."""
    of = _oracle_frame(env, sharpening=sharpening)
    want_eq, _ = of.render(*env["inputs"]["a"])
    want = of.cubemap(fw, fh, fmt)
    ctx = _ctx(env, sharpening=sharpening)
    try:
        ctx.set_cubemap_output(fw, fh, fmt)
        assert ctx.cubemap_size() == (want.shape[1], want.shape[0], 3)
        _upload(ctx, env, ["a"])
        ctx.render()
        got = ctx.download_cubemap()
        _cmp("cubemap with the frame", got, want)
        _cmp("on-demand cubemap", ctx.cubemap(fw, fh, fmt), got)
        _cmp("equirect", ctx.download_equirect(), want_eq)
        assert got.std() > 5
    finally:
        ctx.close()


# ---- the smallest frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,fw,fh", [("video", 33, 17), ("photo", 16, 16)])
@pytest.mark.parametrize("eqr_w,eqr_h", [(28, 14), (42, 21)])
def test_smallest_frames(tmp_path, rig_json, oracle, s360lib, eqr_w, eqr_h, fmt, fw, fh):
    """The smallest frames s360_create accepts (the flags of test_gpu_ops.py::test_tiny_frames_equal_the_oracle) into faces larger
    than the eyes: the boxes of the tiles around the poles are in LDS and wrap in y (tests/test_gpu_cubemap_tiles.py counts them).
    The cubemap rendered with the frame == the oracle's == the on-demand call's."""
    cam = 64
    path = rigutil.scaled_rig_json(rig_json, str(tmp_path / "rig_tiny.json"), cam / 2048.0)
    side, top, bottom = rigutil.frame_inputs(path, cam)
    flags = dict(eqr_width=eqr_w, eqr_height=eqr_h, enable_top=1, enable_bottom=1, final_eqr_width=0, final_eqr_height=0,
                 sharpening=0.25, side_alpha_feather_size=7, std_alpha_feather_size=3)
    cams, _ = oracle.load_rig(path)
    of = oracle.Frame(cams, oracle.make_params(**flags))
    want_eq, _ = of.render(side, top, bottom)
    want = of.cubemap(fw, fh, fmt)
    ctx = R.Context(R.RigDescription(path), R.make_params(**flags))
    try:
        ctx.set_cubemap_output(fw, fh, fmt)
        assert ctx.cubemap_size() == (want.shape[1], want.shape[0], 3)
        ctx.upload_frame(side, top, bottom)
        ctx.render()
        got = ctx.download_cubemap()
        _cmp("cubemap with the frame", got, want)
        _cmp("on-demand cubemap", ctx.cubemap(fw, fh, fmt), got)
        _cmp("equirect", ctx.download_equirect(), want_eq)
        assert got.std() > 5
    finally:
        ctx.close()


# ---- batches --------------------------------------------------------------------------------------------------------
def test_batch_of_three_slots_and_a_subset(env):
    """Three slots with different inputs through render_batch: every slot's cubemap equals that slot rendered alone;
    render_slots on a subset leaves the other slot's cubemap as it was."""
    alone = {}
    for n in "abc":
        ctx = _ctx(env, sharpening=0.25)
        try:
            ctx.set_cubemap_output(96, 80, "video")
            _upload(ctx, env, [n])
            ctx.render()
            alone[n] = ctx.download_cubemap()
        finally:
            ctx.close()
    assert not np.array_equal(alone["a"], alone["b"]) and not np.array_equal(alone["a"], alone["c"])
    ctx = _ctx(env, slots=3, sharpening=0.25)
    try:
        ctx.set_cubemap_output(96, 80, "video")
        _upload(ctx, env, ["a", "b", "c"])
        ctx.render_batch()
        for k, n in enumerate("abc"):
            _cmp("slot %d by name" % k, ctx.download_cubemap(slot=k), alone[n])
            ctx.select_frame_slot(k)
            _cmp("slot %d selected" % k, ctx.download_cubemap(), alone[n])
        ctx.select_frame_slot(0)
        ctx.upload_frame(*env["inputs"]["c"])
        ctx.select_frame_slot(2)
        ctx.upload_frame(*env["inputs"]["a"])
        ctx.render_slots([0, 2])
        _cmp("slot 0 after the subset", ctx.download_cubemap(slot=0), alone["c"])
        _cmp("slot 1 untouched", ctx.download_cubemap(slot=1), alone["b"])
        _cmp("slot 2 after the subset", ctx.download_cubemap(slot=2), alone["a"])
    finally:
        ctx.close()


# ---- temporal chain -------------------------------------------------------------------------------------------------
def test_temporal_chain(env):
    of = _oracle_frame(env)
    ctx = _ctx(env)
    try:
        ctx.set_cubemap_output(64, 64, "photo")
        for step, n in enumerate("ab"):
            of.render(*env["inputs"][n], use_prev=step > 0)
            _upload(ctx, env, [n])
            ctx.render(use_prev=step > 0)
            _cmp("chained frame %d" % step, ctx.download_cubemap(), of.cubemap(64, 64, "photo"))
    finally:
        ctx.close()


# ---- output buffering -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_steps_plain(env):
    """Two steps of a two-slot batch on a plain context: [step][slot] -> (cubemap, equirect)."""
    ctx = _ctx(env, slots=2)
    steps = []
    try:
        ctx.set_cubemap_output(96, 80, "video")
        for names in (["a", "b"], ["c", "a"]):
            _upload(ctx, env, names)
            ctx.render_batch()
            res = []
            for k in range(2):
                ctx.select_frame_slot(k)
                res.append((ctx.download_cubemap(slot=k), ctx.download_equirect()))
            steps.append(res)
    finally:
        ctx.close()
    assert not np.array_equal(steps[0][0][0], steps[1][0][0])
    return steps


@pytest.mark.parametrize("mode", ["double_buffer", "pipelining"])
def test_age_one_is_the_step_before(env, two_steps_plain, mode):
    """Enqueue step k+1, then fetch age 1 = step k's cubemap, for every slot; the equirects still equal the plain ones."""
    ctx = _ctx(env, slots=2)
    try:
        ctx.set_cubemap_output(96, 80, "video")
        if mode == "double_buffer":
            ctx.set_output_double_buffer(True)
        else:
            ctx.set_frame_pipelining(True)
        for names in (["a", "b"], ["c", "a"]):
            _upload(ctx, env, names)
            ctx.render_batch()
        for k in range(2):
            ctx.select_frame_slot(k)
            _cmp("slot %d age 1" % k, ctx.download_cubemap(age=1, slot=k), two_steps_plain[0][k][0])
            _cmp("slot %d age 1 equirect" % k, ctx.download_equirect_of(1), two_steps_plain[0][k][1])
            _cmp("slot %d age 0" % k, ctx.download_cubemap(age=0, slot=k), two_steps_plain[1][k][0])
            _cmp("slot %d age 0 equirect" % k, ctx.download_equirect_of(0), two_steps_plain[1][k][1])
    finally:
        ctx.close()


# ---- switches -------------------------------------------------------------------------------------------------------
def test_switches(env):
    ctx = _ctx(env)
    try:
        _upload(ctx, env, ["a"])
        ctx.render()
        out = np.empty((4 * 80, 3 * 96, 3), np.uint8)
        rc = R.lib().s360_frame_download_cubemap(ctx.h, 0, out.ctypes.data_as(R.C.c_void_p))
        assert rc == S360_ERR_STATE  # rendered with the output off
        with pytest.raises(R.S360Error) as e:
            ctx.cubemap_size()
        assert e.value.code == S360_ERR_STATE
        with pytest.raises(R.S360Error) as e:
            ctx.set_cubemap_output(96, 80, "cross")
        assert e.value.code == S360_ERR_INVALID_ARG
        # the size may change between two frames: the size query and the next frame follow it
        of = _oracle_frame(env)
        of.render(*env["inputs"]["a"])
        ctx.set_cubemap_output(96, 80, "video")
        assert ctx.cubemap_size() == (288, 320, 3)
        ctx.render()
        _cmp("96 x 80 video", ctx.download_cubemap(), of.cubemap(96, 80, "video"))
        ctx.set_cubemap_output(40, 48, "photo")
        assert ctx.cubemap_size() == (40, 576, 3)
        ctx.render()
        _cmp("40 x 48 photo", ctx.download_cubemap(), of.cubemap(40, 48, "photo"))
        # off again: the next frame leaves none
        ctx.set_cubemap_output(0, 0, "video")
        ctx.render()
        rc = R.lib().s360_frame_download_cubemap(ctx.h, 0, out.ctypes.data_as(R.C.c_void_p))
        assert rc == S360_ERR_STATE
    finally:
        ctx.close()


# ---- PNG ------------------------------------------------------------------------------------------------------------
def test_png(env, tmp_path):
    """The cubemap's device-encoded file decodes (PIL; the banded reader of host/png_io.hpp, parallel and sequential) to
    download_cubemap()'s pixels as R,G,B, is no longer than its bound, and needs the encoder on at render time."""
    ctx = _ctx(env, slots=2, sharpening=0.25)
    try:
        ctx.set_cubemap_output(96, 80, "video")
        _upload(ctx, env, ["a", "b"])
        ctx.render_batch()
        with pytest.raises(R.S360Error) as e:
            ctx.download_cubemap_png(slot=0)  # rendered with the encoder off
        assert e.value.code == S360_ERR_STATE
        ctx.set_png_encode(True)
        ctx.render_batch()
        bound = int(R.lib().s360_frame_cubemap_png_bound(ctx.h))
        src = tmp_path / "rd.cpp"
        src.write_text(r'''
#include "png_io.hpp"
int main(int argc, char** argv) {  // argv: in.png out.raw threads
  pngio::g_read_threads = std::atoi(argv[3]);
  pngio::Image im = pngio::read(argv[1], false);
  FILE* f = std::fopen(argv[2], "wb");
  std::fwrite(im.px.data(), 1, im.px.size(), f);
  std::fclose(f);
  return im.c == 3 ? 0 : 1;
}
''')
        exe = str(tmp_path / "rd")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "host"), "-o", exe, str(src), "-lz", "-lpthread"])
        files = []
        for k in range(2):
            px = ctx.download_cubemap(slot=k)
            png = ctx.download_cubemap_png(slot=k).tobytes()
            assert 0 < len(png) <= bound
            p = tmp_path / ("cube%d.png" % k)
            p.write_bytes(png)
            dec = np.asarray(Image.open(str(p)))
            assert dec.shape == px.shape and np.array_equal(dec[:, :, ::-1], px), "slot %d: PIL" % k
            for threads in ("3", "-1"):
                subprocess.check_call([exe, str(p), str(tmp_path / "c.raw"), threads])
                assert np.array_equal(np.fromfile(str(tmp_path / "c.raw"), np.uint8).reshape(px.shape), px), (k, threads)
            # the equirect's file of the same frame is still the equirect
            ctx.select_frame_slot(k)
            eq = np.asarray(Image.open(__import__("io").BytesIO(ctx.download_png().tobytes())))
            assert np.array_equal(eq[:, :, ::-1], ctx.download_equirect())
            files.append(png)
        assert files[0] != files[1]
    finally:
        ctx.close()


# ---- wrap coverage --------------------------------------------------------------------------------------------------
def _float_map(face, W, H, fw, fh):
    """cube_map_entry restated in float32 numpy (counting only: an ulp of acos does not move a tap across the border)."""
    f32 = np.float32
    x = (np.arange(fw, dtype=f32) * f32(1.0 / fw) - f32(0.5))[None, :].repeat(fh, 0)
    y = (np.arange(fh, dtype=f32) * f32(1.0 / fh) - f32(0.5))[:, None].repeat(fw, 1)
    z = np.full_like(x, 0.5)
    d = {"BACK": (x, z, -y), "LEFT": (-z, x, -y), "TOP": (x, y, z), "BOTTOM": (x, -y, -z), "FRONT": (-x, -z, -y),
         "RIGHT": (z, -x, -y)}[face]
    r = np.sqrt(d[0] * d[0] + d[1] * d[1])
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    phi = np.arccos(np.clip(d[2] / n, -1, 1)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = np.where(r > 0, np.arccos(np.clip(np.abs(d[0] / r), 0, 1)), 0).astype(f32)
    th = np.where((d[0] > 0) & (d[1] > 0), th, np.where((d[0] <= 0) & (d[1] > 0), f32(np.pi) - th,
                  np.where((d[0] <= 0) & (d[1] <= 0), f32(np.pi) + th, f32(2 * np.pi) - th))).astype(f32)
    return f32(W) * th / f32(2 * np.pi), f32(H) * phi / f32(np.pi)


def test_wrap_coverage(env):
    """A kernel that clamps or zeroes instead of wrapping must not pass the parity tests above: at 504 x 252 -> 96 x 80 there ARE
    output pixels whose taps wrap in x and in y, and the oracle's eyes differ across the border exactly there."""
    fw, fh = 96, 80
    of = _oracle_frame(env, sharpening=0.25)
    of.render(*env["inputs"]["a"])
    eyes = [of.get_u8("eye_l")[:, :, :3].astype(np.int32), of.get_u8("eye_r")[:, :, :3].astype(np.int32)]
    assert eyes[0].shape[:2] == (EQR_H, EQR_W)
    wrap_x = wrap_y = 0
    rows_x, cols_y = set(), set()
    for face in ("RIGHT", "LEFT", "TOP", "BOTTOM", "BACK", "FRONT"):
        mx, my = _float_map(face, EQR_W, EQR_H, fw, fh)
        sx = (np.rint(mx * np.float32(32)).astype(np.int64) >> 5) - 1
        sy = (np.rint(my * np.float32(32)).astype(np.int64) >> 5) - 1
        wx = (sx < 0) | (sx + 3 >= EQR_W)
        wy = (sy < 0) | (sy + 3 >= EQR_H)
        wrap_x += int(wx.sum())
        wrap_y += int(wy.sum())
        for r in sy[wx]:
            rows_x.update(int(v) % EQR_H for v in range(r, r + 4))
        for c in sx[wy]:
            cols_y.update(int(v) % EQR_W for v in range(c, c + 4))
    print("pixels with taps wrapping in x: %d, in y: %d" % (wrap_x, wrap_y))
    assert wrap_x >= 1 and wrap_y >= 1
    rows_x, cols_y = sorted(rows_x), sorted(cols_y)
    for e in eyes:
        # wrapped taps read the other end of the row / column: different content from a clamped or zeroed border
        left, right = e[rows_x][:, 0:3], e[rows_x][:, EQR_W - 3:EQR_W]
        assert np.abs(left - right).max() > 8 and left.max() > 0 and right.max() > 0
        top, bottom = e[0:3][:, cols_y], e[EQR_H - 3:EQR_H][:, cols_y]
        assert np.abs(top - bottom).max() > 8 and top.max() > 0 and bottom.max() > 0


# ---- full size ------------------------------------------------------------------------------------------------------
@pytest.mark.fullsize
def test_8k_cubemap_1536_two_slots(rig_json, oracle, s360lib):
    """8400 x 4096 eyes -> 1536^2 faces (every preset of batch_process_video.py), both formats, for a two-slot batch, against
    the oracle."""
    flags = dict(eqr_width=8400, eqr_height=4096, enable_top=1, enable_bottom=1, final_eqr_width=8192, final_eqr_height=8192,
                 sharpening=0.25)
    ins = [rigutil.frame_inputs(rig_json, 2048, world_h=4096), rigutil.frame_inputs(rig_json, 2048, world_h=4096, yaw_deg=1.5)]
    cams, _ = oracle.load_rig(rig_json)
    got = {}
    ctx = R.Context(R.RigDescription(rig_json), R.make_params(**flags))
    try:
        ctx.set_frame_slots(2)
        for k in range(2):
            ctx.select_frame_slot(k)
            ctx.upload_frame(*ins[k])
        for fmt in ("video", "photo"):
            ctx.set_cubemap_output(1536, 1536, fmt)
            ctx.render_batch()
            for k in range(2):
                got[fmt, k] = ctx.download_cubemap(slot=k)
    finally:
        ctx.close()
    assert not np.array_equal(got["video", 0], got["video", 1])
    for k in range(2):
        of = oracle.Frame(cams, oracle.make_params(**flags))
        of.render(*ins[k], threaded=True)
        for fmt in ("video", "photo"):
            _cmp("8K cubemap 1536 %s slot %d" % (fmt, k), got[fmt, k], of.cubemap(1536, 1536, fmt))
        del of
