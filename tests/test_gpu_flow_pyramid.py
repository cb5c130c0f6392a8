"""GPU parity of what PixFlow does in front of its level loop and between its levels (flow.hip: FlowEngine::prepare — pre-blur, image
pyramids, previous images, motion map, previous flow, their pyramids, the level factors; flow_kernels.hip: launch_resize_linear_f32,
launch_resize_cubic_f32c2), kernel level, through the test taps of include/s360_debug_flow_pyramid.h against the oracle's
PixFlow::prepare and its resizes. The cases are tests/flow_pyramid_cases.py's; every comparison is bit for bit, on buffers that hold a
byte pattern no result holds, in launch order, so that a failure names the first stage that differs. A case that claims a branch
proves it first: on the oracle's data, on the numpy restatement of the kernels' boxes, or on the kernel the launcher reports."""
import os
import re

import numpy as np
import pytest

import content as K
import flow_pyramid_cases as S
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    yield c
    c.close()


# ---- A: the engine's own preparation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw,dh,oddw,oddh", S.LEVEL0, ids=S.LEVEL0_IDS)
def test_prepare_level0_sizes(ctx, oracle, dw, dh, oddw, oddh):
    """The pre-blur's reflections at 2 .. 5 pixels, the 64 x 16 tile's edges, one level and the first two-level size; with and
    without previous state."""
    S.check_level0(ctx, oracle, dw, dh, oddw, oddh)


@pytest.mark.parametrize("w,h,reach,coarsest", S.TILE_EDGE, ids=["%dx%d" % c[:2] for c in S.TILE_EDGE])
def test_prepare_pyramid_on_tile_edges(ctx, oracle, w, h, reach, coarsest):
    S.check_tile_edge(ctx, oracle, w, h, reach, coarsest)


def test_batch_cases_reach_every_plane_class():
    assert S.all_classes_covered() == ({4, 2}, {4, 2, 1}, {4, 2, 1})  # (2N planes are never odd)


@pytest.mark.parametrize("n,b", S.BATCH, ids=["N%d_B%d" % c for c in S.BATCH])
def test_prepare_batch_classes(ctx, oracle, n, b):
    """2N image planes, B two-channel planes and N motion planes per pyramid step, with 4, 2 and 1 planes per thread; every plane of
    every level is compared, every image has its own content and alpha."""
    S.check_batch(ctx, oracle, n, b)


@pytest.mark.parametrize("w,h", [(64, 52), (75, 75), (58, 61)], ids=["even", "odd", "odd_h"])
def test_prepare_previous_state_scale(ctx, oracle, w, h):
    """rows_down / rows_full exactly 0.5 and not; previous images one allocation each, previous flows through the table."""
    exact = np.float32(h // 2) / np.float32(h) == np.float32(0.5)
    assert exact == (h % 2 == 0)
    imgs, pimgs = S.images(2, w, h, seed=w), S.images(2, w, h, seed=w + 9)
    S.check_prepare(ctx, oracle, ("prev-scale", w, h), imgs, [0, 1], [1, 0], pimgs, S.prev_flows(2, w, h, h))


def test_prepare_motion_of_every_sum(ctx, oracle):
    """content.motion_sums_pair: every channel-difference sum 0 .. 765 at level 0 — shown on the oracle first."""
    i1, p1 = K.motion_sums_pair()
    h, w = i1.shape[:2]
    i0 = np.ascontiguousarray(np.roll(i1, 3, axis=1))
    imgs, pimgs = np.stack([i0, i1]), np.stack([np.ascontiguousarray(np.roll(p1, 3, axis=1)), p1])
    want = S.expected_prepare(oracle, "motion-sums", imgs, [0], [1], pimgs, S.prev_flows(1, w, h, 3))
    sums = {np.float32(k / np.float32(765.0)).view(np.uint32).item() for k in range(766)}
    assert sums <= set(np.unique(S.bits(want["motion"][0][1])).tolist())
    # (the division's precision cannot show: for all 766 sums the float quotient and the double quotient rounded to float agree)
    k = np.arange(766)
    assert np.array_equal(S.bits(k.astype(np.float32) / np.float32(765.0)), S.bits((k.astype(np.float64) / 765.0).astype(np.float32)))
    S.check_prepare(ctx, oracle, "motion-sums", imgs, [0], [1], pimgs, S.prev_flows(1, w, h, 3))


def test_prepare_motion_exactly_zero_and_one(ctx, oracle):
    w, h = 72, 60
    imgs = S.images(2, w, h, seed=77, alpha=255)
    imgs[1, :, : w // 2, :3] = 0
    pimgs = imgs.copy()
    pimgs[1, :, : w // 2, :3] = 255                 # sum 765 on the left half, 0 on the right
    want = S.expected_prepare(oracle, "motion-0-1", imgs, [0], [1], pimgs, S.prev_flows(1, w, h, 4))
    m = want["motion"][0][1]
    assert np.all(S.bits(m[:, :8]) == np.float32(1.0).view(np.uint32)) and np.all(S.bits(m[:, -8:]) == 0)
    assert any(np.any((lv[1] > 0) & (lv[1] < 1)) for lv in want["motion"])   # and the pyramid mixes them
    S.check_prepare(ctx, oracle, "motion-0-1", imgs, [0], [1], pimgs, S.prev_flows(1, w, h, 4))


@pytest.mark.parametrize("alpha", ["zero", "opaque", "stripes"])
def test_prepare_alpha_content(ctx, oracle, alpha):
    """Alpha of 0, of 255, and the stripes that make exactly 0.9f in the pyramid (PixFlow's update threshold)."""
    w, h = 150, 120
    a = {"zero": 0, "opaque": 255, "stripes": K.alpha_stripes(w, h, 5)}[alpha]
    imgs = S.images(2, w, h, seed=31, alpha=a)
    want = S.expected_prepare(oracle, ("alpha", alpha), imgs, [0], [1])
    if alpha == "stripes":
        assert any(np.any(S.bits(lv) == np.float32(0.9).view(np.uint32)) for lv in want["alpha"][1:])
    else:
        assert all(np.all(lv == (0.0 if alpha == "zero" else 1.0)) for lv in want["alpha"])
    S.check_prepare(ctx, oracle, ("alpha", alpha), imgs, [0], [1])


def test_prepare_special_previous_flows(ctx, oracle):
    """Previous flows of 0, -0.0, +-40 px, 1e-16 and subnormals beside ordinary values: a device build that flushes subnormals to
    zero fails here. The oracle's resized flow still holds subnormals at every level, zeros and +-40 * 37 / 75."""
    w, h = 75, 75
    imgs, pimgs, pf = S.images(2, w, h, seed=5), S.images(2, w, h, seed=6), S.prev_flows(2, w, h, 8, "special")
    assert S.is_subnormal(pf).any() and np.any(S.bits(pf) == 0x80000000)
    want = S.expected_prepare(oracle, "special-prev", imgs, [0, 1], [1, 0], pimgs, pf)
    for lv in want["prev"]:
        assert S.is_subnormal(lv).any()
    lv0 = want["prev"][0]
    assert np.any(S.bits(lv0) == 0) and not np.any(S.bits(lv0) == 0x80000000)   # (a block of -0.0 leaves the cubic resize as +0.0)
    assert np.any(lv0 == np.float32(40) * (np.float32(37) / np.float32(75))) and np.any(lv0 == np.float32(-40) * (np.float32(37) / np.float32(75)))
    S.check_prepare(ctx, oracle, "special-prev", imgs, [0, 1], [1, 0], pimgs, pf)


def test_prepare_repeat_calls_read_nothing_stale(ctx, oracle):
    """With previous state, then without, then smaller, then the first again — the engine's buffers left as they were (no fill), so
    a stale plane or table slot that is read shows as the earlier call's data."""
    big = (S.images(3, 120, 96, seed=1), [0, 1, 2], [1, 2, 0], S.images(3, 120, 96, seed=2), S.prev_flows(3, 120, 96, 1))
    small = (S.images(3, 62, 58, seed=3), [0, 1, 2], [1, 2, 0], S.images(3, 62, 58, seed=4), S.prev_flows(3, 62, 58, 2))
    S.check_prepare(ctx, oracle, "repeat-big", *big, fill=None)
    S.check_prepare(ctx, oracle, "repeat-big-first-frame", *big[:3], fill=None)
    S.check_prepare(ctx, oracle, "repeat-small", *small, fill=None)
    S.check_prepare(ctx, oracle, "repeat-small-first-frame", *small[:3], fill=None)
    S.check_prepare(ctx, oracle, "repeat-big", *big, fill=None)
    S.check_prepare(ctx, oracle, "repeat-small", *small, fill=S.FILL)


# ---- B: the linear resize on caller-made planes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh,dw,dh,tiled,why", S.LINEAR_DISPATCH + S.LINEAR_SHAPES,
                         ids=["%dx%d_%dx%d" % c[:4] for c in S.LINEAR_DISPATCH + S.LINEAR_SHAPES])
def test_linear_shapes_and_dispatch(ctx, oracle, sw, sh, dw, dh, tiled, why):
    """Both sides of the dispatch rule (the expected kernel is a literal of the case), ratio 1, upscales, mixed axes, tiny sources
    and destinations, tile edges, unaligned rows. Three planes of one channel (one per thread), then four of two channels."""
    S.check_linear(ctx, oracle, S.special_planes("mixed", 3, sh, sw, sw + dh), dw, dh, tiled)
    S.check_linear(ctx, oracle, S.noise_planes(4, sh, sw, sw + dw, cn=2), dw, dh, tiled)


def test_linear_unaligned_rows_and_the_piece_across_the_row_end(ctx, oracle):
    for sw, sh, dw, dh in ((143, 37, 129, 33), (71, 17, 64, 16), (37, 21, 33, 19), (9, 7, 8, 6)):
        assert sw % 4 != 0 and S.linear_piece_crosses_row_end(sw, dw)       # rows start off 16 bytes; a piece crosses the row's end
        S.check_linear(ctx, oracle, S.noise_planes(2, sh, sw, sw), dw, dh, True)
    assert not S.linear_piece_crosses_row_end(64, 64)
    S.check_linear(ctx, oracle, S.noise_planes(2, 16, 64, 1), 64, 16, True)


@pytest.mark.parametrize("sw,sh,dw,dh,planes,wgs", S.LINEAR_GRIDS, ids=["%d_workgroups" % c[5] for c in S.LINEAR_GRIDS])
def test_linear_grid_sizes_around_the_tile_redeal(ctx, oracle, sw, sh, dw, dh, planes, wgs):
    """xcd_tile deals the workgroups out differently from 64 on: exactly 63, 64 and 65, and a batch of 66 with partial last tiles."""
    assert S.workgroups(dw, dh, planes) == wgs
    if wgs == 66:
        assert dw % S.TW and dh % S.TH
    S.check_linear(ctx, oracle, S.noise_planes(planes, sh, sw, wgs), dw, dh, True, against_c2=(wgs != 64))


@pytest.mark.parametrize("post_scale,do_scale", S.SCALES, ids=["unscaled", "x0.5", "x1_0.9"])
@pytest.mark.parametrize("planes", S.PLANE_COUNTS)
def test_linear_planes_per_thread(ctx, oracle, planes, post_scale, do_scale):
    """B = 1, 2, 3, 4, 6, 8 through the tiled kernel, the generic one-channel kernel (a shape outside the rule: production never
    launches it) and the two-channel kernel, unscaled and with both kinds of factor."""
    S.check_linear(ctx, oracle, S.noise_planes(planes, 20, 72, planes), 65, 18, True, post_scale, do_scale, against_c2=False)
    S.check_linear(ctx, oracle, S.noise_planes(planes, 39, 80, planes + 10), 70, 32, False, post_scale, do_scale)
    S.check_linear(ctx, oracle, S.noise_planes(planes, 20, 72, planes + 20, cn=2), 65, 18, True, post_scale, do_scale)


@pytest.mark.parametrize("kind", S.CONTENT)
def test_linear_content(ctx, oracle, kind):
    """Constants, -0.0, subnormals, single ones in the corners and beside the tile borders — through both one-channel kernels and the
    two-channel one, at x0.9 and upscaled."""
    if kind == "subnormal":
        src = S.special_planes(kind, 2, 36, 143, 1)
        assert S.is_subnormal(src).any() and S.is_subnormal(S.want_linear(oracle, src, 129, 32, 1.0, False)).any()
    for cn in (1, 2):
        S.check_linear(ctx, oracle, S.special_planes(kind, 2, 36, 143, 1, cn), 129, 32, True)
        S.check_linear(ctx, oracle, S.special_planes(kind, 2, 40, 150, 2, cn), 129, 32, False)
        S.check_linear(ctx, oracle, S.special_planes(kind, 2, 17, 65, 3, cn), 130, 35, True, 0.5, True)


# ---- C: the cubic flow resize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh,dw,dh,why", S.CUBIC_TILED, ids=["%dx%d_%dx%d" % c[:4] for c in S.CUBIC_TILED])
def test_cubic_tiled_upscales(ctx, oracle, sw, sh, dw, dh, why):
    """x1/0.9 from both ends of the pyramid, ratio 1, x2, x7, sources of 1 .. 3 pixels, destinations on the tile's edges; each also
    through the pointer table, which forces the generic kernel; batches of 1 and 3; the engine's own factor."""
    S.check_cubic(ctx, oracle, S.special_planes("mixed", 3, sh, sw, sw, cn=2), dw, dh, True, S.INV_PYR)
    S.check_cubic(ctx, oracle, S.noise_planes(1, sh, sw, dw, cn=2), dw, dh, True, 1.0, table_too=False)


def test_cubic_window_with_and_without_extra_columns(ctx, oracle):
    """The window's columns beyond 64 (W > 64) present and absent, shown on the restatement of the window. The pyramid's own x1/0.9
    never has them (64 destination columns span at most 0.92 * 63 + 4 = 61 source columns): only ratios near 1 reach that loop."""
    for sw, dw, extra in ((130, 130, True), (70, 70, True), (69, 70, True), (68, 70, False), (63, 70, False), (20, 64, False), (33, 66, False)):
        widths = [e for _, e in S.cubic_window(sw, dw, "x")]
        assert (max(widths) > S.TW) == extra, widths
        S.check_cubic(ctx, oracle, S.noise_planes(2, 20, sw, sw, cn=2), dw, 20, True, S.INV_PYR)


@pytest.mark.parametrize("sw,sh,dw,dh,why", S.CUBIC_GENERIC, ids=["%dx%d_%dx%d" % c[:4] for c in S.CUBIC_GENERIC])
def test_cubic_generic_downscales_and_mixed_axes(ctx, oracle, sw, sh, dw, dh, why):
    """A downscale on either axis must not go tiled (the window would not fit)."""
    S.check_cubic(ctx, oracle, S.special_planes("mixed", 3, sh, sw, sh, cn=2), dw, dh, False, S.ODD_H_SCALE)


@pytest.mark.parametrize("sw,sh,dw,dh,flows,wgs", S.CUBIC_GRIDS, ids=["%d_workgroups_%d" % (c[5], c[4]) for c in S.CUBIC_GRIDS])
def test_cubic_grid_sizes(ctx, oracle, sw, sh, dw, dh, flows, wgs):
    assert S.workgroups(dw, dh, flows, ppt=1) == wgs
    S.check_cubic(ctx, oracle, S.noise_planes(flows, sh, sw, wgs, cn=2), dw, dh, True, S.INV_PYR, table_too=False)


@pytest.mark.parametrize("post_scale", S.CUBIC_SCALES, ids=["x1", "x1_0.9f", "x37_75"])
def test_cubic_post_scale(ctx, oracle, post_scale):
    """The engine's own two factors as it computes them, and 1: tiled, generic, and through the table."""
    assert S.INV_PYR == float(np.float32(1.0) / np.float32(0.9)) and S.ODD_H_SCALE == float(np.float32(37) / np.float32(75))
    S.check_cubic(ctx, oracle, S.noise_planes(2, 30, 64, 5, cn=2), 71, 33, True, post_scale)
    S.check_cubic(ctx, oracle, S.noise_planes(2, 75, 75, 6, cn=2), 37, 37, False, post_scale)


@pytest.mark.parametrize("kind", S.CONTENT)
def test_cubic_content(ctx, oracle, kind):
    """As for the linear resize; a window of -0.0 comes out as +0.0 wherever one of its weights is negative (the existing content
    test describes it) — shown on the oracle's result first."""
    src = S.special_planes(kind, 2, 30, 64, 9, cn=2)
    if kind == "negzero":
        assert np.all(S.bits(S.want_cubic(oracle, src, 71, 33, 1.0)) == 0)             # every window has a negative weight: +0.0
        assert np.all(S.bits(S.want_cubic(oracle, src, 64, 30, 1.0)) == 0x80000000)    # ratio 1: weights 0, 1, 0, 0 keep -0.0
        S.check_cubic(ctx, oracle, src, 64, 30, True, 1.0)
    if kind == "subnormal":
        assert S.is_subnormal(S.want_cubic(oracle, src, 71, 33, 1.0)).any()
    S.check_cubic(ctx, oracle, src, 71, 33, True, S.INV_PYR)
    S.check_cubic(ctx, oracle, S.special_planes(kind, 2, 61, 75, 10, cn=2), 37, 30, False, S.ODD_H_SCALE)


# ---- the taps themselves ------------------------------------------------------------------------------------------------------------------
def test_test_taps_are_declared_listed_and_exported(s360lib):
    from surround360_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360_debug_flow_pyramid.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_FLOW_PYRAMID_SYMBOLS) == ["s360_debug_flow_prepare", "s360_debug_resize_cubic_flow",
                                                                 "s360_debug_resize_linear_f32"]
    for n in names:
        assert hasattr(s360lib, n), n


def test_taps_refuse_bad_arguments(ctx):
    from surround360_amd._capi import S360Error
    img = S.images(2, 8, 8)
    for kw in (dict(images=img[:, :3]),                                   # 1 row after the entry downscale
               dict(i0=[2]), dict(i1=[-1]),                              # index outside [0, N)
               dict(prev_images=img), dict(prev_flows=np.zeros((1, 8, 8, 2), np.float32))):   # previous state half given
        args = dict(images=img, i0=[0], i1=[1])
        args.update(kw)
        with pytest.raises(S360Error) as e:
            ctx.debug_flow_prepare(**args)
        assert e.value.code == -1, kw
    with pytest.raises(S360Error):
        ctx.debug_resize_linear_f32(np.zeros((1, 4, 4, 3), np.float32), 4, 4)   # three channels
