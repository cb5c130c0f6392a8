"""GPU parity of the stereo cubemap kernels of every frame (render_kernels.hip: k_cubemap_pack + k_cubemap_tiles) and of the
on-demand kernel (k_cubemap), kernel level, through the test taps of include/s360_debug_cubemap.h on caller-made eyes: face maps
against the oracle's bit for bit, tile records and packed dwords against the integer restatement, every slot's pixels against the
oracle's stereoCubemap and against the on-demand kernel, word for word, nothing left out. The cases — legal-frame sizes whose pole
boxes wrap in y, eyes below 28 pixels at the documented limits of the box load's wrap, all-gather shapes, odd and degenerate
faces, both LDS box sizes, xcd_tile's grid classes, 17 slots — are tests/cubemap_tiles_cases.py's; each proves on the restatement
that it reaches its classes before anything is compared."""
import numpy as np
import pytest

import cubemap_tiles_cases as S
from surround360_amd import _capi, render as R

pytestmark = pytest.mark.gpu
FORMATS = ["video", "photo"]


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    yield c
    c.close()


def _taps(ctx):
    return (lambda eyes, fw, fh, fmt, cap, fill: ctx.debug_cubemap_tiles(eyes, fw, fh, fmt, cap, fill),
            lambda eyes, fw, fh, fmt, fill: ctx.debug_cubemap(eyes, fw, fh, fmt, fill))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_shape(ctx, oracle, name, fmt):
    """Two slots of noise (random alpha bytes) per shape and layout, 4096-pixel box; the classes the shape is listed with in
    cubemap_tiles_cases.SHAPES are asserted as reached first. Measured with the restatement (tiles of one eye: lds, y0 < 0, past sh,
    x0 < 0, past sw, past 2 sw, shifted, gather by area, box of exactly 4096, height 1023, 4 x 1024, gather by limits, x limit alone,
    y limit alone, partial x, partial y; a / b = "video" / "photo"):
      legal-28x14-16x16                    6: 6 1 1 0 3 0 3 0 0 0 0 0 0 0 0 0
      legal-28x14-33x17                   36: 36 2 2 2 4/6 0 2/6 0 0 0 0 0 0 0 12 18
      legal-64x32-96x96                  216: 216 4 4 9 15 0 3 0 0 0 0 0 0 0 0 0
      limits-12x6-20x20                   24: 24 1 12 0 9/12 0 4/6 0 0 0 0 0 0 0 12 12
      limits-3x3-20x12                    12: 12 10 10 2 11 2 3/5 0 0 0 0 0 0 0 6 12
      limits-3x3-18x12                    12: 12 10 10 2 11 2 3/5 0 0 0 0 0 0 0 6 12
      limits-2x2-16x16                     6: 5 5 5 2 5 2 2 0 0 0 0 1 0 1 0 0
      limits-2x2-17x16                    12: 12 10 12 7/5 12 2/4 2/4 0 0 0 0 0 0 0 6 0
      limits-1x2-33x17                    36: 32/30 16/15 32/30 32/30 32/30 32/30 0 0 0 0 0 4/6 4/6 0 12 18
      limits-1x3-16x16                     6: 3 3 3 3 3 3 0 0 0 0 0 3 3 0 0 0
      limits-1x5-17x16                    12: 9/7 0 8/7 9/7 9/7 9/7 0 0 0 0 0 3/5 3/5 0 6 0
      limits-7x2-16x16                     6: 5 5 5 1 3 0 2 0 0 0 0 1 0 1 0 0
      all_gather_limits-5x1-16x16          6: 0 0 0 0 0 0 0 0 0 0 0 6 0 6 0 0
      all_gather_limits-5x1-18x16         12: 0 0 0 0 0 0 0 0 0 0 0 12 0 12 6 0
      odd-301x77-37x53                    72: 70 0 0 0 6 0 6 2 0 0 0 0 0 0 24 18
      odd-301x77-36x53                    72: 70 0 0 0 6 0 6 2 0 0 0 0 0 0 24 18
      degenerate-28x14-1x17               12: 12 0 0 0 0 0 0 0 0 0 0 0 0 0 12 6
      degenerate-28x14-20x1               12: 12 0 0 0 1 0 1 0 0 0 0 0 0 0 6 12
      degenerate-28x14-1x1                 6: 6 0 0 0 0 0 0 0 0 0 0 0 0 0 6 6
      degenerate-28x14-4x1                 6: 6 0 0 0 1 0 1 0 0 0 0 0 0 0 6 6
      all_gather_area-2048x1024-32x32     24: 0 0 0 0 0 0 0 24 0 0 0 0 0 0 0 0
      all_gather_area-2048x1024-30x32     24: 0 0 0 0 0 0 0 24 0 0 0 0 0 0 12 0
      exact_cap-499x249-32x32             24: 16 0 0 0 2 0 0 8 4 0 0 0 0 0 0 0
      tall-1x2736-1x16                     6: 6 0 0 6 6 6 0 0 0 4 0 0 0 0 6 0
      tall-1x2739-1x16                     6: 2 0 0 2 2 2 0 4 0 0 4 0 0 0 6 0"""
    sw, sh, fw, fh, reaches = S.SHAPES[name]
    eyes = S.noise_eyes(sw * 1000 + fw, 2, sw, sh)
    assert len({int(v) for v in eyes[..., 3].ravel()}) > 1 or sw * sh == 1
    S.check_case(*_taps(ctx), oracle, eyes, fw, fh, fmt, 4096, reaches)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh,fw,fh", S.BOTH_BOXES, ids=["%dx%d-%dx%d" % s for s in S.BOTH_BOXES])
@pytest.mark.parametrize("cap", [4096, 2560])
def test_both_box_sizes(ctx, oracle, cap, sw, sh, fw, fh, fmt):
    """700 x 350 eyes -> 40 x 40 (42 x 40) faces: 54 tiles, 26 (24) from LDS with the 4096-pixel box, 14 with the 2560-pixel one;
    the records of the two differ (asserted), the pixels do not. Both instantiations in one process."""
    eyes = S.noise_eyes(cap + fw, 1, sw, sh)
    S.check_case(*_taps(ctx), oracle, eyes, fw, fh, fmt, cap, ("lds", "gather_area", "partial_x", "partial_y"),
                 expect_different_from=4096 + 2560 - cap)


def test_box_of_exactly_the_small_capacity(ctx, oracle):
    """254 x 127 eyes -> 32 x 32 faces: one tile's box is 64 x 40 = 2560 pixels and must render from LDS (`> CAP`, not `>=`)."""
    S.check_case(*_taps(ctx), oracle, S.noise_eyes(2560, 1, 254, 127), 32, 32, "video", 2560, ("lds_exact_cap", "gather_area"))


@pytest.mark.parametrize("cap", [4096, 2560])
@pytest.mark.parametrize("sw,sh,fw,fh", [(28, 14, 33, 17), (3, 3, 20, 12)])
def test_small_box_at_the_wrap_shapes(ctx, oracle, sw, sh, fw, fh, cap):
    """The y wrap and the second step up in x through the 2560-pixel instantiation as well."""
    S.check_case(*_taps(ctx), oracle, S.noise_eyes(cap, 2, sw, sh), fw, fh, "video", cap, ("lds_y0_negative", "lds_past_sh", "lds_past_sw"))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(S.GRIDS))
def test_grid_class(ctx, oracle, name, fmt):
    """xcd_tile's re-deal of the workgroups of k_cubemap_tiles, T = tiles x * 6 tiles y * 2 eyes * slots: T = 12 (< 64), T = 72
    (T % 8 == 0), T = 108 (T % 8 == 4); every pixel stored once."""
    sw, sh, fw, fh, slots, T = S.GRIDS[name]
    assert -(-fw // 16) * 6 * -(-fh // 16) * 2 * slots == T and (T < 64 or (T % 8 == 0) == (name == "T72"))
    S.check_case(*_taps(ctx), oracle, S.noise_eyes(T, slots, sw, sh), fw, fh, fmt, 4096, ("lds",))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("sw,sh,fw,fh", [(28, 14, 33, 17), (64, 32, 40, 40), (3, 3, 20, 12), (301, 77, 36, 53)])
def test_checker_reaches_both_ends_of_the_saturation(ctx, oracle, sw, sh, fw, fh, fmt):
    """0 / 255 eyes: the sums before sat_u8 pass below 0 and above 255 — shown by the unclamped numpy restatement of the taps, which
    check_case first pins to the oracle's pixels — and both 0 and 255 are among the expected bytes."""
    S.check_case(*_taps(ctx), oracle, S.checker_eyes(fw, 2, sw, sh), fw, fh, fmt, 4096, ("lds",), overshoot=True)


@pytest.mark.parametrize("sw,sh,fw,fh,fmt", S.SEVENTEEN, ids=["%dx%d-%dx%d-%s" % s for s in S.SEVENTEEN])
def test_seventeen_slots(ctx, oracle, sw, sh, fw, fh, fmt):
    """Two launches of k_cubemap_tiles, the second with base 16 into the pointer lists: 34 different eyes, every slot's cubemap
    against the oracle's for that slot, the fill byte nowhere."""
    eyes = S.noise_eyes(17, S.MAX_SLOTS + 1, sw, sh)
    S.check_case(*_taps(ctx), oracle, eyes, fw, fh, fmt, 4096, ("lds", "lds_y0_negative", "lds_past_sh", "lds_past_sw", "partial_x"))


def test_bad_arguments_are_refused(ctx):
    eyes = np.zeros((1, 2, 4, 4, 4), np.uint8)
    with pytest.raises(_capi.S360Error) as e:
        ctx.debug_cubemap_tiles(eyes, 8, 8, "video", 4095)
    assert e.value.code == _capi.ERR_INVALID_ARG
    L, C = _capi.lib(), R.C
    out, maps = np.zeros((32, 24, 3), np.uint8), np.zeros((6, 8, 8, 2), np.float32)
    packed, tiles = np.zeros((16, 24), np.uint32), np.zeros((6, 1, 1, 4), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ctx.h, p(eyes), 1, 4, 4, 8, 8, 1, 4096, p(out), p(maps), p(packed), p(tiles)]
    assert L.s360_debug_cubemap_tiles(*good) == 0
    for k, v in ((1, None), (9, None), (10, None), (11, None), (12, None), (2, 0), (2, 65), (3, 0), (4, -1), (5, 0), (6, 0), (7, 2), (8, 0),
                 (8, 2561)):
        a = list(good)
        a[k] = v
        assert L.s360_debug_cubemap_tiles(*a) == _capi.ERR_INVALID_ARG, (k, v)
    assert L.s360_debug_cubemap(ctx.h, p(eyes), 1, 4, 4, 8, 8, 1, p(out), p(maps)) == 0
    for k, v in ((1, None), (8, None), (9, None), (2, 0), (3, 0), (6, -3), (7, 2)):
        a = [ctx.h, p(eyes), 1, 4, 4, 8, 8, 1, p(out), p(maps)]
        a[k] = v
        assert L.s360_debug_cubemap(*a) == _capi.ERR_INVALID_ARG, (k, v)
    assert L.s360_debug_cubemap_tiles(*([None] + good[1:])) == _capi.ERR_INVALID_ARG


def test_test_taps_are_declared_listed_and_exported(s360lib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "s360_debug_cubemap.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_CUBEMAP_SYMBOLS) == ["s360_debug_cubemap", "s360_debug_cubemap_tiles"]
    for n in names:
        assert hasattr(s360lib, n), n
