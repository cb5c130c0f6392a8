"""k_debug_views (surround360_amd/csrc/debug_views.hip: the crops, wrapped panoramas, padded layers and 3-channel eyes of
s360_set_debug_images) through its test tap, include/s360_debug_views.h, against a numpy restatement — crop, np.roll, zero pad,
drop alpha — byte for byte, canary bytes behind every destination included. The views: tests/debug_views_cases.py."""
import numpy as np
import pytest

import debug_views_cases as V
from surround360_amd import _capi, debug_images as DI, render as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=7, eqr_height=3))  # (no renderable frame: the tap works on any context)
    yield c
    c.close()


def test_every_view_in_one_call(ctx):
    V.check_all(ctx)


def test_one_view_alone_and_the_pixel_paths(ctx):
    """A single descriptor per call (grid.y = 1), for a row that takes the 16-byte load (aligned source, no wrap), the pixel loads
    (a wrap inside the chunk; a source row that is not 16-byte aligned) and the byte stores (3 channels, odd width)."""
    for v in (dict(w=64, h=4, shift=0, pad_rows=0, channels_out=4, base=0, x0=0, y0=0, src_pitch=64, src_rows=4),
              dict(w=64, h=4, shift=2, pad_rows=1, channels_out=4, base=4, x0=0, y0=0, src_pitch=64, src_rows=4),
              dict(w=61, h=5, shift=20, pad_rows=2, channels_out=4, base=0, x0=1, y0=1, src_pitch=63, src_rows=7),
              dict(w=61, h=5, shift=20, pad_rows=2, channels_out=3, base=4, x0=1, y0=1, src_pitch=63, src_rows=7)):
        taps, src, dst, want = V.layout([v], seed=9)
        assert np.array_equal(DI.debug_views(ctx, taps, src, dst), want), v


def test_descriptors_the_kernel_would_not_index_are_refused(ctx):
    good = dict(src_off=0, dst_off=0, src_pitch=8, src_rows=4, x0=1, y0=1, w=6, h=3, shift=2, pad_rows=1, channels_in=4, channels_out=3)
    src, dst = np.zeros(8 * 4 * 4, np.uint8), np.zeros(6 * 4 * 3, np.uint8)
    DI.debug_views(ctx, [good], src, dst)
    for k, val in (("x0", 3), ("y0", 2), ("x0", -1), ("shift", 6), ("shift", -1), ("channels_out", 2), ("channels_in", 3), ("w", 0),
                   ("pad_rows", 2), ("pad_rows", -1), ("src_off", 4), ("src_off", 2), ("dst_off", 4), ("src_rows", 5), ("h", 0)):
        with pytest.raises(_capi.S360Error) as e:
            DI.debug_views(ctx, [dict(good, **{k: val})], src, dst)
        assert e.value.code == _capi.ERR_INVALID_ARG, (k, val)
    with pytest.raises(_capi.S360Error):
        DI.debug_views(ctx, [dict(good, channels_out=4, dst_off=2)], src, np.zeros(200, np.uint8))
