"""GPU parity of PixFlow's entry downscale through LDS (flow_kernels.hip: k_resize_cubic_u8c4_tiled, launch_entry_downscale).

Kernel level, through the library's test tap (s360_debug_entry_downscale): the shapes of tests/test_cpu_entry_downscale.py on the
device — the tiled kernel against the one-thread-per-pixel kernel it replaces and against the oracle's resize, byte for byte; its
grey and alpha planes against k_gray_alpha on the device, bit for bit; with the resized image stored and not stored; shapes whose
source box does not fit, which must take the generic kernels.
Then whole flows against the oracle: without temporal state (the downscaled image is not stored) and chained (it is, and the
previous images go through the same kernel), at sizes where both axes are halved exactly, neither is, and the side crops' mix."""
import numpy as np
import pytest

import test_cpu_entry_downscale as E
from surround360_amd import render as R, synth

pytestmark = pytest.mark.gpu

SIZES = {"both_exact": (260, 148), "neither_exact_odd_output_width": (243, 131), "width_exact_height_not": (268, 177)}


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (name, int(bad.sum()), bad.size, np.argwhere(bad)[0])


@pytest.mark.parametrize("sw,sh,dw,dh,tiled", E.SHAPES, ids=E.IDS)
def test_entry_downscale_on_the_device(ctx, oracle, sw, sh, dw, dh, tiled):
    src = E._images(sw, sh)
    g_down, g_gray, g_alpha, _ = ctx.debug_entry_downscale(src, dw, dh, generic=True)
    for b in range(len(src)):
        assert np.array_equal(g_down[b], oracle.resize_cubic_u8(src[b], dw, dh)), "generic kernel against the oracle, image %d" % b
    down, gray, alpha, took = ctx.debug_entry_downscale(src, dw, dh)
    assert took == tiled, "the shape went to the %s kernel" % ("tiled" if took else "generic")
    assert np.array_equal(down, g_down), "image against k_resize_cubic_u8c4"
    _same("grey plane against k_gray_alpha", gray, g_gray)
    _same("alpha plane against k_gray_alpha", alpha, g_alpha)
    _, gray2, alpha2, _ = ctx.debug_entry_downscale(src, dw, dh, keep_down=False)  # as without previous images
    _same("grey plane, image not stored", gray2, g_gray)
    _same("alpha plane, image not stored", alpha2, g_alpha)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_flows_through_the_tiled_entry(ctx, oracle, name):
    w, h = SIZES[name]
    i0, i1 = synth.flow_pair(w, h, seed=11)  # (noise with a feathered alpha border: alphas of every value)
    want = oracle.compute_optical_flow(i0, i1, "pixflow_low", "LEFT")
    _same(name, ctx.compute_optical_flow(i0, i1, "pixflow_low", "LEFT"), want)
    prev_flow = np.ascontiguousarray(want * np.float32(0.5) + np.float32(0.25))
    p0, p1 = np.ascontiguousarray(np.roll(i0, 2, axis=1)), np.ascontiguousarray(np.roll(i1, 1, axis=0))
    chained = oracle.compute_optical_flow(i0, i1, "pixflow_low", "LEFT", prev_flow=prev_flow, prev_i0=p0, prev_i1=p1)
    _same(name + " chained", ctx.compute_optical_flow(i0, i1, "pixflow_low", "LEFT", prev_flow=prev_flow, prev_i0=p0, prev_i1=p1),
          chained)
    # ... and once more without: the stored image of the chained call must not be what this one reads
    _same(name + " again", ctx.compute_optical_flow(i0, i1, "pixflow_low", "LEFT"), want)
