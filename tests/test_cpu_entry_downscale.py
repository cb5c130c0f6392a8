"""PixFlow's entry downscale through LDS (flow_kernels.hip: k_resize_cubic_u8c4_tiled, launch_entry_downscale) without a GPU,
on the CPU emulation of the HIP sources (tools/flow_emulate.cpp).

The tiled kernel against the one-thread-per-pixel kernel it replaces and against the oracle's resize, byte for byte; its grey
and alpha planes against k_gray_alpha on the resized image and against the oracle's entry, bit for bit; with the resized image
stored (batches with previous images) and not stored. Shapes: the benchmark's two (1214x1769 -> 607x884, 10080x2104 ->
5040x1052) scaled down, exact halvings (the 10-column wide-read path) and odd sizes (the per-tap path, and the scalar tail
column of an odd output width), several tiles with ragged edges, images smaller than the filter, and shapes whose source box
does not fit, which must take the generic kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "libflow_emu.so"])
    lib = C.CDLL(os.path.join(ROOT, "tools", "libflow_emu.so"))
    lib.emu_resize_cubic_u8c4.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.emu_resize_cubic_u8c4_generic.argtypes = lib.emu_resize_cubic_u8c4.argtypes
    lib.emu_entry_downscale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int]
    lib.emu_gray_alpha.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _images(sw, sh, n=2):
    """Noise; the left half 0 / 255 only, where the cubic over- and undershoots into the saturation."""
    rng = np.random.RandomState(sw * 7 + sh)
    src = rng.randint(0, 256, (n, sh, sw, 4)).astype(np.uint8)
    src[:, :, : sw // 2] = np.where(rng.rand(n, sh, sw // 2, 4) < 0.5, 0, 255).astype(np.uint8)
    return src


# (sw, sh, dw, dh, tiled): the last says which kernel must take the shape
SHAPES = [
    (242, 354, 121, 177, True),    # the side crops' shape / 5 (1214x1769 -> 607x884: width halved exactly, height not), odd output width
    (1214, 70, 607, 35, True),     # their full width: 10 tiles per row, the last 31 columns wide with the tail column
    (504, 106, 252, 53, True),     # the pole images' shape / 20 (10080x2104 -> 5040x1052): both axes halved exactly
    (260, 72, 130, 36, True),      # exact halving, even width: 3 x 3 tiles, ragged at the right and at the bottom
    (243, 355, 121, 177, True),    # odd sources: neither axis exact (scale 2.008 / 2.006), per-tap path, odd output width
    (331, 271, 165, 135, True),    # tests/test_gpu_known_result.py's flow size
    (129, 33, 64, 16, True),       # exactly one tile, odd sources
    (131, 37, 65, 18, True),       # one column and two rows more than a tile
    (7, 5, 3, 2, True),            # smaller than the filter: every tap clamped
    (5, 4, 2, 2, True),            # scale 2.5 on two columns
    (300, 100, 200, 50, True),     # scale 1.5 horizontally: the lower end of "around 2"
    (300, 40, 140, 20, False),     # 2.14: a 64-column tile's source box has 140 columns
    (100, 160, 50, 64, False),     # 2.5 vertically
    (240, 90, 80, 30, False),      # x3
    (100, 40, 90, 36, False),      # 1.11: not around 2
]
IDS = ["%dx%d_to_%dx%d" % s[:4] for s in SHAPES]


@pytest.mark.parametrize("sw,sh,dw,dh,tiled", SHAPES, ids=IDS)
@pytest.mark.parametrize("keep_down", [True, False], ids=["with_previous_images", "without"])
def test_entry_downscale(emu, sw, sh, dw, dh, tiled, keep_down):
    """The entry launch as FlowEngine makes it (sources by table): image, grey and alpha planes."""
    src = _images(sw, sh)
    generic = np.zeros((2, dh, dw, 4), np.uint8)
    assert emu.emu_resize_cubic_u8c4_generic(_vp(src), sw, sh, 2, dw, dh, _vp(generic)) == 0
    want_g = np.zeros((2, dh, dw), np.float32)
    want_a = np.zeros((2, dh, dw), np.float32)
    assert emu.emu_gray_alpha(_vp(generic), dw * dh, 2, _vp(want_g), _vp(want_a)) == 0
    down = np.full((2, dh, dw, 4), 7, np.uint8) if keep_down else None
    gray = np.full((2, dh, dw), 7.0, np.float32)
    alpha = np.full((2, dh, dw), 7.0, np.float32)
    took = emu.emu_entry_downscale(_vp(src), sw, sh, 2, dw, dh, _vp(down), _vp(gray), _vp(alpha), 1)
    assert took == (1 if tiled else 0), "the shape went to the %s kernel" % ("tiled" if took else "generic")
    for b in range(2):
        want = O.resize_cubic_u8(src[b], dw, dh)
        assert np.array_equal(generic[b], want), "generic kernel against the oracle, image %d" % b
        if keep_down:
            assert np.array_equal(down[b], want), "image %d" % b
        inv255 = np.float32(1.0 / 255.0)
        g8 = (want[..., 0].astype(np.int64) * 1868 + want[..., 1].astype(np.int64) * 9617 + want[..., 2].astype(np.int64) * 4899
              + (1 << 13)) >> 14
        assert np.array_equal(_bits(gray[b]), _bits(g8.astype(np.float32) * inv255)), "grey plane against its formula, image %d" % b
        assert np.array_equal(_bits(alpha[b]), _bits(want[..., 3].astype(np.float32) * inv255)), "alpha plane, image %d" % b
    assert np.array_equal(_bits(gray), _bits(want_g)) and np.array_equal(_bits(alpha), _bits(want_a)), "against k_gray_alpha"


@pytest.mark.parametrize("sw,sh,dw,dh,tiled", SHAPES, ids=IDS)
def test_resize_launcher(emu, sw, sh, dw, dh, tiled):
    """launch_resize_cubic_u8c4 (the previous images' downscale; sources in one allocation here) takes the same kernel."""
    src = _images(sw, sh)
    out = np.full((2, dh, dw, 4), 7, np.uint8)
    assert emu.emu_resize_cubic_u8c4(_vp(src), sw, sh, 2, dw, dh, _vp(out)) == 0
    for b in range(2):
        assert np.array_equal(out[b], O.resize_cubic_u8(src[b], dw, dh)), "image %d" % b


def test_entry_equals_the_oracles_entry(emu):
    """x0.5 of an odd-sized picture with a feathered alpha, against the oracle's PixFlow entry (before the 5x5 pre-blur the
    grey plane is not exposed: its alpha plane and its image are)."""
    from surround360_amd import synth
    i0, _ = synth.flow_pair(331, 271, seed=3)
    down_want, _, alpha_want = O.pixflow_entry(i0)
    dh, dw = alpha_want.shape
    src = np.ascontiguousarray(i0[None])
    down = np.zeros((1, dh, dw, 4), np.uint8)
    gray = np.zeros((1, dh, dw), np.float32)
    alpha = np.zeros((1, dh, dw), np.float32)
    assert emu.emu_entry_downscale(_vp(src), 331, 271, 1, dw, dh, _vp(down), _vp(gray), _vp(alpha), 0) == 1
    assert np.array_equal(down[0], down_want)
    assert np.array_equal(_bits(alpha[0]), _bits(alpha_want))


def test_test_tap_is_declared_listed_and_exported(s360lib):
    """include/s360_debug.h declares the entry's test tap, surround360_amd/_capi.py lists it, the library exports it."""
    import re
    from surround360_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360_debug.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_SYMBOLS) == ["s360_debug_entry_downscale"]
    for n in names:
        assert hasattr(s360lib, n), n
