"""GPU parity of the frame's packed bicubic remap (render_kernels.hip: k_remap_pack + k_remap_cubic_u8c4_packed — the 14 side
projections, both pole projections and the pole warp of every frame) and of pole removal's warp (k_remap_cubic_u8c4_tiled
<MapFromFlowAdd>), kernel level, through the test taps of include/s360_debug_remap.h on caller-made maps and flows: pixels against
the oracle, packed dwords and tile records against the numpy restatement, word for word, nothing left out. The cases — grid
classes of xcd_tile, tile classes, box limits, map values, sources, weights, feather — are tests/remap_packed_cases.py's; each
proves on the restatement that it reaches its class before anything is compared."""
import pytest

import remap_packed_cases as S
from surround360_amd import _capi, render as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    yield c
    c.close()


def _run(ctx):
    return lambda src, mp, mode, start, size, weights, fill: ctx.debug_remap_packed(src, mp, mode, start, size, weights, fill)


@pytest.mark.parametrize("name", list(S.GRIDS))
def test_grid_class(ctx, oracle, name):
    """xcd_tile's re-deal of the workgroups: 1 tile, T < 64, T = 64, T % 8 = 1 and 7, a batch in z; every pixel stored once."""
    S.check_case(_run(ctx), oracle, S.grid_case(name))


@pytest.mark.parametrize("source", ["noise", "checker"])
def test_tile_classes(ctx, oracle, source):
    """16 tile classes (no live pixel, boxes over every edge and two corners, live beside far dead pixels, the 4096-pixel limit
    from both sides, a gathered tile with both tap branches, the special map values, half-way coordinates), rotated over a batch
    of three."""
    S.check_case(_run(ctx), oracle, S.classes_case(getattr(S, source)))


def test_tall_boxes(ctx, oracle):
    """4 x 1020, 4 x 1023 and 4 x 512 fit; 4 x 1024 falls back through the height field's limit, 5 x 1000 through the area."""
    S.check_case(_run(ctx), oracle, S.tall_case())


@pytest.mark.parametrize("sw,sh", S.TINY, ids=["%dx%d" % s for s in S.TINY])
def test_tiny_source(ctx, oracle, sw, sh):
    S.check_case(_run(ctx), oracle, S.tiny_case(sw, sh))


def test_checker_reaches_both_ends_of_the_saturation(ctx, oracle):
    S.check_case(_run(ctx), oracle, S.checker_case(oracle))


@pytest.mark.parametrize("alpha_mode,feather_size", S.FEATHERS, ids=["mode%d-feather%d" % f for f in S.FEATHERS])
def test_feather(ctx, oracle, alpha_mode, feather_size):
    S.check_case(_run(ctx), oracle, S.feather_case(oracle, alpha_mode, feather_size))


@pytest.mark.parametrize("alpha_mode", [0, 1, 2])
def test_every_fraction_index_every_tap(ctx, oracle, alpha_mode):
    """The table and the weights rebuilt in the kernel (and the configured choice) against the oracle on 32 samples per fraction
    index, each on a rounding boundary of one tap (S.weights_case has the arithmetic)."""
    S.check_case(_run(ctx), oracle, S.weights_case(oracle, alpha_mode))


@pytest.mark.parametrize("flow,ramp", S.POLE_CASES, ids=["%s-%s" % c for c in S.POLE_CASES])
def test_pole_warp(ctx, oracle, flow, ramp):
    S.check_pole_warp(lambda ext, fl, radius, start, mid, end, fill: ctx.debug_pole_warp_packed(ext, fl, radius, start, mid, end, fill),
                      oracle, flow, ramp)


@pytest.mark.parametrize("kind,w,h", S.BY_FLOW, ids=[c[0] for c in S.BY_FLOW])
def test_remap_by_flow(ctx, oracle, kind, w, h):
    S.check_remap_by_flow(lambda src, fl, fill: ctx.debug_remap_by_flow(src, fl, fill), oracle, kind, w, h)


def test_bad_arguments_are_refused(ctx):
    import numpy as np
    src, mp = np.zeros((1, 4, 4, 4), np.uint8), np.zeros((1, 3, 5, 2), np.float32)
    for kw in (dict(alpha_mode=3), dict(weights=3), dict(alpha_mode=1, feather_size=0)):
        with pytest.raises(_capi.S360Error) as e:
            ctx.debug_remap_packed(src, mp, **kw)
        assert e.value.code == _capi.ERR_INVALID_ARG


def test_test_taps_are_declared_listed_and_exported(s360lib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "s360_debug_remap.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_REMAP_SYMBOLS) == ["s360_debug_pole_warp_packed", "s360_debug_remap_by_flow", "s360_debug_remap_packed"]
    for n in names:
        assert hasattr(s360lib, n), n
