"""GPU parity of ONE PixFlow pyramid level, stage by stage (flow.hip: FlowEngine::level — gradients, search init, the 15x15 blur into
the sweeps' records, row flags, sweep, median, sweep, median, diffusion, adjustment toward the previous flow), through the library's
test tap (include/s360_debug_flow_level.h) against the oracle's level with its intermediates. The cases are
tests/flow_level_cases.py's; every comparison is bit for bit and names the first stage that differs."""
import os
import subprocess
import sys

import pytest

import flow_level_cases as S
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMULATED = os.environ.get("S360_TEST_EMULATED_LIB") == "1"


@pytest.fixture(scope="module")
def ctx(gpu_rig):
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    yield c
    c.close()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("w,h,why", S.SHAPES, ids=S.SHAPE_IDS)
def test_level_shape(ctx, oracle, w, h, why, mode):
    """B = 3 flows over N = 4 images, (0,1), (1,0), (2,3): once from a noise flow, once from nothing with pixflow_search_20's search."""
    S.check_shape(ctx, oracle, mode, w, h)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("hint", S.SEARCH_HINTS)
@pytest.mark.parametrize("w,h", S.SEARCH_SIZES, ids=["%dx%d" % s for s in S.SEARCH_SIZES])
def test_level_search_hint(ctx, oracle, w, h, hint, mode):
    """k_search_init outside the coarsest level's sizes and with every hint's box (the shape cases run LEFT)."""
    S.check_search_hint(ctx, oracle, mode, w, h, hint)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("w,h", S.CONTENT_SIZES, ids=["%dx%d" % s for s in S.CONTENT_SIZES])
@pytest.mark.parametrize("name,init,alpha", S.CONTENT, ids=S.CONTENT_IDS)
def test_level_content(ctx, oracle, name, init, alpha, w, h, mode):
    """Initial flows and alpha layouts that the pyramid never hands to a level; each case first shows on the oracle's mask and
    counters that it reaches the edge it is named after."""
    S.check_content(ctx, oracle, mode, w, h, name, init, alpha)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("prev_scale", S.PREV_SCALES, ids=["x1", "x41_50"])
@pytest.mark.parametrize("w,h", S.TEMPORAL_SIZES, ids=["%dx%d" % s for s in S.TEMPORAL_SIZES])
def test_level_with_previous_state(ctx, oracle, w, h, prev_scale, mode):
    """The diffusion fused with adjustFlowTowardPrevious: motion 0, 1 and between, the previous flow rescaled as it is read."""
    S.check_temporal(ctx, oracle, mode, w, h, prev_scale)


@pytest.mark.skipif(EMULATED, reason="hardware only: the CPU emulation runs a launch's workgroups to completion one after another, so "
                                     "it cannot show an ordering fault between persistent waves on different CUs")
@pytest.mark.parametrize("w,h,B", S.DISPATCH, ids=["%dx%d_B%d" % d for d in S.DISPATCH])
def test_level_dispatch_as_production(ctx, oracle, w, h, B):
    """The sweep instantiation of the production batch — three lanes per pixel, 20-row bands, more band tickets than persistent
    waves — which needs B * ceil(h / 16) >= 4096: B flows over 8 images, four distinct pairs cycled, all against the oracle."""
    S.check_dispatch(ctx, oracle, w, h, B)


# ---- forced variants: the switches are read once per process, so each runs the shape list in a child of its own ----------------
VARIANTS = [("S360_QUAD_LPP", "3", S.SHAPES), ("S360_QUAD_WAVES_PER_CU", "1", S.SHAPES), ("S360_SWEEP_DIV", "ieee", S.SHAPES)] + \
           [("S360_MEDIAN_BX", str(bx), S.MEDIAN_SHAPES) for bx in (32, 16, 8, 4)]
CHILD = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch  # noqa: F401
from surround360_amd import _capi
if os.environ.get("S360_TEST_EMULATED_LIB") == "1":  # tests/conftest.py's developer switch, for this child too
    _capi.LIB_PATH = os.environ.get("S360_TEST_EMULATED_LIB_PATH") or os.path.join(%(root)r, "tools", "libs360_emu.so")
from surround360_amd import render as R
import flow_level_cases as S
import oracle_lib as O
forced = {sys.argv[1]: sys.argv[2]}
S.load_expected(sys.argv[4])  # the oracle's side of the shape cases, computed once by the parent
shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[3].split(",")]
ctx = R.Context(R.RigDescription(os.path.join(%(root)r, "tests", "golden", "rig_17cam.json")), R.make_params(eqr_width=1008, eqr_height=504))
for w, h in shapes:
    for mode in S.MODES:
        S.check_shape(ctx, O, mode, w, h, forced)
ctx.close()
print("VARIANT OK", len(shapes))
'''


@pytest.fixture(scope="module")
def shape_expectations(oracle, tmp_path_factory):
    """The oracle's results of the shape cases (already there if the shape tests ran before), in a file for the children."""
    for w, h, _ in S.SHAPES:
        gray, alpha = S.gray_planes(w, h), S.shape_alpha(w, h)
        for kind, alg, hint in S.SHAPE_INITS:
            S.expected(oracle, ("shape", w, h, kind), gray, alpha, S.I0, S.I1, None if kind is None else S.initial_flow(kind, w, h), alg, hint)
    path = str(tmp_path_factory.mktemp("flow_level") / "expected.pickle")
    S.save_expected(path)
    return path


_child_lost = []  # a child that ended on a signal or at its timeout: no further child is started


@pytest.mark.parametrize("var,value,shapes", VARIANTS, ids=["%s=%s" % v[:2] for v in VARIANTS])
def test_level_shapes_with_forced_variant(s360lib, shape_expectations, var, value, shapes):
    assert not _child_lost, "not started: the child of %s ended on a signal or at its timeout" % _child_lost[0]
    cmd = [sys.executable, "-c", CHILD % {"root": ROOT}, var, value, ",".join("%dx%d" % s[:2] for s in shapes), shape_expectations]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **{var: value}), timeout=300)
    except subprocess.TimeoutExpired:
        _child_lost.append("%s=%s (timeout)" % (var, value))
        raise AssertionError("%s=%s: the child ran into its timeout" % (var, value))
    if r.returncode < 0:
        _child_lost.append("%s=%s (signal %d)" % (var, value, -r.returncode))
    assert r.returncode == 0, "%s=%s: exit %d\n%s" % (var, value, r.returncode, (r.stdout + r.stderr)[-3000:])
    assert "VARIANT OK %d" % len(shapes) in r.stdout


def test_test_tap_is_declared_listed_and_exported(s360lib):
    import re
    from surround360_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s360_debug_flow_level.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(s360_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(_capi.DEBUG_FLOW_LEVEL_SYMBOLS) == ["s360_debug_flow_level"]
    for n in names:
        assert hasattr(s360lib, n), n


def test_tap_refuses_bad_arguments(ctx):
    import numpy as np
    from surround360_amd._capi import S360Error
    g = np.full((2, 4, 4), 0.5, np.float32)
    a = np.ones((2, 4, 4), np.float32)
    f = np.zeros((1, 4, 4, 2), np.float32)
    for kw in (dict(gray=g[:, :1], alpha=a[:, :1]),                       # h < 2
               dict(i0=[2]), dict(i1=[-1]),                                # index outside [0, N)
               dict(prev_flow=f), dict(motion=a),                          # previous state half given
               dict(prev_flow=f, motion=a, want=["diffused"]),             # no diffused flow with previous state
               dict(i0=[0] * 2049, i1=[1] * 2049, want=[])):               # B > kMaxFlows
        args = dict(gray=g, alpha=a, i0=[0], i1=[1])
        args.update(kw)
        with pytest.raises(S360Error) as e:
            ctx.debug_flow_level(**args)
        assert e.value.code == -1, kw
