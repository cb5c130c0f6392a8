"""GPU parity on content the noise generators never produce (tests/content.py): exact ties, alpha exactly at PixFlow's
update threshold (0.9f), operands below 2^-96 that send the sweeps through their IEEE re-run, huge previous flows,
divisions by zero in pixflow_search_20's search, signed zeros in the median, holes that end on the sweeps' band edges,
remaps and sharpening that saturate.

Every case asserts two things: that the oracle reaches the edge the case is named after — its coverage counters
(oracle/cvlite.h: CoverageCounter, counted while the oracle computes the same operands as the kernels), or where no
counter applies a property of the oracle's own intermediates — and that the device result is the oracle's bit for bit
(uint32 view for floats, bytes for images)."""
import numpy as np
import pytest

import content as K
import rigutil
from surround360_amd import render as R, synth

pytestmark = pytest.mark.gpu

SIZE = (203, 157)  # x0.5: 101 x 78; neither is a multiple of 8, 16 or 20
SMALL = (45, 37)   # x0.5: 22 x 18, at or below kPyrMinImageSize: one pyramid level
ALGS = ("pixflow_low", "pixflow_search_20")
HINTS = ("LEFT", "RIGHT", "UNKNOWN")
MODES = ("throughput", "latency")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    if got.dtype == np.float32:
        bad = bits(got) != bits(want)
        assert not bad.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (
            name, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
    else:
        d = got.astype(np.int32) - want.astype(np.int32)
        assert not d.any(), "%s: %d mismatching bytes, max |d| %d" % (name, int((d != 0).sum()), int(np.abs(d).max()))


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


# ---- flows --------------------------------------------------------------------------------------------------------------
def _finest_alpha(oracle, img):
    return oracle.pixflow_entry(img)[2]


def _motion_sums(oracle, i1, prev_i1):
    """k_motion's integer operand: the channel-difference sum of the x0.5 cubic downscales (PixFlow.h:112-115)."""
    h, w = i1.shape[:2]
    d1 = oracle.resize_cubic_u8(i1, int(w * 0.5), int(h * 0.5)).astype(np.int32)
    p1 = oracle.resize_cubic_u8(prev_i1, int(w * 0.5), int(h * 0.5)).astype(np.int32)
    return np.abs(d1[..., :3] - p1[..., :3]).sum(-1)


def _noise(w, h):
    return synth.flow_pair(w, h, seed=3)


def _prev(i0, i1, flow, prev_i1=None):
    return dict(prev_flow=flow, prev_i0=i0, prev_i1=i1 if prev_i1 is None else prev_i1)


def _hole_rows(r):
    def make(w, h):
        pair = K.with_alpha(_noise(w, h), K.alpha_hole_rows(w, h, r))
        return pair, None
    return make


def _hole_cols(dc):
    def make(w, h):
        return K.with_alpha(_noise(w, h), K.alpha_hole_cols(w, h, int(w * 0.5) - 1 - dc)), None
    return make


def _tiny_prev(w, h):
    i0, i1 = K.constant_pair(w, h)
    return (i0, i1), _prev(i0, i1, K.tiny_flow(w, h))


def _tiny_prev_hole(w, h):
    """Tiny previous flows under a transparent band, which the sweeps leave to the inter-level upscale alone.

    No flow input found reaches a median window that holds both +0 and -0 (the median_signed_zeros counter stays 0
    here and in every case of this file; it is printed, not asserted): the sweeps make -0 only from a -0 they are
    given, adjustFlowTowardPrevious gives -0 only where the flow is negative and the previous flow is -0, and the
    cubic upscale turns a window of -0 into +0 wherever one of its weights is negative."""
    i0, i1 = K.with_alpha(K.constant_pair(w, h), K.alpha_hole_rows(w, h, 31))
    return (i0, i1), _prev(i0, i1, K.tiny_flow(w, h))


def _huge_prev(w, h):
    """Previous flows of 60 ... 200 px: the proposals leave k_sweep_quad's LDS window (32 columns) for global memory.
    Measured on the emulated library (g_quad_fallbacks, sweep_quad.hip), pixflow_low LEFT at 203 x 157: 659 904 of
    774 400 update wave-steps take the fallback, against 0 with a zero previous flow."""
    i0, i1 = _noise(w, h)
    return (i0, i1), _prev(i0, i1, K.huge_flow(w, h))


def _half_static(w, h):
    i0, i1 = _noise(w, h)
    flow = np.dstack([np.full((h, w), 2.5, np.float32), np.full((h, w), -0.75, np.float32)])
    return (i0, i1), _prev(i0, i1, flow, K.half_static_prev(i1))


def _motion_sums_case(w, h):
    i1, p1 = K.motion_sums_pair()
    i0 = np.ascontiguousarray(np.roll(i1, 3, axis=1))
    hh, ww = i1.shape[:2]
    flow = np.dstack([np.full((hh, ww), -3.0, np.float32), np.full((hh, ww), 0.25, np.float32)])
    return (i0, i1), _prev(i0, i1, flow, p1)


# name: (builder(w, h) -> ((I0, I1), prev state or None), counters that must be > 0, size)
FLOW_CASES = {
    "constant": (lambda w, h: (K.constant_pair(w, h), None), ("tie_rejected", "search_tie"), SIZE),
    "black": (lambda w, h: (K.level_pair(w, h, 0), None), ("tie_rejected", "search_nonfinite"), SIZE),
    "white": (lambda w, h: (K.level_pair(w, h, 255), None), ("tie_rejected", "search_tie"), SIZE),
    "step_0_255": (lambda w, h: (K.step_pair(w, h, 0, 255), None), ("tiny_operand", "tie_rejected", "search_tie"), SIZE),
    "step_60_61": (lambda w, h: (K.step_pair(w, h, 60, 61), None), ("tiny_operand", "tie_rejected"), SIZE),
    "checker": (lambda w, h: (K.checker_pair(w, h), None), ("tiny_operand", "tie_rejected"), SIZE),
    "ramp_h": (lambda w, h: (K.ramp_pair(w, h, 1), None), ("tiny_operand", "tie_rejected"), SIZE),
    "ramp_v": (lambda w, h: (K.ramp_pair(w, h, 0), None), ("tiny_operand", "tie_rejected"), SIZE),
    "cartoon": (lambda w, h: (K.cartoon_pair(w, h), None), ("tiny_operand", "tie_rejected", "search_tie"), SIZE),
    "alpha_stripes_1": (lambda w, h: (K.with_alpha(_noise(w, h), K.alpha_stripes(w, h, 1)), None), ("alpha_at_threshold",), SIZE),
    "alpha_stripes_2": (lambda w, h: (K.with_alpha(_noise(w, h), K.alpha_stripes(w, h, 2)), None), ("alpha_at_threshold",), SIZE),
    "i0_transparent": (lambda w, h: (K.with_alpha(_noise(w, h), 0, 255), None), ("search_nonfinite",), SIZE),
    "i1_transparent": (lambda w, h: (K.with_alpha(_noise(w, h), 255, 0), None), ("search_nonfinite",), SIZE),
    "tiny_prev_flow": (_tiny_prev, ("tiny_operand", "tie_rejected"), SIZE),
    "tiny_prev_flow_hole": (_tiny_prev_hole, ("tiny_operand",), SIZE),
    "huge_prev_flow": (_huge_prev, ("tie_rejected",), SIZE),
    "half_static_prev": (_half_static, (), SIZE),
    "motion_sums_0_765": (_motion_sums_case, (), None),
    "small_step_0_255": (lambda w, h: (K.step_pair(w, h, 0, 255), None), ("tiny_operand", "tie_rejected", "search_tie"), SMALL),
    "small_cartoon": (lambda w, h: (K.cartoon_pair(w, h), None), ("tiny_operand", "tie_rejected", "search_tie"), SMALL),
    "small_black": (lambda w, h: (K.level_pair(w, h, 0), None), ("search_nonfinite",), SMALL),
    "small_hole_row_8": (_hole_rows(8), ("search_nonfinite",), SMALL),
}
for _r in (7, 8, 15, 16, 19, 20, 31, 32):
    FLOW_CASES["hole_row_%d" % _r] = (_hole_rows(_r), (), SIZE)
for _dc in (0, 1):
    FLOW_CASES["hole_col_w-%d" % (_dc + 1)] = (_hole_cols(_dc), (), SIZE)


def _edge_property(name, oracle, i0, i1, prev):
    """The cases without a counter of their own prove their edge on the oracle's intermediates."""
    if name.startswith("hole_row_") or name.startswith("small_hole_row_"):
        r = int(name.rsplit("_", 1)[1])
        a = _finest_alpha(oracle, i0)
        cols = a.shape[1] // 2
        low = np.nonzero(a[:, cols] <= np.float32(0.9))[0]
        assert low.size and low.max() == r, "hole's last row at the finest level: %s, not %d" % (low.max(), r)
    if name.startswith("hole_col_"):
        a = _finest_alpha(oracle, i0)
        low = np.nonzero(a[a.shape[0] // 2] <= np.float32(0.9))[0]
        want = a.shape[1] - 1 if name.endswith("w-1") else a.shape[1] - 2
        assert low.size and low.max() == want, "hole's last column at the finest level: %s, not %d" % (low.max(), want)
    if name == "half_static_prev":
        s = _motion_sums(oracle, i1, prev["prev_i1"])
        half = s.shape[1] // 2
        assert not s[:, : half - 2].any() and (s[:, half + 2:] > 0).mean() > 0.9
    if name == "motion_sums_0_765":
        assert set(np.unique(_motion_sums(oracle, i1, prev["prev_i1"]))) == set(range(766))


@pytest.mark.parametrize("name", sorted(FLOW_CASES))
def test_flow_content(ctxs, oracle, name):
    """Both algorithms, hints LEFT / RIGHT / UNKNOWN, both sweep kernels; every pyramid level where there is no
    previous state (s360_debug_flow_levels runs without it)."""
    make, need, size = FLOW_CASES[name]
    (i0, i1), prev = make(*(size or (0, 0)))
    _edge_property(name, oracle, i0, i1, prev)
    want, counts = {}, dict.fromkeys(oracle.COVERAGE_NAMES, 0)
    for alg in ALGS:
        for hint in HINTS:
            with oracle.coverage() as cov:
                want[alg, hint] = oracle.compute_optical_flow(i0, i1, alg, hint, want_levels=prev is None, **(prev or {}))
            for k, v in cov.counts.items():
                counts[k] += v
    print("coverage %s: %s" % (name, counts))
    for k in need:
        assert counts[k] > 0, "%s does not reach %s: %s" % (name, k, counts)
    for mode, ctx in ctxs.items():
        for (alg, hint), w in want.items():
            tag = "%s %s %s %s" % (name, mode, alg, hint)
            if prev is None:
                final, levels = w
                _same(tag, ctx.compute_optical_flow(i0, i1, alg, hint), final)
                buf, n = ctx.debug_flow_levels(i0, i1, alg, hint)
                assert n == len(levels), tag
                off = 0
                for li, wl in enumerate(levels):
                    _same("%s level %d (coarsest first)" % (tag, li), buf[off:off + wl.size].reshape(wl.shape), wl)
                    off += wl.size
            else:
                _same(tag, ctx.compute_optical_flow(i0, i1, alg, hint, **prev), w)


def test_tiny_prev_flow_ieee_division(gpu_rig, oracle, monkeypatch):
    """The tiny-operand case with S360_SWEEP_DIV=ieee (no fast division / square root at all): same bits."""
    monkeypatch.setenv("S360_SWEEP_DIV", "ieee")
    (i0, i1), prev = _tiny_prev(*SIZE)
    c = R.Context(gpu_rig, R.make_params(eqr_width=1008, eqr_height=504))
    try:
        for mode in MODES:
            c.set_sweep_mode(mode)
            for hint in ("LEFT", "RIGHT"):
                with oracle.coverage() as cov:
                    want = oracle.compute_optical_flow(i0, i1, "pixflow_low", hint, **prev)
                assert cov.counts["tiny_operand"] > 0, cov.counts
                _same("ieee %s %s" % (mode, hint), c.compute_optical_flow(i0, i1, "pixflow_low", hint, **prev), want)
    finally:
        c.close()


# ---- whole frames -------------------------------------------------------------------------------------------------------
EQR_W, EQR_H, CAM, WORLD_H = 1008, 504, 512, 1024
WORLDS = {
    "constant": lambda: K.world_constant(WORLD_H),
    "cartoon": lambda: K.world_cartoon(WORLD_H),
    "checker": lambda: K.world_checker(WORLD_H),
    "black_white_spots": lambda: K.world_black_white_spots(WORLD_H),
}
STAGES_U8 = [("projection", i) for i in (0, 5, 13)] + [(n, i) for n in ("overlap_l", "overlap_r") for i in (0, 7, 13)] + [
    ("top_spherical", 0), ("bottom_spherical", 0)] + [(n, u) for n in ("extended_side", "extended_fisheye", "pole_warped")
                                                      for u in range(4)] + [("side_pano_l", 0), ("side_pano_r", 0)]
STAGES_F32 = [(n, i) for n in ("flow_l_to_r", "flow_r_to_l") for i in range(14)] + [("flow_pole", u) for u in range(4)]


@pytest.fixture(scope="module")
def rig_small(tmp_path_factory, rig_json):
    d = tmp_path_factory.mktemp("rig_content")
    return rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)


def _compare_frame(ctx, of, got, want, tag):
    for n, i in STAGES_U8:
        _same("%s %s %d" % (tag, n, i), ctx.get_u8(n, i), of.get_u8(n, i))
    for n, i in STAGES_F32:
        _same("%s %s %d" % (tag, n, i), ctx.get_f32(n, i), of.get_f32(n, i))
    _same("%s equirect" % tag, got, want)


@pytest.mark.parametrize("world_name", sorted(WORLDS))
def test_frame_content(rig_small, oracle, s360lib, world_name):
    """One frame per world texture (sharpening 0.25, final resize), every stage compared; then a chained second frame
    of the same world (motion 0 everywhere) and one where half the world's texture changes."""
    flags = dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=960,
                 final_eqr_height=960, sharpening=0.25)
    world = WORLDS[world_name]()
    frames = [world, world, K.world_half_changed(world)]
    ctx = R.Context(R.RigDescription(rig_small), R.make_params(**flags))
    ctx.keep_intermediates(True)
    cams, _ = oracle.load_rig(rig_small)
    of = oracle.Frame(cams, oracle.make_params(**flags))
    counts = dict.fromkeys(oracle.COVERAGE_NAMES, 0)
    try:
        for k, wd in enumerate(frames):
            side, top, bottom = synth.rig_frame(rig_small, size=CAM, world=wd, nearest=True)
            with oracle.coverage() as cov:
                want, _ = of.render(side, top, bottom, use_prev=k > 0)
            for n, v in cov.counts.items():
                counts[n] += v
            ctx.upload_frame(side, top, bottom)
            ctx.render(use_prev=k > 0)
            _compare_frame(ctx, of, ctx.download_equirect(), want, "%s frame %d" % (world_name, k))
    finally:
        ctx.close()
    print("coverage frame %s: %s" % (world_name, counts))
    assert counts["tie_rejected"] > 0, counts


# ---- operators ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(rig_small, oracle, s360lib):
    flags = dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=0, final_eqr_height=0)
    rig = R.RigDescription(rig_small)
    ctx = R.Context(rig, R.make_params(**flags))
    cams, ids = oracle.load_rig(rig_small)
    of = oracle.Frame(cams, oracle.make_params(**flags))
    side, top, bottom = synth.rig_frame(rig_small, size=CAM, world=K.world_cartoon(WORLD_H), nearest=True)
    of.render(side, top, bottom)

    def side_cam(idx):
        c = rig.rig_side_only[idx]
        return c, cams[ids.index(c.id.decode())]

    yield dict(ctx=ctx, of=of, side_cam=side_cam)
    ctx.close()


@pytest.mark.parametrize("src_kind,sc,dc", [("step", 3, 4), ("checker", 3, 3), ("checker", 4, 4)])
def test_bicubic_remap_saturates(env, oracle, src_kind, sc, dc):
    """bicubicRemapToSpherical of 0 / 255 sources: the bicubic overshoots below 0 and above 255 and sat_u8 clamps — in
    k_remap_cubic_u8c4_tiled, the kernel of this entry point; the same for the packed kernels of the frame's projections is
    tests/test_gpu_remap_packed.py::test_checker_reaches_both_ends_of_the_saturation."""
    cam, ocam = env["side_cam"](0)
    src = K.grey(K.checker(CAM, CAM, 8)) if src_kind == "checker" else K.step_pair(CAM, CAM, 0, 255)[0][..., :3]
    if sc == 4:
        src = K.bgra(src, K.checker(CAM, CAM, 5, 0, 255))
    fov = 77.8 * np.pi / 180.0
    l, r, t, b = 0.3, -0.5, fov / 2, -fov / 2
    dw, dh = 219, 213
    unclamped = oracle.remap_cubic_f32(src.astype(np.float32), oracle.spherical_warp_map(ocam, dw, dh, l, r, t, b))
    assert unclamped.min() < -1.0 and unclamped.max() > 256.0, (unclamped.min(), unclamped.max())
    got = env["ctx"].bicubic_remap_to_spherical(src, cam, dw, dh, dc, l, r, t, b)
    want = oracle.bicubic_remap_to_spherical(ocam, src, dw, dh, dc, l, r, t, b)
    _same("bicubicRemapToSpherical %s" % src_kind, got, want)


@pytest.mark.parametrize("h,w", [(96, 200), (131, 203)])
def test_sharpen_saturates(env, oracle, h, w):
    """sharpen of 0 / 255 content: every pixel saturates (the oracle's output is its input), while the same pattern
    at 1 / 254 moves."""
    img = K.grey(K.checker(w, h, 8))
    img[:, :, 1] = K.checker(w, h, 3)
    soft = (1 + img.astype(np.int32) * 253 // 255).astype(np.uint8)
    want = oracle.sharpen(img, 0.25)
    assert np.array_equal(want, img) and not np.array_equal(oracle.sharpen(soft, 0.25), soft)
    _same("sharpen 0/255", env["ctx"].sharpen(img, 0.25), want)
    _same("sharpen 1/254", env["ctx"].sharpen(soft, 0.25), oracle.sharpen(soft, 0.25))


@pytest.mark.parametrize("w,h", [(256, 64), (333, 47)])
def test_flatten_layers_alpha_edges(env, oracle, w, h):
    """flattenLayersDeghostPreferBase with alpha 0, 1, 254, 255 on both layers and exact base / top duplicates."""
    rng = np.random.default_rng(w + h)
    base = K.bgra(K.cartoon_pair(w, h, seed=w)[0][..., :3])
    top = base.copy()
    other = K.bgra(K.cartoon_pair(w, h, seed=h)[0][..., :3])
    dup = rng.random((h, w)) < 0.5
    top[~dup] = other[~dup]
    levels = np.array([0, 1, 254, 255], np.uint8)
    base[..., 3] = levels[rng.integers(0, 4, (h, w))]
    top[..., 3] = np.where(dup & (rng.random((h, w)) < 0.5), base[..., 3], levels[rng.integers(0, 4, (h, w))])
    want = oracle.flatten_layers(base, top)
    _same("flatten", env["ctx"].flatten_layers_deghost_prefer_base(base, top), want)


@pytest.mark.parametrize("flows", ["zero", "outside"])
def test_combine_lazy_novel_views_edge_flows(env, flows):
    """combineLazyNovelViews with all-zero flows, and with flows that point far outside the image."""
    of = env["of"]
    il, ir = of.get_u8("overlap_l", 2), of.get_u8("overlap_r", 2)
    h, w = il.shape[:2]
    if flows == "zero":
        fl = np.zeros((h, w, 2), np.float32)
        fr = np.zeros((h, w, 2), np.float32)
    else:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        fl = np.dstack([np.where(xx < w / 2, -3.0 * w, 3.0 * w), np.where(yy < h / 2, -2.0 * h, 1.5 * h)]).astype(np.float32)
        fr = -fl[:, ::-1].copy()
    gl, gr = env["ctx"].combine_lazy_novel_views(il, ir, fl, fr)
    wl, wr = of.combine_lazy_novel_views(il, ir, fl, fr)
    _same("chunk L %s" % flows, gl, wl)
    _same("chunk R %s" % flows, gr, wr)


@pytest.mark.parametrize("w,h,e", [(256, 128, 31), (301, 77, 31), (200, 90, 5)])
def test_feather_alpha_channel_border_holes(env, oracle, w, h, e):
    """featherAlphaChannel with transparent holes that touch each border and the corners."""
    img = K.bgra(K.cartoon_pair(w, h, seed=e)[0][..., :3])
    a = np.full((h, w), 255, np.uint8)
    a[0, w // 3: w // 2] = 0
    a[h - 3:, : w // 4] = 0
    a[h // 3: h // 2, 0] = 0
    a[: h // 5, w - 2:] = 0
    a[h - 1, w - 1] = 0
    a[h // 2, w // 2] = 0
    img[..., 3] = a
    _same("featherAlphaChannel e=%d" % e, env["ctx"].feather_alpha_channel(img, e), oracle.feather_alpha_channel(img, e))
