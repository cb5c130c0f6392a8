"""Cases and checks of tests/test_gpu_flow_pyramid.py: what FlowEngine::compute does in front of its level loop (flow.hip:
FlowEngine::prepare — pre-blur, image pyramids, previous images, motion, previous flow, their pyramids, the level factors) against the
oracle's PixFlow::prepare, and the pyramids' two resizes (launch_resize_linear_f32, launch_resize_cubic_f32c2) on caller-made planes
against the oracle's resizes, through the test taps of include/s360_debug_flow_pyramid.h.

Every comparison is on uint32 views, stage by stage in launch order, and names the first stage that differs. Device buffers hold
FILL in every byte before a launch: as a float word that is a NaN no resize of finite data gives, so an unwritten word shows.
numpy only; the restatements of the kernels' boxes and windows (linear_box, cubic_window) follow resize_coord's definition, the
coordinate rounded to float and then floored, with the kernels' clamps — tests/test_cpu_flow_pyramid.py sweeps them against the
launcher's dispatch rules."""
import numpy as np

import content as K

FILL = 0xFF
FILL_WORD = 0xFFFFFFFF
TW, TH = 64, 16            # the output tile of both tiled kernels
RL_BW, RL_BH = 76, 20      # k_resize_linear_f32c1_tiled's box of floats in LDS
UC_SW, UC_SH = 72, 24      # k_resize_cubic_f32c2_tiled's window


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(stage, got, want):
    """Bit equality of two float arrays; the message names the stage, the count and the first differing element."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (stage, got.shape, want.shape)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    unwritten = int(np.count_nonzero(g == FILL_WORD)) if got.dtype == np.float32 else 0
    raise AssertionError("%s: %d of %d words differ, first at %s: got %r (0x%08x), expected %r (0x%08x); %d words never written"
                         % (stage, len(bad), g.size, i, got[i], int(g[i]), want[i], int(w[i]), unwritten))


# ---- resize_coord and the kernels' boxes, restated ---------------------------------------------------------------------------------
def resize_coords(dn, sn):
    """resize_coord for every destination index of an axis: float((d + 0.5) * scale - 0.5) in double, then floored."""
    scale = 1.0 / (float(dn) / float(sn))
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def _tile_ends(dn, size):
    """First and last destination index of every tile of an axis (positions beyond the image repeat the last one)."""
    first = np.arange(0, dn, size)
    return first, np.minimum(first + size - 1, dn - 1)


def linear_box(sn, dn, axis):
    """Per tile of the axis ('x': 64 columns, 'y': 16 rows) what k_resize_linear_f32c1_tiled stages: [(first source index, floats or
    rows staged, last source index tapped)]. On x the box is read in 16-byte pieces from its first column, so the width staged is a
    multiple of 4. (The coordinates do not decrease along the axis: a tile's first and last position bound its box.)"""
    s, _ = resize_coords(dn, sn)
    assert np.all(np.diff(s) >= 0)
    first, last = _tile_ends(dn, TW if axis == "x" else TH)
    if axis == "x":
        sx = np.where(s < 0, 0, s)
        sx = np.where(sx >= sn - 1, sn - 1, sx)
        bx0, end = sx[first], np.minimum(sx[last] + 1, sn - 1)
        return [(int(a), int(4 * ((e - a + 4) >> 2)), int(e)) for a, e in zip(bx0, end)]
    r0, r1 = np.clip(s, 0, sn - 1), np.clip(s + 1, 0, sn - 1)
    return [(int(a), int(e - a + 1), int(e)) for a, e in zip(r0[first], r1[last])]


def linear_piece_crosses_row_end(sw, dw):
    """True if some tile's last 16-byte piece reaches beyond the source row (the kernel's scalar path)."""
    return any(bx0 + width > sw for bx0, width, _ in linear_box(sw, dw, "x"))


def cubic_window(sn, dn, axis):
    """Per tile of the axis what k_resize_cubic_f32c2_tiled stages: [(first source index, extent)]."""
    s, _ = resize_coords(dn, sn)
    assert np.all(np.diff(s) >= 0)
    first, last = _tile_ends(dn, TW if axis == "x" else TH)
    lo, hi = np.clip(s[first] - 1, 0, sn - 1), np.clip(s[last] + 2, 0, sn - 1)
    return [(int(a), int(e - a + 1)) for a, e in zip(lo, hi)]


def planes_per_thread(planes):
    return 4 if planes % 4 == 0 else 2 if planes % 2 == 0 else 1


def workgroups(dw, dh, planes, ppt=None):
    """Workgroups of a tiled launch: tiles x planes / planes per thread (the linear launcher's pick unless given; the cubic has 1)."""
    return -(-dw // TW) * -(-dh // TH) * (planes // (ppt or planes_per_thread(planes)))


# ---- content ---------------------------------------------------------------------------------------------------------------------
def noise_planes(b, h, w, seed, cn=1):
    rng = np.random.default_rng(seed)
    shape = (b, h, w) if cn == 1 else (b, h, w, cn)
    return (rng.standard_normal(shape) * 3.0 + 0.25 * np.arange(b).reshape((b,) + (1,) * (len(shape) - 1))).astype(np.float32)


def tile_border_columns(n, size):
    """Indices beside every tile border of an axis of n, and its two ends."""
    idx = {0, n - 1}
    for e in range(size, n, size):
        idx.update((e - 1, e))
    return sorted(i for i in idx if 0 <= i < n)


def special_planes(kind, b, h, w, seed, cn=1):
    """Content the noise never gives. constant: one value per plane; negzero: all -0.0; subnormal: noise of magnitudes below 2^-126
    in both signs with zeros of both signs; ones: zeros with a single 1.0 in each corner and on some of the positions at and beside
    every multiple of the tile size (at ratios near 1 they are tapped from both sides of a tile border); mixed: noise with blocks of
    -0.0, subnormals and 1e-16."""
    rng = np.random.default_rng(seed)
    shape = (b, h, w) if cn == 1 else (b, h, w, cn)
    if kind == "noise":
        return noise_planes(b, h, w, seed, cn)
    if kind == "constant":
        a = np.empty(shape, np.float32)
        for k in range(b):
            a[k] = np.float32([0.9, -40.0, 1e-16, 255.0][k % 4])
        return a
    if kind == "negzero":
        return np.full(shape, -0.0, np.float32)
    if kind == "subnormal":
        mant = rng.integers(0, 1 << 23, shape).astype(np.uint32)       # exponent field 0: subnormals and zeros
        mant[rng.random(shape) < 0.1] = 0
        sign = (rng.integers(0, 2, shape).astype(np.uint32) << 31)
        return (mant | sign).view(np.float32)
    if kind == "ones":
        a = np.zeros(shape, np.float32)
        ys = sorted(set(tile_border_columns(h, TH)) | {min(h - 1, y + 1) for y in tile_border_columns(h, TH)})
        xs = sorted(set(tile_border_columns(w, TW)) | {min(w - 1, x + 1) for x in tile_border_columns(w, TW)})
        for k in range(b):
            for iy, y in enumerate(ys):
                for ix, x in enumerate(xs):
                    corner = y in (0, h - 1) and x in (0, w - 1)
                    if corner or (ix + iy + k) % 3 == 0:
                        a[(k, y, x) if cn == 1 else (k, y, x, (ix + k) % cn)] = 1.0
        return a
    if kind == "mixed":
        a = noise_planes(b, h, w, seed, cn)
        a[:, : max(1, h // 3), : max(1, w // 3)] = -0.0
        a[:, h // 2:, : max(1, w // 4)] = special_planes("subnormal", b, h - h // 2, max(1, w // 4), seed + 1, cn)
        a[:, : max(1, h // 4), w // 2:] = np.float32(1e-16)
        return a
    raise KeyError(kind)


def image(w, h, seed, alpha="mixed"):
    """A BGRA image: blocky colour noise with fine noise on top; alpha per `alpha`: an array, a level, or 'mixed' — regions of 255, of
    0, of the two levels around 0.9 and of noise, laid out differently for every seed."""
    rng = np.random.default_rng(1000 + seed)
    blocks = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4, 3))
    bgr = np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:h, :w] + rng.integers(-12, 13, (h, w, 3))
    bgr = np.clip(bgr, 0, 255).astype(np.uint8)
    if isinstance(alpha, str):
        yy, xx = np.mgrid[0:h, 0:w]
        region = ((yy * 3) // max(h, 1) + (xx * 2) // max(w, 1) + seed) % 4
        a = np.select([region == 0, region == 1, region == 2], [255, 0, 229 + ((xx // 2 + yy // 2) % 2)],
                      rng.integers(0, 256, (h, w))).astype(np.uint8)
    else:
        a = alpha
    return K.bgra(bgr, a)


def images(n, w, h, seed=0, alpha="mixed"):
    return np.stack([image(w, h, seed * 16 + k, alpha) for k in range(n)])


def prev_flows(b, w, h, seed, kind="noise"):
    rng = np.random.default_rng(2000 + seed)
    if kind == "noise":
        return (rng.standard_normal((b, h, w, 2)) * 4.0).astype(np.float32)
    # special: 8 x 8 blocks (the x0.5 cubic downscale keeps the inner pixels of a block at its value) of 0, -0, +-40 px, 1e-16, subnormals
    vals = np.array([0.0, -0.0, 40.0, -40.0, 1e-16, 1e-40, -1e-40, 2.5, -0.75, 1.4e-45], np.float32)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    pick = rng.integers(0, len(vals), (b, bh, bw, 2))
    pick.reshape(-1)[:len(vals)] = np.arange(len(vals))
    return np.ascontiguousarray(np.repeat(np.repeat(vals[pick], 8, axis=1), 8, axis=2)[:, :h, :w])


def flow_pairs(n, b):
    """B flows over N images: flow k matches image k % N against (k + 1) % N, so with N, B >= 2 some image is I0 of one flow and
    I1 of another."""
    return [k % n for k in range(b)], [(k + 1) % n for k in range(b)]


# ---- A: the engine's preparation -----------------------------------------------------------------------------------------------------
_expected = {}


def expected_prepare(oracle, key, imgs, i0, i1, pimgs=None, pflows=None):
    """The oracle's side of a case, once per key: per image its grey, alpha (and motion) pyramids, per flow its previous flow's
    pyramid and the factors. The pair calls also show that a flow's I0 / I1 are the planes of images i0[b] / i1[b]."""
    if key in _expected:
        return _expected[key]
    n, use_prev = len(imgs), pflows is not None
    per_image = [oracle.pixflow_prepare(imgs[k], imgs[k], pflows[0] if use_prev else None, pimgs[k] if use_prev else None) for k in range(n)]
    e = {"sizes": per_image[0]["sizes"], "gray": [], "alpha": []}
    L = len(e["sizes"])
    for l in range(L):
        e["gray"].append(np.stack([p["I1"][l] for p in per_image]))
        e["alpha"].append(np.stack([p["A1"][l] for p in per_image]))
    if use_prev:
        per_flow = [oracle.pixflow_prepare(imgs[a], imgs[c], pflows[k], pimgs[c]) for k, (a, c) in enumerate(zip(i0, i1))]
        for k, (a, c) in enumerate(zip(i0, i1)):  # one computation hands out all of it: the pair's planes are the images' planes
            for l in range(L):
                assert np.array_equal(bits(per_flow[k]["I0"][l]), bits(e["gray"][l][a])) and np.array_equal(bits(per_flow[k]["I1"][l]), bits(e["gray"][l][c]))
                assert np.array_equal(bits(per_flow[k]["motion"][l]), bits(per_image[c]["motion"][l]))
        e["motion"] = [np.stack([p["motion"][l] for p in per_image]) for l in range(L)]
        e["prev"] = [np.stack([p["prev"][l] for p in per_flow]) for l in range(L)]
        e["factors"] = per_flow[0]["factors"]
        for p in per_flow:
            assert np.array_equal(bits(p["factors"]), bits(e["factors"]))
    _expected[key] = e
    return e


def compare_prepare(got, want):
    """In launch order: entry (alpha of level 0), pre-blur (grey of level 0), the image pyramid level by level, the motion map, the
    previous flow's downscale, their pyramids level by level, the factors."""
    assert got["sizes"] == want["sizes"], "level sizes %s, expected %s" % (got["sizes"], want["sizes"])
    L = len(want["sizes"])
    same("alpha level 0 (entry downscale)", got["alpha"][0], want["alpha"][0])
    same("grey level 0 (pre-blur)", got["gray"][0], want["gray"][0])
    for l in range(1, L):
        same("grey level %d (image pyramid, %dx%d -> %dx%d)" % ((l,) + want["sizes"][l - 1] + want["sizes"][l]), got["gray"][l], want["gray"][l])
        same("alpha level %d (image pyramid)" % l, got["alpha"][l], want["alpha"][l])
    assert ("prev" in got) == ("prev" in want)
    if "prev" in want:
        same("motion level 0 (previous images' downscale, k_motion)", got["motion"][0], want["motion"][0])
        same("previous flow level 0 (cubic downscale through the table, x dh/h)", got["prev"][0], want["prev"][0])
        for l in range(1, L):
            same("previous flow level %d (two-channel pyramid)" % l, got["prev"][l], want["prev"][l])
            same("motion level %d (motion pyramid)" % l, got["motion"][l], want["motion"][l])
        same("level factors", got["factors"], want["factors"])


def check_prepare(ctx, oracle, key, imgs, i0, i1, pimgs=None, pflows=None, fill=FILL):
    want = expected_prepare(oracle, key, imgs, i0, i1, pimgs, pflows)
    got = ctx.debug_flow_prepare(imgs, i0, i1, pimgs, pflows, fill=fill)
    compare_prepare(got, want)
    return got, want


# level-0 sizes (after the x0.5 entry) at the pre-blur's edges, as (dw, dh, odd input width, odd input height)
LEVEL0 = [(2, 2, 0, 0), (3, 2, 1, 0), (2, 3, 0, 1), (4, 5, 0, 1), (5, 4, 1, 0), (3, 17, 1, 1), (63, 15, 0, 0), (64, 16, 0, 0), (65, 17, 1, 1),
          (64, 2, 0, 0), (2, 64, 0, 0), (27, 27, 0, 1), (28, 28, 0, 0), (28, 27, 1, 0), (27, 40, 0, 0)]
LEVEL0_IDS = ["%dx%d" % c[:2] for c in LEVEL0]


def check_level0(ctx, oracle, dw, dh, oddw, oddh):
    w, h = 2 * dw + oddw, 2 * dh + oddh
    assert oracle.pixflow_levels(w, h)[0] == (dw, dh)
    imgs, pimgs, pf = images(2, w, h, seed=dw * 7 + dh), images(2, w, h, seed=dw * 7 + dh + 500), prev_flows(1, w, h, dw + dh)
    nlev = len(oracle.pixflow_levels(w, h))
    assert nlev == (1 if min(dw, dh) <= 27 else 2 if min(dw, dh) == 28 else nlev)
    check_prepare(ctx, oracle, ("level0", w, h), imgs, [0], [1], pimgs, pf)
    check_prepare(ctx, oracle, ("level0-first-frame", w, h), imgs, [0], [1])


# Input sizes whose x0.9 chains put a level (not the first: a destination of the pyramid's resize) on the linear resize's tile edges,
# 63 / 64 / 65 wide and 32 / 33 / 48 / 49 high, and sizes whose coarsest level is 25, the smallest a pyramid holds. No input gives
# both at once: int(x * 0.9f + 0.5f) reaches 25 only through 28, 31, 34, 38, 42, 47, 52, 58, 64, 71 ..., which holds none of those
# heights, and the chains from 63 and 65 end at 27 and 26. (w, h, level reached, coarsest level)
TILE_EDGE = [(140, 70, (63, 32), (51, 26)), (142, 74, (64, 33), (52, 27)), (144, 106, (65, 48), (35, 26)), (142, 108, (64, 49), (34, 26)),
             (140, 108, (63, 49), (33, 26)), (144, 70, (65, 32), (53, 26)), (142, 142, (64, 64), (25, 25)), (142, 56, (64, 25), (64, 25)),
             (56, 144, (25, 65), (25, 65))]


def check_tile_edge(ctx, oracle, w, h, reach, coarsest):
    sizes = oracle.pixflow_levels(w, h)
    assert reach in sizes[1:] and sizes[-1] == coarsest, sizes
    imgs, pimgs, pf = images(3, w, h, seed=w + h), images(3, w, h, seed=w + h + 300), prev_flows(2, w, h, w)
    got, _ = check_prepare(ctx, oracle, ("tile-edge", w, h), imgs, [0, 2], [1, 0], pimgs, pf)
    assert got["sizes"] == sizes


BATCH = [(n, b) for n in (1, 2, 3, 4) for b in (1, 2, 3, 4)]


def check_batch(ctx, oracle, n, b):
    """66 x 58 -> 33 x 29 -> 30 x 26: one pyramid step with 2N one-channel, B two-channel and N one-channel planes."""
    w, h = 66, 58
    assert oracle.pixflow_levels(w, h) == [(33, 29), (30, 26)]
    i0, i1 = flow_pairs(n, b)
    if n >= 2 and b >= 2:
        assert set(i0) & set(i1)
    imgs, pimgs, pf = images(n, w, h, seed=n), images(n, w, h, seed=n + 40), prev_flows(b, w, h, 10 * n + b)
    for k in range(1, n):  # different alpha and content everywhere: a plane in its neighbour's slot cannot pass
        assert not np.array_equal(imgs[k], imgs[k - 1]) and not np.array_equal(imgs[k, ..., 3], imgs[k - 1, ..., 3])
    check_prepare(ctx, oracle, ("batch", n, b), imgs, i0, i1, pimgs, pf)


def all_classes_covered():
    """The three launches of a pyramid step over BATCH: which planes-per-thread classes each runs with."""
    return ({planes_per_thread(2 * n) for n, _ in BATCH}, {planes_per_thread(b) for _, b in BATCH}, {planes_per_thread(n) for n, _ in BATCH})


def is_subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < np.float32(2.0) ** -126)


# ---- B: the linear resize ---------------------------------------------------------------------------------------------------------------
def want_linear(oracle, src, dw, dh, post_scale, do_scale):
    out = np.stack([oracle.resize_linear_f32(p, dw, dh) for p in src])
    return out * np.float32(post_scale) if do_scale else out


def prove_linear_kernel(sw, sh, dw, dh, tiled):
    """The dispatch literal of a case against the boxes the tiled kernel would form: tiled only if every box fits; where a case is
    listed as generic because of its extent, some box must indeed not fit."""
    wmax = max(b[1] for b in linear_box(sw, dw, "x"))
    hmax = max(b[1] for b in linear_box(sh, dh, "y"))
    if tiled:
        assert wmax <= RL_BW and hmax <= RL_BH, (wmax, hmax)
    return wmax, hmax


def check_linear(ctx, oracle, src, dw, dh, tiled, post_scale=1.0, do_scale=False, against_c2=True):
    """launch_resize_linear_f32 on caller-made planes against the oracle; `tiled` is the kernel the case expects for ONE channel.
    A fitting one-channel case is run again as two interleaved channels through the generic kernel: same data, same bits."""
    src = np.ascontiguousarray(src, np.float32)
    b, sh, sw = src.shape[:3]
    cn = 1 if src.ndim == 3 else 2
    prove_linear_kernel(sw, sh, dw, dh, tiled and cn == 1)
    want = want_linear(oracle, src, dw, dh, post_scale, do_scale)
    got, took = ctx.debug_resize_linear_f32(src, dw, dh, post_scale, do_scale, fill=FILL)
    assert took == (tiled and cn == 1), "the launcher took the %s kernel" % ("tiled" if took else "generic")
    same("linear %dx%d -> %dx%d, %d planes x %d, %s" % (sw, sh, dw, dh, b, cn, "tiled" if took else "generic"), got, want)
    if cn == 1 and tiled and against_c2:
        pairs = np.stack([src, np.roll(src, 1, axis=0)], axis=-1)  # plane k beside plane k - 1
        got2, took2 = ctx.debug_resize_linear_f32(pairs, dw, dh, post_scale, do_scale, fill=FILL)
        assert not took2
        same("linear %dx%d -> %dx%d, generic two-channel kernel on the tiled kernel's planes" % (sw, sh, dw, dh), got2[..., 0], want)
        same("... second channel", got2[..., 1], np.roll(want, 1, axis=0))


# (source w, h, destination w, h, tiled, why) — the literals are computed from the launcher's rule by hand; prove_linear_kernel and
# tests/test_cpu_flow_pyramid.py check them against the boxes
LINEAR_DISPATCH = [
    (144, 18, 128, 16, True, "fits"),
    (145, 18, 128, 16, False, "x extent too large"),
    (73, 18, 64, 16, True, "fits only because the extent is clamped to the source width"),
    (72, 38, 64, 32, True, "fits"),
    (72, 39, 64, 32, False, "y extent too large"),
    (200, 18, 177, 16, False, "x fails, y fits"),
    (2, 2, 64, 16, True, "tiny source"),
    (2, 2, 70, 20, True, "tiny source"),
    (9, 7, 8, 6, True, "tiny source and destination"),
]
LINEAR_SHAPES = [  # (sw, sh, dw, dh, tiled, why)
    (70, 20, 70, 20, True, "ratio exactly 1"),
    (64, 16, 64, 16, True, "ratio exactly 1 on the tile"),
    (20, 9, 61, 23, True, "upscale x3"),
    (33, 40, 70, 36, True, "up on x, down on y"),
    (71, 17, 64, 33, True, "down on x, up on y"),
    (1, 1, 5, 4, True, "source of one pixel"),
    (2, 1, 3, 1, True, "source of 2 x 1"),
    (1, 2, 1, 5, True, "source of 1 x 2"),
    (40, 40, 1, 1, True, "destination of one pixel: a tile of one column and one row"),
    (5, 4, 2, 3, True, "destination 2 x 3"),
    (6, 6, 4, 5, True, "destination 4 x 5"),
    (70, 17, 63, 15, True, "tile edge"), (71, 18, 64, 16, True, "tile edge"), (72, 19, 65, 17, True, "tile edge"),
    (71, 19, 64, 17, True, "tile edge"), (72, 17, 65, 15, True, "tile edge"),
    (143, 37, 129, 33, True, "odd source width: rows not 16-byte aligned"),
    (300, 30, 133, 27, False, "x2.26 on x"),
    (31, 300, 28, 100, False, "x3 on y"),
    (20, 60, 61, 20, False, "up on x, x3 down on y: the generic kernel's clamps at both ends of a row (a downscale never reaches them)"),
    (70, 60, 70, 20, False, "ratio 1 on x, x3 down on y: generic, every fraction 0 on x"),
    (200, 9, 80, 23, False, "x2.5 down on x, up on y: the generic kernel's row clamps"),
]
# (sw, sh, dw, dh, planes, workgroups): the xcd_tile re-deal starts at 64 workgroups
LINEAR_GRIDS = [(213, 124, 192, 112, 3, 63), (284, 284, 256, 256, 1, 64), (71, 231, 64, 208, 5, 65), (111, 44, 100, 40, 11, 66)]
PLANE_COUNTS = (1, 2, 3, 4, 6, 8)
SCALES = ((1.0, False), (0.5, True), (1.0 / 0.9, True))
CONTENT = ("noise", "constant", "negzero", "subnormal", "ones", "mixed")


# ---- C: the cubic flow resize -------------------------------------------------------------------------------------------------------------
def want_cubic(oracle, src, dw, dh, post_scale):
    return np.stack([oracle.resize_cubic_f32(p, dw, dh) for p in src]) * np.float32(post_scale)


def check_cubic(ctx, oracle, src, dw, dh, tiled, post_scale=1.0, table_too=True):
    """launch_resize_cubic_f32c2 on caller-made flows against the oracle's resize and float multiply. A tiled case runs again
    through the pointer table, which forces the generic kernel: generic against tiled on the same data."""
    src = np.ascontiguousarray(src, np.float32)
    b, sh, sw = src.shape[:3]
    if tiled:
        wx, wy = max(e for _, e in cubic_window(sw, dw, "x")), max(e for _, e in cubic_window(sh, dh, "y"))
        assert wx <= UC_SW and wy <= UC_SH, (wx, wy)
    want = want_cubic(oracle, src, dw, dh, post_scale)
    got, took = ctx.debug_resize_cubic_flow(src, dw, dh, post_scale, False, fill=FILL)
    assert took == tiled, "the launcher took the %s kernel" % ("tiled" if took else "generic")
    same("cubic %dx%d -> %dx%d, %d flows, x%r, %s" % (sw, sh, dw, dh, b, post_scale, "tiled" if took else "generic"), got, want)
    if table_too:
        got2, took2 = ctx.debug_resize_cubic_flow(src, dw, dh, post_scale, True, fill=FILL)
        assert not took2
        same("cubic %dx%d -> %dx%d through the pointer table (generic)" % (sw, sh, dw, dh), got2, want)


INV_PYR = float(np.float32(1.0) / np.float32(0.9))        # FlowEngine::compute: 1.0f / pc.pyrScaleFactor
ODD_H_SCALE = float(np.float32(37) / np.float32(75))      # ... and float(dh) / float(h) for h = 75
CUBIC_TILED = [  # (sw, sh, dw, dh, why)
    (25, 25, 28, 28, "x1/0.9, coarsest"), (63, 25, 70, 28, "x1/0.9"), (64, 30, 71, 33, "x1/0.9"), (65, 44, 72, 49, "x1/0.9"),
    (70, 20, 70, 20, "ratio exactly 1"), (64, 16, 64, 16, "ratio exactly 1 on the tile"),
    (33, 9, 66, 18, "x2"), (10, 5, 70, 35, "x7"),
    (1, 1, 5, 4, "source 1 x 1"), (2, 1, 64, 3, "source 2 x 1"), (1, 3, 2, 17, "source 1 x 3"), (3, 2, 65, 16, "source 3 x 2"),
    (57, 14, 63, 15, "tile edge"), (58, 15, 64, 16, "tile edge"), (59, 16, 65, 17, "tile edge"),
    (130, 40, 130, 40, "ratio 1: a second tile column needs window columns beyond 64"),
]
CUBIC_GENERIC = [  # (sw, sh, dw, dh, why)
    (75, 60, 37, 30, "x0.5 both axes"), (28, 28, 25, 25, "x0.9 both axes"), (80, 20, 40, 40, "down on x, up on y"),
    (20, 80, 40, 40, "up on x, down on y"), (75, 75, 37, 37, "odd size halved"), (5, 4, 1, 1, "destination of one pixel"),
]
CUBIC_GRIDS = [(120, 230, 128, 256, 1, 32), (120, 230, 128, 256, 3, 96), (230, 120, 256, 128, 1, 32), (58, 229, 64, 254, 4, 64)]
CUBIC_SCALES = (1.0, INV_PYR, ODD_H_SCALE)
