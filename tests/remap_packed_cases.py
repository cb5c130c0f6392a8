"""The cases tests/test_gpu_remap_packed.py runs on the device and the CPU emulation replays
(test_cpu_library_emulation.py::test_operator_level_gpu_tests_pass_on_the_emulated_library): the frame's packed bicubic remap
(render_kernels.hip: k_remap_pack + k_remap_cubic_u8c4_packed — every projection and the pole warp of a frame) and pole removal's
warp (k_remap_cubic_u8c4_tiled<MapFromFlowAdd>) through the test taps of include/s360_debug_remap.h, on maps and flows made here.

References. Pixels: the oracle's remap_cubic_u8 (per-tap integer sums) on the 4-channel source, on the 3-channel source for alpha
mode 1, and preparePoleImage's alpha rule in numpy; the pole warp's map is the oracle's own loop (pole_warp_map). Packed dwords and
tile records: the numpy restatement below of remap_coord and of the box rule — integer, exact. Every comparison is word for word
over the whole buffer; the outputs are pre-filled with a byte the reference does not contain, so a pixel, dword or record that no
workgroup stores (or that a second one overwrites with another tile's value) shows.

Every case first proves ON THE RESTATEMENT that it reaches the class it is named for, then compares."""
import numpy as np

PT_W, PT_H, PT_CAP = 64, 16, 4096  # the packed kernels' destination tile and LDS box (render_kernels.hip)
RT_W, RT_H, RT_CAP = 64, 8, 4608   # the tiled kernel's
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NAN, INF = float("nan"), float("inf")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cv_round(v):
    """cvRound of a float32 array: round-half-even, INT_MIN where the value is not in [-2^31, 2^31) (NaN included)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    return np.where(ok, np.rint(np.where(ok, v, np.float32(0))).astype(np.int64), INT_MIN)


def remap_coord(mp):
    """first tap (sx, sy), fraction index and the 1/32-pixel integers (ix, iy) of a map (.. x 2, float32)."""
    mp = np.asarray(mp, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        i = cv_round(mp * np.float32(32))
    ix, iy = i[..., 0], i[..., 1]
    fxy = (iy & 31) * 32 + (ix & 31)
    sx = np.clip(ix >> 5, -32768, 32767) - 1
    sy = np.clip(iy >> 5, -32768, 32767) - 1
    return sx, sy, fxy, ix, iy


def restate(mp, sw, sh, tile_h=PT_H, cap=PT_CAP, field_limits=True):
    """What k_remap_pack must store for one map (dh x dw x 2) over a source of sw x sh: packed dwords, tile records, and the
    per-pixel integers they come from. Box rule: min / max of the LIVE first taps, + 4; no live pixel: (INT_MAX, INT_MAX, 0, 0);
    area > cap, width > 2047 or height > 1023: height -1."""
    dh, dw = mp.shape[:2]
    sx, sy, fxy, ix, iy = remap_coord(mp)
    live = ~((sx >= sw) | (sx + 4 <= 0) | (sy >= sh) | (sy + 4 <= 0))
    ty, tx = -(-dh // tile_h), -(-dw // PT_W)
    tiles = np.empty((ty, tx, 4), np.int64)
    packed = np.zeros((dh, dw), np.int64)
    for j in range(ty):
        for i in range(tx):
            s = (slice(j * tile_h, (j + 1) * tile_h), slice(i * PT_W, (i + 1) * PT_W))
            lv = live[s]
            if not lv.any():
                tiles[j, i] = (INT_MAX, INT_MAX, 0, 0)
                continue
            x0, y0 = sx[s][lv].min(), sy[s][lv].min()
            bw, bh = sx[s][lv].max() + 4 - x0, sy[s][lv].max() + 4 - y0
            if bw * bh > cap or (field_limits and (bw > 2047 or bh > 1023)):
                bh = -1
            tiles[j, i] = (x0, y0, bw, bh)
            if bh > 0:
                packed[s] = np.where(lv, 0x80000000 | ((sy[s] - y0) << 21) | ((sx[s] - x0) << 10) | fxy[s], 0)
    assert packed.max() < 2 ** 32 and packed.min() >= 0
    return dict(packed=packed.astype(np.uint32), tiles=tiles.astype(np.int32), sx=sx, sy=sy, fxy=fxy, ix=ix, iy=iy, live=live,
                sw=sw, sh=sh, tile_h=tile_h)


def tile_view(R, j, i):
    """the restatement of one tile: its record and its pixels' integers"""
    s = (slice(j * R["tile_h"], (j + 1) * R["tile_h"]), slice(i * PT_W, (i + 1) * PT_W))
    t = {k: R[k][s] for k in ("sx", "sy", "fxy", "ix", "iy", "live")}
    t["rec"] = tuple(int(v) for v in R["tiles"][j, i])
    t["sw"], t["sh"] = R["sw"], R["sh"]
    t["interior"] = t["live"] & (t["sx"] >= 0) & (t["sx"] + 4 <= R["sw"]) & (t["sy"] >= 0) & (t["sy"] + 4 <= R["sh"])
    return t


def accumulators(src, R, tab):
    """The 16-tap integer sums of the live pixels, BEFORE the rounding shift and the saturation (dead pixels: 0), from the
    restated coordinates and the oracle's weight table: dh x dw x channels, int64."""
    sh, sw, cn = src.shape
    P = np.zeros((sh + 7, sw + 7, cn), np.int64)
    P[3:3 + sh, 3:3 + sw] = src
    lv = R["live"]
    px, py = np.where(lv, R["sx"] + 3, 0), np.where(lv, R["sy"] + 3, 0)
    W = tab.astype(np.int64)[R["fxy"]]
    acc = np.zeros(lv.shape + (cn,), np.int64)
    for r in range(4):
        for q in range(4):
            acc += P[py + r, px + q] * W[..., r * 4 + q, None]
    return acc * lv[..., None]


def from_accumulators(acc):
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def feather_alpha(dh, y_feather_start, feather_size):
    """preparePoleImage's ramp: uint8(255.0f * (1.0f - float(y - start) / float(size))) for the rows y >= start; None above."""
    y = np.arange(dh)
    a = np.float32(1) - (y - y_feather_start).astype(np.float32) / np.float32(feather_size)
    v = (np.float32(255) * a).astype(np.int32)
    assert ((v >= 0) & (v <= 255))[y >= y_feather_start].all(), "the ramp leaves 0..255: float -> uint8_t is undefined there"
    return [int(v[k]) if k >= y_feather_start else None for k in range(dh)]


def pixels_reference(O, src, mp, alpha_mode, y_feather_start, feather_size):
    if alpha_mode == 1:  # the remap runs on 3 channels, cvtColor adds 255, the feather rows are overwritten
        out = np.concatenate([O.remap_cubic_u8(src[..., :3], mp), np.full(mp.shape[:2] + (1,), 255, np.uint8)], axis=2)
    else:
        out = O.remap_cubic_u8(src, mp)
    if alpha_mode:
        for y, a in enumerate(feather_alpha(mp.shape[0], y_feather_start, feather_size)):
            if a is not None:
                out[y, :, 3] = a if alpha_mode == 1 else np.minimum(out[y, :, 3], a)
    return out


def pick_fill(*arrays):
    """a byte that, repeated over a pixel / a word, occurs nowhere in the references: what was not stored stays visible"""
    for f in (0xA5, 0x5A, 0x3C, 0xC3, 0x96, 0x69, 0x77, 0xEE):
        hit = False
        for a in arrays:
            if a.dtype == np.uint8:
                hit |= bool(np.all(a == f, axis=-1).any())
            else:
                hit |= bool((a.view(np.uint32) == f * 0x01010101).any())
        if not hit:
            return f
    raise AssertionError("no free fill byte")


def same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (name, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s, want %s" % (
        name, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])


# ---- sources and maps -----------------------------------------------------------------------------------------------------------
def noise(rng, h, w):
    """every channel, the alpha plane included, varies from pixel to pixel"""
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def checker(rng, h, w):
    """0 / 255 in runs of one and two pixels, per channel: the cubic's overshoot reaches both ends of the saturation"""
    return (rng.integers(0, 2, (h, w, 4), dtype=np.uint8) * 255).astype(np.uint8)


def uniform(rng, th, tw, x0, x1, y0, y1):
    b = np.empty((th, tw, 2), np.float32)
    b[..., 0] = rng.uniform(x0, x1, (th, tw))
    b[..., 1] = rng.uniform(y0, y1, (th, tw))
    return b


def rand_map(rng, dw, dh, sw, sh):
    """every pixel on its own, around and beyond all four image edges: live and dead pixels, partial and whole taps; the box of a
    tile is at most (sw + 6) x (sw + 6)"""
    return uniform(rng, dh, dw, -3.4, sw + 0.9, -3.4, sh + 0.9)


class Case:
    """src: B x sh x sw x 4; map: B x dh x dw x 2; prove(list of restatements, one per image) asserts the class"""

    def __init__(self, src, mp, prove, alpha_mode=0, feather_size=None, weights=(0,)):
        self.src, self.map, self.prove, self.alpha_mode, self.weights = src, mp, prove, alpha_mode, weights
        dh = mp.shape[1]
        self.feather_size = feather_size if feather_size is not None else 1
        self.y_feather_start = dh - 1 - self.feather_size  # as the frame sets it (TestRenderStereoPanorama.cpp:629, 669)


# ---- grid classes of xcd_tile ---------------------------------------------------------------------------------------------------
# name: (dw, dh, batch, tiles x, tiles y): 1 tile; T < 64; T = 64 (T % 8 == 0); 65 and 71 (T % 8 != 0, remainder 1 and 7); a batch in z
GRIDS = {"1_tile": (5, 3, 1, 1, 1), "63_tiles": (530, 100, 1, 9, 7), "64_tiles": (490, 120, 1, 8, 8), "65_tiles": (317, 203, 1, 5, 13),
         "71_tiles": (4485, 3, 1, 71, 1), "72_tiles_batch": (330, 50, 3, 6, 4)}


def grid_case(name):
    dw, dh, batch, tx, ty = GRIDS[name]
    rng = np.random.default_rng(dw * 1000 + dh)
    sw, sh = 37, 29
    src = np.stack([noise(rng, sh, sw) for _ in range(batch)])
    mp = np.stack([rand_map(rng, dw, dh, sw, sh) for _ in range(batch)])

    def prove(Rs):
        for R in Rs:
            assert R["tiles"].shape[:2] == (ty, tx)
            assert (R["tiles"][..., 3] > 0).all(), "every tile of a grid case renders from LDS"
            assert R["live"].any() and not R["live"].all()
        assert batch * tx * ty == int(name.split("_")[0])
        if tx * ty > 1 and name != "64_tiles":
            assert dw % PT_W and (dh % PT_H or ty == 1), "partial last tiles"
    return Case(src, mp, prove)


# ---- tile classes ---------------------------------------------------------------------------------------------------------------
FAR = np.array([1e9, -1e9, 7e7, -7e7, NAN, INF, -INF, 40000.0, -40000.0], np.float32)
EMPTY = (INT_MAX, INT_MAX, 0, 0)


def _t_dead_nan(rng, th, tw, sw, sh):
    return np.full((th, tw, 2), NAN, np.float32)


def _t_dead_outside(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, sw + 1.5, sw + 60, -60, -2.6)
    far = rng.random((th, tw)) < 0.3
    b[far, rng.integers(0, 2, int(far.sum()))] = FAR[rng.integers(0, len(FAR), int(far.sum()))]
    return b


def _t_interior(rng, th, tw, sw, sh):
    return uniform(rng, th, tw, 11.1, 30.9, 11.1, 25.9)


def _t_left(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, -3.4, 6, 20, 30)
    b[0, 0, 0] = -2.0
    return b


def _t_top(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, 20, 30, -3.4, 6)
    b[0, 0, 1] = -2.0
    return b


def _t_right(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, sw - 8, sw + 0.9, 20, 30)
    b[0, 0, 0] = sw + 0.9
    return b


def _t_bottom(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, 20, 30, sh - 8, sh + 0.9)
    b[0, 0, 1] = sh + 0.9
    return b


def _t_corner_tl(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, -3.4, 4, -3.4, 4)
    b[0, 0] = (-2.0, -2.0)
    return b


def _t_corner_br(rng, th, tw, sw, sh):
    b = uniform(rng, th, tw, sw - 6, sw + 0.9, sh - 6, sh + 0.9)
    b[0, 0] = (sw + 0.9, sh + 0.9)
    return b


def _t_mixed(rng, th, tw, sw, sh):
    b = _t_interior(rng, th, tw, sw, sh)
    far = rng.random((th, tw)) < 0.4
    far[0, 0], far[-1, -1] = False, True
    b[far, rng.integers(0, 2, int(far.sum()))] = FAR[rng.integers(0, len(FAR), int(far.sum()))]
    return b


def _box(x1, y1):
    """first taps from (10, 5) to (x1, y1): the box is (x1 - 6) x (y1 - 1)"""
    def make(rng, th, tw, sw, sh):
        b = uniform(rng, th, tw, 11.1, x1 + 0.9, 6.1, y1 + 0.9)
        b[0, 0] = (11.0, 6.0)
        b[-1, -1] = (x1 + 1.0, y1 + 1.0)
        return b
    return make


def _t_fallback_both(rng, th, tw, sw, sh):
    return uniform(rng, th, tw, -3.4, sw + 0.9, -3.4, sh + 0.9)


COMMON_VALUES = [NAN, INF, -INF, 1e9, -1e9, 7e7, -7e7, 6.7e7, -6.7e7, 32766.5, 32767.0, 32767.99, 32768.0, 32769.0, -32767.0, -32768.0,
                 -32769.0, 40000.0, -40000.0]


def special_values(n, low):
    """NaN, infinities, values whose 1/32-pixel integer overflows (cvRound gives INT_MIN), the short saturation, -0.0, and the values
    around one end of the live range: mx = -2 - 1/32 is the last dead one on the left (sx + 4 <= 0), n + 1 - 1/32 the last live
    one on the right (sx >= n), the half-way values between them round to even"""
    ends = [-0.0, 0.0, -3.0, -2.03125, -2.0 - 1 / 64, -2.0 - 3 / 64, -2.0, -1.98] if low else \
        [n + 0.5, n + 1 - 1 / 32, n + 1 - 1 / 64, n + 1 - 3 / 64, n + 1.0, n + 2.0]
    return np.array(COMMON_VALUES + ends, np.float32)


def _values(low):
    """each special value once as x and once as y, the other coordinate live near the same end of the image, so the tile's box fits
    and the values are PACKED, and whether the pixel lives hangs on the special coordinate alone"""
    def make(rng, th, tw, sw, sh):
        b = (uniform(rng, th, tw, 1.1, 8.9, 1.1, 8.9) if low else uniform(rng, th, tw, sw - 9, sw - 0.1, sh - 9, sh - 0.1)).reshape(-1, 2)
        vx, vy = special_values(sw, low), special_values(sh, low)
        assert len(b) >= 2 * len(vx) + 2
        b[:len(vx), 0] = vx
        b[len(vx):2 * len(vx), 1] = vy
        b[2 * len(vx)] = (NAN, NAN)
        b[2 * len(vx) + 1] = (-2.0, -2.0) if low else (sw + 1 - 1 / 32, sh + 1 - 1 / 32)
        return b.reshape(th, tw, 2)
    return make


def _t_halfway(rng, th, tw, sw, sh):
    """k / 64 with k odd: mx * 32 ends in .5 exactly, of both signs (the dead ones are outside: they test the rounding of the
    live test, the live ones the fraction index)"""
    b = np.empty((th, tw, 2), np.float32)
    b[..., 0] = (2 * rng.integers(-110, 640, (th, tw)) + 1) / 64.0
    b[..., 1] = (2 * rng.integers(-110, 640, (th, tw)) + 1) / 64.0
    return b


def _is_fit(t):
    return t["rec"][3] > 0


def _e_dead(t):
    assert t["rec"] == EMPTY and not t["live"].any()


def _e_interior(t):
    x0, y0, bw, bh = t["rec"]
    assert _is_fit(t) and x0 >= 0 and y0 >= 0 and x0 + bw <= t["sw"] and y0 + bh <= t["sh"] and t["live"].all()


def _e_mixed(t):
    x0, y0, bw, bh = t["rec"]
    assert _is_fit(t) and x0 >= 10 and y0 >= 10 and x0 + bw <= 34 and y0 + bh <= 29, "the dead pixels' coordinates stayed out of the box"
    assert t["live"].any() and (~t["live"]).sum() >= 2
    assert (np.abs(t["sx"][~t["live"]]) > 30000).any() and (np.abs(t["sy"][~t["live"]]) > 30000).any()


def _e_values(low):
    def e(t):
        for s, n in ((t["sx"], t["sw"]), (t["sy"], t["sh"])):
            for v, lv in (((-4, False), (-3, True)) if low else ((n - 1, True), (n, False))):  # both sides of the end of the live range
                assert (s[t["live"] == lv] == v).any(), (v, lv)
            assert (s == 32766).any() and (s == -32769).any(), "the short saturation on both sides"
        assert (t["ix"] == INT_MIN).sum() >= 8 and (t["iy"] == INT_MIN).sum() >= 8, "NaN, the infinities and the overflowing values"
        assert _is_fit(t), "the values are packed, not gathered"
    return e


def _e_halfway(t):
    assert _is_fit(t) and t["live"].sum() > 100 and (~t["live"]).sum() > 3
    assert (t["ix"] < 0).any() and (t["ix"] > 0).any() and (t["iy"] < 0).any() and (t["iy"] > 0).any()


def _e_fallback_both(t):
    assert t["rec"][3] == -1 and t["rec"][2] > 64
    border = t["live"] & ~t["interior"]
    assert t["interior"].sum() > 20 and border.sum() > 20 and (~t["live"]).any(), "both branches of remap_cubic_u8c4_at"


def _e_rec(*rec):
    def e(t):
        assert t["rec"] == rec, (t["rec"], rec)
    return e


def _e_edges(left=None, top=None, right=None, bottom=None):
    def e(t):
        x0, y0, bw, bh = t["rec"]
        assert _is_fit(t) and t["live"].any()
        if left:
            assert x0 == -3, "negative origin"
        if top:
            assert y0 == -3, "negative origin"
        if right:
            assert x0 + bw == t["sw"] + 3
        if bottom:
            assert y0 + bh == t["sh"] + 3
    return e


TILE_CLASSES = [
    ("dead_nan", _t_dead_nan, _e_dead), ("dead_outside", _t_dead_outside, _e_dead), ("interior", _t_interior, _e_interior),
    ("left", _t_left, _e_edges(left=True)), ("top", _t_top, _e_edges(top=True)), ("right", _t_right, _e_edges(right=True)),
    ("bottom", _t_bottom, _e_edges(bottom=True)), ("corner_top_left", _t_corner_tl, _e_edges(left=True, top=True)),
    ("corner_bottom_right", _t_corner_br, _e_edges(right=True, bottom=True)), ("live_and_far_dead", _t_mixed, _e_mixed),
    ("box_64x64", _box(70, 65), _e_rec(10, 5, 64, 64)), ("box_65x64", _box(71, 65), _e_rec(10, 5, 65, -1)),
    ("box_63x65", _box(69, 66), _e_rec(10, 5, 63, 65)), ("fallback_both_branches", _t_fallback_both, _e_fallback_both),
    ("map_values_low", _values(True), _e_values(True)), ("map_values_high", _values(False), _e_values(False)),
    ("halfway", _t_halfway, _e_halfway),
]


def classes_case(source, classes=TILE_CLASSES, sw=101, sh=90, tx=4, last_w=37, last_h=9, batch=3):
    """One tile per class, 4 tiles per row, the last column 37 wide and the last row 9 high; image b has the classes rotated by 5 b
    tiles: the images' records differ tile by tile (a wrong stride between the images' records shows), and every class sits in
    whole and in partial tiles."""
    ty = -(-len(classes) // tx)
    dw, dh = (tx - 1) * PT_W + last_w, (ty - 1) * PT_H + last_h
    rng = np.random.default_rng(sw * 7 + sh + len(classes))
    src = np.stack([source(rng, sh, sw) for _ in range(batch)])
    mp = np.empty((batch, dh, dw, 2), np.float32)
    order = [[classes[(k + 5 * b) % len(classes)] for k in range(tx * ty)] for b in range(batch)]
    for b in range(batch):
        for k, (_, make, _) in enumerate(order[b]):
            j, i = divmod(k, tx)
            th, tw = min(PT_H, dh - j * PT_H), min(PT_W, dw - i * PT_W)
            mp[b, j * PT_H:j * PT_H + th, i * PT_W:i * PT_W + tw] = make(rng, th, tw, sw, sh)

    def prove(Rs):
        for b, R in enumerate(Rs):
            for k, (name, _, expect) in enumerate(order[b]):
                try:
                    expect(tile_view(R, *divmod(k, tx)))
                except AssertionError as e:
                    raise AssertionError("image %d tile %d (%s): %s" % (b, k, name, e))
        if batch > 1:
            assert not np.array_equal(Rs[0]["tiles"], Rs[1]["tiles"]) and not np.array_equal(Rs[1]["tiles"], Rs[2]["tiles"])
    return Case(src, mp, prove)


def _tall(y1, x1=3):
    """first taps (2 .. x1 - 1, 10 .. y1) in a source 8 wide: a box of (x1 + 1) x (y1 - 6)"""
    def make(rng, th, tw, sw, sh):
        b = uniform(rng, th, tw, 3.1, x1 + 0.9, 11.1, y1 + 0.9)
        b[0, 0] = (3.0, 11.0)
        b[-1, -1] = (float(x1), y1 + 1.0)
        return b
    return make


def _e_tall_fallback(rec):
    def e(t):
        assert t["rec"] == rec and t["interior"].all(), "the gather's interior branch"
    return e


# bh > 1023 decides at exactly 4 x 1024 = 4096 = PT_CAP (the narrowest box is 4 wide); its sibling bw > 2047 never does
TALL_CLASSES = [("4x1020", _tall(1026), _e_rec(2, 10, 4, 1020)), ("4x1023", _tall(1029), _e_rec(2, 10, 4, 1023)),
                ("4x1024_field_limit", _tall(1030), _e_tall_fallback((2, 10, 4, -1))),
                ("5x1000_area", _tall(1006, 4), _e_tall_fallback((2, 10, 5, -1))), ("4x1024_again", _tall(1030), _e_tall_fallback((2, 10, 4, -1))),
                ("4x512", _tall(518), _e_rec(2, 10, 4, 512))]


def tall_case():
    return classes_case(noise, TALL_CLASSES, sw=8, sh=1100, tx=3, last_w=64, last_h=16, batch=1)


# ---- tiny sources, saturation, feather ------------------------------------------------------------------------------------------
TINY = [(1, 1), (2, 3), (3, 2), (5, 1), (1, 5), (5, 5), (7, 6)]


def tiny_case(sw, sh):
    rng = np.random.default_rng(sw * 10 + sh)
    src = np.stack([noise(rng, sh, sw), checker(rng, sh, sw)])
    mp = np.stack([rand_map(rng, 70, 20, sw, sh) for _ in range(2)])

    def prove(Rs):
        for R in Rs:
            assert R["live"].sum() > 200 and (~R["live"]).any() and (R["tiles"][..., 3] > 0).all()
            interior = R["live"] & (R["sx"] >= 0) & (R["sx"] + 4 <= sw) & (R["sy"] >= 0) & (R["sy"] + 4 <= sh)
            assert interior.any() == (sw >= 4 and sh >= 4), "below 4 x 4 every tap window hangs over an edge"
    return Case(src, mp, prove)


def checker_case(O):
    rng = np.random.default_rng(5)
    sw, sh = 37, 29
    src, mp = checker(rng, sh, sw)[None], rand_map(rng, 130, 40, sw, sh)[None]

    def prove(Rs):
        v = (accumulators(src[0], Rs[0], O.bicubic_tab_i()) + (1 << 14)) >> 15
        for ch in range(4):
            assert (v[..., ch] < 0).sum() > 10 and (v[..., ch] > 255).sum() > 10, "both ends of the saturation, channel %d" % ch
    return Case(src, mp, prove)


FEATHERS = [(m, f) for m in (1, 2) for f in (1, 3, 31, 50)]


def feather_case(O, alpha_mode, feather_size):
    rng = np.random.default_rng(alpha_mode * 100 + feather_size)
    sw, sh, dw, dh = 37, 29, 70, 40
    src, mp = noise(rng, sh, sw)[None], rand_map(rng, dw, dh, sw, sh)[None]

    def prove(Rs):
        ramp = feather_alpha(dh, dh - 1 - feather_size, feather_size)
        rows = [y for y, a in enumerate(ramp) if a is not None]
        assert len(rows) == min(dh, feather_size + 1) and ramp[dh - 1] == 0
        if feather_size > dh:
            assert dh - 1 - feather_size < 0 and ramp[0] is not None and 0 < ramp[0] < 255, "negative start: the ramp begins above row 0"
        if alpha_mode == 2 and feather_size > 1:  # the minimum takes each side somewhere
            a = from_accumulators(accumulators(src[0], Rs[0], O.bicubic_tab_i()))[..., 3]
            r = np.array([x if x is not None else 999 for x in ramp])[:, None]
            assert ((a < r) & (r < 999) & Rs[0]["live"]).sum() > 5 and ((a > r) & Rs[0]["live"]).sum() > 5
    return Case(src, mp, prove, alpha_mode=alpha_mode, feather_size=feather_size)


# ---- the weights: every fraction index, every tap on a rounding boundary --------------------------------------------------------
# The three fraction indices whose sums cannot come within 255 of a rounding boundary, whatever the source: a weight off by one is
# invisible there in every output (an error of 64 or more is not; their 32 samples each are ordinary ones). Index 0: weights 32767 and
# 1, the sum 32767 p + q + 16384 has a remainder of 16384 - p + q. Indices 16 and 512 (one fraction 1/2, the other 0): the weights
# -3072, 19456, 19456, -3072 are multiples of 1024, so is the remainder, and at most 255 is added.
NO_BOUNDARY = (0, 16, 512)
_WEIGHTS = {}


def weights_case(O, alpha_mode):
    if "base" not in _WEIGHTS:  # (the search once for the three alpha modes)
        _WEIGHTS["base"] = _weights_base(O)
    src, mp, prove = _WEIGHTS["base"]
    return Case(src, mp, prove, alpha_mode=alpha_mode, feather_size=31, weights=(1, 2, 0))


def _weights_base(O):
    """512 x 64 destination = 32768 samples: for each of the 1024 fraction indices and each of its 16 taps, one sample whose sum
    sits so close below a rounding boundary that the tap's weight + 1 raises the output byte, and one so close above that the
    weight - 1 lowers it (32 samples per index, each on one of the channels B, G, R, unsaturated on both sides of the step). Found
    by search in a 70 x 58 noise source: position (11055 tap windows x channels) against index, the window is the tap's own pixel
    value wide, so ~40 candidates per sample exist. With random samples a weight that is off by one moves the sum by at most 255 of
    32768 and flips a byte in under 0.8 % of them; here a weight off by ANY amount on ANY tap of ANY index flips one surely.
    (Three indices admit no such sample: NO_BOUNDARY above.) The source's 4060 pixels fit the LDS box, so every tile renders through the weights under test, not through the gather."""
    rng = np.random.default_rng(77)
    tab = O.bicubic_tab_i().astype(np.int64)
    sw, sh, dw, dh = 70, 58, 512, 64
    src = noise(rng, sh, sw)
    nx, ny = sw - 3, sh - 3
    win = np.lib.stride_tricks.sliding_window_view(src[..., :3].astype(np.int64), (4, 4), axis=(0, 1))  # ny x nx x 3 x 4 x 4
    P = np.ascontiguousarray(win.reshape(ny * nx * 3, 16))
    acc = (tab.astype(np.float64) @ P.T.astype(np.float64)).astype(np.int64) + (1 << 14)  # exact: |sums| < 2^53
    out, fr = acc >> 15, acc & 32767
    ok = (out >= 1) & (out <= 254)
    samples = np.empty((1024, 16, 2), np.int64)  # -> candidate (window * 3 + channel)
    for t in range(16):
        for d, hit in enumerate((ok & (fr + P[None, :, t] >= 32768), ok & (fr - P[None, :, t] < 0))):
            first = hit.argmax(axis=1)
            none = ~hit[np.arange(1024), first]
            assert set(np.nonzero(none)[0]) <= set(NO_BOUNDARY), "no sample for tap %d of index %s" % (t, np.nonzero(none)[0])
            samples[:, t, d] = np.where(none, ok.argmax(axis=1), first)
    e = np.broadcast_to(np.arange(1024)[:, None, None], samples.shape).reshape(-1)
    pos = samples.reshape(-1) // 3
    order = rng.permutation(e.size)  # every tile gets samples from all over the source
    e, pos = e[order], pos[order]
    mp = np.empty((dh * dw, 2), np.float32)
    mp[:, 0] = (pos % nx) + 1 + (e & 31) / 32.0
    mp[:, 1] = (pos // nx) + 1 + (e >> 5) / 32.0
    mp = mp.reshape(1, dh, dw, 2)
    tap, sign, chan = [np.broadcast_to(a, samples.shape).reshape(-1)[order].reshape(dh, dw) for a in
                       (np.arange(16)[None, :, None], np.array([1, -1])[None, None, :], samples % 3)]

    def prove(Rs):
        R = Rs[0]
        assert (R["tiles"][..., 3] > 0).all() and R["live"].all()
        assert np.array_equal(np.unique(R["fxy"]), np.arange(1024)) and (np.bincount(R["fxy"].reshape(-1)) == 32).all()
        a = np.take_along_axis(accumulators(src, R, tab), chan[..., None], axis=2)[..., 0] + (1 << 14)
        padded = np.zeros((sh + 7, sw + 7), np.int64)
        value = np.zeros((dh, dw), np.int64)
        for ch in range(3):
            padded[3:3 + sh, 3:3 + sw] = src[..., ch]
            value = np.where(chan == ch, padded[R["sy"] + 3 + tap // 4, R["sx"] + 3 + tap % 4], value)
        now, then = a >> 15, (a + sign * value) >> 15
        on = ~np.isin(R["fxy"], NO_BOUNDARY)
        assert (then == now + sign)[on].all() and (now >= 1).all() and (now <= 254).all(), "a weight off by one changes the sample's byte"
    return src[None], mp, prove


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def check_case(run, O, case):
    """run(src, map, alpha_mode, y_feather_start, feather_size, weights, fill) -> (images, packed, tiles)"""
    B = case.src.shape[0]
    Rs = [restate(case.map[b], case.src.shape[2], case.src.shape[1]) for b in range(B)]
    case.prove(Rs)
    want = np.stack([pixels_reference(O, case.src[b], case.map[b], case.alpha_mode, case.y_feather_start, case.feather_size) for b in range(B)])
    if case.alpha_mode == 0:  # the restatement's own pixels: a second, independent statement of the sums
        tab = O.bicubic_tab_i()
        same("numpy pixels against the oracle", np.stack([from_accumulators(accumulators(case.src[b], Rs[b], tab)) for b in range(B)]), want)
    packed, tiles = np.stack([R["packed"] for R in Rs]), np.stack([R["tiles"] for R in Rs])
    fill = pick_fill(want, packed, tiles)
    for weights in case.weights:
        got, gpacked, gtiles = run(case.src, case.map, case.alpha_mode, case.y_feather_start, case.feather_size, weights, fill)
        same("tile records (weights %d)" % weights, gtiles, tiles)
        same("packed dwords (weights %d)" % weights, gpacked, packed)
        same("pixels (weights %d)" % weights, got, want)


# ---- the pole warp --------------------------------------------------------------------------------------------------------------
POLE_W, POLE_ROWS = 150, 37  # 3 x 3 tiles, the last 22 wide and 5 high
RAMPS = {"ramp": (90.0, 30.0, 60.0, 75.0), "zero_divisor": (90.0, 45.0, 45.0, 60.0)}
POLE_FLOWS = ("zero", "constant", "large", "outside", "nan")
POLE_CASES = [(f, "ramp") for f in POLE_FLOWS] + [("zero", "zero_divisor"), ("constant", "zero_divisor"), ("nan", "zero_divisor")]


def pole_flow(kind, rng, h=POLE_ROWS, w=POLE_W):
    f = np.zeros((h, w, 2), np.float32)
    if kind == "constant":
        f[...] = (3.3, -1.7)
    elif kind == "large":  # neighbours point far apart: boxes beyond the LDS tile
        f = rng.uniform(-90, 90, (h, w, 2)).astype(np.float32)
        f[:, :64] /= 30  # (the first tile column's boxes still fit)
    elif kind == "outside":  # the left tiles point far outside, the rest over the edges
        f = rng.uniform(-4, 4, (h, w, 2)).astype(np.float32)
        f[:, :70, 0] += 1000
        f[:, 70:, 1] -= 25
    elif kind == "nan":
        f = rng.uniform(-6, 6, (h, w, 2)).astype(np.float32)
        bad = rng.random((h, w)) < 0.15
        f[bad, rng.integers(0, 2, int(bad.sum()))] = np.array([NAN, INF, -INF, 1e9], np.float32)[rng.integers(0, 4, int(bad.sum()))]
    return f


def rampf(x, a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.float32(x) - np.float32(a)) / (np.float32(b) - np.float32(a))
    m = np.where(t < 1, t, np.float32(1))  # std::min(1.0f, t): 1 for NaN
    return np.where(0 < m, m, np.float32(0))


def check_pole_warp(run, O, kind, ramp):
    """run(ext, flow, radius, start, mid, end, fill) -> (warped, packed, tiles)"""
    radius, start, mid, end = RAMPS[ramp]
    rng = np.random.default_rng(len(kind) * 10 + len(ramp))
    ext, flow = noise(rng, POLE_ROWS, POLE_W), pole_flow(kind, rng)
    mp = O.pole_warp_map(flow, radius, start, mid)
    R = restate(mp, POLE_W, POLE_ROWS)
    phi = np.float32(radius) * (np.arange(POLE_ROWS) + np.float32(0.5)).astype(np.float32) / np.float32(POLE_ROWS)
    r = rampf(phi, start, mid)
    assert (r == 0).any() and (r == 1).any(), "rows without and with the whole flow"
    if ramp == "ramp":
        assert ((r > 0) & (r < 1)).sum() >= 5, "rows inside the ramp"
    else:
        assert ((r == 0) | (r == 1)).all() and (phi == np.float32(start)).any(), "a row with 0 / 0: std::min(1.0f, NaN) = 1"
        assert (r[phi == np.float32(start)] == 1).all()
    assert POLE_W % PT_W and POLE_ROWS % PT_H
    if kind == "zero":
        assert (R["fxy"] == 0).all() and R["live"].all()
    if kind == "constant":  # the three kinds of rows map differently: alpha and 1 - alpha cannot be exchanged
        assert np.array_equal(mp[r == 0][:, :, 1], np.broadcast_to(np.arange(POLE_ROWS, dtype=np.float32)[r == 0, None], mp[r == 0].shape[:2]))
        assert (mp[r == 1][:, 0, 0] == np.float32(3.3)).all()
    if kind == "large":
        assert (R["tiles"][..., 3] == -1).sum() >= 3 and (R["tiles"][..., 3] > 0).any()
        t = [tile_view(R, j, i) for j in range(3) for i in range(3) if R["tiles"][j, i, 3] == -1]
        assert sum(x["interior"].sum() for x in t) > 50 and sum((x["live"] & ~x["interior"]).sum() for x in t) > 50
    if kind == "outside":
        assert (R["tiles"][..., 3] == 0).any() and (~R["live"]).sum() > 1000 and (R["tiles"][..., 1] < 0).any()
    if kind == "nan":
        assert np.isnan(mp).any() and (R["ix"] == INT_MIN).sum() > 100
    want = O.remap_cubic_u8(ext, mp)
    if kind == "zero":  # index 0's weights are 32767 on the pixel itself and 1 on its diagonal neighbour: the image comes back
        same("the oracle's warp by a zero flow against the input", want, ext)
    fill = pick_fill(want, R["packed"], R["tiles"])
    got, gpacked, gtiles = run(ext, flow, radius, start, mid, end, fill)
    same("tile records", gtiles, R["tiles"])
    same("packed dwords", gpacked, R["packed"])
    same("pixels", got, want)
    if kind == "zero":
        same("warp by a zero flow against the input", got, ext)


# ---- pole removal's warp (the tiled kernel) -------------------------------------------------------------------------------------
BY_FLOW = [("small", 150, 37), ("large", 150, 37), ("nan", 70, 9), ("mixed_tiles", 200, 40)]


def check_remap_by_flow(run, O, kind, w, h):
    """run(src, flow, fill) -> image"""
    rng = np.random.default_rng(w + h + len(kind))
    src = noise(rng, h, w)
    if kind == "small":
        flow = rng.uniform(-5, 5, (h, w, 2)).astype(np.float32)
    elif kind == "large":
        flow = rng.uniform(-90, 90, (h, w, 2)).astype(np.float32)
    elif kind == "nan":
        flow = pole_flow("nan", rng, h, w)
    else:  # left tiles fit, right tiles do not
        flow = rng.uniform(-5, 5, (h, w, 2)).astype(np.float32)
        flow[:, 100:] *= 20
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    mp = np.stack([xx + flow[..., 0], yy + flow[..., 1]], axis=2).astype(np.float32)  # PoleRemoval.cpp:128-133
    R = restate(mp, w, h, tile_h=RT_H, cap=RT_CAP, field_limits=False)
    fits = R["tiles"][..., 3]
    if kind == "small":
        assert (fits > 0).all()
    if kind == "large":
        assert (fits == -1).sum() >= 10, "all but the narrow last column"
    if kind == "mixed_tiles":
        assert (fits > 0).any() and (fits == -1).any()
    if kind == "nan":
        assert (R["ix"] == INT_MIN).sum() > 20 and w % RT_W and h % RT_H
    want = O.remap_cubic_u8(src, mp)
    fill = pick_fill(want)
    same("pixels", run(src, flow, fill), want)
