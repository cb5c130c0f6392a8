"""The cases tests/test_gpu_cubemap_tiles.py runs on the device and the CPU emulation replays
(test_cpu_library_emulation.py::test_operator_level_gpu_tests_pass_on_the_emulated_library): the stereo cubemap of every frame
(render_kernels.hip: k_cubemap_pack + k_cubemap_tiles) and the on-demand kernel (k_cubemap) through the test taps of
include/s360_debug_cubemap.h, on eyes made here.

References, compared in this order, the first differing word named:
  1. maps: the oracle's cubemapWarpMap per face, bit for bit (both are the host's libm on the same machine);
  2. tile records and packed dwords: the integer restatement below, computed from the TAP'S OWN maps — remap_coord, per 16 x 16
     tile of one face the plain and the seam-shifted box and the narrower of the two, the + 4 extents, the area and the limit
     tests, the dword layout; exact, no float arithmetic beyond remap_coord's one multiplication;
  3. pixels: the oracle's stereoCubemap of every slot's two eyes (B, G, R planes of the BGRA eyes), byte for byte; the on-demand
     kernel's output on the same eyes; and a numpy restatement of the 16 wrapped taps from the restated coordinates and the oracle's
     weight table, which also gives the sums BEFORE the saturation (the checker case shows with it that it overshoots both ends).
Every output is pre-filled with a byte its reference does not contain: a pixel, dword or record nobody stores shows.

Every case first proves ON THE RESTATEMENT that it reaches the classes it is named for (REACHES), then compares."""
import numpy as np

from remap_packed_cases import pick_fill, remap_coord, same

CT = 16  # k_cubemap_tiles' tile of output pixels (CT_W = CT_H)
MAX_SLOTS = 16  # kCubeMaxSlots: slots per launch of k_cubemap_tiles


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def geometry(fw, fh, fmt):
    video = fmt == "video"
    return dict(fw=fw, fh=fh, video=video, ow=3 * fw if video else fw, eyeH=2 * fh if video else 6 * fh, txN=-(-fw // CT), tyN=-(-fh // CT))


def face_slot(G, s):
    """origin in one eye's half of the stacked layout and index in the maps' face list of face slot s"""
    if G["video"]:  # rows {LEFT, RIGHT, TOP}, {BOTTOM, BACK, FRONT} = list indices {1, 0, 2}, {3, 4, 5}
        row = int(s >= 3)
        return (s - 3 * row) * G["fw"], row * G["fh"], (1 - s if s < 2 else s)
    return 0, s * G["fh"], s


def restate(maps, sw, sh, fmt, cap):
    """What k_cubemap_pack must store for the face maps (6 x fh x fw x 2) over eyes of sw x sh: packed dwords of one eye's half,
    tile records, the per-pixel integers in the layout's order and, per tile, the classes it falls into."""
    fh, fw = maps.shape[1:3]
    G = geometry(fw, fh, fmt)
    half = sw >> 1
    packed = np.zeros((G["eyeH"], G["ow"]), np.int64)
    SX, SY, FXY = (np.zeros((G["eyeH"], G["ow"]), np.int64) for _ in range(3))
    tiles = np.empty((6, G["tyN"], G["txN"], 4), np.int64)
    cls = []
    for s in range(6):
        fx0, fy0, lst = face_slot(G, s)
        m = maps[lst][:, ::-1] if G["video"] else maps[lst]  # (video: faces flipped horizontally)
        sx, sy, fxy, _, _ = remap_coord(m)
        SX[fy0:fy0 + fh, fx0:fx0 + fw], SY[fy0:fy0 + fh, fx0:fx0 + fw], FXY[fy0:fy0 + fh, fx0:fx0 + fw] = sx, sy, fxy
        for ty in range(G["tyN"]):
            for tx in range(G["txN"]):
                t = (slice(ty * CT, (ty + 1) * CT), slice(tx * CT, (tx + 1) * CT))
                x, y = sx[t], sy[t]
                xs = x + np.where(x < half, sw, 0)  # the seam's view of the columns
                shifted = bool(xs.max() - xs.min() < x.max() - x.min())
                xk = xs if shifted else x
                bx0, by0 = int(xk.min()), int(y.min())
                bw, bh = int(xk.max()) + 4 - bx0, int(y.max()) + 4 - by0
                area = bw * bh > cap or bw > 2047 or bh > 1023
                limits = bx0 < -sw or bx0 + bw > 3 * sw or by0 < -sh or by0 + bh > 2 * sh
                lds = not (area or limits)
                tiles[s, ty, tx] = (bx0, by0, bw, bh if lds else -1)
                if lds:
                    packed[fy0 + ty * CT:fy0 + ty * CT + x.shape[0], fx0 + tx * CT:fx0 + tx * CT + x.shape[1]] = \
                        0x80000000 | ((y - by0) << 21) | ((xk - bx0) << 10) | fxy[t]
                cls.append(dict(slot=s, ty=ty, tx=tx, lds=lds, shifted=shifted, area=area, limits=limits, box=(bx0, by0, bw, bh),
                                only_x_limit=bx0 + bw > 3 * sw and not (area or by0 + bh > 2 * sh),
                                only_y_limit=by0 + bh > 2 * sh and not (area or bx0 + bw > 3 * sw),
                                partial_x=x.shape[1] < CT, partial_y=x.shape[0] < CT, exact_cap=bw * bh == cap))
    assert packed.max() < 2 ** 32 and packed.min() >= 0
    return dict(packed=packed.astype(np.uint32), tiles=tiles.astype(np.int32), sx=SX, sy=SY, fxy=FXY, classes=cls, G=G, sw=sw, sh=sh)


# class name -> predicate on a tile's classes and the eye size
REACHES = {
    "lds": lambda c, sw, sh: c["lds"],
    "lds_y0_negative": lambda c, sw, sh: c["lds"] and c["box"][1] < 0,
    "lds_past_sh": lambda c, sw, sh: c["lds"] and c["box"][1] + c["box"][3] > sh,
    "lds_x0_negative": lambda c, sw, sh: c["lds"] and c["box"][0] < 0,
    "lds_past_sw": lambda c, sw, sh: c["lds"] and c["box"][0] + c["box"][2] > sw,
    "lds_past_2sw": lambda c, sw, sh: c["lds"] and c["box"][0] + c["box"][2] > 2 * sw,
    "shifted": lambda c, sw, sh: c["lds"] and c["shifted"],
    "gather_area": lambda c, sw, sh: c["area"],
    "lds_exact_cap": lambda c, sw, sh: c["lds"] and c["exact_cap"],  # the box fills the LDS tile to the last pixel
    "lds_height_1023": lambda c, sw, sh: c["lds"] and c["box"][3] == 1023,
    "gather_height_field": lambda c, sw, sh: c["box"][3] > 1023 and c["exact_cap"],  # 4 x 1024: fits the area, not the 10-bit row field
    "gather_limits": lambda c, sw, sh: c["limits"] and not c["area"],
    "gather_only_x_limit": lambda c, sw, sh: c["only_x_limit"],  # (bx0 < -sw and by0 < -sh cannot happen: the first tap is >= -1)
    "gather_only_y_limit": lambda c, sw, sh: c["only_y_limit"],
    "partial_x": lambda c, sw, sh: c["partial_x"],
    "partial_y": lambda c, sw, sh: c["partial_y"],
}


def counts(R):
    return {k: sum(1 for c in R["classes"] if f(c, R["sw"], R["sh"])) for k, f in REACHES.items()}


def accumulators(eye, R, tab):
    """The 16-tap integer sums (BORDER_WRAP in x and y) of one eye's half of the layout BEFORE the rounding shift and the
    saturation, from the restated coordinates and the oracle's weight table: eyeH x ow x 3, int64."""
    sh, sw = eye.shape[:2]
    src = eye[..., :3].astype(np.int64)
    W = tab.astype(np.int64)[R["fxy"]]
    acc = np.zeros(R["sx"].shape + (3,), np.int64)
    for r in range(4):
        for q in range(4):
            acc += src[(R["sy"] + r) % sh, (R["sx"] + q) % sw] * W[..., r * 4 + q, None]
    return acc


def from_accumulators(acc):
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


# ---- eyes -----------------------------------------------------------------------------------------------------------------------
def noise_eyes(seed, slots, sw, sh):
    """per-slot seeded noise, every channel and the ALPHA byte random: alpha must not reach the output"""
    return np.stack([np.random.default_rng([seed, k]).integers(0, 256, (2, sh, sw, 4), dtype=np.uint8) for k in range(slots)])


def checker_eyes(seed, slots, sw, sh):
    """0 / 255 per channel in runs of one and two pixels (the cubic's overshoot), random alpha bytes"""
    out = []
    for k in range(slots):
        rng = np.random.default_rng([seed, k, 7])
        e = (rng.integers(0, 2, (2, sh, sw, 4), dtype=np.uint8) * 255).astype(np.uint8)
        e[..., 3] = rng.integers(0, 256, (2, sh, sw), dtype=np.uint8)
        out.append(e)
    return np.stack(out)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# name: (sw, sh, fw, fh, classes every format must reach). The measured counts per shape are in the docstring of
# tests/test_gpu_cubemap_tiles.py::test_shape; the assertions are ">= 1", an ulp of acosf may move a count by one.
SHAPES = {}


def _shape(group, sw, sh, fw, fh, *reaches):
    SHAPES["%s-%dx%d-%dx%d" % (group, sw, sh, fw, fh)] = (sw, sh, fw, fh, reaches)


def check_case(tiles_tap, plain_tap, O, eyes, fw, fh, fmt, cap, reaches=(), expect_different_from=None, overshoot=False):
    """eyes: S x 2 x sh x sw x 4. tiles_tap(eyes, fw, fh, fmt, cap, fill) -> (out, maps, packed, tiles); plain_tap(eyes, fw, fh,
    fmt, fill) -> (out, maps). Returns the restatement."""
    slots, _, sh, sw = eyes.shape[:4]
    want_maps = np.stack([O.cubemap_warp_map(f, sw, sh, fw, fh) for f in range(6)])
    R = restate(want_maps, sw, sh, fmt, cap)
    n = counts(R)
    print("%dx%d -> %dx%d %s cap %d: %d tiles, %s" % (sw, sh, fw, fh, fmt, cap, len(R["classes"]), n))
    for k in reaches:
        assert n[k] >= 1, "the case does not reach '%s': %s" % (k, n)
    if expect_different_from is not None:
        other = restate(want_maps, sw, sh, fmt, expect_different_from)
        assert (other["tiles"] != R["tiles"]).any() and (other["packed"] != R["packed"]).any(), "the two box sizes give the same records"
    for a in range(slots):
        for b in range(a):
            assert not np.array_equal(eyes[a], eyes[b]) and not np.array_equal(eyes[a, 0], eyes[b, 1])
        assert not np.array_equal(eyes[a, 0], eyes[a, 1])
    tab = O.bicubic_tab_i()
    want = np.stack([O.stereo_cubemap(eyes[k, 0, :, :, :3], eyes[k, 1, :, :, :3], fw, fh, fmt) for k in range(slots)])
    acc = np.stack([np.concatenate([accumulators(eyes[k, e], R, tab) for e in range(2)]) for k in range(slots)])
    same("the numpy restatement of the pixels against the oracle", from_accumulators(acc), want)
    if overshoot:  # (shown with the unclamped restatement that was just pinned to the oracle)
        v = (acc + (1 << 14)) >> 15
        print("unclamped range %d .. %d" % (v.min(), v.max()))
        assert v.min() < 0 and v.max() > 255, "the eyes do not overshoot both ends of sat_u8"
        assert (want == 0).any() and (want == 255).any()
    fill = pick_fill(want, R["packed"], R["tiles"], want_maps)
    out, maps, packed, tiles = tiles_tap(eyes, fw, fh, fmt, cap, fill)
    same("maps", maps.view(np.uint32), want_maps.view(np.uint32))
    Rt = R if np.array_equal(maps.view(np.uint32), want_maps.view(np.uint32)) else restate(maps, sw, sh, fmt, cap)
    same("tile records", tiles, Rt["tiles"])
    same("packed dwords", packed, Rt["packed"])
    for k in range(slots):
        same("pixels of slot %d" % k, out[k], want[k])
    assert not np.all(out == fill, axis=-1).any()
    out2, maps2 = plain_tap(eyes, fw, fh, fmt, fill)
    same("maps of the on-demand mode", maps2.view(np.uint32), want_maps.view(np.uint32))
    same("pixels of the on-demand kernel", out2, want)
    return R


# legal-frame sizes (the smallest frame of the rig is 28 x 14): the pole's boxes in LDS, the y wrap
_shape("legal", 28, 14, 16, 16, "lds", "shifted", "lds_past_sw", "lds_y0_negative", "lds_past_sh")
_shape("legal", 28, 14, 33, 17, "lds", "shifted", "lds_x0_negative", "lds_past_sw", "lds_y0_negative", "lds_past_sh", "partial_x", "partial_y")
_shape("legal", 64, 32, 96, 96, "lds", "shifted", "lds_x0_negative", "lds_past_sw", "lds_y0_negative", "lds_past_sh")
# the documented limits of the box load's wrap: eyes no frame makes
_shape("limits", 12, 6, 20, 20, "lds", "shifted", "lds_past_sw", "lds_y0_negative", "lds_past_sh", "partial_x", "partial_y")
_shape("limits", 3, 3, 20, 12, "lds", "shifted", "lds_x0_negative", "lds_past_sw", "lds_past_2sw", "lds_y0_negative", "lds_past_sh")
_shape("limits", 3, 3, 18, 12, "lds", "lds_past_2sw", "partial_x", "partial_y")
_shape("limits", 2, 2, 16, 16, "lds", "lds_past_2sw", "gather_limits")
_shape("limits", 2, 2, 17, 16, "lds", "lds_past_2sw", "lds_x0_negative", "partial_x")
_shape("limits", 1, 2, 33, 17, "gather_limits", "partial_x", "partial_y")
# the x limit alone (sw = 1 with sh >= 3: at sw = 2 no box passes 3 sw), the y limit alone (sh < 3 with sw >= 2)
_shape("limits", 1, 3, 16, 16, "gather_only_x_limit")
_shape("limits", 1, 5, 17, 16, "gather_only_x_limit", "partial_x")
_shape("limits", 7, 2, 16, 16, "gather_only_y_limit")
# sh = 1: every tile gathers, chosen by the limits
_shape("all_gather_limits", 5, 1, 16, 16, "gather_limits", "gather_only_y_limit")
_shape("all_gather_limits", 5, 1, 18, 16, "gather_limits", "gather_only_y_limit", "partial_x")
# odd eyes (half = sw >> 1) and faces: scalar stores, partial tiles both ways
_shape("odd", 301, 77, 37, 53, "lds", "shifted", "partial_x", "partial_y")
_shape("odd", 301, 77, 36, 53, "lds", "shifted", "partial_x", "partial_y")
# degenerate faces
_shape("degenerate", 28, 14, 1, 17, "partial_x", "partial_y")
_shape("degenerate", 28, 14, 20, 1, "partial_x", "partial_y")
_shape("degenerate", 28, 14, 1, 1, "partial_x", "partial_y")
_shape("degenerate", 28, 14, 4, 1, "partial_x", "partial_y")
# every tile gathers by its area
_shape("all_gather_area", 2048, 1024, 32, 32, "gather_area")
_shape("all_gather_area", 2048, 1024, 30, 32, "gather_area", "partial_x")

# a box of exactly the LDS capacity (64 x 64 of 4096; found by a search over 100 .. 1500 x 8 face sizes: none below 32 x 32 faces)
_shape("exact_cap", 499, 249, 32, 32, "lds_exact_cap", "gather_area")
# the height field: a 4 x 1023 box renders from LDS, 4 x 1024 (area 4096, not above it) gathers; a width above 2047 cannot
# happen below the area limit (height >= 4), so `bw > 2047` has no case
_shape("tall", 1, 2736, 1, 16, "lds_height_1023")
_shape("tall", 1, 2739, 1, 16, "gather_height_field")

# both box sizes: (sw, sh, fw, fh): records differ between 4096 and 2560
BOTH_BOXES = [(700, 350, 40, 40), (700, 350, 42, 40)]

# xcd_tile's grid classes, T = txN * 6 tyN * 2 slots: (sw, sh, fw, fh, slots, T)
GRIDS = {"T12": (28, 14, 16, 16, 1, 12), "T72": (28, 14, 33, 17, 1, 72), "T108": (64, 32, 40, 40, 1, 108)}

# two launches, the second with base 16: (sw, sh, fw, fh, fmt)
SEVENTEEN = [(28, 14, 33, 17, "video"), (12, 6, 20, 12, "photo")]
