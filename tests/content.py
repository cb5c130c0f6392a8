"""Edge-content generators for the GPU parity tests (tests/test_gpu_content.py): inputs the band-limited noise of
surround360_amd/synth.py never produces — exact ties, alpha exactly at PixFlow's update threshold, tiny and huge
previous-frame flows, saturating remaps, signed zeros in the median, holes that end on the sweeps' band edges.

numpy only, every generator seeded. Flow pairs are (I0, I1) BGRA uint8 H x W x 4; world textures are (2h x h BGR uint8,
depth in cm) for surround360_amd.synth.rig_frame(world=...). bench.py draws from synth alone, so nothing here can move
its inputs."""
import numpy as np

OPAQUE = 255


def bgra(bgr, alpha=OPAQUE):
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[:2]
    a = np.broadcast_to(np.asarray(alpha, np.uint8), (h, w))
    return np.ascontiguousarray(np.dstack([bgr, a]))


def grey(v):
    v = np.asarray(v, np.uint8)
    return np.repeat(v[..., None], 3, axis=-1)


# ---- BGRA flow pairs --------------------------------------------------------------------------------------------------
def constant_pair(w, h, bgr=(90, 140, 200)):
    """I0 = I1 = one colour: every data term is zero."""
    i0 = bgra(np.broadcast_to(np.asarray(bgr, np.uint8), (h, w, 3)))
    return i0, i0.copy()


def level_pair(w, h, v):
    """All-v images (0: black, 255: white). With v = 0 the intensity ratio of pixflow_search_20 divides by zero."""
    i0 = bgra(grey(np.full((h, w), v, np.uint8)))
    return i0, i0.copy()


def step_pair(w, h, lo, hi, disp=3):
    """A vertical two-level step edge at w/2 in I0, at w/2 - disp in I1 (0 | 255 or 60 | 61)."""
    x = np.arange(w)
    i0 = grey(np.where(x[None, :] < w // 2, lo, hi).repeat(h, axis=0).astype(np.uint8))
    i1 = grey(np.where(x[None, :] < w // 2 - disp, lo, hi).repeat(h, axis=0).astype(np.uint8))
    return bgra(i0), bgra(i1)


def checker(w, h, cell=8, lo=0, hi=255, x0=0, y0=0):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((((xx + x0) // cell) + ((yy + y0) // cell)) % 2 == 0, lo, hi).astype(np.uint8)


def checker_pair(w, h, cell=8):
    """An 8-px checkerboard; I1 is I0 shifted by one whole period (2 cells), so every period is a perfect match."""
    return bgra(grey(checker(w, h, cell))), bgra(grey(checker(w, h, cell, x0=2 * cell)))


def ramp_pair(w, h, axis, disp=2):
    """1-LSB ramps: neighbouring pixels differ by one grey level along `axis` (1: horizontal, 0: vertical)."""
    n = w if axis == 1 else h
    v = (40 + np.arange(n + disp) % 176).astype(np.uint8)
    if axis == 1:
        i0 = np.broadcast_to(v[None, :w], (h, w))
        i1 = np.broadcast_to(v[None, disp:disp + w], (h, w))
    else:
        i0 = np.broadcast_to(v[:h, None], (h, w))
        i1 = np.broadcast_to(v[disp:disp + h, None], (h, w))
    return bgra(grey(i0)), bgra(grey(i1))


PALETTE = np.array([[0, 0, 0], [255, 255, 255], [0, 0, 255], [255, 128, 0], [30, 200, 30], [0, 0, 0], [255, 255, 255]],
                   np.uint8)


def cartoon_labels(w, h, seed, n=9):
    """Voronoi regions of n seeded sites (integer label map)."""
    rng = np.random.default_rng(seed)
    sx, sy = rng.integers(0, w, n), rng.integers(0, h, n)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (xx[None] - sx[:, None, None]) ** 2 + (yy[None] - sy[:, None, None]) ** 2
    return np.argmin(d, axis=0)


def cartoon_pair(w, h, seed=1):
    """Piecewise-constant regions whose colours repeat exactly (a palette of 7 with duplicates); I1 = I0 displaced by
    an integer disparity per region (0..6 px to the left)."""
    rng = np.random.default_rng(seed + 100)
    lab = cartoon_labels(w + 8, h, seed)
    col = PALETTE[rng.integers(0, len(PALETTE), lab.max() + 1)]
    disp = rng.integers(0, 7, lab.max() + 1)
    img = col[lab]
    i0 = img[:, :w]
    xx = np.arange(w)[None, :] + disp[lab[:, :w]]
    i1 = img[np.arange(h)[:, None], np.clip(xx, 0, w + 7)]
    return bgra(i0), bgra(i1)


# ---- alpha patterns (applied to a pair; both images unless told otherwise) -------------------------------------------------
def with_alpha(pair, a0, a1=None):
    i0, i1 = (np.ascontiguousarray(p.copy()) for p in pair)
    i0[..., 3] = a0
    i1[..., 3] = a0 if a1 is None else a1
    return i0, i1


def alpha_stripes(w, h, period):
    """Stripes of alpha 229 / 230 (the two u8 levels around 0.9 * 255 = 229.5) across both rows and columns, `period`
    px wide at the finest pyramid level (2 * period input px: the entry downscale halves the image, and 1-px input
    stripes come out of it uniform). The pyramid's linear resizes mix them into values of exactly 0.9f."""
    p = 2 * period
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // p) + (xx // p)) % 2 == 0, 229, 230).astype(np.uint8)


def alpha_hole_rows(w, h, last_row):
    """Alpha 0 on input rows [2, 2 * (last_row + 1)) over the middle half of the columns: the hole's last row at the
    finest pyramid level (after the x0.5 entry downscale) is `last_row`, on or next to the sweeps' band edges (8 rows
    per workgroup in k_sweep_lock, 16 / 20 rows per wave in k_sweep_quad)."""
    a = np.full((h, w), 255, np.uint8)
    a[2:2 * (last_row + 1), w // 4: 3 * w // 4] = 0
    return a


def alpha_hole_cols(w, h, last_col):
    """Alpha 0 on input columns [w // 2, 2 * (last_col + 1)) of the middle rows: a hole whose last column at the finest
    pyramid level is `last_col` (the level's last or last but one column)."""
    a = np.full((h, w), 255, np.uint8)
    a[h // 4: 3 * h // 4, w // 2: 2 * (last_col + 1)] = 0
    return a


# ---- previous-frame state ---------------------------------------------------------------------------------------------
def tiny_flow(w, h, seed=5):
    """A prev_flow whose entries cover every binade from 2^-149 to 2^-60 in both signs, plus +0 and -0, in 4 x 4
    blocks (so that the x0.5 downscale keeps most of them), in a seeded order."""
    rng = np.random.default_rng(seed)
    mags = [np.float32(2.0) ** e for e in range(-149, -59)]
    vals = np.array([s * m * np.float32(1.0 + 0.5 * rng.random()) if e > -149 else s * m
                     for e, m in zip(range(-149, -59), mags) for s in (1.0, -1.0)] + [0.0, -0.0], np.float32)
    bh, bw = (h + 3) // 4, (w + 3) // 4
    blocks = vals[rng.integers(0, len(vals), (bh, bw, 2))]
    blocks.reshape(-1)[:len(vals)] = vals  # every value at least once
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:h, :w])


def huge_flow(w, h, seed=6):
    """A prev_flow of 60 ... 200 px in either sign (x) and +-(60 ... 120) px (y), smooth in 16 x 16 blocks."""
    rng = np.random.default_rng(seed)
    bh, bw = (h + 15) // 16, (w + 15) // 16
    mag = np.stack([rng.uniform(60, 200, (bh, bw)), rng.uniform(60, 120, (bh, bw))], -1)
    sgn = rng.choice(np.array([-1.0, 1.0]), (bh, bw, 2))
    f = (mag * sgn).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(f, 16, axis=0), 16, axis=1)[:h, :w])


def half_static_prev(i1, seed=7):
    """prev_i1 equal to i1 on the left half (motion 0: adjustFlowTowardPrevious hands the previous flow to the next
    level as it is) and different on the right half (motion > 0)."""
    rng = np.random.default_rng(seed)
    p = i1.copy()
    w = i1.shape[1]
    p[:, w // 2:, :3] = rng.integers(0, 256, p[:, w // 2:, :3].shape, dtype=np.uint8)
    return p


def motion_sums_pair(block=8):
    """(i1, prev_i1) of 28 x 28 constant blocks of `block` px whose per-pixel channel-difference sums
    |b1 - b0| + |g1 - g0| + |r1 - r0| take every value 0 ... 765 (block k has sum k; signs alternate), with a
    background of sum 0. Blocks of 8 input px keep a 2 x 2 core of the x0.5 cubic downscale exactly at their values."""
    n = 28
    s = np.arange(n * n) % 766
    hi = np.stack([np.minimum(s, 255), np.clip(s - 255, 0, 255), np.clip(s - 510, 0, 255)], -1).astype(np.int32)
    lo = np.zeros_like(hi)
    swap = (np.arange(n * n) % 2) == 1
    a = np.where(swap[:, None], lo, hi).astype(np.uint8).reshape(n, n, 3)
    b = np.where(swap[:, None], hi, lo).astype(np.uint8).reshape(n, n, 3)
    up = lambda im: np.repeat(np.repeat(im, block, axis=0), block, axis=1)  # noqa: E731
    return bgra(up(a)), bgra(up(b))


# ---- world textures (2h x h BGR + depth in cm) for synth.rig_frame(world=...) -------------------------------------------
FAR = 1.0e6


def _near_boxes(h, seed):
    """A depth map: far field with a few near boxes (200 / 500 cm), so that the side flows see parallax."""
    rng = np.random.default_rng(seed + 11)
    depth = np.full((h, 2 * h), FAR, np.float32)
    for _ in range(8):
        y0, x0 = rng.integers(h // 4, 3 * h // 4), rng.integers(0, 2 * h - h // 4)
        depth[y0: y0 + h // 10, x0: x0 + h // 6] = rng.choice([200.0, 500.0])
    return depth


def world_constant(h, v=128):
    return np.full((h, 2 * h, 3), v, np.uint8), np.full((h, 2 * h), FAR, np.float32)


def world_cartoon(h, seed=3):
    """Piecewise-constant regions of 0 / 255 colours (hard edges; sample with nearest=True to keep them hard)."""
    rng = np.random.default_rng(seed)
    lab = cartoon_labels(2 * h, h, seed, n=40)
    col = np.array([[0, 0, 0], [255, 255, 255], [0, 0, 255], [255, 0, 0], [0, 255, 0], [255, 255, 0]], np.uint8)
    tex = col[rng.integers(0, len(col), lab.max() + 1)][lab]
    return np.ascontiguousarray(tex), _near_boxes(h, seed)


def world_checker(h, seed=4):
    return grey(checker(2 * h, h, 8)), _near_boxes(h, seed)


def world_black_white_spots(h, seed=5):
    """Black, with a few saturated white discs."""
    rng = np.random.default_rng(seed)
    tex = np.zeros((h, 2 * h, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:2 * h]
    for _ in range(12):
        cy, cx, r = rng.integers(h // 5, 4 * h // 5), rng.integers(0, 2 * h), rng.integers(h // 40, h // 12)
        tex[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 255
    return tex, _near_boxes(h, seed)


def world_half_changed(world, seed=9):
    """The same world with the texture of its right half (azimuth) replaced: a chained frame where half the rig moves."""
    tex, depth = world
    rng = np.random.default_rng(seed)
    t = tex.copy()
    h = t.shape[0]
    t[:, h:] = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8) ^ t[:, h:]
    return t, depth
