"""The ISP's edge cases: the shapes at which isp_kernels.hip takes another branch, and content the smooth scene of
isputil.bayer_frame never holds. Shared by tests/test_gpu_isp_stages.py (the kernels' float intermediates against the oracle's, bit
for bit), tests/test_cpu_isp.py (the oracle on the same cases against the reference's compiled ISP and its committed digests) and
tests/golden/make_isp_edge_golden.py. numpy only, seeded.

A case's w x h is the INPUT's size. Shapes are the smallest at which a branch is taken:
  k_isp_iir_rows_t   64-position tiles (IR_T), 21-row blocks (IR_ROWS); PIPE: the tile that holds the chain's first element
  k_isp_iir_cols_t   32-row batches in two register banks (IC_U), fast path for full batches only; PIPE: the first / last batch
  green vote         32 x 32 tiles (GP_T); the pipeline's over the image extended by 2
  point kernels      256-thread rows; k_pipe_site over the image extended by 8"""
import collections
import json

import numpy as np

import isputil

SOFT, PIPE, PIPE_FAST = 0, 1, 2
Case = collections.namedtuple("Case", "id pipe config w h bpp dm resize content seed stuck counters")

SOFT_SHAPES = [
    (8, 8), (9, 8), (8, 9),                                               # the minimum size
    (63, 20), (64, 21), (65, 22), (128, 42), (129, 43),                   # row tiles and row blocks on, below and above their edges
    (20, 31), (64, 32), (66, 33), (22, 63), (20, 64), (22, 65), (24, 97),  # 1 / 2 / 3 / 4 column batches: both banks' loop tails
    (32, 33), (33, 32),                                                   # vote tiles
    (255, 8), (256, 8), (257, 9),                                         # 256-thread rows
]
PIPE_SHAPES = [s for s in SOFT_SHAPES if min(s) >= 16] + [
    (16, 16), (17, 16), (16, 17),  # the minimum size
    (28, 16), (29, 17),            # w + 4 on the vote tile's edge
    (240, 16), (241, 16),          # w + 16 on the row's edge
    (128, 64),                     # (with 64 x 32 above) a tile / batch that is both the chain's first and last; the first full tile
]                                  # takes the slow loop while the second takes the fast one
BPP8_SOFT_SHAPES = [(8, 8), (65, 22), (66, 33)]  # the tone table and the clamp's maxVal depend on the output depth
BPP8_PIPE_SHAPES = [(16, 16), (65, 22), (66, 33)]
RESIZE = [(131, 71, 2), (203, 157, 4), (205, 163, 8), (18, 17, 2), (64, 64, 8)]  # inputs that are no multiple; 64 / 8 = the minimum
STUCK = [(1, 1, 0.5), (3, 0, 0.4), (2, 1, 2.0)]  # (radius, threshold, darkness)
STUCK_SHAPES = [(8, 8), (9, 11), (64, 21), (65, 33)]
CONFIGS = ("full", "grbg", "empty")
# ... and one more for the content cases: every default but the sharpening, i.e. the default sharpeningSupport (10 / 2048), with which
# the low pass of a full-scale 16-bit image rounds one ulp above 65535 and the soft ISP's clamp to [0, maxVal] changes a value.
# With "full"'s support (0.006) no input reaches that clamp: x (1 - a) + v a never rounds above max(x, v) there.
CONFIG_SHARP_DEFAULT = json.dumps({"CameraIsp": {"sharpening": [0.3, 0.25, 0.35]}})
CONTENT_SIZE = (97, 67)


# ---- content ---------------------------------------------------------------------------------------------------------------------
def _const(v):
    return lambda w, h, rng: np.full((h, w), v, np.uint16)


def _pattern(fn, lo=3000, hi=60000):
    def make(w, h, rng):
        yy, xx = np.mgrid[0:h, 0:w]
        return np.where(fn(xx, yy) & 1, hi, lo).astype(np.uint16)
    return make


def _noise(w, h, rng):
    return rng.integers(0, 65536, (h, w), dtype=np.uint16)


def _hot(w, h, rng):
    raw = (2000 + rng.integers(0, 200, (h, w))).astype(np.uint16)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (h // 3, 1), (1, w // 3), (h - 2, w - 3)):
        raw[y, x] = 65535
    return raw


def _steps(w, h, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    level = (xx >= w // 3).astype(np.int64) + (xx >= (2 * w) // 3) + 2 * (yy >= h // 2)
    return np.array([1500, 30000, 9000, 52000, 65535], np.uint16)[level]


def _mixed(w, h, rng):
    """Flat quarters beside noisy ones: along their borders the 9 x 9 vote crosses its threshold (counts of 39 and 40), and the
    flat parts hold dH == dV."""
    yy, xx = np.mgrid[0:h, 0:w]
    raw = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    flat = ((xx * 4 // max(w, 1)) + (yy * 4 // max(h, 1))) & 1
    return np.where(flat == 1, np.uint16(20000), raw).astype(np.uint16)


def _bright_noise(w, h, rng):
    """Samples within a few counts of full scale, full scale included: the black-level branch that is skipped, the clamps' upper
    ends, the last tone table entry, the output at its maximum."""
    return (65535 - rng.integers(0, 3, (h, w)) * rng.integers(0, 2, (h, w))).astype(np.uint16)


CONTENT = collections.OrderedDict([
    ("zero", _const(0)), ("full_scale", _const(65535)), ("black_level", _const(1210)),  # ("full"'s red black level)
    ("checker1", _pattern(lambda x, y: x + y)), ("checker2", _pattern(lambda x, y: (x >> 1) + (y >> 1))),
    ("stripes_v", _pattern(lambda x, y: x)), ("stripes_h", _pattern(lambda x, y: y)),
    ("noise", _noise), ("hot", _hot), ("steps", _steps),
    ("mixed", _mixed), ("bright_noise", _bright_noise),
])


def raw_of(case):
    if case.content == "scene":
        return isputil.bayer_frame(case.w, case.h, seed=case.seed, pattern="RGGB" if case.config == "full" else "GBRG")
    return CONTENT[case.content](case.w, case.h, np.random.default_rng(case.seed))


def json_of(case):
    if case.stuck:
        return isputil.stuck_pixel_config(*case.stuck)
    return CONFIG_SHARP_DEFAULT if case.config == "sharp_default" else isputil.CONFIGS[case.config]


# The counters (oracle/cvlite.h: COV_ISP_* / COV_PIPE_*, tests/oracle_lib.py's names without their prefix) each content case must
# make non-zero, for configuration "full" at CONTENT_SIZE with the edge-aware demosaic (soft) / the full pipeline. Found on the CPU
# with the oracle; together with "sharp_default"'s full-scale case (isp_iir_clamped) they reach every counter.
SOFT_COUNTERS = {
    "zero": ("flag_tie", "clamp_lo", "lut_first", "core_zero"),
    "full_scale": ("flag_tie", "clamp_hi", "raw_ge_one", "lut_last", "out_at_max"),
    "black_level": ("flag_tie", "clamp_lo", "lut_first"),
    "checker1": ("flag_tie",),
    "checker2": ("flag_tie",),
    "stripes_v": (),
    "stripes_h": (),
    "noise": ("vote_39", "vote_40", "clamp_lo", "clamp_hi", "lut_first", "lut_last", "core_saturated"),
    "hot": ("clamp_hi", "raw_ge_one"),
    "steps": ("flag_tie", "clamp_hi", "raw_ge_one"),
    "mixed": ("flag_tie", "vote_39", "vote_40"),
    "bright_noise": ("raw_ge_one", "clamp_hi", "lut_last", "out_at_max"),
}
PIPE_COUNTERS = {
    "zero": ("flag_tie", "clamp_lo", "lut_first", "core_zero"),
    "full_scale": ("flag_tie", "clamp_hi", "lut_last", "out_at_max"),
    "black_level": ("flag_tie", "clamp_lo", "lut_first"),
    "checker1": ("flag_tie",),
    "checker2": ("flag_tie",),
    "stripes_v": (),
    "stripes_h": (),
    "noise": ("vote_39", "vote_40", "clamp_lo", "clamp_hi", "lut_first", "lut_last", "core_saturated"),
    "hot": ("clamp_hi",),
    "steps": ("flag_tie", "clamp_hi"),
    "mixed": ("flag_tie", "vote_39", "vote_40"),
    "bright_noise": ("clamp_hi", "lut_last", "out_at_max"),
}


# ---- the case lists ---------------------------------------------------------------------------------------------------------------
def _mk(pipe, config, w, h, bpp, dm, resize=1, content="scene", stuck=None, counters=()):
    kind = ("soft-dm%d" % dm, "pipe", "fast")[pipe]
    cid = "%s-%s-%dx%d-bpp%d" % (kind, config, w, h, bpp)
    if resize != 1:
        cid += "-r%d" % resize
    if stuck:
        cid += "-stuck%d_%d_%g" % stuck
    if content != "scene":
        cid += "-" + content
    return Case(cid, pipe, config, w, h, bpp, dm, resize, content, 1000 * w + h, stuck, tuple(counters))


def _order(shapes):
    """Small, large, small again ...: consecutive frames of one object differ in size, so its buffers grow and are reused."""
    s = sorted(shapes, key=lambda wh: wh[0] * wh[1])
    lo, hi = s[:len(s) // 2], s[len(s) // 2:][::-1]
    out = []
    for k in range(max(len(lo), len(hi))):
        out += lo[k:k + 1] + hi[k:k + 1]
    return out


def groups():
    """{group id: [Case, ...]}: the cases one ISP object develops one after the other (one configuration, depth and pipeline)."""
    g = collections.OrderedDict()
    for config in CONFIGS:
        for dm in (0, 2):
            key = "soft-dm%d-%s" % (dm, config)
            g[key + "-bpp16-shapes"] = [_mk(SOFT, config, w, h, 16, dm) for w, h in _order(SOFT_SHAPES)]
            g[key + "-bpp8-shapes"] = [_mk(SOFT, config, w, h, 8, dm) for w, h in BPP8_SOFT_SHAPES]
            for r in (2, 4, 8):
                g[key + "-bpp16-resize%d" % r] = [_mk(SOFT, config, w, h, 16, dm, resize=rr) for w, h, rr in RESIZE if rr == r]
            g[key + "-bpp16-content"] = [
                _mk(SOFT, config, w, h, 16, dm, content=c,
                    counters=SOFT_COUNTERS[c] if (config, dm, (w, h)) == ("full", 2, CONTENT_SIZE) else ())
                for c in CONTENT for w, h in (CONTENT_SIZE, (8, 8))]
        for pipe in (PIPE, PIPE_FAST):
            key = "%s-%s" % ("pipe" if pipe == PIPE else "fast", config)
            g[key + "-bpp16-shapes"] = [_mk(pipe, config, w, h, 16, 2) for w, h in _order(PIPE_SHAPES)]
            g[key + "-bpp8-shapes"] = [_mk(pipe, config, w, h, 8, 2) for w, h in BPP8_PIPE_SHAPES]
            g[key + "-bpp16-content"] = [
                _mk(pipe, config, w, h, 16, 2, content=c,
                    counters=PIPE_COUNTERS[c] if (config, pipe, (w, h)) == ("full", PIPE, CONTENT_SIZE) else ())
                for c in CONTENT for w, h in (CONTENT_SIZE, (16, 16))]
    g["soft-dm2-sharp_default-bpp16-content"] = [
        _mk(SOFT, "sharp_default", w, h, 16, 2, content=c,
            counters=("iir_clamped",) if (c, (w, h)) == ("full_scale", CONTENT_SIZE) else ())
        for c in CONTENT for w, h in (CONTENT_SIZE, (8, 8))]
    for stuck in STUCK:  # (the configuration is "full" with the pass switched on; a dark patch with hot sites gives it work)
        g["soft-dm2-stuck%d_%d_%g" % stuck] = [_mk(SOFT, "full", w, h, 16, 2, content="hot", stuck=stuck) for w, h in STUCK_SHAPES]
    return g


def all_cases():
    return [c for cases in groups().values() for c in cases]


# ---- final outputs: the oracle, the reference's compiled ISP, digests -------------------------------------------------------------------
def oracle_output(O, case):
    cfg = O.isp_config_from_json(json_of(case), case.bpp, case.dm, case.resize)
    if case.pipe:
        return O.isp_pipe_run(cfg, raw_of(case), fast=case.pipe == PIPE_FAST)
    return O.isp_run(cfg, raw_of(case))


def reference_output(O, case):
    """The case through the reference's own sources (oracle/_ref: CameraIsp.h compiled, CameraIspGen.cpp executed)."""
    if case.pipe:
        return O.ref_isp_pipe_run(json_of(case), raw_of(case), case.bpp, case.pipe == PIPE_FAST)
    return O.ref_isp_run(json_of(case), raw_of(case), case.bpp, case.dm, case.resize)


def digest(a):
    import hashlib
    return hashlib.sha256(repr((a.shape, str(a.dtype))).encode() + np.ascontiguousarray(a).tobytes()).hexdigest()[:24]
