"""The cases of tests/test_gpu_flow_level.py: ONE pyramid level of PixFlow on the device (the library's test tap
s360_debug_flow_level, which runs the body of FlowEngine::compute's level loop) against the oracle's level with its intermediates
(oracle/pixflow.h: LevelStages), stage by stage and bit for bit, so that a failure names the first stage that differs: gradients,
initial flow (search init), update mask, blurred flow (the sweeps' records decoded), row flags, forward sweep, first median,
backward sweep, second median, diffusion, final flow (adjusted toward the previous one if there is one).

A level's inputs are made here and handed to the tap directly: sizes no pyramid produces, a different alpha plane for every image,
flows i0 -> i1 that share gradient planes in both roles, initial flows that no bicubic upscale gives.

numpy only, every generator seeded; the oracle's result of a case is computed once per process and shared (EXPECTED)."""
import numpy as np

# flows of the shape, content and temporal cases: B = 3 over N = 4 images; planes 0 and 1 serve as I0 and as I1
N_IMAGES = 4
I0 = (0, 1, 2)
I1 = (1, 0, 3)

# (w, h, why): level sizes
SHAPES = [
    (2, 2, "the smallest the engine accepts"),
    (3, 2, "the smallest, odd width"),
    (7, 5, "narrower than the blur's radius 7: BORDER_REFLECT_101 reflects more than once"),
    (15, 15, "one band, one 16-step chunk, one short"),
    (16, 16, "one band, one 16-step chunk"),
    (17, 33, "one more than a chunk; three 16-row bands"),
    (31, 20, "exactly one 20-row band, no interior chunk"),
    (32, 21, "one 32x32 blur tile; a 20-row band plus one row"),
    (33, 33, "one 32x32 blur tile plus one"),
    (48, 40, "two 20-row bands, five 8-row ones"),
    (63, 17, "the widest level of the narrow median"),
    (64, 16, "the narrowest level of the row-8 median; one 64x16 gradient tile"),
    (65, 41, "one gradient tile and one more"),
    (130, 21, "three gradient tiles wide"),
    (200, 70, "several tiles of every kernel"),
    (101, 78, "odd everywhere"),
]
SHAPE_IDS = ["%dx%d" % s[:2] for s in SHAPES]
MEDIAN_SHAPES = [s for s in SHAPES if s[0] >= 64]  # levels that take the row-8 median (S360_MEDIAN_BX)
# (initial flow kind or None = zeros + search, algorithm, hint)
SHAPE_INITS = [("noise", "pixflow_low", "UNKNOWN"), (None, "pixflow_search_20", "LEFT")]
MODES = ("latency", "throughput")

# the search of pixflow_search_20 with the other three hints (the shape cases run LEFT): its box changes side and orientation
SEARCH_HINTS = ("RIGHT", "DOWN", "UP")
SEARCH_SIZES = [(7, 5), (33, 33), (65, 41)]

CONTENT_SIZES = [(48, 40), (101, 78)]
# (name, initial flow, alpha): every initial flow and every alpha layout at least once
CONTENT = [
    ("zero_opaque", "zero", "opaque"),
    ("smooth_opaque", "smooth", "opaque"),
    ("outliers_opaque", "outliers", "opaque"),
    ("tiny_opaque", "tiny", "opaque"),
    ("noise_at_threshold", "noise", "at_threshold"),
    ("noise_hole_to_row_15", "noise", "hole_15"),
    ("smooth_hole_to_row_16", "smooth", "hole_16"),
    ("outliers_hole_to_row_19", "outliers", "hole_19"),
    ("noise_hole_to_row_20", "noise", "hole_20"),
    ("zero_hole_to_row_39", "zero", "hole_39"),
    ("tiny_hole_to_row_40", "tiny", "hole_40"),
    ("noise_first_band_transparent", "noise", "first_band"),
    ("smooth_last_band_transparent", "smooth", "last_band"),
    ("outliers_all_transparent", "outliers", "all_transparent"),
    ("noise_hole_in_i1_only", "noise", "hole_i1"),
]
CONTENT_IDS = [c[0] for c in CONTENT]

TEMPORAL_SIZES = [(33, 33), (65, 41), (101, 78)]
PREV_SCALES = [1.0, float(np.float32(41) / np.float32(50))]  # level 0's factor, and float(rows of a level) / float(rows of level 0)

# production dispatch (hardware only): (w, h, B) with B * ceil(h / 16) >= 4096, the library's own rule for three lanes per pixel
DISPATCH = [(48, 40, 1400), (101, 78, 820)]
DISPATCH_IMAGES = 8
DISPATCH_FLOWS = [(0, 1), (3, 2), (4, 5), (7, 6)]  # four distinct flows, cycled over the batch

FLOW_STAGES = ("sweep_forward", "median_first", "sweep_backward", "median_second", "diffused", "final_flow")
ALL_ONES = 0xFFFFFFFF
T = np.float32(0.9)  # kUpdateAlphaThreshold


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _texture(rng, w, h):
    t = rng.random((h + 2, w + 2 + 8)).astype(np.float32)
    t = (t[:-2, :-2] + t[1:-1, 1:-1] + t[2:, 2:] + t[:-2, 2:] + t[2:, :-2]) / np.float32(5)
    return np.float32(0.1) + np.float32(0.8) * t


def gray_planes(w, h, n=N_IMAGES, seed=0):
    """n grey planes in [0.1, 0.9]: odd planes are their even neighbour seen 2 px further left plus a little noise."""
    rng = np.random.default_rng(7919 * h + w + 101 * seed)
    out = np.empty((n, h, w), np.float32)
    for k in range(0, n, 2):
        t = _texture(rng, w, h)
        out[k] = t[:, 4:4 + w]
        if k + 1 < n:
            out[k + 1] = t[:, 6:6 + w] + (rng.random((h, w)).astype(np.float32) - np.float32(0.5)) * np.float32(0.02)
    return np.ascontiguousarray(out)


def initial_flow(kind, w, h, b=len(I0), seed=0):
    rng = np.random.default_rng(104729 * h + w + 13 * seed + len(kind))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = np.zeros((b, h, w, 2), np.float32)
    if kind == "zero":
        return f
    if kind == "smooth":
        for k in range(b):
            f[k, ..., 0] = np.float32(-2.0 - k) + np.float32(0.03) * xx + np.sin(yy / np.float32(9.0)).astype(np.float32)
            f[k, ..., 1] = np.float32(0.5 * k) - np.float32(0.02) * yy
        return f
    if kind in ("noise", "outliers"):
        f[:] = rng.uniform(-3.0, 3.0, f.shape).astype(np.float32)
        if kind == "outliers":  # 1 in 80: taps far outside the sweeps' LDS window, clamped at the borders
            hit = rng.random((b, h, w)) < 1.0 / 80
            hit[:, h // 2, w // 2] = True
            f[hit] = (rng.choice(np.array([-40.0, 40.0], np.float32), (int(hit.sum()), 2))
                      + rng.uniform(-1, 1, (int(hit.sum()), 2)).astype(np.float32))
        return f
    if kind == "tiny":  # 1e-16 beside zeros: squares below 2^-96, where the sweeps' fast division re-runs the IEEE expansion
        hit = rng.random(f.shape) < 0.25
        f[hit] = rng.choice(np.array([1e-16, -1e-16], np.float32), int(hit.sum()))
        return f
    raise ValueError(kind)


def shape_alpha(w, h, n=N_IMAGES):
    """The shape cases' alpha: a different plane per image, a block of 0.5 and sprinkled values around the threshold; never below
    0.25, so that no patch of the search has alpha sum 0."""
    rng = np.random.default_rng(15485863 + 31 * h + w)
    a = np.ones((n, h, w), np.float32)
    for k in range(n):
        y0, x0 = (h // 3 + k) % h, (w // 4 + 2 * k) % w
        a[k, y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 3)] = 0.5
        r = rng.random((h, w))
        a[k][r < 0.04] = np.float32(0.25)
        a[k][(r >= 0.04) & (r < 0.07)] = T
        a[k][(r >= 0.07) & (r < 0.10)] = np.nextafter(T, np.float32(1))
    return a


def content_alpha(kind, w, h, n=N_IMAGES):
    """A different alpha plane for every image. hole_R: transparent rows ending at row R (clipped to the level) — full width in
    the even images, the middle columns in the odd ones, one row more per image index."""
    rng = np.random.default_rng(32452843 + 31 * h + w + len(kind))
    a = np.ones((n, h, w), np.float32)
    for k in range(n):
        a[k][rng.random((h, w)) < 0.02] = np.float32(0.95) + np.float32(0.01) * k  # (above the threshold: the mask stays the layout's)
    if kind == "opaque":
        return a
    if kind == "at_threshold":
        for k in range(n):
            r = rng.random((h, w))
            a[k][r < 0.2] = T
            a[k][(r >= 0.2) & (r < 0.4)] = np.nextafter(T, np.float32(1))
        return a
    if kind.startswith("hole_") and kind != "hole_i1":
        last = min(int(kind[5:]), h - 1)
        for k in range(n):
            cols = slice(0, w) if k % 2 == 0 else slice(w // 4 + k, 3 * w // 4 - k)
            a[k, max(0, last - 5 - k):last + 1, cols] = 0
        return a
    if kind == "first_band":
        for k in range(n):
            a[k, :20, :] = np.float32(0.1) * k
        return a
    if kind == "last_band":
        for k in range(n):
            a[k, h - 20:, :] = np.float32(0.1) * k
        return a
    if kind == "all_transparent":
        for k in range(n):
            a[k] = np.float32(0.2) * k
        return a
    if kind == "hole_i1":  # images 1 and 3: I1 of flows 0 and 2, I0 of flow 1
        for k in (1, 3):
            a[k, h // 4 + k:h // 2 + k, w // 3 - k:2 * w // 3] = 0
        return a
    raise ValueError(kind)


def prev_state(w, h, n=N_IMAGES, b=len(I0)):
    """(previous flow b x h x w x 2, motion n x h x w): motion exactly 0 on the left third, exactly 1 on the right third, between
    them values between (multiples of 1 / 765, as the reference's motion has them)."""
    rng = np.random.default_rng(49979687 + 31 * h + w)
    prev = rng.uniform(-4.0, 4.0, (b, h, w, 2)).astype(np.float32)
    mo = (rng.integers(0, 766, (n, h, w)) / np.float32(255.0 * 3.0)).astype(np.float32)
    mo[:, :, :w // 3] = 0
    mo[:, :, w - w // 3:] = 1
    return prev, mo


# ---- the oracle's side ------------------------------------------------------------------------------------------------------
EXPECTED = {}  # key -> (stages per flow, coverage counters): computed once, shared by the tests of both sweep modes, never changed


def save_expected(path):
    import pickle
    with open(path, "wb") as f:
        pickle.dump(EXPECTED, f)


def load_expected(path):
    """(a child process of the forced-variant tests takes its parent's oracle results instead of computing them again)"""
    import pickle
    with open(path, "rb") as f:
        EXPECTED.update(pickle.load(f))


def expected(oracle, key, gray, alpha, i0, i1, init, alg, hint, prev=None, motion=None, prev_scale=1.0):
    if key not in EXPECTED:
        with oracle.coverage() as cov:
            flows = [oracle.pixflow_level_stages(
                gray[i0[b]], gray[i1[b]], alpha[i0[b]], alpha[i1[b]], None if init is None else init[b], hint,
                alg == "pixflow_search_20", None if prev is None else prev[b], None if motion is None else motion[i1[b]], prev_scale)
                for b in range(len(i0))]
        EXPECTED[key] = (flows, cov.counts)
    return EXPECTED[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differs(tag, stage, b, got, want, where=None):
    bad = bits(got) != bits(want)
    if where is not None:
        bad &= where
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: first differing stage: %s, flow %d: %d of %d values differ, first at %s (got %r, oracle %r)" % (
            tag, stage, b, int(bad.sum()), bad.size, at, float(got[at]), float(want[at])))


def compare(tag, got, info, want, i0, i1, has_prev=False):
    """Stage by stage in launch order; the first stage that differs fails. `got` may hold a subset of the stages."""
    assert info["sweep_error"] == 0, "%s: sweep error word %#x" % (tag, info["sweep_error"])
    B = len(i0)
    if "gradients" in got:
        for b in range(B):
            _differs(tag, "gradients (I0 = image %d).x" % i0[b], b, got["gradients"][i0[b], ..., 0], want[b]["I0x"])
            _differs(tag, "gradients (I0 = image %d).y" % i0[b], b, got["gradients"][i0[b], ..., 1], want[b]["I0y"])
            _differs(tag, "gradients (I1 = image %d).x" % i1[b], b, got["gradients"][i1[b], ..., 0], want[b]["I1x"])
            _differs(tag, "gradients (I1 = image %d).y" % i1[b], b, got["gradients"][i1[b], ..., 1], want[b]["I1y"])
    if "initial_flow" in got:
        for b in range(B):
            _differs(tag, "initial_flow", b, got["initial_flow"][b], want[b]["initial_flow"])
    if "updated" in got:
        for b in range(B):
            bad = got["updated"][b] != want[b]["updated"]
            assert not bad.any(), "%s: first differing stage: updated mask, flow %d: %d pixels, first at %s" % (
                tag, b, int(bad.sum()), tuple(int(v) for v in np.argwhere(bad)[0]))
    if "blurred_flow" in got:
        for b in range(B):  # both record formats mark a pixel that is not updated with NaN: compared where the mask is set
            _differs(tag, "blurred_flow", b, got["blurred_flow"][b], want[b]["blurred_flow"],
                     np.repeat(want[b]["updated"][..., None] != 0, 2, axis=-1))
    if "row_flags" in got:
        for b in range(B):
            flags = np.where(want[b]["updated"].any(axis=1), 0, ALL_ONES).astype(np.uint32)
            bad = got["row_flags"][b] != flags
            assert not bad.any(), "%s: first differing stage: row_flags, flow %d: rows %s" % (tag, b, np.flatnonzero(bad)[:8])
    for stage in FLOW_STAGES:
        if stage in got and not (stage == "diffused" and has_prev):
            for b in range(B):
                _differs(tag, stage, b, got[stage][b], want[b][stage])


# ---- cases ------------------------------------------------------------------------------------------------------------------
def check_info(tag, info, mode, w, forced=None):
    forced = forced or {}
    if mode == "latency":
        assert info["lanes_per_pixel"] == 0, (tag, info)
    else:
        assert info["lanes_per_pixel"] == int(forced.get("S360_QUAD_LPP", 4)), (tag, info)
    assert info["bands"] >= 1 and info["waves"] >= 1, (tag, info)
    if w < 64:
        assert info["median_tile"] == 0, (tag, info)
    elif "S360_MEDIAN_BX" in forced:
        assert info["median_tile"] == int(forced["S360_MEDIAN_BX"]), (tag, info)
    else:
        assert info["median_tile"] in (32, 16, 8, 4), (tag, info)
    if forced.get("S360_SWEEP_DIV") == "ieee":
        assert info["fast_division"] == 0, (tag, info)


def check_shape(ctx, oracle, mode, w, h, forced=None):
    ctx.set_sweep_mode(mode)
    gray, alpha = gray_planes(w, h), shape_alpha(w, h)
    for kind, alg, hint in SHAPE_INITS:
        tag = "%dx%d %s %s init=%s" % (w, h, mode, alg, kind)
        init = None if kind is None else initial_flow(kind, w, h)
        want, _ = expected(oracle, ("shape", w, h, kind), gray, alpha, I0, I1, init, alg, hint)
        got, info = ctx.debug_flow_level(gray, alpha, I0, I1, init, alg, hint)
        compare(tag, got, info, want, I0, I1)
        check_info(tag, info, mode, w, forced)


def check_search_hint(ctx, oracle, mode, w, h, hint):
    ctx.set_sweep_mode(mode)
    gray, alpha = gray_planes(w, h), shape_alpha(w, h)
    want, _ = expected(oracle, ("search", w, h, hint), gray, alpha, I0, I1, None, "pixflow_search_20", hint)
    assert any(f["initial_flow"].any() for f in want), "the search moved no pixel"
    got, info = ctx.debug_flow_level(gray, alpha, I0, I1, None, "pixflow_search_20", hint)
    compare("%dx%d %s search %s" % (w, h, mode, hint), got, info, want, I0, I1)


def reaches_its_edge(name, alpha_kind, init_kind, want, counts, w, h, alpha):
    """The oracle's own mask and counters say that the case is what its name says."""
    upd = [f["updated"] != 0 for f in want]
    if alpha_kind == "opaque":
        assert all(u.all() for u in upd), name
    if init_kind == "tiny":
        assert counts["tiny_operand"] > 0, (name, counts)
    if alpha_kind == "at_threshold":
        assert counts["alpha_at_threshold"] > 0 and all(u.any() and not u.all() for u in upd), (name, counts)
    if alpha_kind.startswith("hole_") and alpha_kind != "hole_i1":
        last = min(int(alpha_kind[5:]), h - 1)
        for u in upd:  # rows with no updated pixel end at `last`: a row flag set beside one that is not
            assert not u[last].any() and not u[last - 5].any() and u[last - 9].any(), (name, last)
            assert last == h - 1 or u[last + 1].any(), (name, last)
    if alpha_kind == "first_band":
        assert all(not u[:20].any() and u[20].any() for u in upd), name  # a 16-row and a 20-row band with no updated pixel
    if alpha_kind == "last_band":
        assert all(not u[h - 20:].any() and u[h - 21].any() for u in upd), name
    if alpha_kind == "all_transparent":
        assert not any(u.any() for u in upd), name
    if alpha_kind == "hole_i1":
        assert (alpha[I0[0]] > T).all() and not (alpha[I1[0]] > T).all() and not upd[0].all() and upd[0].any(axis=1).all(), name


def check_content(ctx, oracle, mode, w, h, name, init_kind, alpha_kind):
    ctx.set_sweep_mode(mode)
    gray, alpha = gray_planes(w, h, seed=1), content_alpha(alpha_kind, w, h)
    assert len({alpha[k].tobytes() for k in range(N_IMAGES)}) == N_IMAGES, "every image its own alpha plane"
    init = initial_flow(init_kind, w, h, seed=1)
    want, counts = expected(oracle, ("content", w, h, name), gray, alpha, I0, I1, init, "pixflow_low", "UNKNOWN")
    reaches_its_edge(name, alpha_kind, init_kind, want, counts, w, h, alpha)
    got, info = ctx.debug_flow_level(gray, alpha, I0, I1, init, "pixflow_low", "UNKNOWN")
    compare("%dx%d %s %s" % (w, h, mode, name), got, info, want, I0, I1)


def check_temporal(ctx, oracle, mode, w, h, prev_scale):
    ctx.set_sweep_mode(mode)
    gray, alpha = gray_planes(w, h, seed=2), shape_alpha(w, h)
    init = initial_flow("noise", w, h, seed=2)
    prev, motion = prev_state(w, h)
    assert (motion == 0).any() and (motion == 1).any() and ((motion > 0) & (motion < 1)).any()
    want, _ = expected(oracle, ("temporal", w, h, prev_scale), gray, alpha, I0, I1, init, "pixflow_low", "UNKNOWN", prev, motion,
                       prev_scale)
    got, info = ctx.debug_flow_level(gray, alpha, I0, I1, init, "pixflow_low", "UNKNOWN", prev, motion, prev_scale)
    assert "diffused" not in got
    compare("%dx%d %s previous state x%r" % (w, h, mode, prev_scale), got, info, want, I0, I1, has_prev=True)


def check_dispatch(ctx, oracle, w, h, B):
    """Throughput mode with as many flows as a batch of frame slots has: three lanes per pixel, more band tickets than
    persistent waves. Every flow of the batch against the oracle's flow for its pair."""
    assert B * ((h + 15) // 16) >= 4096
    ctx.set_sweep_mode("throughput")
    gray = gray_planes(w, h, n=DISPATCH_IMAGES, seed=3)
    alpha = np.concatenate([shape_alpha(w, h), content_alpha("hole_20", w, h)])
    i0 = [DISPATCH_FLOWS[b % 4][0] for b in range(B)]
    i1 = [DISPATCH_FLOWS[b % 4][1] for b in range(B)]
    init4 = initial_flow("noise", w, h, b=4, seed=3)
    want4, _ = expected(oracle, ("dispatch", w, h), gray, alpha, i0[:4], i1[:4], init4, "pixflow_low", "UNKNOWN")
    init = np.ascontiguousarray(np.broadcast_to(init4[None], (B // 4, 4, h, w, 2)).reshape(B, h, w, 2))
    got, info = ctx.debug_flow_level(gray, alpha, i0, i1, init, "pixflow_low", "UNKNOWN",
                                     want=["sweep_forward", "sweep_backward", "final_flow"])
    print("dispatch %dx%d B=%d: %r" % (w, h, B, info))
    assert info["sweep_error"] == 0, info
    assert info["lanes_per_pixel"] == 3, info
    assert info["waves"] < info["bands"] * B, info
    for stage in ("sweep_forward", "sweep_backward", "final_flow"):
        for k in range(4):
            ref = bits(want4[k][stage])
            bad = (bits(got[stage][k::4]) != ref[None]).reshape(B // 4, -1).any(axis=1)
            assert not bad.any(), "%dx%d B=%d: first differing stage: %s: %d of %d flows of pair %r differ, first b = %d" % (
                w, h, B, stage, int(bad.sum()), B // 4, DISPATCH_FLOWS[k], 4 * int(np.flatnonzero(bad)[0]) + k)
