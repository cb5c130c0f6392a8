"""The cases tests/test_gpu_final_flow.py (on the GPU, through the library's test tap s360_debug_upscale_blur) and
tests/test_cpu_final_flow.py (the same kernels on the CPU emulation, tools/libflow_emu.so) share: PixFlow's final step
(PixFlow.h:175-182: resize INTER_LINEAR to the original size, flow *= s, GaussianBlur 3x3) by the tiled kernel
(flow_kernels.hip: k_upscale_blur_tiled) against the blur kernel that resizes while it loads its tile (k_sepblur<1, 2, 0, 2>), and
both against the oracle's resize, multiplication and blur, bit for bit."""
import numpy as np

# (full width, full height, source size or None = int(w * 0.5) x int(h * 0.5), tiled kernel expected, why)
SHAPES = [
    (242, 354, None, True, "both exact halvings"),
    (243, 355, None, True, "neither exact: scales 2.008 / 2.006"),
    (1214, 70, None, True, "19 tiles per row, the last 62 wide"),
    (504, 106, None, True, "the pole shape / 20"),
    (128, 32, None, True, "exactly 2 x 2 tiles"),
    (129, 33, None, True, "one column and one row more than whole tiles: the reflected halo of a 1-wide tile"),
    (131, 37, None, True, "a few more than whole tiles"),
    (64, 16, None, True, "one tile"),
    (65, 17, None, True, "one tile and one element more"),
    (7, 5, None, True, "smaller than the stencil plus box"),
    (5, 4, None, True, "every border rule at once"),
    (4, 4, None, True, "2 x 2 source"),
    (300, 80, (100, 40), False, "x3 horizontally: not around 2, the other kernel"),
]
IDS = ["%dx%d" % s[:2] for s in SHAPES]
BATCH = 3
CONTENTS = ("noise", "signed_zeros_and_extremes", "constant")
POST_SCALES = (2.0, 1.7)


def source_size(w, h, src):
    return src if src is not None else (int(w * 0.5), int(h * 0.5))


def field(content, sw, sh):
    rng = np.random.default_rng(1000 * sh + sw)
    if content == "noise":
        return (rng.standard_normal((BATCH, sh, sw, 2)) * 30).astype(np.float32)
    if content == "constant":
        f = np.empty((BATCH, sh, sw, 2), np.float32)
        f[..., 0], f[..., 1] = 3.25, -0.7
        return f
    # -0.0f, +0.0f and magnitudes 1e30 beside 1e-30, in no pattern
    vals = np.array([-0.0, 0.0, 1e30, -1e30, 1e-30, -1e-30, 1.0], np.float32)
    return vals[rng.integers(0, len(vals), (BATCH, sh, sw, 2))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (name, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def check_shape(run, oracle, w, h, src, tiled):
    """run(src_flows, dw, dh, post_scale, generic) -> (flows, tiled kernel taken)"""
    sw, sh = source_size(w, h, src)
    for content in CONTENTS:
        f = field(content, sw, sh)
        for post in POST_SCALES:
            tag = "%dx%d -> %dx%d %s x%g" % (sw, sh, w, h, content, post)
            want = np.stack([oracle.gaussian_blur_f32(oracle.resize_linear_f32(f[b], w, h) * np.float32(post), 3, 1.0) for b in range(BATCH)])
            gen, took = run(f, w, h, post, True)
            assert not took
            same(tag + ": generic against the oracle", gen, want)
            got, took = run(f, w, h, post, False)
            assert took == tiled, "%s went to the %s kernel" % (tag, "tiled" if took else "generic")
            same(tag + ": against the generic kernel", got, gen)
            same(tag + ": against the oracle", got, want)
