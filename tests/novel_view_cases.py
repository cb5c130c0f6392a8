"""Inputs of the view-interpolation tests (tests/test_cpu_novel_view.py, tests/test_gpu_novel_view.py) and of the generator of
their expected values (tests/golden/make_novel_view_golden.py). numpy only, every case deterministic; the expected values are
the reference's own generateNovelView compiled where it lies (see the generator), recorded in tests/golden/novel_view_golden.*.

  (a) "synth": a surround360_amd.synth.flow_pair with the real pixflow_low flows of it (NovelViewGeneratorAsymmetricFlow::prepare);
  (b) "edge":  content the noise generator never produces: alpha holes in both images, alpha strictly between 0 and 255, flows that
               carry the sampling position outside the image, identical colours (colorDiff 0), opposite saturated colours (765),
               zero flow;
  (c) three Middlebury-shaped datasets (<p>_10.png, <p>_11.png, <p>_10i11.png), one of them stored as three-channel PNGs.
"""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_NPZ = os.path.join(HERE, "golden", "novel_view_golden.npz")
GOLDEN_JSON = os.path.join(HERE, "golden", "novel_view_golden.json")

W, H = 192, 160
SHIFTS4 = [0.0, 0.3, 0.5, 1.0]


def mode_test_shifts(n):
    """shiftFromLeft of TestOpticalFlow --mode test: double(v) / double(n - 1)"""
    return [float(v) / float(n - 1) for v in range(n)]


ALL_SHIFTS = mode_test_shifts(11)  # holds 0, 0.3, 0.5 and 1 as the very same doubles
PROGRAM_VIEWS = 5                  # --num_intermediate_views of the program tests: 0, 0.25, 0.5, 0.75, 1
RECORDED = {"synth": sorted(set(ALL_SHIFTS + mode_test_shifts(PROGRAM_VIEWS))), "edge": ALL_SHIFTS}
# every view of every case is recorded as a SHA-256 digest; these also as images, so that a failing test can name the pixel
FULL = {"synth": [0.3, 0.5], "edge": SHIFTS4}  # merged
FULL_SIDES = {"synth": [0.3], "edge": [0.3]}   # fromL / fromR
FULLSIZE = dict(w=2048, h=2048, seed=11, merged=[0.25, 0.5], sides=[0.5])
MIDDLEBURY = ["blobs", "rings", "stripes"]
MIDDLEBURY_BGR = "rings"  # stored without alpha


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key(case, what, shift):
    return "%s-%s-%s" % (case, what, repr(float(shift)))


def synth_pair():
    from surround360_amd import synth
    return synth.flow_pair(W, H, seed=23)


def prepare_flows(compute_optical_flow, img_l, img_r, alg="pixflow_low"):
    """NovelViewGeneratorAsymmetricFlow::prepare (NovelView.cpp:270-299) with any implementation of the flow"""
    return compute_optical_flow(img_l, img_r, alg, "LEFT"), compute_optical_flow(img_r, img_l, alg, "RIGHT")


def edge_case():
    """(imgL, imgR, flowLtoR, flowRtoL). Columns, left to right: a hole in imageL (0..23), a hole on either side of imageR
    (0..11 and the last 40), both of them overlapping over 0..11 so that all four alpha cases of combineNovelViews are
    populated; bands of rows carry the colour / alpha / flow specials."""
    yy, xx = np.mgrid[0:H, 0:W]
    img_l = np.empty((H, W, 4), np.uint8)
    img_r = np.empty((H, W, 4), np.uint8)
    # base: smooth colour ramps, different in the two images
    img_l[..., 0] = (xx * 255 // (W - 1)).astype(np.uint8)
    img_l[..., 1] = (yy * 255 // (H - 1)).astype(np.uint8)
    img_l[..., 2] = ((xx + yy) * 7 % 256).astype(np.uint8)
    img_r[..., 0] = ((W - 1 - xx) * 255 // (W - 1)).astype(np.uint8)
    img_r[..., 1] = ((yy * 3 + xx) % 256).astype(np.uint8)
    img_r[..., 2] = (255 - (xx * 5 + yy * 2) % 256).astype(np.uint8)
    img_l[..., 3] = 255
    img_r[..., 3] = 255
    # rows 32..63: identical colours (colorDiff 0); rows 64..95: opposite saturated colours (sum of differences 765)
    img_r[32:64, :, :3] = img_l[32:64, :, :3]
    img_l[64:96, :, :3] = np.where(((xx[64:96] // 16) % 2 == 0)[..., None], 255, 0).astype(np.uint8)
    img_r[64:96, :, :3] = 255 - img_l[64:96, :, :3]
    # rows 96..127: alpha strictly between 0 and 255, different ramps in the two images
    img_l[96:128, :, 3] = (1 + (xx[96:128] * 253 // (W - 1))).astype(np.uint8)
    img_r[96:128, :, 3] = (254 - (xx[96:128] * 253 // (W - 1))).astype(np.uint8)
    # holes
    img_l[:, :24, 3] = 0
    img_r[:, :12, 3] = 0
    img_r[:, W - 40:, 3] = 0
    img_l[140:, 60:100, 3] = 0
    img_r[140:, 80:120, 3] = 0
    # flows: about +-3 px with a fractional part, smooth; zero flow in rows 0..15; a block that points far outside the image
    f_lr = np.empty((H, W, 2), np.float32)
    f_rl = np.empty((H, W, 2), np.float32)
    f_lr[..., 0] = (-3.0 + 0.37 * np.sin(yy / 9.0) + 0.011 * xx).astype(np.float32)
    f_lr[..., 1] = (0.45 * np.cos(xx / 13.0)).astype(np.float32)
    f_rl[..., 0] = (3.0 + 0.41 * np.cos(yy / 7.0) - 0.009 * xx).astype(np.float32)
    f_rl[..., 1] = (-0.35 * np.sin(xx / 11.0)).astype(np.float32)
    f_lr[:16] = 0.0
    f_rl[:16] = 0.0
    f_lr[16:32, 100:140] = (-400.0, 7.5)   # fromR samples left of the image: border -> alpha 0
    f_rl[16:32, 60:100] = (12.25, 300.0)   # fromL samples below the image
    f_rl[128:140, 150:] = (90.0, -0.5)     # fromL leaves through the right edge as t grows: partial border taps
    return img_l, img_r, f_lr, f_rl


def middlebury_dataset(name):
    """(frame10, frame11, true mid frame), BGR uint8 96 x 64: a textured background with shapes that move between the frames."""
    w, h = 96, 64
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def frame(t):
        if name == "blobs":
            cx, cy = 30 + 8 * t, 30 + 2 * t
            fg = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 90.0)
            base = 90 + 50 * np.sin(xx / 5.0) * np.cos(yy / 7.0)
            return np.dstack([base + 100 * fg, base * 0.8 + 40 * fg, 200 - base * 0.5 - 60 * fg])
        if name == "rings":
            cx = 48 - 6 * t
            r = np.sqrt((xx - cx) ** 2 + (yy - 32) ** 2)
            ring = 0.5 + 0.5 * np.cos(r / 2.5)
            base = 60 + 0.9 * xx + 0.7 * yy
            return np.dstack([base + 70 * ring, 220 - base * 0.6, 40 + 150 * ring])
        s = 0.5 + 0.5 * np.sin((xx - 5 * t) / 3.0 + yy / 11.0)  # "stripes"
        return np.dstack([40 + 180 * s, 128 + 60 * np.cos(yy / 6.0), 230 - 170 * s])

    return tuple(np.clip(np.rint(frame(t)), 0, 255).astype(np.uint8) for t in (0.0, 1.0, 0.5))


def add_alpha(bgr):
    """cvtColor(BGR2BGRA)"""
    return np.ascontiguousarray(np.dstack([bgr, np.full(bgr.shape[:2], 255, np.uint8)]))


def write_middlebury_dir(path):
    """the directory of case (c) as PNG files (PIL stores RGB(A): channels swapped on the way out)"""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    for name in MIDDLEBURY:
        for suffix, im in zip(("10", "11", "10i11"), middlebury_dataset(name)):
            rgb = im[..., ::-1]
            if name != MIDDLEBURY_BGR:
                rgb = np.dstack([rgb, np.full(rgb.shape[:2], 255, np.uint8)])
            Image.fromarray(np.ascontiguousarray(rgb)).save(os.path.join(path, "%s_%s.png" % (name, suffix)))


def fmt_g(x):
    """a double as glog's / iostream's operator<< prints it (precision 6, %g)"""
    return "%g" % x


def image_diff_rmse(a, b):
    """imageDiffRMSE of the reference's TestOpticalFlow.cpp:145-163 restated: both four-channel images are walked as THREE-byte
    elements (Vec3b over Vec4b rows), so pixel x of a row reads bytes 3x .. 3x+2 of that row."""
    h, w = a.shape[:2]
    ra = a.reshape(h, w * 4)[:, :3 * w].astype(np.int64)
    rb = b.reshape(h, w * 4)[:, :3 * w].astype(np.int64)
    return float(np.sqrt(float(((ra - rb) ** 2).sum()) / float(3 * h * w)))
