"""The cases tests/test_gpu_sharpen_shapes.py (on the GPU) and tests/test_cpu_sharpen_shapes.py (the same kernels on the CPU
emulation of the library) share: sharpen against the oracle byte for byte at the shapes where the IIR passes change path, and
the batched frame with a final resize that keeps the eye height."""
import numpy as np

import rigutil
from surround360_amd import render as R

# (h, w): chain lengths 2 and 3; one below, at and one above one and two 64-position tiles in each direction; chain counts
# that are no multiple of the 16 chains of a wave. (A side of 1 is left out: the reference's reflect reads out of bounds there.)
SHAPES = [(2, 2), (2, 65), (3, 17), (17, 3), (63, 64), (64, 63), (65, 66), (66, 129), (129, 130), (33, 191)]
AMOUNTS = (0.25, 1.0)
CONTENTS = ("noise", "half_saturated", "constant")

EQR_W, EQR_H, CAM = 1008, 504, 512
# the final equirect keeps the eye height (2 x 504 rows) and its width is no multiple of 4: the resize that only changes the
# width, with a ragged end of row in the B,G,R output
FINAL_W, FINAL_H = 957, 2 * EQR_H
# frame slots whose eyes one set of sharpen launches takes (SlotScratch::kSharpenGroup = 32 images): a batch of one slot more
# has a ragged last group
GROUP_SLOTS = 16


def image(content, h, w):
    rng = np.random.default_rng(1000 * h + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if content == "half_saturated":  # the clamp and the truncation on both sides: the left half is only 0 / 255
        img[:, : (w + 1) // 2] = np.where(img[:, : (w + 1) // 2] < 128, 0, 255)
    elif content == "constant":
        img[:] = (7, 200, 255)
    return img


def same(name, got, want):
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
    d = got.astype(np.int32) - want.astype(np.int32)
    assert not d.any(), "%s: %d mismatching bytes, max |d| %d" % (name, int((d != 0).sum()), int(np.abs(d).max()))


def check_shape(ctx, oracle, h, w, content):
    img = image(content, h, w)
    for amount in AMOUNTS:
        same("sharpen %dx%d %s %g" % (h, w, content, amount), ctx.sharpen(img, amount), oracle.sharpen(img, amount))


def make_rig(rig_json, tmpdir):
    return rigutil.scaled_rig_json(rig_json, str(tmpdir / "rig_small.json"), CAM / 2048.0)


def frame_flags():
    return dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=FINAL_W,
                final_eqr_height=FINAL_H, sharpening=0.25)


def check_batch(path, nslots, oracle=None, cam=CAM, flags=None):
    """nslots frame slots rendered as one batch: every slot equals the same frame rendered alone; with `oracle`, slot 0
    equals the oracle's frame."""
    flags = flags or frame_flags()
    rig = R.RigDescription(path)
    frames = [rigutil.frame_inputs(path, cam, yaw_deg=y) for y in (0.0, 1.1, 2.3)]
    cb = R.Context(rig, R.make_params(**flags))
    c1 = R.Context(rig, R.make_params(**flags))
    try:
        cb.set_frame_slots(nslots)
        cb.set_sweep_mode("throughput")
        for k in range(nslots):
            cb.select_frame_slot(k)
            cb.upload_frame(*frames[k % 3])
        cb.render_batch()
        alone = []
        for f in frames:
            c1.upload_frame(*f)
            c1.render()
            alone.append(c1.download_equirect())
        assert alone[0].shape == (flags["final_eqr_height"], flags["final_eqr_width"], 3)
        assert not np.array_equal(alone[0], alone[1])  # the slots hold different frames
        for k in range(nslots):
            cb.select_frame_slot(k)
            same("sharpened batched slot %d of %d" % (k, nslots), cb.download_equirect(), alone[k % 3])
        if oracle is not None:
            cams, _ = oracle.load_rig(path)
            want, _ = oracle.Frame(cams, oracle.make_params(**flags)).render(*frames[0])
            cb.select_frame_slot(0)
            same("sharpened batched slot 0 against the oracle", cb.download_equirect(), want)
    finally:
        cb.close()
        c1.close()
