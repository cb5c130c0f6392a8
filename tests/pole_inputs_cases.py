"""Shared by tests/test_gpu_pole_inputs.py, tests/test_gpu_zz_pole_inputs_host.py and tests/test_cpu_pole_inputs.py: inputs and check
functions for pole removal on the device input paths with the pole masks resident per context (include/s360_pole_inputs.h).

Every comparison is byte equality; there is no tolerance. The oracle of the resident path (s360_set_pole_masks + the secondary bottom
camera handed in as a camera) is the per-frame path (s360_frame_upload_pole_removal) on a second context; the oracle of both is the
CPU oracle's frame (tests/test_gpu_frame.py::test_pole_removal_two_frames). Everything runs on the 17-camera golden rig scaled to
refprog.CAM = 256 with an equirect of 504 x 252; the bottom cameras' images also at 250 x 254 and 253 x 251."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
from PIL import Image

import isputil
import refprog
import rigutil

ROOT = refprog.ROOT
CAM = refprog.CAM
FLAGS = dict(eqr_width=refprog.EQR_W, eqr_height=refprog.EQR_H, enable_top=0, enable_bottom=1, enable_pole_removal=1,
             final_eqr_width=0, final_eqr_height=0)
GOLDEN_RIG = os.path.join(ROOT, "tests", "golden", "rig_17cam.json")
# (w, h) of the two bottom cameras' images: the plain case; rows that are no multiple of 16 bytes with a pixel count that is a
# multiple of 4; an odd pixel count (the scalar tail, and with flip180 the reversed read whose 16-byte groups are misaligned)
SIZES = ((256, 256), (250, 254), (253, 251))
STATE = ("bottom_image", "bottom_image2")
DEBUG_NAMES = ("bottomImage.png", "bottomImage2.png", "bottomWarp2.png", "_bottomCombined.png")
BOTTOM2 = -3  # S360_CAMERA_BOTTOM2


# ---- rigs ---------------------------------------------------------------------------------------------------------------------
def small_rig(dirpath, cam=CAM):
    return rigutil.scaled_rig_json(GOLDEN_RIG, os.path.join(str(dirpath), "rig_small.json" if cam == CAM else "rig_%d.json" % cam), cam / 2048.0)


def bottom_ids(rig_path):
    """(id of the bottom camera, id of the secondary one) as the library finds them."""
    from surround360_amd import render as R
    rig = R.RigDescription(rig_path)
    return rig.get_bottom_camera_id(), rig.get_bottom_camera2_id()


def turned_rig(rig_path, dst_path):
    """A copy of the rig whose secondary bottom camera has `up` and `right` negated: the same optical axis, the image turned by 180
    degrees, so that up1 . up2 changes its sign."""
    rig = json.load(open(rig_path))
    _, b2 = bottom_ids(rig_path)
    for c in rig["cameras"]:
        if c["id"] == b2:
            c["up"] = [-v for v in c["up"]]
            c["right"] = [-v for v in c["right"]]
    json.dump(rig, open(dst_path, "w"))
    return dst_path


def up_sign(rig_path):
    """The sign of up1 . up2 of the two bottom cameras, from the rig file (negative: the secondary image is flipped, TRSP:580)."""
    b, b2 = bottom_ids(rig_path)
    cams = {c["id"]: c for c in json.load(open(rig_path))["cameras"]}
    d = float(np.dot(cams[b]["up"], cams[b2]["up"]))
    assert d != 0
    return 1 if d > 0 else -1


# ---- inputs --------------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(rig_path, yaw=0.0, cam=CAM):
    """dict(side, bottom, bottom2, m1, m2) of one synthetic frame (rigutil.pole_removal_inputs), computed once per (rig, yaw)."""
    key = (open(rig_path).read(), yaw)
    if key not in _INPUTS:
        side, _, bottom, imgs, m1, m2 = rigutil.pole_removal_inputs(rig_path, cam, yaw_deg=yaw)
        _INPUTS[key] = dict(side=side, bottom=bottom, bottom2=imgs[bottom_ids(rig_path)[1]], m1=m1, m2=m2)
    return _INPUTS[key]


def cropped(fr, size):
    """The frame with its two bottom images and masks cut to size = (w, h); the side cameras stay."""
    w, h = size
    out = dict(fr)
    for k in ("bottom", "bottom2", "m1", "m2"):
        out[k] = np.ascontiguousarray(fr[k][:h, :w])
    return out


def mask_cases(w, h):
    """name -> (mask 1, mask 2), B,G,R: what the red test and the mask cut can get wrong."""
    white = np.full((h, w, 3), 255, np.uint8)
    red = np.zeros((h, w, 3), np.uint8)
    red[..., 2] = 255
    corners = white.copy()
    for y, x in ((0, 0), (h - 1, w - 1), (h // 2, 0), (h // 2, w - 1)):  # pixel 0, pixel w*h - 1, both ends of a middle row
        corners[y, x] = (0, 0, 255)
    near = white.copy()  # near-reds, which must not count: blocks large enough to survive the feather if they did
    near[h // 2 - 20:h // 2, w // 2 - 30:w // 2 - 10] = (0, 0, 254)
    near[h // 2 - 20:h // 2, w // 2 - 5:w // 2 + 15] = (1, 0, 255)
    near[h // 2 + 5:h // 2 + 25, w // 2 - 30:w // 2 - 10] = (0, 1, 255)
    return {"no_red": (white, white.copy()), "all_red_1": (red, white.copy()), "corners": (corners, corners[::-1, ::-1].copy()),
            "near_reds": (near, near.copy())}


# ---- contexts and what is compared ------------------------------------------------------------------------------------------------
def make_ctx(rig_path, debug=False, **more):
    from surround360_amd import debug_images as DI
    from surround360_amd import render as R
    c = R.Context(R.RigDescription(rig_path), R.make_params(**dict(FLAGS, **more)))
    if debug:
        DI.set_debug_images(c, True)
    return c


def feed_per_frame(c, fr):
    c.upload_frame(fr["side"], None, fr["bottom"])
    c.upload_pole_removal(fr["bottom2"], fr["m1"], fr["m2"])


def feed_resident(c, fr):
    """(the masks are the context's already)"""
    c.upload_frame(fr["side"], None, fr["bottom"])
    c.upload_bottom2(fr["bottom2"])


def result_of(c, debug=False):
    from surround360_amd import debug_images as DI
    out = {"equirect": c.download_equirect(), "flow_bottom_secondary": c.get_f32("flow_bottom_secondary").view(np.uint32)}
    for n in STATE:
        out[n] = c.get_u8(n)
    if debug:
        names = [e[0] for e in DI.debug_image_list(c)]
        for n in DEBUG_NAMES:
            assert n in names, (n, names)
            out[n] = DI.get_debug_image(c, names.index(n))
    return out


def differing(a, b):
    """The entries of two results that are not byte for byte the same (empty: equal)."""
    assert a.keys() == b.keys()
    return ["%s: %s" % (k, "%d bytes differ" % int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else "shapes %s %s" % (a[k].shape, b[k].shape))
            for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]


def render_per_frame(rig_path, frames, debug=False, **flags):
    """The frames (chained with use_prev from the second on) through s360_frame_upload_pole_removal: the list of their results."""
    c = make_ctx(rig_path, debug, **flags)
    try:
        out = []
        for k, fr in enumerate(frames):
            feed_per_frame(c, fr)
            c.render(use_prev=k > 0)
            out.append(result_of(c, debug))
        return out
    finally:
        c.close()


def render_resident(rig_path, frames, debug=False, masks_of=None, **flags):
    """... and through s360_set_pole_masks (once, or before frame k with masks_of[k]) + s360_frame_upload_bottom2."""
    c = make_ctx(rig_path, debug, **flags)
    try:
        out = []
        for k, fr in enumerate(frames):
            if k == 0 or masks_of:
                m1, m2 = masks_of[k] if masks_of else (fr["m1"], fr["m2"])
                c.set_pole_masks(m1, m2)
            feed_resident(c, fr)
            c.render(use_prev=k > 0)
            out.append(result_of(c, debug))
        return out
    finally:
        c.close()


# ---- the program --------------------------------------------------------------------------------------------------------------------
POLE_MSG = "--bin_list is not available with --enable_pole_removal"


def write_masks(mdir, rig_path):
    os.makedirs(str(mdir), exist_ok=True)
    _, _, bottoms = refprog.rig_ids(rig_path)
    for j, cid in enumerate(bottoms):
        Image.fromarray(np.ascontiguousarray(refprog.pole_mask(CAM, 10 - j, 20)[:, :, ::-1])).save(os.path.join(str(mdir), cid + ".png"))
    return str(mdir)


def _state_files(out, frame):
    """What case a compares of a frame: the equirect's pixels, flow_bottom_secondary.bin's bytes, the bottomImage*.png pixels."""
    d = {"eqr": refprog._digest_png(os.path.join(out, "eqr_%s.png" % frame))}
    flow = os.path.join(out, "flow", frame, "flow_bottom_secondary.bin")
    if os.path.exists(flow):
        d["flow_bottom_secondary.bin"] = hashlib.sha256(open(flow, "rb").read()).hexdigest()
    for n in ("bottomImage.png", "bottomImage2.png"):
        p = os.path.join(out, "debug", frame, "flow_images", n)
        if os.path.exists(p):
            d[n] = refprog._digest_png(p)
    return d


def check_bin_list_pole_removal(unpacker_exe, trsp_exe, tmp_path, bits=12):
    """host/TestRenderStereoPanorama --bin_list --enable_pole_removal against the chain through files (host/Unpacker -> --imgs_dir,
    the same program): shaped like tests/test_gpu_zz_unpacker.py::check_bin_list — one frame, the chained second frame,
    --num_frames 2, and --num_streams 2 --stream_gpus 1. On the commit before this feature the program dies with POLE_MSG."""
    import test_gpu_zz_unpacker as U  # (its check_bin_list is the model; nothing of it is edited)
    assert callable(U.check_bin_list)
    rig = small_rig(tmp_path)
    ids = [c["id"] for c in json.load(open(rig))["cameras"]]
    n = len(ids)
    serials = [40000 + 7 * k for k in range(n)]  # ascending: Unpacker's cam<k> is the k-th smallest serial number
    configs = [isputil.CONFIG_GRBG_NOSHARP if k % 3 else isputil.CONFIG_FULL for k in range(n)]
    pats = ["GRBG" if k % 3 else "RGGB" for k in range(n)]
    frames = [[isputil.bayer_frame(CAM, CAM, seed=100 * f + k, pattern=pats[k]) for k in range(n)] for f in range(2)]
    binp = tmp_path / "0.bin"
    isputil.footage_file(str(binp), frames, bits, serials)
    ispd, imgs = tmp_path / "isp", tmp_path / "imgs"
    ispd.mkdir()
    imgs.mkdir()
    for s, js in zip(serials, configs):
        (ispd / ("%d.json" % s)).write_text(js)
    mdir = write_masks(tmp_path / "masks", rig)
    r = subprocess.run([unpacker_exe, "--isp_dir", str(ispd), "--output_dir", str(imgs), "--bin_list", str(binp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    common = ["--rig_json_file", rig, "--eqr_width", str(refprog.EQR_W), "--eqr_height", str(refprog.EQR_H), "--final_eqr_width",
              str(refprog.FINAL), "--final_eqr_height", str(refprog.FINAL), "--enable_top", "--enable_bottom", "--enable_pole_removal",
              "--bottom_pole_masks_dir", mdir, "--sharpening", "0.25"]

    def run(tag, src, frame, prev, extra=(), frames_made=1):
        out = tmp_path / tag
        for k in range(frames_made):
            f = "%06d" % (int(frame) + k)
            for d in (out, out / "flow", out / "debug", out / "flow" / f, out / "debug" / f, out / "debug" / f / "flow_images"):
                d.mkdir(exist_ok=True)
        cmd = [trsp_exe] + common + src + ["--frame_number", frame, "--output_data_dir", str(out), "--prev_frame_data_dir", prev,
                                           "--output_equirect_path", str(out / "eqr_{frame}.png")] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, "%s: rc %d\n%s" % (tag, r.returncode, r.stderr[-2000:])
        return str(out)

    files = ["--imgs_dir", str(imgs)]
    bins = ["--bin_list", str(binp), "--isp_dir", str(ispd)]
    a = run("files", files, "000000", "NONE")
    b = run("bins", bins, "000000", "NONE")
    assert refprog.png_pixels_bgr(os.path.join(a, "eqr_000000.png")).std() > 5
    want0 = _state_files(a, "000000")
    assert len(want0) == 4 and _state_files(b, "000000") == want0, "bins, one frame"
    run("files", files, "000001", "000000")
    run("bins", bins, "000001", "000000")
    want1 = _state_files(a, "000001")
    assert len(want1) == 4 and want1 != want0 and _state_files(b, "000001") == want1, "bins, the chained second frame"
    c = run("stream", bins, "000000", "NONE", ["--num_frames", "2"], frames_made=2)
    # (a stream writes state files behind its last frame only: frame 0 leaves its equirect and nothing else to compare)
    assert _state_files(c, "000000") == {"eqr": want0["eqr"]} and _state_files(c, "000001") == want1, "--num_frames 2"
    # two streams in the frame slots of ONE context (frame 1 starts a stream of its own: no previous frame), shared masks
    alone = run("bins1", bins, "000001", "NONE")
    e = run("slots2", bins, "000000", "NONE", ["--num_frames", "2", "--num_streams", "2", "--stream_gpus", "1"], frames_made=2)
    assert _state_files(e, "000000") == want0 and _state_files(e, "000001") == _state_files(alone, "000001"), "--num_streams 2 --stream_gpus 1"


def run_pole_case(exe, rig, imgs, out, mdir, more_args=(), ext_check=True):
    """refprog.CASES["pole_removal"] over an imgs_dir that is there already (refprog.run_case writes its own): the frames chained
    with --prev_frame_data_dir; returns the stderr of every process."""
    frames, extra = refprog.CASES["pole_removal"]
    prev, logs = "NONE", []
    for f in frames:
        cmd = [exe, "--rig_json_file", rig, "--imgs_dir", imgs, "--frame_number", f, "--output_data_dir", out, "--prev_frame_data_dir", prev,
               "--output_equirect_path", os.path.join(out, "eqr_%s.png" % f), "--eqr_width", str(refprog.EQR_W), "--eqr_height",
               str(refprog.EQR_H), "--final_eqr_width", str(refprog.FINAL), "--final_eqr_height", str(refprog.FINAL)] + extra
        cmd += ["--output_cubemap_path", os.path.join(out, "cube_%s.png" % f), "--bottom_pole_masks_dir", mdir, "--v", "1"] + list(more_args)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, "frame %s: rc %d\n%s" % (f, r.returncode, r.stderr[-2000:])
        logs.append(r.stderr)
        prev = f
    return logs


def pole_case_inputs(tmp_path, tag, rewrite):
    """(rig, imgs_dir, out_dir, masks_dir) of refprog.CASES["pole_removal"]; rewrite(camera id, B,G,R image) -> the bytes of the
    camera's file (None: PIL's PNG stays)."""
    rig = small_rig(tmp_path)
    frames, _ = refprog.CASES["pole_removal"]
    imgs, out, mdir = refprog.write_inputs(str(tmp_path / tag), rig, frames, masks=True)
    for cid in os.listdir(imgs):
        for f in frames:
            p = os.path.join(imgs, cid, f + ".png")
            data = rewrite(cid, np.ascontiguousarray(np.asarray(Image.open(p))[:, :, ::-1]))
            if data is not None:
                open(p, "wb").write(data)
    return rig, imgs, out, mdir


def decoded_where(log):
    m = re.findall(r"camera images:\s+(\d+) files decoded on the device, (\d+) on the host", log)
    assert m, log[-1500:]
    return int(m[-1][0]), int(m[-1][1])


def used(rig):
    """The camera files a frame of the pole-removal case reads: the side cameras and the two bottom cameras (no top camera)."""
    return len(refprog.rig_ids(rig)[0]) + 2


def assert_golden(out):
    got = refprog.digests(out, "pole_removal")
    golden = json.load(open(refprog.GOLDEN))["pole_removal"]
    assert not sorted(k for k in golden if k not in got)
    differing_files = sorted(k for k in golden if got[k] != golden[k])
    assert not differing_files, "%d of %d files differ from the reference program's: %s" % (len(differing_files), len(golden), differing_files[:12])


def check_device_input_png(exe, tmp_path, encode):
    """Case b: every camera file, the secondary bottom camera's included, rewritten as a banded file by the device encoder
    (encode(B,G,R image) -> file) and read with --device_input_png: the golden digests, and one more device-decoded file per frame
    than the cameras without the secondary."""
    rig, imgs, out, mdir = pole_case_inputs(tmp_path, "png", lambda cid, a: encode(a))
    for log in run_pole_case(exe, rig, imgs, out, mdir, ["--device_input_png"]):
        assert decoded_where(log) == (used(rig), 0) and used(rig) == len(refprog.rig_ids(rig)[0]) + 1 + 1
    assert_golden(out)


def check_device_input_jpeg(exe, tmp_path):
    """Case c: the same case on JPEG files (the side cameras' as .jpg, the bottom cameras' under the names the program reads), with
    and without --device_input_jpeg: the same files written, and the secondary counted on the device path."""
    import input_jpeg_cases as IJ
    import test_gpu_zz_input_png_host as Z
    side_ids = refprog.rig_ids(small_rig(tmp_path))[0]
    outs = {}
    for tag, flag in (("off", []), ("on", ["--device_input_jpeg"])):
        rig, imgs, out, mdir = pole_case_inputs(tmp_path, "jpeg_" + tag, lambda cid, a: IJ.pil_encode(a, 95, 2, False))
        for cid in side_ids:
            for f in os.listdir(os.path.join(imgs, cid)):
                os.rename(os.path.join(imgs, cid, f), os.path.join(imgs, cid, f[:-4] + ".jpg"))
        for log in run_pole_case(exe, rig, imgs, out, mdir, flag):
            if flag:
                assert decoded_where(log) == (used(rig), 0)
            else:
                assert "camera images:" not in log
        outs[tag] = out
    assert refprog.png_pixels_bgr(os.path.join(outs["off"], "eqr_000000.png")).std() > 5
    Z.assert_same(outs["off"], outs["on"], 60)


def check_secondary_on_the_host_path(exe, tmp_path, encode):
    """Case d: the secondary camera's file stays PIL's PNG (one zlib stream: not the device decoder's) in an otherwise device-decoded
    directory: the golden digests again, and --v 1 shows that one file on the host path."""
    rig0 = small_rig(tmp_path)
    secondary = refprog.rig_ids(rig0)[2]
    b, b2 = bottom_ids(rig0)
    assert b2 in secondary and b in secondary
    rig, imgs, out, mdir = pole_case_inputs(tmp_path, "mixed", lambda cid, a: None if cid == b2 else encode(a))
    for log in run_pole_case(exe, rig, imgs, out, mdir, ["--device_input_png"]):
        assert decoded_where(log) == (used(rig) - 1, 1)
    assert_golden(out)
