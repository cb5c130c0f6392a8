"""Cases of the preview tests (tests/test_cpu_preview.py, tests/test_gpu_preview.py, tests/golden/make_preview_golden.py):
small rigs, raw frames in the capture's packed formats, hand-made maps.

Shapes. Raw 128 x 96 (half resolution 64 x 48: not square, so min(rows, cols) and rows / cols mix-ups show) onto a 96 x 48
equirect, and raw 66 x 130 (portrait; 12-bit packing needs the even width) onto 70 x 37 (no multiple of any tile: the compose
kernel's tiles are 64 x 4, the develop kernel's rows 256 wide). The rig is tests/golden/rig_17cam.json with its pole cameras
rescaled to the raw size the way Camera::createRescaledCamera rescales. The first shape keeps the cameras' field of view
(1.61443 rad: top and bottom overlap at the horizon, every direction is seen by a camera, only the fov test of sees() ever
fails); the second narrows it to 1.2 rad and doubles the focal lengths, so that a band around the horizon is seen by NO camera
(the 0 * NaN pixels of flattenLayersAlphaSoftmax) and the resolution test of sees() fails for some directions too."""
import copy
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIG_JSON = os.path.join(ROOT, "tests", "golden", "rig_17cam.json")
POLE_IDS = ("cam0", "cam15", "cam16")  # top, bottom, secondary bottom of rig_17cam.json

# name -> (raw_w, raw_h, eqr_w, eqr_h, fov or None, focal factor)
SHAPES = {
    "landscape": (128, 96, 96, 48, None, 1.0),
    "portrait": (66, 130, 70, 37, 1.2, 2.0),
}
CONTENTS = ("spread", "zeros", "max", "checker")
BITS = (8, 12)


def small_rig(shape):
    """The rig's JSON with every camera rescaled to the shape's raw size (and the shape's fov / focal change on the poles)."""
    raw_w, raw_h, _, _, fov, fmul = SHAPES[shape]
    rig = copy.deepcopy(json.load(open(RIG_JSON)))
    rig.pop("_provenance", None)
    for c in rig["cameras"]:
        res = c["resolution"]
        sx, sy = raw_w / res[0], raw_h / res[1]
        c["principal"] = [c["principal"][0] * sx, c["principal"][1] * sy]
        c["focal"] = [c["focal"][0] * sx, c["focal"][1] * sy]
        c["resolution"] = [raw_w, raw_h]
        if c["id"] in POLE_IDS:
            c["focal"] = [c["focal"][0] * fmul, c["focal"][1] * fmul]
            if fov is not None:
                c["fov"] = fov
    return rig


def pole_cameras(rig):
    by_id = {c["id"]: c for c in rig["cameras"]}
    return [by_id[i] for i in POLE_IDS]


def write_rig(rig, path):
    json.dump(rig, open(path, "w"))
    return path


def pack(values, bits):
    """h x w sample values (0..255 for 8 bits, 0..4095 for 12) -> the packed bytes of one frame of a .bin container."""
    v = np.asarray(values).astype(np.uint32)
    if bits == 8:
        return v.astype(np.uint8).reshape(-1)
    h, w = v.shape
    assert w % 2 == 0
    e, o = v[:, 0::2], v[:, 1::2]
    out = np.empty((h, w // 2, 3), np.uint8)
    out[..., 0] = e >> 4
    out[..., 1] = (e & 0xF) | ((o & 0xF) << 4)
    out[..., 2] = o >> 4
    return out.reshape(-1)


def content(name, w, h, bits, seed=0):
    """Sample values of one raw frame. spread: over the whole range, skewed (the cube of a gradient plus noise) so that most
    pixels stay below the point where the preview's 8-bit output saturates (raw 16-bit 29 400 or so: 13 / 29 of full scale);
    zeros; max; checker: 0 and the maximum pixel by pixel, which makes the cubic interpolation overshoot at both ends; dark (not
    in CONTENTS): the lowest values only, the one content whose output does not saturate at gamma 2.2."""
    top = 255 if bits == 8 else 4095
    if name == "zeros":
        return np.zeros((h, w), np.uint32)
    if name == "max":
        return np.full((h, w), top, np.uint32)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "checker":
        return (((yy // 2 + xx // 2) & 1) * top).astype(np.uint32)
    rng = np.random.RandomState(1000 + seed)
    if name == "dark":  # gamma 2.2 only: (v / 13) ^ 2.2 * 29 saturates the 8-bit output from raw 16-bit 434 (12-bit 27) on
        return rng.randint(0, 41 if bits == 12 else 3, size=(h, w)).astype(np.uint32)
    assert name == "spread"
    u = (0.6 * ((xx * 3 + yy * 5) % (w + h)) / float(w + h) + 0.4 * rng.rand(h, w))
    u[0, 0], u[0, 1] = 0.0, 1.0  # both ends of the range are present
    return np.minimum(top, np.floor((top + 1) * u ** 3)).astype(np.uint32)


def frames(shape, name, bits):
    """Three packed frames (top, bottom, bottom2) of one content; the three differ where the content is not constant."""
    raw_w, raw_h = SHAPES[shape][:2]
    return [pack(content(name, raw_w, raw_h, bits, seed=l), bits) for l in range(3)]


def hand_made_map(eqr_w, eqr_h, hw, hh, layer):
    """A map no camera makes, for the compose kernel: a slanted sweep over the whole layer and past all four of its edges in steps
    that are no multiple of 1/32, with entries put on exact rounding ties of the 1/32 quantisation (k/32 + 1/64: half-way cases,
    round-half-even decides), entries at -1 (the 'not seen' mark, one coordinate or both), on the last column and row, just
    outside them, far outside (the int16 saturation of the integer part), and rows 3..5 not seen by any layer."""
    yy, xx = np.mgrid[0:eqr_h, 0:eqr_w].astype(np.float64)
    mx = -3.0 + (xx * (hw + 6.0) / eqr_w) + 0.013 * yy + 0.37 * layer
    my = -3.0 + (yy * (hh + 6.0) / eqr_h) + 0.021 * xx - 0.23 * layer
    m = np.stack([mx, my], axis=-1).astype(np.float32)
    tie = ((xx + 2 * yy + layer) % 5 == 0)
    m[tie] = (np.floor(m[tie] * 32) / 32 + 1.0 / 64).astype(np.float32)
    special = [(-1.0, -1.0), (-1.0, 5.0), (5.0, -1.0), (hw - 1.0, hh - 1.0), (hw - 1.0, 2.5), (2.5, hh - 1.0), (hw - 0.5, 3.0),
               (hw, hh), (hw + 0.984375, 1.0), (3.0, hh + 2.0), (-2.984375, -2.984375), (-3.0, 4.0), (40000.0, 3.0), (3.0, -40000.0),
               (1.0 + 1.0 / 64, 2.0 + 3.0 / 64), (hw - 3.0, hh - 3.0), (hw - 3.0 + 1.0 / 32, hh - 3.0 + 1.0 / 32), (0.0, 0.0)]
    for k, s in enumerate(special):
        m[(7 + layer) % eqr_h, (3 + 2 * k + layer) % eqr_w] = s
    m[3:6] = -1.0
    return m


# ---- a capture: two .bin containers, 17 cameras, three frames (the program's tests) ---------------------------------------
# camera c of a frame set lives in file c % 2. The serial numbers' order as decimal STRINGS ("123" < "17" < ... < "31" < "5" <
# "8" < "9") differs from their numeric order, and TestHyperPreview indexes the string-sorted list: its defaults 0 / 15 / 16
# mean the cameras with serial 123 (top), 8 (bottom) and 9 (secondary bottom); sorted as numbers they would be 5, 31 and 123.
CAPTURE_SERIALS = [5, 17, 123, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 8, 9]
CAPTURE_POLES = (2, 15, 16)  # positions in CAPTURE_SERIALS of the top, bottom and secondary bottom camera
CAPTURE_FRAMES = 3


def capture_frames(shape, bits):
    """[frame][camera] packed frames: the three pole cameras carry the 'spread' content (another seed per frame and layer), the
    other fourteen noise; bytes 4..7 of every frame are the camera's serial number, as in a real capture."""
    raw_w, raw_h = SHAPES[shape][:2]
    out = []
    for f in range(CAPTURE_FRAMES):
        row = []
        for c, serial in enumerate(CAPTURE_SERIALS):
            if c in CAPTURE_POLES:
                fr = pack(content("spread", raw_w, raw_h, bits, seed=10 * f + CAPTURE_POLES.index(c)), bits)
            else:
                fr = np.random.RandomState(77 + 100 * f + c).randint(0, 256, size=frames_bytes(raw_w, raw_h, bits)).astype(np.uint8)
            fr = fr.copy()
            fr[4:8] = np.frombuffer(np.uint32(serial).tobytes(), np.uint8)
            row.append(fr)
        out.append(row)
    return out


def frames_bytes(raw_w, raw_h, bits):
    return raw_w * raw_h if bits == 8 else raw_h * (3 * raw_w // 2)


def write_capture(directory, shape, bits, file_count=2, magic=0xfaceb00c, claimed_file_count=None):
    """<directory>/0.bin ... : a 4096-byte metadata page {magic, timestamp, fileIndex, fileCount, width, height, bitsPerPixel,
    numberOfCameras}, then the frame sets, cameras interleaved. Returns capture_frames(shape, bits)."""
    raw_w, raw_h = SHAPES[shape][:2]
    fr = capture_frames(shape, bits)
    n = len(CAPTURE_SERIALS)
    for i in range(file_count):
        cams = list(range(i, n, file_count))
        page = np.zeros(1024, np.uint32)
        page[:8] = [magic, 1476000000 + i, i, claimed_file_count or file_count, raw_w, raw_h, bits, len(cams)]
        with open(os.path.join(directory, "%d.bin" % i), "wb") as f:
            f.write(page.tobytes())
            for fs in fr:
                for c in cams:
                    f.write(fs[c].tobytes())
    return fr
