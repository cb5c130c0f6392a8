#!/usr/bin/env python
"""What the unpack step costs with the camera PNGs deflated on host threads and with --device_png, on an MI355X:
one synthetic capture (17 cameras, 2048 x 2048, 12 bits packed, `--frames` frame sets) through host/Unpacker without and with the
flag, `--rounds` alternating rounds on the same box and build. Reported per round: wall time of the process and per frame set,
the device time per image of the ISP's kernels (flag off) / the ISP's and the encoder's kernels (flag on) from HIP events on every
camera's own stream (S360_ISP_TIMES=1: the library prints the mean per ISP object; 17 streams share the GPU, so an image's
interval holds the other cameras' kernels too), and the files' sizes. A capture of ONE camera follows: the same intervals with
nothing else on the GPU.
usage: python tools/unpack_time.py [--rounds 3] [--frames 3] [--out profiles/unpack_png16.txt]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--cameras", type=int, default=17)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--program", default=os.path.join(ROOT, "host", "Unpacker"))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_png16.txt"))
ap.add_argument("--timeout", type=int, default=300)
args = ap.parse_args()

ISP_JSON = json.dumps({"CameraIsp": {
    "bitsPerPixel": 12, "blackLevel": [1210.0, 1302.5, 1188.0], "clampMin": [0.0, 0.0, 0.0], "clampMax": [1.0, 1.0, 1.0],
    "vignetteRollOffH": [[1.3, 1.3, 1.3], [1.0, 1.0, 1.0], [1.3, 1.3, 1.3]], "vignetteRollOffV": [[1.2, 1.2, 1.2], [1.0, 1.0, 1.0], [1.2, 1.2, 1.2]],
    "whiteBalanceGain": [1.37, 1.0, 1.81], "ccm": [[1.11, -0.07, 0.02], [0.13, 1.21, -0.28], [-0.12, -0.09, 1.3]],
    "sharpening": [0.5, 0.5, 0.5], "sharpeningSupport": 0.006, "noiseCore": 850.0, "saturation": 1.2, "contrast": 1.0,
    "gamma": [0.4545, 0.4545, 0.4545], "bayerPattern": "GBRG"}})
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bayer12(n, seed):
    """A smooth colour scene with edges and sensor noise, mosaiced GBRG, as 12-bit samples."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    s = 2048.0 / n
    rgb = [0.35 + 0.25 * np.sin(xx * s / 130.0 + 0.3 * seed) * np.cos(yy * s / 170.0), 0.40 + 0.30 * np.cos(xx * s / 190.0) * np.sin(yy * s / 110.0 + 0.7),
           0.30 + 0.20 * np.sin((xx + yy) * s / 230.0)]
    box = (xx > n * 0.3) & (xx < n * 0.55) & (yy > n * 0.25) & (yy < n * 0.7)
    rgb[0][box] += 0.3
    rgb[1][box] -= 0.2
    raw = np.zeros((n, n), np.float32)
    for i, j, c in ((0, 0, 1), (0, 1, 2), (1, 0, 0), (1, 1, 1)):
        raw[i::2, j::2] = rgb[c][i::2, j::2]
    raw += 0.004 * rng.standard_normal((n, n), dtype=np.float32)
    return np.clip(raw * 4095.0 + 250.0, 0, 4095).astype(np.uint32)


def pack12(v):
    a, b = v[:, 0::2], v[:, 1::2]
    out = np.zeros((v.shape[0], v.shape[1] // 2, 3), np.uint8)
    out[..., 0] = a >> 4
    out[..., 1] = (a & 0xF) | ((b & 0xF) << 4)
    out[..., 2] = b >> 4
    return out.ravel()


def capture(path, ncam, frames, n):
    """BinaryFootageFile's layout: a 4096-byte metadata page, then the packed frames interleaved by camera; the camera's serial number
    over bytes 4..7 of every frame."""
    serials = [50000 + 11 * k for k in range(ncam)]
    packed = [pack12(bayer12(n, k)) for k in range(ncam)]
    page = np.zeros(4096, np.uint8)
    page[:32] = np.array([0xfaceb00c, 1234, 0, 1, n, n, 12, ncam], np.uint32).view(np.uint8)
    with open(path, "wb") as f:
        f.write(page.tobytes())
        for k in range(frames):
            for c in range(ncam):
                fr = np.roll(packed[c], 3 * n // 2 * 64 * k)  # (another frame: the same scene 64 rows further)
                fr[4:8] = np.array([serials[c]], np.uint32).view(np.uint8)
                f.write(fr.tobytes())
    return serials


def unpack(binp, ispd, out, on):
    os.makedirs(out)
    cmd = [args.program, "--isp_dir", ispd, "--output_dir", out, "--bin_list", binp] + (["--device_png"] if on else [])
    t = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=args.timeout, env=dict(os.environ, S360_ISP_TIMES="1"))
    wall = time.perf_counter() - t
    if r.returncode != 0:
        raise RuntimeError("rc %d: %s" % (r.returncode, r.stderr[-400:]))
    per = [(int(m.group(1)), float(m.group(2))) for m in re.finditer(r"s360_isp times: (\d+) images, ([0-9.]+) ms", r.stderr)]
    images = sum(k for k, _ in per)
    gpu_ms = sum(k * v for k, v in per) / max(images, 1)
    size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(out) for f in fs)
    shutil.rmtree(out, ignore_errors=True)
    return wall, images, gpu_ms, size


def table(title, ncam):
    binp = os.path.join(work, "%d.bin" % ncam)
    ispd = os.path.join(work, "isp%d" % ncam)
    os.makedirs(ispd)
    for s in capture(binp, ncam, args.frames, args.size):
        with open(os.path.join(ispd, "%d.json" % s), "w") as f:
            f.write(ISP_JSON)
    pixels = ncam * args.frames * args.size * args.size * 6
    say(title)
    say("%-5s %-4s %9s %14s %8s %16s %12s %9s" % ("round", "flag", "wall s", "s / frame set", "images", "GPU ms / image", "files MB", "of input"))
    rows = []
    unpack(binp, ispd, os.path.join(work, "warm"), False)  # (page cache, the driver's first start)
    for rnd in range(args.rounds):
        for on in (False, True):
            wall, images, gpu_ms, size = unpack(binp, ispd, os.path.join(work, "out_%d_%d_%d" % (ncam, rnd, on)), on)
            rows.append((on, wall, gpu_ms, size))
            say("%-5d %-4s %9.3f %14.3f %8d %16.3f %12.1f %9.3f" % (rnd, "on" if on else "off", wall, wall / args.frames, images, gpu_ms, size / 1e6,
                                                                     size / pixels))
    off, onn = [r[1] for r in rows if not r[0]], [r[1] for r in rows if r[0]]
    say("wall time with the flag below without it in every round: %s (off %.3f..%.3f s, on %.3f..%.3f s)" % (
        "yes" if all(a < b for a, b in zip(onn, off)) else "NO", min(off), max(off), min(onn), max(onn)))
    os.remove(binp)


work = tempfile.mkdtemp(prefix="s360_unpack_")
try:
    say("# host/Unpacker, camera images as 16-bit PNG files: %d x %d, 12 bits packed, %d frame sets, %d alternating rounds" % (
        args.size, args.size, args.frames, args.rounds))
    say("# flag off: ISP on the device, 16-bit B,G,R to the host, zlib level 1 / Z_RLE on the camera's host thread; flag on: --device_png")
    say("# GPU ms / image: HIP events around the image's kernels on the camera's own stream (off: ISP; on: ISP + encode)")
    table("## 1. %d cameras, one host thread and one stream per camera" % args.cameras, args.cameras)
    table("## 2. one camera alone (nothing else on the GPU)", 1)
finally:
    shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
