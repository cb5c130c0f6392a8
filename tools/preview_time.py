#!/usr/bin/env python
"""What the preview costs on an MI355X (profiles/preview.txt).
(1) The two per-frame kernels at the real shape — 2048 x 2048 raw, 12 bits packed, equirect 2048 x 1024, the rig of
tests/golden/rig_17cam.json: device ms of k_preview_develop (three layers) and k_preview_compose from the object's own HIP events
(s360_preview_last_times), warm, median / min / max of `--reps` frames, nothing else on the GPU.
(2) host/TestHyperPreview over a synthetic capture of 17 cameras in two .bin files (sparse files: only the three pole cameras'
frames and every camera's serial number are written; the program reads nothing else): frames per second, and with
S360_PREVIEW_TIMES=1 where the wall time went — reading, enqueueing, waiting for the device, JPEG encoding + writing on the
encoder threads.
(3) --device_jpeg (profiles/preview_jpeg.txt): the JPEG encoder on the device (include/s360_jpeg.h behind the compose kernel,
s360_preview_set_jpeg) — its device time per frame from the object's HIP events (s360_preview_last_jpeg_time), median of `--reps`
warm frames, next to (1); and the program of (2) with --device_jpeg off and on ALTERNATING within every round of one call, for
--jpeg_threads 8, 16 and 1: the same binary with the switch off is the baseline.
usage: python tools/preview_time.py [--device_jpeg] [--reps 30] [--frames 48] [--rounds 3] [--out profiles/preview.txt]"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--program", default=os.path.join(ROOT, "host", "TestHyperPreview"))
ap.add_argument("--out", default=None)
ap.add_argument("--device_jpeg", action="store_true")
ap.add_argument("--timeout", type=int, default=240)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "preview_jpeg.txt" if args.device_jpeg else "preview.txt")
RIG = os.path.join(ROOT, "tests", "golden", "rig_17cam.json")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def pack12(v):
    e, o = v[:, 0::2].astype(np.uint32), v[:, 1::2].astype(np.uint32)
    out = np.empty(v.shape[:1] + (v.shape[1] // 2, 3), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = e >> 4, (e & 0xF) | ((o & 0xF) << 4), o >> 4
    return out.reshape(-1)


def scene(n, seed):
    """Smooth gradients, edges and noise, mostly below the preview's saturation point (12-bit 1836)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    v = 700 + 500 * np.sin(xx / 97.0 + seed) * np.cos(yy / 61.0) + 300 * ((xx // 128 + yy // 96) & 1) + rng.normal(0, 25, (n, n))
    return np.clip(v, 0, 4095).astype(np.uint16)


def kernels():
    from surround360_amd import render as R
    from surround360_amd.preview import Preview
    n = args.size
    pv = Preview(R.RigDescription(RIG).rig, n, n, 2048, 1024)
    frames = [[pack12(scene(n, 3 * k + l)) for l in range(3)] for k in range(2)]
    for k in range(5):
        pv.render_packed(*frames[k & 1], 12)
    dev, comp = [], []
    for k in range(args.reps):
        pv.render_packed(*frames[k & 1], 12)
        d, c = pv.last_times()
        dev.append(d)
        comp.append(c)
    for name, t, nbytes in (("k_preview_develop (3 layers)", dev, 3 * (n * n * 3 // 2 + (n // 2) ** 2 * 16)),
                            ("k_preview_compose", comp, 3 * 2048 * 1024 * 8 + 2048 * 1024 * 3 + 3 * (n // 2) ** 2 * 16)):
        med = float(np.median(t))
        say("%-30s median %.4f ms  min %.4f  max %.4f  (%d frames; compulsory traffic %.1f MB = %.0f GB/s at the median)" %
            (name, med, min(t), max(t), len(t), nbytes / 1e6, nbytes / 1e6 / med if med > 0 else 0.0))
    say("  (compulsory traffic: every input and output byte once; compose's 16 taps per layer and pixel mostly hit in cache)")
    if args.device_jpeg:
        pv.set_jpeg(True, 95)
        enc, size = [], 0
        for k in range(5 + args.reps):
            size = len(pv.render_packed_jpeg(*frames[k & 1], 12))
            if k >= 5:
                enc.append(pv.last_jpeg_time())
        say("%-30s median %.4f ms  min %.4f  max %.4f  (%d frames, quality 95, a file of %.2f MB; the host writer needs about 33 ms of one thread per frame: profiles/preview.txt)" %
            ("JPEG encoder (11 kernels)", float(np.median(enc)), min(enc), max(enc), len(enc), size / 1e6))
    pv.close()


def capture(directory, frames):
    n, serials = args.size, [5, 17, 123, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 8, 9]
    fs = n * n * 3 // 2
    imgs = [pack12(scene(n, s)) for s in range(6)]
    for i in range(2):
        cams = list(range(i, 17, 2))
        with open(os.path.join(directory, "%d.bin" % i), "wb") as f:
            page = np.zeros(1024, np.uint32)
            page[:8] = [0xfaceb00c, 1, i, 2, n, n, 12, len(cams)]
            f.write(page.tobytes())
            f.truncate(4096 + fs * len(cams) * frames)  # sparse: the cameras nobody reads stay holes
            for k in range(frames):
                for j, c in enumerate(cams):
                    off = 4096 + (k * len(cams) + j) * fs
                    if c in (2, 15, 16):
                        f.seek(off)
                        f.write(imgs[(k + c) % 6].tobytes())
                    if k == 0 or c in (2, 15, 16):
                        f.seek(off + 4)
                        f.write(np.uint32(serials[c]).tobytes())


def program():
    tmp = tempfile.mkdtemp(prefix="s360_preview_time_")
    try:
        capture(tmp, args.frames)
        for r in range(args.rounds):
            for threads, on in [(t, o) for t in (8, 16, 1) for o in ((False, True) if args.device_jpeg else (False,))]:
                dest = os.path.join(tmp, "out_%d_%d_%d" % (r, threads, on))
                t0 = time.time()
                p = subprocess.run([args.program, "--rig_json_file", RIG, "--binary_prefix", tmp, "--preview_dest", dest, "--jpeg_threads", str(threads)] +
                                   (["--device_jpeg"] if on else []),
                                   capture_output=True, text=True, timeout=args.timeout, env=dict(os.environ, S360_PREVIEW_TIMES="1"))
                wall = time.time() - t0
                if p.returncode != 0:
                    say("round %d, %d encoder threads: exit status %d: %s" % (r, threads, p.returncode, p.stderr[-300:]))
                    return
                m = re.search(r"preview times: (.*)", p.stderr)
                size = sum(os.path.getsize(os.path.join(dest, f)) for f in os.listdir(dest))
                say("round %d, --jpeg_threads %2d%s: process %.2f s; %s; %d files, %.1f MB" %
                    (r, threads, (", --device_jpeg" if on else ", host encoder") if args.device_jpeg else "", wall, m.group(1) if m else "?",
                     len(os.listdir(dest)), size / 1e6))
                shutil.rmtree(dest)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


say("preview: %d x %d raw, 12 bits packed, equirect 2048 x 1024, gamma 1, softmax_coef 30" % (args.size, args.size))
kernels()
say("host/TestHyperPreview, %d frame sets of 17 cameras in two .bin files (page cache warm after the first round), .jpg output" % args.frames)
program()
if args.device_jpeg:
    say("(with --device_jpeg 'encoding + writing' is writing alone: the pool's threads receive finished files. The windows are short, "
        "0.1 - 1.6 s for %d frames; 'process' includes start-up, the page-locked buffers and the maps)" % args.frames)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
