"""Cases of the device JPEG encoder's tests (tests/test_gpu_jpeg.py, tests/test_cpu_jpeg_device.py): sizes, contents, qualities, and
the two byte oracles — host/jpeg_io.hpp's writer behind tools/jpeg_host_encode, and PIL's save(quality=q, subsampling=2). No
reference data is needed: everything is byte equality against those two.

Sizes, each for a way the kernels can go wrong: 1 x 1 (the smallest image), 8 x 8 (one real Y block, three dummies), 9 x 9,
16 x 16 (one MCU), 17 x 9, 15 x 33 and 33 x 15 (dummies on one edge only), 48 x 32, 70 x 37, 257 x 3 and 3 x 257 (one MCU row /
column), 640 x 33, 64 x 64, 400 x 304 (2850 blocks), 1030 x 70.

The kernels' constants (surround360_amd/csrc/jpeg.hpp, jpeg.hip) these sizes must exceed by a non-multiple:
  JPEG_SCAN_ITEMS = 1024   blocks (and stream tiles) one workgroup of the scan kernels takes: 400 x 304 has 2850 = 2 x 1024 + 802
                           blocks, 1030 x 70 has 1950 = 1024 + 926;
  JPEG_STUFF_TILE = 4096   stream bytes one workgroup of the stuffing kernels takes: the 400 x 304 and 1030 x 70 scans of noise are
                           many tiles long and no multiple of it (asserted in test_cpu_jpeg_device.py's preconditions);
  JB_MCUS = 4, JE_WAVES = 4   MCUs / blocks per workgroup of the block and entropy kernels: 17 x 9 has 2 MCUs, 70 x 37 has 15
                           MCUs and 90 blocks.

A padded last byte that is 0xFF (stuffed like any other: the file then ends FF 00 FF D9) does not occur in 1 x 1 images at all: the
last block is Cr and ends with its EOB code, two 0 bits, unless its coefficient 63 is non-zero. At quality 100 noise makes it
non-zero; a search over seeds found the LAST_FF cases below, which the preconditions pin."""
import functools
import io
import os
import subprocess
import tempfile

import numpy as np

import preview_cases as PC

ROOT = PC.ROOT
SCAN_ITEMS, STUFF_TILE = 1024, 4096  # JPEG_SCAN_ITEMS, JPEG_STUFF_TILE

SIZES = [(1, 1), (8, 8), (9, 9), (16, 16), (17, 9), (15, 33), (33, 15), (48, 32), (70, 37), (257, 3), (3, 257), (640, 33), (64, 64),
         (400, 304), (1030, 70)]
CONTENTS = ("spread", "noise", "checker1", "checker3", "ramps", "constant")
SWEEP_QUALITIES = (100, 50, 1)
SWEEP_CONTENTS = ("noise", "checker1", "checker3")
SWEEP_SIZES = [(17, 9), (64, 64), (400, 304)]
# (w, h, noise seed) at quality 100: the scan's last byte is 0xFF
LAST_FF = [(8, 8, 10), (8, 8, 59), (8, 8, 83), (3, 5, 11)]
MAX_W, MAX_H = 1030, 304  # one encoder object serves every size


def image(w, h, kind, seed=1):
    """h x w x 3 uint8, B,G,R."""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "spread":  # preview_cases.content's skewed spread, another seed per channel (it needs two columns: cropped below that)
        return np.stack([PC.content("spread", max(w, 2), h, 8, seed=c)[:, :w] for c in range(3)], axis=-1).astype(np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "checker1":
        return np.repeat((((xx + yy) & 1) * 255)[..., None], 3, axis=-1).astype(np.uint8)
    if kind == "checker3":
        return np.repeat((((xx // 3 + yy // 3) & 1) * 255)[..., None], 3, axis=-1).astype(np.uint8)
    if kind == "ramps":  # B along x, G along y, R along the diagonal
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], axis=-1).astype(np.uint8)
    assert kind == "constant"
    return np.full((h, w, 3), (31, 200, 90), np.uint8)


def cases():
    """(w, h, content, quality, seed) of every case: quality 95 for every size x content, the quality sweep, the LAST_FF cases."""
    out = [(w, h, c, 95, 1) for w, h in SIZES for c in CONTENTS]
    out += [(w, h, c, q, 1) for q in SWEEP_QUALITIES for c in SWEEP_CONTENTS for w, h in SWEEP_SIZES]
    out += [(w, h, "noise", 100, s) for w, h, s in LAST_FF]
    return out


def case_image(case):
    w, h, kind, _, seed = case
    return image(w, h, kind, seed)


def n_blocks(w, h):
    return 6 * ((w + 15) // 16) * ((h + 15) // 16)


@functools.lru_cache(maxsize=None)
def host_tool():
    """tools/jpeg_host_encode: jpegio::encode and its two halves behind a main(), g++ -O2, no sanitizer."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "jpeg_host_encode"])
    return os.path.join(ROOT, "tools", "jpeg_host_encode")


def host_encode(bgr, quality):
    """(file, coefficients n x 64 int16, bit lengths n uint32) of the host writer."""
    h, w = bgr.shape[:2]
    with tempfile.TemporaryDirectory(prefix="s360_jpeg_") as d:
        src, dst, blk = os.path.join(d, "in.bgr"), os.path.join(d, "out.jpg"), os.path.join(d, "blocks.bin")
        np.ascontiguousarray(bgr, np.uint8).tofile(src)
        r = subprocess.run([host_tool(), src, str(w), str(h), dst, str(quality), "--blocks", blk], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        raw = open(blk, "rb").read()
        n = n_blocks(w, h)
        assert len(raw) == n * 64 * 2 + n * 4
        coef = np.frombuffer(raw[:n * 128], np.int16).reshape(n, 64)
        bits = np.frombuffer(raw[n * 128:], np.uint32)
        return open(dst, "rb").read(), coef, bits


@functools.lru_cache(maxsize=None)
def host_case(case):
    """host_encode of a case; computed once, never written to (the arrays are read-only views of bytes)."""
    return host_encode(case_image(case), case[3])


def pil_encode(bgr, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def scan_of(data):
    """The entropy-coded segment of a file: between the SOS header and the EOI marker."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        p += 2 + n
        if m == 0xDA:
            assert data[-2:] == b"\xff\xd9"
            return data[p:-2]
