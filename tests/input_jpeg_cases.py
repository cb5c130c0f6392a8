"""Cases of the device JPEG decoder's tests (tests/test_gpu_input_jpeg.py, tests/test_cpu_input_jpeg.py): sizes, contents, qualities,
samplings, writers, and the two byte oracles — host/jpeg_io.hpp's jpegio::decode_any behind tools/jpeg_host_decode, and PIL's
Image.open(...).convert("RGB") (libjpeg-turbo). No reference data is needed: everything is byte equality against those two.

Sizes, each for a way the kernels can go wrong: 1 x 1 (one MCU, every block but one a dummy), 8 x 8, 16 x 16 (exactly one 4:2:0 MCU),
17 x 16 (a dummy luma column), 33 x 17 (a dummy row and column, odd chroma size), 37 x 53, 64 x 64, 200 x 128, 400 x 304 (2850 blocks
at 4:2:0: more than one IDCT / DC workgroup by a non-multiple), 1030 x 304 (a scan of noise longer than one synchronisation
workgroup's 128 KiB and than one unstuffing workgroup's 16 KiB, by non-multiples: asserted in test_cpu_input_jpeg.py).

The kernels' constants (surround360_amd/csrc/jpeg_decode.hpp) these cases must exceed: SUB_BITS = 4096 bits a subsequence,
SYNC_THREADS = 256 subsequences a workgroup, UNSTUFF_SEG = 16384 stuffed bytes a workgroup."""
import functools
import io
import os
import subprocess
import tempfile

import numpy as np

import jpeg_cases as JC

ROOT = JC.ROOT
SYNC_THREADS, UNSTUFF_SEG = 256, 16384
SUB_BITS = int(os.environ.get("S360_JPEG_SUB_BITS", "4096"))  # (the library's developer switch: the CPU replay also runs a small S)

SIZES = [(1, 1), (8, 8), (16, 16), (17, 16), (33, 17), (37, 53), (64, 64), (200, 128), (400, 304), (1030, 304)]
CONTENTS = ("noise", "checker1", "constant", "ramps", "photo")
QUALITIES = (30, 75, 95, 100)
SAMPLINGS = (2, 1, 0)  # PIL's numbers: 4:2:0, 4:2:2, 4:4:4
CROSS_SIZES = [(37, 53), (200, 128)]  # every content x quality x sampling x optimize at these


def image(w, h, kind, seed=1):
    """h x w x 3 uint8, B,G,R: jpeg_cases' contents, plus "photo" — smooth shapes with mild noise."""
    if kind != "photo":
        return JC.image(w, h, kind, seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    base = np.stack([128 + 90 * np.sin(xx / 17.0 + c) * np.cos(yy / 23.0 - c) + 30 * np.sin((xx + 2 * yy) / 5.0 + c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 4.0, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_encode(bgr, quality, sampling, optimize):
    from PIL import Image, ImageFile
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)  # (optimize=True needs the whole file in one buffer)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=quality, subsampling=sampling, optimize=optimize)
    return b.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


@functools.lru_cache(maxsize=None)
def pil_cases():
    """((w, h, content, quality, sampling, optimize), file) of every PIL-written case: every size x content x sampling with quality
    and optimize cycling, and the full cross at CROSS_SIZES. Computed once; the files are bytes."""
    keys = []
    i = 0
    for w, h in SIZES:
        for c in CONTENTS:
            for s in SAMPLINGS:
                keys.append((w, h, c, QUALITIES[i % 4], s, bool((i // 4) & 1)))
                i += 1
    for w, h in CROSS_SIZES:
        keys += [(w, h, c, q, s, o) for c in CONTENTS for q in QUALITIES for s in SAMPLINGS for o in (False, True)]
    keys = list(dict.fromkeys(keys))
    return tuple((k, pil_encode(image(k[0], k[1], k[2]), k[3], k[4], k[5])) for k in keys)


def host_writer_cases():
    """jpeg_cases-style cases (w, h, content, quality, seed) for the host writer and the device encoder: every size, jpeg_cases'
    noise, checker, constant and gradient, the qualities cycling."""
    out = []
    i = 0
    for w, h in SIZES:
        for c in ("noise", "checker1", "constant", "ramps"):
            out.append((w, h, c, QUALITIES[i % 4], 1))
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def host_tool():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "jpeg_host_decode"])
    return os.path.join(ROOT, "tools", "jpeg_host_decode")


def host_decode(files):
    """jpegio::decode_any of every file (bytes) in one process: a list of (h, w, 3) uint8 B,G,R arrays, or the failure message (str)."""
    with tempfile.TemporaryDirectory(prefix="s360_jpegin_") as d:
        lines = []
        for i, f in enumerate(files):
            p = os.path.join(d, "%05d.jpg" % i)
            open(p, "wb").write(bytes(f))
            lines.append("%s %s" % (p, p + ".raw"))
        lst = os.path.join(d, "list.txt")
        open(lst, "w").write("\n".join(lines) + "\n")
        r = subprocess.run([host_tool(), lst], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        res = r.stdout.splitlines()
        assert len(res) == len(files)
        out = []
        for i, ln in enumerate(res):
            if ln.startswith("ok "):
                w, h = (int(v) for v in ln.split()[1:3])
                out.append(np.fromfile(os.path.join(d, "%05d.jpg.raw" % i), np.uint8).reshape(h, w, 3))
            else:
                out.append(ln[5:])
        return out


@functools.lru_cache(maxsize=None)
def pil_case_pixels():
    """jpegio's pixels of every pil_cases() file, computed once and shared; read-only."""
    out = host_decode([f for _, f in pil_cases()])
    for a in out:
        assert not isinstance(a, str), a
        a.setflags(write=False)
    return tuple(out)


def scan_of(data):
    """The entropy-coded segment of a baseline file: between the SOS header and the EOI marker (byte stuffing included)."""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        if m == 0xDA:
            assert data[-2:] == b"\xff\xd9"
            return p + 2 + n, data[p + 2 + n:-2]
        p += 2 + n


def unstuffed_bits(data):
    return 8 * len(scan_of(data)[1].replace(b"\xff\x00", b"\xff"))


def n_blocks(w, h, sampling):
    hs, vs = {2: (2, 2), 1: (2, 1), 0: (1, 1)}[sampling]
    return (-(-w // (8 * hs))) * (-(-h // (8 * vs))) * (hs * vs + 2)


def expected_failure(data):
    """The S360_JPEG_DECODE_FAILURE_* reason include/s360_input_jpeg.h states for a decodable file's scan (0: none), from a serial walk
    of the tokens written here independently of the library: canonical codes from the DHT segments, one token at a time, to the
    end of the bits. 3 invalid code (with at least 16 bits left), 4 run past 63, 5 the scan ends inside a block or token, 6 blocks
    missing at a clean end, 7 bits left over (8 or more, or whole extra blocks), 8 a marker inside the scan."""
    p, huff, comps, sof = 2, {}, [], None
    while True:
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        seg = data[p + 4:p + 2 + n]
        if m == 0xC0:
            sof = (int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[7] >> 4, seg[7] & 15)
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc_th, counts = seg[q], seg[q + 1:q + 17]
                q += 17
                code, table = 0, {}
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = seg[q]
                        code += 1
                        q += 1
                    code <<= 1
                huff[tc_th] = table
        elif m == 0xDA:
            comps = [(seg[2 + 2 * i] >> 4, 0x10 | (seg[2 + 2 * i] & 15)) for i in range(3)]
            p += 2 + n
            break
        p += 2 + n
    end = p
    while not (data[end] == 0xFF and data[end + 1] not in (0,) + tuple(range(0xD0, 0xD8)) + (0xFF,)):
        end += 1
    scan = data[p:end]
    if any(scan[i] == 0xFF and (i + 1 == len(scan) or scan[i + 1] != 0) for i in range(len(scan))):
        return 8
    raw = scan.replace(b"\xff\x00", b"\xff")
    nbits, big, total = 8 * len(raw), int.from_bytes(raw + bytes(4), "big"), 8 * (len(raw) + 4)
    h, w, hs, vs = sof
    per_mcu = [comps[0]] * (hs * vs) + [comps[1], comps[2]]
    want = (-(-w // (8 * hs))) * (-(-h // (8 * vs))) * len(per_mcu)
    pos = begun = zz = blk = 0
    while pos < nbits:
        rem = nbits - pos
        table = huff[per_mcu[blk][1 if zz else 0]]
        tok = next(((ln, table[(ln, (big >> (total - pos - ln)) & ((1 << ln) - 1))]) for ln in range(1, 17)
                    if (ln, (big >> (total - pos - ln)) & ((1 << ln) - 1)) in table), None)
        if tok is None:
            if rem >= 16:
                return 3
            break
        ln, sym = tok
        if ln > rem:
            break
        if zz == 0:
            if sym > 11:
                return 3
            if ln + sym > rem:
                break
            begun, zz, pos = begun + 1, 1, pos + ln + sym
            continue
        r, sz = sym >> 4, sym & 15
        if sz == 0:
            done = r != 15 or zz + 16 > 63
            zz, pos = zz + 16, pos + ln
        else:
            if ln + sz > rem:
                break
            if zz + r > 63:
                return 4
            zz, pos = zz + r + 1, pos + ln + sz
            done = zz > 63
        if done:
            zz, blk = 0, (blk + 1) % len(per_mcu)
    left = nbits - pos
    if begun < want:
        return 6 if zz == 0 and left < 8 else 5
    if begun > want:
        return 7
    return 5 if zz else (7 if left >= 8 else 0)
