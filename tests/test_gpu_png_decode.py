"""Banded PNG files inflated and unfiltered on the device (surround360_amd/csrc/png_decode.hip, include/s360_png_decode.h) and
previous-frame state handed in as such files.

The oracles are not ours: PIL (libpng + zlib) decodes every file the device decodes, and the files that exercise the general
inflate are made here with Python's zlib in the banded layout (one raw-deflate segment per band, chunk "sbNd"). The per-call
counters show which path ran: the fast path (speculative, a wave per band) on what the device encoder and Z_RLE write, the general
path (serial) on distances above 1 and on several blocks per band. Replayed on the CPU emulation by tests/test_cpu_png_decode.py."""
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import rigutil
import test_gpu_png as T
import test_gpu_state_png as SP
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

CAM, EQR_W, EQR_H = T.CAM, T.EQR_W, T.EQR_H
SIG = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def make_ctx(path, eqr=(EQR_W, EQR_H)):
    c = R.Context(R.RigDescription(path), R.make_params(eqr_width=eqr[0], eqr_height=eqr[1], enable_top=1, enable_bottom=1,
                                                        final_eqr_width=240, final_eqr_height=240, sharpening=0.25))
    c.rig_path = path
    return c


@pytest.fixture(scope="module")
def rig_path(tmp_path_factory, rig_json, s360lib):
    d = tmp_path_factory.mktemp("rig_png_decode")
    return rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)


@pytest.fixture(scope="module")
def ctx(rig_path):
    c = make_ctx(rig_path)
    yield c
    c.close()


def pil_pixels(png):
    """The file's pixels as PIL decodes them, in our channel order (B,G,R or B,G,R,A)."""
    Image.MAX_IMAGE_PIXELS = None
    a = np.asarray(Image.open(io.BytesIO(png)))
    return np.ascontiguousarray(a[..., [2, 1, 0, 3]] if a.shape[2] == 4 else a[..., ::-1])


def encode(ctx, a, band_rows=None):
    if band_rows is None:
        return ctx.encode_png(a)
    os.environ["S360_PNG_BAND_ROWS"] = str(band_rows)
    try:
        return ctx.encode_png(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]


def nbands(png):
    return len(T.chunks(png)) - 5  # IHDR, sbNd, zlib header, ..., Adler-32, IEND


def all_cases():
    c4 = SP.cases4()
    out = {}
    for k, a in c4.items():
        out[k + "_4"] = a
        out[k + "_3"] = np.ascontiguousarray(a[..., :3])
    return out


# ---- round trip of device-encoded files -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(all_cases()))
def test_round_trip_of_device_encoded_files(ctx, name):
    a = all_cases()[name]
    png = encode(ctx, a)
    assert R.png_decodable(png)[:3] == (a.shape[1], a.shape[0], a.shape[2])
    got = ctx.decode_png_batch([png])[0]
    assert got.shape == a.shape
    assert np.array_equal(got, a), "%d bytes differ" % int((got != a).sum())
    assert np.array_equal(got, pil_pixels(png))
    fast, general, stored, rounds = ctx.png_decode_stats()
    print("%s: fast %d general %d stored %d, most rounds %d" % (name, fast, general, stored, rounds))
    assert general == 0 and fast + stored == nbands(png)
    if name.startswith("noise"):
        assert stored > 0
    if name.startswith("smooth"):
        assert fast > 0 and 1 <= rounds <= 65


@pytest.mark.parametrize("band_rows", [1, 3, 7, 1000])
@pytest.mark.parametrize("ch", [3, 4])
def test_band_heights(ctx, band_rows, ch):
    rng = np.random.default_rng(band_rows)
    a = np.repeat(rng.integers(0, 256, (40, 31, ch), dtype=np.uint8), 3, axis=1)  # 40 x 93
    png = encode(ctx, a, band_rows)
    assert R.png_decodable(png) == (93, 40, ch, min(band_rows, 40))
    got = ctx.decode_png_batch([png])[0]
    assert np.array_equal(got, a) and np.array_equal(got, pil_pixels(png))
    fast, general, stored, _ = ctx.png_decode_stats()
    assert general == 0 and fast + stored == -(-40 // min(band_rows, 40))


def test_fifteen_bit_codes_on_the_fast_path(ctx):
    """The device encoder's own length-limited code (tests/test_gpu_state_png.py::test_rgba_length_limit): one band, one dynamic
    block whose longest codes have 15 bits — longer than the decoder's lookup table reaches."""
    a, _ = fifteen_bit_file(26, 1500)
    png = encode(ctx, a, a.shape[0])
    assert nbands(png) == 1
    lit, dist = dynamic_code_lengths(T.chunks(png)[3][1])
    assert max(lit) == 15
    got = ctx.decode_png_batch([png])[0]
    assert np.array_equal(got, a) and np.array_equal(got, pil_pixels(png))
    assert ctx.png_decode_stats()[:3] == (1, 0, 0)


def test_one_batch_of_mixed_sizes_and_channel_counts(ctx):
    cs = all_cases()
    order = ["one_pixel_4", "smooth_4", "noise_3", "flat_4", "one_column_3", "mixed_3", "one_row_4", "one_pixel_4"]
    files = [encode(ctx, cs[k]) for k in order]
    single = [ctx.decode_png_batch([f])[0] for f in files]
    got = ctx.decode_png_batch(files)
    fast, general, stored, _ = ctx.png_decode_stats()
    assert general == 0 and fast + stored == sum(nbands(f) for f in files)
    for k, g, s in zip(order, got, single):
        assert g.shape == cs[k].shape and np.array_equal(g, s) and np.array_equal(g, cs[k]), k


# ---- files made with Python's zlib in the banded layout ---------------------------------------------------------------------
def chunk(typ, data):
    return len(data).to_bytes(4, "big") + typ + data + zlib.crc32(typ + data).to_bytes(4, "big")


def filtered(a, ftype=1):
    """The scanlines of an 8-bit RGB(A) file of the B,G,R(,A) image `a`, every row with filter `ftype` (0 None, 1 Sub)."""
    c = a.shape[2]
    rgb = a[:, :, [2, 1, 0, 3] if c == 4 else [2, 1, 0]].astype(np.int16)
    f = rgb.copy()
    if ftype == 1:
        f[:, 1:] -= rgb[:, :-1]
    f = (f & 255).astype(np.uint8).reshape(a.shape[0], -1)
    return np.concatenate([np.full((a.shape[0], 1), ftype, np.uint8), f], axis=1)


def banded_file(w, h, c, band_rows, segments, scanlines, adler=None, declared_rows=None):
    """The container around the bands' raw-deflate `segments`."""
    ihdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 6 if c == 4 else 2, 0, 0, 0])
    ad = zlib.adler32(scanlines) if adler is None else adler
    return (SIG + chunk(b"IHDR", ihdr) + chunk(b"sbNd", (declared_rows or band_rows).to_bytes(4, "big")) + chunk(b"IDAT", b"\x78\x01") +
            b"".join(chunk(b"IDAT", s) for s in segments) + chunk(b"IDAT", ad.to_bytes(4, "big")) + chunk(b"IEND", b""))


def zlib_banded(a, band_rows, level, strategy, pieces=1, ftype=1):
    """`a` as a banded file whose bands zlib deflates: a compressobj per band (a band's matches stay inside the band), closed by
    Z_SYNC_FLUSH, the last one by Z_FINISH; pieces > 1: the band is fed in that many pieces with Z_FULL_FLUSH between them."""
    f = filtered(a, ftype)
    h = a.shape[0]
    segs = []
    for y0 in range(0, h, band_rows):
        raw = f[y0:y0 + band_rows].tobytes()
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        z = b""
        step = -(-len(raw) // pieces)
        for k in range(pieces):
            z += co.compress(raw[k * step:(k + 1) * step])
            if k + 1 < pieces:
                z += co.flush(zlib.Z_FULL_FLUSH)
        z += co.flush(zlib.Z_FINISH if y0 + band_rows >= h else zlib.Z_SYNC_FLUSH)
        segs.append(z)
    return banded_file(a.shape[1], h, a.shape[2], band_rows, segs, f.tobytes())


def repeated_image(c=4):
    rng = np.random.default_rng(21)
    return np.repeat(rng.integers(0, 256, (40, 31, c), dtype=np.uint8), 3, axis=1)  # 40 x 93, every pixel three times


def smooth_image(c=4):
    rng = np.random.default_rng(22)
    h, w = 64, 257
    yy, xx = np.mgrid[0:h, 0:w]
    col = ((np.sin(xx * 0.05)[..., None] * np.cos(yy * 0.07)[..., None] * 90 + 128) + rng.integers(-2, 3, (h, w, 3))).clip(0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.dstack([col, np.full((h, w), 255, np.uint8)])) if c == 4 else col


def far_image():
    """72 rows of 300 pixels that repeat every 20 rows: 1201 bytes a line, so a row's match lies 24 020 bytes back — further than the
    decoder's 16 KB output window, in a band of 86 KB."""
    rng = np.random.default_rng(23)
    return np.ascontiguousarray(np.tile(rng.integers(0, 256, (20, 300, 4), dtype=np.uint8), (4, 1, 1))[:72])


def run_image():
    flat = np.zeros((2, 500, 4), np.uint8)
    flat[:] = 7  # with filter type 0: 2000 equal bytes per row
    return flat


class BitReader:
    def __init__(self, data):
        self.d, self.p = data, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << i
            self.p += 1
        return v


def dynamic_code_lengths(seg):
    """The literal/length and distance code lengths of the dynamic block a raw-deflate segment starts with (RFC 1951, 3.2.7)."""
    r = BitReader(seg)
    r.bits(1)
    assert r.bits(2) == 2, "not a dynamic block"
    hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = r.bits(3)
    codes, code = {}, 0  # (length, code) -> symbol
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in codes:
            c = (c << 1) | r.bits(1)
            n += 1
            assert n <= 7
        s = codes[(n, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + r.bits(2))
        elif s == 17:
            lens += [0] * (3 + r.bits(3))
        else:
            lens += [0] * (11 + r.bits(7))
    return lens[:hlit], lens[hlit:hlit + hdist]


def fifteen_bit_file(terms, w):
    """Literal frequencies in Fibonacci proportions (tests/test_gpu_png.py::test_length_limit) under Z_HUFFMAN_ONLY: zlib's
    length-limited code uses all 15 bits. 19 terms are 10 945 literals, which zlib sends as one block (its symbol buffer holds
    16 383) but whose code zlib's tie-breaking keeps shallow; 26 terms are 317 810, many blocks in the one band, 15 bits in the
    first already."""
    fib = [1, 1]
    while len(fib) < terms:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(c, 3 + 2 * i, np.uint8) for i, c in enumerate(fib)])
    np.random.default_rng(2).shuffle(vals)
    h = len(vals) // (4 * w)
    a = SP.image_from_filtered4(vals[:h * 4 * w], h, w)
    return a, zlib_banded(a, h, 6, zlib.Z_HUFFMAN_ONLY)


def zlib_cases():
    rep, smo = repeated_image(), smooth_image()
    out = {}
    for nm, a in (("repeated", rep), ("smooth", smo), ("repeated3", repeated_image(3))):
        out[nm + "_rle1"] = (a, zlib_banded(a, 5, 1, zlib.Z_RLE))               # what host/png_io.hpp writes
        out[nm + "_rle1_rows1"] = (a, zlib_banded(a, 1, 1, zlib.Z_RLE))         # small bands: zlib may choose fixed blocks
        out[nm + "_fixed"] = (a, zlib_banded(a, 7, 6, zlib.Z_FIXED))
        out[nm + "_huffman_only"] = (a, zlib_banded(a, 7, 6, zlib.Z_HUFFMAN_ONLY))
        out[nm + "_level0"] = (a, zlib_banded(a, 9, 0, zlib.Z_DEFAULT_STRATEGY))  # stored blocks only
        out[nm + "_one_band"] = (a, zlib_banded(a, 1000, 1, zlib.Z_RLE))        # band_rows >= h
    out["repeated_level9"] = (rep, zlib_banded(rep, 10, 9, zlib.Z_DEFAULT_STRATEGY))   # distances above 1, matches that cross rows
    out["repeated_level9_none"] = (rep, zlib_banded(rep, 10, 9, zlib.Z_DEFAULT_STRATEGY, ftype=0))  # filter type 0 rows
    out["smooth_full_flush"] = (smo, zlib_banded(smo, 16, 6, zlib.Z_DEFAULT_STRATEGY, pieces=3))  # several blocks in a band
    out["smooth_rle_full_flush"] = (smo, zlib_banded(smo, 16, 1, zlib.Z_RLE, pieces=4))
    far = far_image()
    out["far_level9"] = (far, zlib_banded(far, 72, 9, zlib.Z_DEFAULT_STRATEGY))      # matches that reach into flushed windows
    out["far_level9_bands"] = (far, zlib_banded(far, 50, 9, zlib.Z_DEFAULT_STRATEGY, ftype=0))
    run = run_image()
    out["run_2000"] = (run, zlib_banded(run, 2, 1, zlib.Z_RLE, ftype=0))         # length-258 tokens
    out["run_2000_level9"] = (run, zlib_banded(run, 2, 9, zlib.Z_DEFAULT_STRATEGY, ftype=0))
    out["fifteen_bits_many_blocks"] = fifteen_bit_file(26, 1500)
    return out


ZLIB_CASES = None


def zcases():
    global ZLIB_CASES
    if ZLIB_CASES is None:
        ZLIB_CASES = zlib_cases()
    return ZLIB_CASES


def test_the_zlib_files_are_what_they_claim():
    """On the CPU: the 15-bit file's code is 15 bits deep, the level-9 file has distance codes above distance 1, the level-0 file
    only stored blocks, the full-flush file several blocks in a band."""
    zc = zcases()
    assert nbands(zc["fifteen_bits_many_blocks"][1]) == 1
    lit, dist = dynamic_code_lengths(T.chunks(zc["fifteen_bits_many_blocks"][1])[3][1])
    assert max(lit) == 15
    seg9 = T.chunks(zc["repeated_level9"][1])[3][1]
    lit9, dist9 = dynamic_code_lengths(seg9)
    assert any(dist9[1:])
    # the far file's rows are random bytes that repeat 20 rows (24 020 bytes) further down and nowhere else: 20 rows of it cannot
    # shrink, and the band is far below its 86 KB only if the other 52 rows went out as matches at that distance
    segf = T.chunks(zc["far_level9"][1])[3][1]
    assert 20 * 1201 < len(segf) < 20 * 1201 + 4096 and nbands(zc["far_level9"][1]) == 1
    assert (T.chunks(zc["repeated_level0"][1])[3][1][0] >> 1) & 3 == 0
    for nm, (a, png) in zc.items():
        assert np.array_equal(pil_pixels(png), a), nm


@pytest.mark.parametrize("name", list(zlib_cases()))
def test_zlib_made_files_decode_to_what_pil_decodes(ctx, name):
    a, png = zcases()[name]
    assert R.png_decodable(png)[:3] == (a.shape[1], a.shape[0], a.shape[2])
    got = ctx.decode_png_batch([png])[0]
    want = pil_pixels(png)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    fast, general, stored, rounds = ctx.png_decode_stats()
    print("%s: fast %d general %d stored %d, most rounds %d" % (name, fast, general, stored, rounds))
    assert fast + general + stored == nbands(png)
    if "level0" in name:
        assert stored == nbands(png)
    if "level9" in name or "full_flush" in name or "many_blocks" in name:
        assert general > 0
    if name.endswith("_huffman_only"):
        assert fast == nbands(png)


def test_the_general_path_runs_in_a_batch_of_all_zlib_files(ctx):
    names = list(zcases())
    got = ctx.decode_png_batch([zcases()[n][1] for n in names])
    fast, general, stored, rounds = ctx.png_decode_stats()
    assert general > 0 and fast > 0 and stored > 0
    assert fast + general + stored == sum(nbands(zcases()[n][1]) for n in names)
    for n, g in zip(names, got):
        assert np.array_equal(g, zcases()[n][0]), n
    hist = ctx.png_decode_round_histogram()
    assert sum(hist) == fast and max(i for i, v in enumerate(hist) if v) == rounds


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def pil_file(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG", **kw)
    return b.getvalue()


def not_ours(ctx):
    a = SP.cases4()["smooth"]
    good = ctx.encode_png(a)
    ch = T.chunks(good)
    assert len(ch) > 7
    one_missing = SIG + b"".join(chunk(t, d) for i, (t, d) in enumerate(ch) if i != 4)
    sixteen = SIG + chunk(b"IHDR", ch[0][1][:8] + b"\x10" + ch[0][1][9:]) + good[33:]
    interlaced = SIG + chunk(b"IHDR", ch[0][1][:12] + b"\x01") + good[33:]
    grey = SIG + chunk(b"IHDR", ch[0][1][:9] + b"\x00" + ch[0][1][10:]) + good[33:]
    return {"pil": pil_file(a[..., [2, 1, 0, 3]]), "sixteen_bit": sixteen, "interlaced": interlaced, "one_band_missing": one_missing,
            "greyscale": grey, "pil_16": pil_file((np.arange(64, dtype=np.uint16) * 900).reshape(8, 8)), "empty": b"", "truncated": good[:40]}


def test_files_of_other_writers_are_refused(ctx):
    good = ctx.encode_png(SP.cases4()["one_row"])
    want = ctx.decode_png_batch([good])[0]
    for nm, f in not_ours(ctx).items():
        assert R.png_decodable(f) is None, nm
        assert "not a banded PNG file" in R.lib().s360_last_error(None).decode(), nm
        out = [np.full(want.size, 0xA5, np.uint8), np.full(1 << 20, 0xA5, np.uint8)]
        with pytest.raises(R.S360Error, match="image 1"):
            ctx.decode_png_batch([good, f], outs=out)
        assert (out[0] == 0xA5).all() and (out[1] == 0xA5).all(), nm  # nothing was written
        assert ctx.png_decode_failure() == (1, 1), nm
    assert np.array_equal(ctx.decode_png_batch([good])[0], want)


def test_a_buffer_one_byte_short_is_refused(ctx):
    a = SP.cases4()["mixed"]
    png = ctx.encode_png(a)
    out = [np.full(a.size, 0xA5, np.uint8)]
    with pytest.raises(R.S360Error, match="image 0.*too small"):
        ctx.decode_png_batch([png], caps=[a.size - 1], outs=out)
    assert (out[0] == 0xA5).all() and ctx.png_decode_failure() == (0, 2)
    assert np.array_equal(ctx.decode_png_batch([png], caps=[a.size], outs=out)[0], a)
    assert ctx.png_decode_failure() == (-1, 0)


# ---- damaged but well-formed files -----------------------------------------------------------------------------------------
def damaged_files(ctx):
    noise = SP.cases4()["noise"]      # stored bands
    good = ctx.encode_png(noise)
    ch = T.chunks(good)
    rebuild = lambda c: SIG + b"".join(chunk(t, d) for t, d in c)  # noqa: E731
    out = {}
    c = list(ch)
    c[-2] = (b"IDAT", bytes([c[-2][1][0] ^ 1]) + c[-2][1][1:])
    out["adler_changed"] = rebuild(c)
    c = list(ch)
    d = bytearray(c[3][1])
    assert (d[0] >> 1) & 3 == 0  # a stored block: 5 bytes of header, the filter byte, pixels
    d[9] ^= 0x10
    c[3] = (b"IDAT", bytes(d))
    out["stored_pixel_changed"] = rebuild(c)
    c = list(ch)
    d = bytearray(c[3][1])
    assert d[5] == 1
    d[5] = 2  # the first row's filter byte (the Adler-32 is made to fit: only the filter type is wrong)
    c[3] = (b"IDAT", bytes(d))
    rows = int.from_bytes(ch[1][1], "big")
    f = bytearray(filtered(noise).tobytes())
    f[0] = 2
    c[-2] = (b"IDAT", zlib.adler32(bytes(f)).to_bytes(4, "big"))
    out["filter_type_2"] = rebuild(c)
    # sbNd rewritten: twice the rows per band are announced for bands that hold `rows` each
    a = SP.cases4()["smooth"]
    os.environ["S360_PNG_BAND_ROWS"] = "10"
    try:
        g2 = ctx.encode_png(a[:40])
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    c2 = T.chunks(g2)
    assert len(c2) == 5 + 4
    c2[1] = (b"sbNd", (20).to_bytes(4, "big"))
    c2 = c2[:3] + c2[3:5] + c2[-2:]  # 2 bands announced at 20 rows each: every segment inflates to 10 rows
    out["band_inflates_short"] = rebuild(c2)
    return out, rows


def test_damaged_files_are_errors_that_name_the_image(ctx):
    bad, _ = damaged_files(ctx)
    cs = SP.cases4()
    g0, g2 = ctx.encode_png(cs["mixed"]), ctx.encode_png(cs["one_column"])
    for nm, f in bad.items():
        assert R.png_decodable(f) is not None, nm  # well-formed: only the device finds out
        with pytest.raises(R.S360Error, match="image 1") as e:
            ctx.decode_png_batch([g0, f, g2])
        print(nm, "->", e.value)
        assert ctx.png_decode_failure() == (1, 3), nm
        if nm == "filter_type_2":
            assert "unsupported filter" in str(e.value)
        if nm in ("adler_changed", "stored_pixel_changed"):
            assert "Adler-32" in str(e.value)
        if nm == "band_inflates_short":
            assert "less output" in str(e.value)
        got = ctx.decode_png_batch([g0, g2])  # the other images of the batch decode in a following call
        assert np.array_equal(got[0], cs["mixed"]) and np.array_equal(got[1], cs["one_column"]), nm


# ---- frame level ------------------------------------------------------------------------------------------------------------
FLOWS_SIDE = ("flow_l_to_r", "flow_r_to_l")


# The small rig of tests/test_gpu_state_png.py, whose 36-pixel overlaps are below the flow pyramid's smallest level (its flows are
# zero with or without a previous frame), and the rig of the host-program tests (tests/refprog.py), on which the previous state
# changes frame 1.
RIGS = {"small": (CAM, (EQR_W, EQR_H)), "flowing": (256, (504, 252))}


@pytest.fixture(scope="module", params=list(RIGS))
def frames(request, tmp_path_factory, rig_json, s360lib):
    """Frame 0's state (raw pixels, device-encoded files, flows), frame 1 rendered from it through the existing calls, and frame 1
    rendered with no state."""
    cam, eqr = RIGS[request.param]
    rig_path = rigutil.scaled_rig_json(rig_json, str(tmp_path_factory.mktemp("rig_" + request.param) / "rig.json"), cam / 2048.0)
    mk = lambda: make_ctx(rig_path, eqr)  # noqa: E731
    side, top, bottom = rigutil.frame_inputs(rig_path, cam)
    side2, top2, bottom2 = rigutil.frame_inputs(rig_path, cam, yaw_deg=1.5)
    c = mk()
    names = SP.state_names(c)
    c.upload_frame(side, top, bottom)
    c.render(False)
    raw = {nk: c.get_u8(*nk) for nk in names}
    c.encode_state_pngs(names)
    files = {nk: c.download_state_png(i).tobytes() for i, nk in enumerate(names)}
    npairs = len(side)
    flows = {(n, p): c.get_f32(n, p) for p in range(npairs) for n in FLOWS_SIDE}
    flows.update({("flow_pole", u): c.get_f32("flow_pole", u) for u in range(4)})
    c.close()
    # frame 1 behind the existing calls
    c = mk()
    L = R.lib()
    for p in range(npairs):
        R.check(L.s360_frame_set_prev_side(c.h, p, R._p(flows[("flow_l_to_r", p)]), R._p(flows[("flow_r_to_l", p)]),
                                           R._p(raw[("overlap_l", p)]), R._p(raw[("overlap_r", p)])), c.h)
    for u in range(4):
        R.check(L.s360_frame_set_prev_pole(c.h, u, R._p(flows[("flow_pole", u)]), R._p(raw[("extended_side", u)]),
                                           R._p(raw[("extended_fisheye", u)])), c.h)
    c.upload_frame(side2, top2, bottom2)
    c.render(True)
    want = result_of(c, npairs)
    c.close()
    # ... and frame 1 with no state at all
    c = mk()
    c.upload_frame(side2, top2, bottom2)
    c.render(True)
    nostate = result_of(c, npairs)
    c.close()
    differing = [k for k in want if not np.array_equal(want[k], nostate[k])]
    print("previous state changes:", differing)
    if request.param == "flowing":
        assert len(differing) > 4  # the previous state matters: side flows and pole flows differ
    return dict(mk=mk, side2=side2, top=top2, bottom=bottom2, names=names, files=files, flows=flows, want=want, nostate=nostate,
                npairs=npairs)


def result_of(c, npairs):
    out = {"equirect": c.download_equirect()}
    for p in range(npairs):
        for n in FLOWS_SIDE:
            out[(n, p)] = c.get_f32(n, p).view(np.uint32)
    for u in range(4):
        out[("flow_pole", u)] = c.get_f32("flow_pole", u).view(np.uint32)
    return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def hand_in_flows(c, fr):
    for (n, k), f in fr["flows"].items():
        c.set_prev_flow(n, k, f)


def hand_in_images(c, fr):
    c.set_prev_images_png(fr["names"], [fr["files"][nk] for nk in fr["names"]])
    fast, general, stored, _ = c.png_decode_stats()
    assert general == 0 and fast > 0 and fast + stored == sum(nbands(f) for f in fr["files"].values())


@pytest.mark.parametrize("order", ["images_first", "flows_first"])
def test_frame_resumed_from_files_equals_frame_resumed_from_pixels(frames, order):
    c = frames["mk"]()
    try:
        if order == "images_first":
            hand_in_images(c, frames)
            hand_in_flows(c, frames)
        else:
            hand_in_flows(c, frames)
            hand_in_images(c, frames)
        c.upload_frame(frames["side2"], frames["top"], frames["bottom"])
        c.render(True)
        assert same(result_of(c, frames["npairs"]), frames["want"])
    finally:
        c.close()


def test_images_alone_are_no_previous_state(frames):
    c = frames["mk"]()
    try:
        hand_in_images(c, frames)
        c.upload_frame(frames["side2"], frames["top"], frames["bottom"])
        c.render(True)
        assert same(result_of(c, frames["npairs"]), frames["nostate"])
    finally:
        c.close()


def test_frame_level_refusals(frames):
    c = frames["mk"]()
    try:
        f = frames["files"]
        with pytest.raises(R.S360Error):
            c.set_prev_images_png([("bottom_image", 0)], [f[("overlap_l", 0)]])  # this context runs no pole removal
        with pytest.raises(R.S360Error):
            c.set_prev_images_png([("no_such_image", 0)], [f[("overlap_l", 0)]])
        with pytest.raises(R.S360Error):
            c.set_prev_images_png([("overlap_l", 1000)], [f[("overlap_l", 0)]])
        with pytest.raises(R.S360Error, match="wrong size"):
            c.set_prev_images_png([("overlap_l", 0)], [f[("extended_side", 0)]])
        with pytest.raises(R.S360Error, match="image 0"):
            c.set_prev_images_png([("overlap_l", 0)], [b"not a file"])
        with pytest.raises(R.S360Error):
            c.set_prev_flow("flow_sideways", 0, frames["flows"][("flow_l_to_r", 0)])
        c.set_partition(0, 2)
        with pytest.raises(R.S360Error, match="outside the block"):
            c.set_prev_images_png([("overlap_l", 3)], [f[("overlap_l", 3)]])
        with pytest.raises(R.S360Error, match="outside the block"):
            c.set_prev_flow("flow_l_to_r", 3, frames["flows"][("flow_l_to_r", 3)])
        # a damaged file: nothing is marked as handed in
        bad = bytearray(f[("overlap_l", 0)])
        ch = T.chunks(bytes(bad))
        ch[-2] = (b"IDAT", bytes(4))
        bad = SIG + b"".join(chunk(t, d) for t, d in ch)
        c.set_partition(0, frames["npairs"])
        hand_in_flows(c, frames)
        names = frames["names"]
        with pytest.raises(R.S360Error, match="image 0.*Adler-32"):
            c.set_prev_images_png(names, [bad] + [f[nk] for nk in names[1:]])
        c.upload_frame(frames["side2"], frames["top"], frames["bottom"])
        c.render(True)
        assert same(result_of(c, frames["npairs"]), frames["nostate"])
    finally:
        c.close()
