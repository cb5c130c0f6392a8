"""16-bit RGB PNG files encoded on the device (k_png_band<6> in surround360_amd/csrc/png.hip, include/s360_isp_png.h): the operator
form s360_encode_png16, and the ISP's result leaving as a finished file without a trip through host memory
(s360_isp_process_png / s360_isp_process_packed_png) — what host/Unpacker --device_png and host/Raw2Rgb --device_png write.

The oracle is a decoder that is not ours: the IDAT chunks concatenated go through zlib.decompress (which checks the Adler-32), Sub
at a distance of 6 bytes is undone by refprog.png_unfilter, and all 16 bits of every sample are compared. Beside it every band's
IDAT must inflate on its own as raw deflate to that band's filtered bytes, PIL must open and verify() the file (its 8-bit view of
16-bit RGB, value >> 8, is a second opinion only), and the chunk order and the IHDR bytes are asserted. Replayed on the CPU
emulation by tests/test_cpu_png16.py."""
import ctypes as C
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import isputil
import refprog
import rigutil
import test_gpu_png as T
from surround360_amd import isp as I
from surround360_amd import render as R
from surround360_amd._capi import ERR_INVALID_ARG

pytestmark = pytest.mark.gpu

CAM, EQR_W, EQR_H = T.CAM, T.EQR_W, T.EQR_H


@pytest.fixture(scope="module")
def ctx(tmp_path_factory, rig_json, s360lib):
    d = tmp_path_factory.mktemp("rig_png16")
    path = rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)
    c = R.Context(R.RigDescription(path), R.make_params(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1,
                                                        final_eqr_width=240, final_eqr_height=240, sharpening=0.25))
    yield c
    c.close()


def png_bytes16(bgr16):
    """The unfiltered bytes of a 16-bit RGB PNG's scanlines: samples in R,G,B order, high byte first (h x 6w uint8)."""
    rgb = bgr16[:, :, ::-1]
    return np.stack([rgb >> 8, rgb & 255], axis=-1).astype(np.uint8).reshape(bgr16.shape[0], -1)


def filtered_scanlines16(bgr16):
    """The bytes a PNG encoder deflates for a 16-bit RGB image with the Sub filter (distance 6) on every row."""
    b = png_bytes16(bgr16).astype(np.int16)
    f = b.copy()
    f[:, 6:] -= b[:, :-6]
    return np.concatenate([np.ones((bgr16.shape[0], 1), np.uint8), (f & 255).astype(np.uint8)], axis=1)


def image_from_filtered16(f, h, w):
    """The B,G,R uint16 image whose Sub-filtered bytes are f (h x 6w): running sums per byte of the pixel along a row."""
    b = (np.cumsum(f.reshape(h, w, 6).astype(np.int64), axis=1) & 255).astype(np.uint16)
    rgb = (b[..., 0::2] << 8) | b[..., 1::2]
    return np.ascontiguousarray(rgb[:, :, ::-1])


def decode16(png):
    """The decoder that is not ours: (B,G,R uint16 image, rows per band, the bands' IDAT payloads)."""
    assert png[:8] == bytes([137, 80, 78, 71, 13, 10, 26, 10])
    ch = T.chunks(png)
    assert [t for t, _ in ch[:3]] == [b"IHDR", b"sbNd", b"IDAT"] and ch[-1][0] == b"IEND" and ch[2][1] == b"\x78\x01"
    w, h = int.from_bytes(ch[0][1][:4], "big"), int.from_bytes(ch[0][1][4:8], "big")
    assert ch[0][1][8:10] == bytes([16, 2]) and ch[0][1][10:] == bytes(3)  # 16 bits, colour type 2
    rows = int.from_bytes(ch[1][1], "big")
    bands = ch[3:-2]
    assert all(t == b"IDAT" for t, _ in bands) and len(bands) == -(-h // rows)
    assert ch[-2][0] == b"IDAT" and len(ch[-2][1]) == 4  # the Adler-32
    raw = zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT"))
    lines = np.frombuffer(raw, np.uint8).reshape(h, 1 + 6 * w)
    px = refprog.png_unfilter(lines, 6).reshape(h, w, 3, 2).astype(np.uint16)
    return ((px[..., 0] << 8) | px[..., 1])[..., ::-1], rows, [d for _, d in bands]


def decode_check16(png, a):
    png = bytes(png)
    got, rows, bands = decode16(png)
    assert got.shape == a.shape
    assert np.array_equal(got, a), "%d samples differ" % int((got != a).sum())
    line = 1 + 6 * a.shape[1]
    f = filtered_scanlines16(a).tobytes()
    for i, data in enumerate(bands):  # every band is a raw-deflate segment of its own
        d = zlib.decompressobj(-15)
        assert d.decompress(data) + d.flush() == f[i * rows * line:(i + 1) * rows * line], "band %d" % i
    Image.MAX_IMAGE_PIXELS = None
    Image.open(io.BytesIO(png)).verify()  # signature, chunk CRCs
    im = Image.open(io.BytesIO(png))
    assert im.size == (a.shape[1], a.shape[0])
    second = np.asarray(im.convert("RGB"))
    if second.dtype == np.uint8:  # (this Pillow gives 16-bit RGB as value >> 8: a second opinion on the high bytes)
        assert np.array_equal(second[:, :, ::-1], (a >> 8).astype(np.uint8))
    return rows, len(bands)


def smooth16(h, w, rng, noise):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(xx * 0.05)[..., None] * np.cos(yy * 0.03)[..., None] * 20000 + 32768 + np.array([0, 3000, -2500])
    return (base + rng.normal(0, noise, (h, w, 3))).clip(0, 65535).astype(np.uint16)


def cases16():
    rng = np.random.default_rng(16)
    h, w = 97, 333  # odd width: rows on 2-byte boundaries only, 6 w mod 64 != 0
    smooth = smooth16(h, w, rng, 3.0)
    mixed = smooth.copy()
    mixed[20:40] = 0x4D4D          # flat, all bytes equal: runs that cross samples and pixels
    mixed[60:, 100:200] = (0, 0, 0xFFFF)
    mixed[5:15, 30:300] = 0        # all-zero blocks
    mixed[70:90, 220:330] = 0
    const = np.empty((h, w, 3), np.uint16)
    const[:] = (0x00FF, 0xFF00, 0x1234)  # B, G, R: byte order and channel order
    flat = np.full((50, 4100, 3), 0x4141, np.uint16)  # more than two 2048-pixel tiles per row
    return {"smooth": smooth, "mixed": mixed, "const_colour": const, "flat": flat,
            "w2048": smooth16(5, 2048, rng, 3.0), "w2049": smooth16(5, 2049, rng, 3.0),
            "noise": rng.integers(0, 65536, (64, 200, 3), dtype=np.uint16),
            "one_pixel": np.array([[[0x0102, 0xA0B0, 0xFFFE]]], np.uint16),
            "one_column": rng.integers(0, 65536, (300, 1, 3), dtype=np.uint16), "one_row": smooth[:1].copy()}


@pytest.mark.parametrize("name", list(cases16()))
def test_png16_decodes_to_the_input(ctx, name):
    a = cases16()[name]
    png = ctx.encode_png16(a)
    rows, nb = decode_check16(png, a)
    if name == "flat":
        print("png16 flat: %d bytes of file for %d bytes of pixels" % (len(png), a.nbytes))
        assert len(png) < a.nbytes // 20  # (1/20 of the pixels' bytes, as the 8-bit tests hold their flat image)
    if name == "noise":  # nothing to gain: stored blocks, a few bytes of framing per band
        assert len(png) <= a.nbytes + a.shape[0] + 17 * nb + 200


@pytest.mark.parametrize("band_rows", [1, 3, 7, 1000])
def test_png16_band_heights(ctx, band_rows):
    rng = np.random.default_rng(band_rows)
    a = np.repeat(rng.integers(0, 65536, (40, 31, 3), dtype=np.uint16), 3, axis=1)  # 40 x 93
    os.environ["S360_PNG_BAND_ROWS"] = str(band_rows)
    try:
        png = ctx.encode_png16(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check16(png, a)
    assert rows == min(band_rows, 40) and nb == -(-40 // rows)


def test_png16_length_limit(ctx):
    """The Fibonacci-frequency image of test_gpu_state_png.py::test_rgba_length_limit at 6 bytes per pixel, one band: the code is
    limited to 15 bits and complete (zlib refuses over-subscribed and incomplete codes)."""
    fib = [1, 1]
    while len(fib) < 26:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(c, 3 + 2 * i, np.uint8) for i, c in enumerate(fib)])
    rng = np.random.default_rng(2)
    rng.shuffle(vals)
    w = 1000
    h = len(vals) // (6 * w)
    a = image_from_filtered16(vals[:h * 6 * w], h, w)
    os.environ["S360_PNG_BAND_ROWS"] = str(h)
    try:
        png = ctx.encode_png16(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check16(png, a)
    assert nb == 1
    assert len(png) < 0.45 * a.nbytes  # ~2.6 bits of entropy per byte: coded, not stored


def test_png16_size_against_zlib_rle_on_camera_sized_bands(ctx):
    """Bands of the size a 2048-wide camera image has (16 rows of 12289 bytes = 196 KB), smooth content + sigma 120 noise: zlib at
    Z_BEST_SPEED / Z_RLE shrinks the filtered bytes to 0.783, so every band takes the dynamic-Huffman path. Measured on the CPU
    emulation (the encoder is deterministic, the emulated library runs the same source): device 616 507 bytes, zlib 616 060 bytes,
    ratio 1.00073 — inside the bound of the 8-bit tests, 1.01 x zlib + 2048, which is therefore the bound here."""
    rng = np.random.default_rng(5)
    h, w = 64, 2048
    a = smooth16(h, w, rng, 120.0)
    os.environ["S360_PNG_BAND_ROWS"] = "16"
    try:
        png = ctx.encode_png16(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check16(png, a)
    assert rows == 16 and nb == 4
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    ref = len(c.compress(filtered_scanlines16(a).tobytes()) + c.flush())
    print("png16 size: device %d bytes, zlib Z_RLE %d bytes, ratio %.5f, zlib / input %.4f" % (len(png), ref, len(png) / ref, ref / a.nbytes))
    assert ref < 0.8 * a.nbytes  # (coded, not stored)
    assert len(png) < 1.01 * ref + 2048, (len(png), ref)


def isp_object(pipe, bpp, resize=1, name="full"):
    return I.CameraIsp(I.config_from_json(isputil.CONFIGS[name], bpp, 2, resize, 0, 0, pipe=pipe))


def check_isp_file(ctx, png, px):
    """`png` is the file of the ISP's result `px`: it decodes to exactly that array and equals the operator call's file for it."""
    if px.dtype == np.uint16:
        decode_check16(png, px)
        assert bytes(png) == ctx.encode_png16(px)
    else:
        T.decode_check(bytes(png), px)
        assert bytes(png) == ctx.encode_png(px)


@pytest.mark.parametrize("bpp", [16, 8])
@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("bits", [8, 12])
def test_isp_packed_png_is_the_file_of_the_isps_pixels(ctx, bits, pipe, bpp):
    w, h = 128, 96
    raw = isputil.bayer_frame(w, h, seed=bits + pipe, pattern="RGGB")
    frame = isputil.pack_frame(raw, bits)
    isp = isp_object(pipe, bpp)
    try:
        px = isp.get_image_packed(frame, bits, w, h)
        assert px.shape == (h, w, 3) and px.dtype == (np.uint16 if bpp == 16 else np.uint8) and px.std() > 5
        png = isp.get_png_packed(frame, bits, w, h)
        assert len(png) <= isp.png_bound(w, h)
        check_isp_file(ctx, png, px)
        assert np.array_equal(isp.get_image_packed(frame, bits, w, h), px)  # the object still develops pixels
    finally:
        isp.close()


@pytest.mark.parametrize("bpp", [16, 8])
@pytest.mark.parametrize("pipe,resize", [(0, 1), (1, 1), (0, 2)], ids=["soft", "pipe", "soft_resize2"])
def test_isp_png_from_raw16_and_with_resize(ctx, pipe, resize, bpp):
    w, h = 128, 96
    raw = isputil.bayer_frame(w, h, seed=3 + resize, pattern="RGGB")
    isp = isp_object(pipe, bpp, resize)
    try:
        px = isp.get_image(raw)
        assert px.shape == (h // resize, w // resize, 3)
        bound = isp.png_bound(w, h)
        lib = R.lib()
        assert bound == (lib.s360_png_bound_16 if bpp == 16 else lib.s360_png_bound)(w // resize, h // resize)
        check_isp_file(ctx, isp.get_png(raw), px)
    finally:
        isp.close()


def test_one_isp_object_changing_sizes(ctx):
    """128 x 96, then 256 x 64 (more bands, a longer line), then 128 x 96 again through one object: the encoder's buffers grow only."""
    isp = isp_object(1, 16)
    try:
        for k, (w, h) in enumerate([(128, 96), (256, 64), (128, 96)]):
            raw = isputil.bayer_frame(w, h, seed=20 + k, pattern="RGGB")
            px = isp.get_image(raw)
            check_isp_file(ctx, isp.get_png(raw), px)
    finally:
        isp.close()


def test_refusals(ctx):
    lib = R.lib()
    a = cases16()["smooth"]
    h, w = a.shape[:2]
    guard = 64
    # cap one byte below the bound: refused, the bytes behind `out` untouched
    bound = int(lib.s360_png_bound_16(w, h))
    buf = np.full(bound - 1 + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    assert lib.s360_encode_png16(ctx.h, a.ctypes.data, w, h, buf.ctypes.data, C.c_size_t(bound - 1), C.byref(n)) == ERR_INVALID_ARG
    assert (buf == 0xA5).all()
    assert lib.s360_encode_png16(ctx.h, a.ctypes.data, w, h, buf.ctypes.data, C.c_size_t(bound), C.byref(n)) == 0  # (the guard is room enough)
    decode_check16(buf[:n.value].tobytes(), a)
    raw = isputil.bayer_frame(128, 96, seed=1, pattern="RGGB")
    frame = isputil.pack_frame(raw, 12)
    for bpp in (16, 8):
        isp = isp_object(1, bpp)
        try:
            bound = isp.png_bound(128, 96)
            assert bound > 0
            buf = np.full(bound - 1 + guard, 0xA5, np.uint8)
            for call in (lambda cap: lib.s360_isp_process_png(isp.h, raw.ctypes.data, 128, 96, buf.ctypes.data, C.c_size_t(cap), C.byref(n)),
                         lambda cap: lib.s360_isp_process_packed_png(isp.h, frame.ctypes.data, 12, 128, 96, buf.ctypes.data, C.c_size_t(cap), C.byref(n))):
                assert call(bound - 1) == ERR_INVALID_ARG
                assert (buf == 0xA5).all()
            # w or h of 0
            assert isp.png_bound(0, 96) == 0 and isp.png_bound(128, 0) == 0
            for ww, hh in ((0, 96), (128, 0)):
                assert lib.s360_isp_process_png(isp.h, raw.ctypes.data, ww, hh, buf.ctypes.data, C.c_size_t(buf.size), C.byref(n)) == ERR_INVALID_ARG
                assert lib.s360_isp_process_packed_png(isp.h, frame.ctypes.data, 12, ww, hh, buf.ctypes.data, C.c_size_t(buf.size),
                                                       C.byref(n)) == ERR_INVALID_ARG
            assert (buf == 0xA5).all()
            check_isp_file(ctx, isp.get_png(raw), isp.get_image(raw))  # the refused calls harmed nothing
        finally:
            isp.close()
    assert lib.s360_png_bound_16(0, 5) == 0 and lib.s360_png_bound_16(5, 0) == 0
    for ww, hh in ((0, h), (w, 0)):
        assert lib.s360_encode_png16(ctx.h, a.ctypes.data, ww, hh, buf.ctypes.data, C.c_size_t(buf.size), C.byref(n)) == ERR_INVALID_ARG
    # the batch encoder and the decoder stay 8-bit
    six = np.zeros((4, 4, 6), np.uint8)
    assert lib.s360_png_bound_c(4, 4, 6) == 0
    out = np.zeros(4096, np.uint8)
    one = lambda t, v: (t * 1)(v)  # noqa: E731
    assert lib.s360_encode_png_batch(ctx.h, 1, one(C.c_void_p, six.ctypes.data), one(C.c_int, 4), one(C.c_int, 4), one(C.c_int, 6),
                                     one(C.c_void_p, out.ctypes.data), one(C.c_size_t, out.size), (C.c_size_t * 1)()) == ERR_INVALID_ARG
    assert R.png_decodable(ctx.encode_png16(a)) is None
    assert b"not a banded PNG file of this decoder" in lib.s360_last_error(None)
