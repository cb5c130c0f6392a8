"""PNG files of B,G,R,A images and of many images per launch sequence, encoded on the device (surround360_amd/csrc/png.hip,
include/s360_state_png.h): the temporal state a per-frame caller leaves on disk (TestRenderStereoPanorama.cpp:201-208, 413-416,
PoleRemoval.cpp:118-126) as finished files.

The oracle is a decoder that is not ours, as in tests/test_gpu_png.py: PIL (libpng + zlib) must open every file as RGBA and give
back the pixels that went in, every band must inflate on its own as raw deflate to its rows of Sub-filtered scanlines at filter
distance 4, and host/png_io.hpp must read the file back through its parallel band path and its sequential path. The size is held
against zlib at Z_BEST_SPEED / Z_RLE on the same filtered bytes (the project's criterion for 3 channels). The 3-channel files must
stay byte for byte what they were: tests/golden/png_rgb_digests.json was recorded from the commit in front of the 4-channel
encoder (tests/golden/make_png_rgb_digests.py). Replayed on the CPU emulation by tests/test_cpu_state_png.py."""
import hashlib
import io
import json
import os
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import rigutil
import test_gpu_png as T
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, EQR_W, EQR_H = T.CAM, T.EQR_W, T.EQR_H


@pytest.fixture(scope="module")
def ctx(tmp_path_factory, rig_json, s360lib):
    d = tmp_path_factory.mktemp("rig_state_png")
    path = rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), CAM / 2048.0)
    c = R.Context(R.RigDescription(path), R.make_params(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1,
                                                        final_eqr_width=240, final_eqr_height=240, sharpening=0.25))
    c.rig_path = path
    yield c
    c.close()


def filtered_scanlines4(bgra):
    """The bytes a PNG encoder deflates for an 8-bit RGBA image with the Sub filter (distance 4) on every row."""
    rgba = bgra[:, :, [2, 1, 0, 3]].astype(np.int16)
    f = rgba.copy()
    f[:, 1:] -= rgba[:, :-1]
    f = (f & 255).astype(np.uint8).reshape(bgra.shape[0], -1)
    return np.concatenate([np.ones((bgra.shape[0], 1), np.uint8), f], axis=1)


def image_from_filtered4(f, h, w):
    """The B,G,R,A image whose Sub-filtered R,G,B,A bytes are f (h x 4w): running sums per channel along a row."""
    rgba = np.cumsum(f.reshape(h, w, 4).astype(np.int64), axis=1) & 255
    return np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]].astype(np.uint8))


def decode_check4(png, bgra):
    assert png[:8] == bytes([137, 80, 78, 71, 13, 10, 26, 10])
    Image.MAX_IMAGE_PIXELS = None
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGBA" and im.size == (bgra.shape[1], bgra.shape[0])
    got = np.asarray(im)
    want = bgra[..., [2, 1, 0, 3]]
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    ch = T.chunks(png)
    assert [t for t, _ in ch[:3]] == [b"IHDR", b"sbNd", b"IDAT"] and ch[-1][0] == b"IEND" and ch[2][1] == b"\x78\x01"
    assert ch[0][1][8:10] == bytes([8, 6])  # 8 bits, colour type 6
    rows = int.from_bytes(ch[1][1], "big")
    bands = ch[3:-2]
    assert all(t == b"IDAT" for t, _ in bands) and len(bands) == -(-bgra.shape[0] // rows) and len(ch[-2][1]) == 4
    line = 1 + 4 * bgra.shape[1]
    f = filtered_scanlines4(bgra).tobytes()
    for i, (_, data) in enumerate(bands):
        d = zlib.decompressobj(-15)
        assert d.decompress(data) + d.flush() == f[i * rows * line:(i + 1) * rows * line], "band %d" % i
    return rows, len(bands)


def check_any(png, a):
    return decode_check4(png, a) if a.shape[2] == 4 else T.decode_check(png, a)


def cases4():
    rng = np.random.default_rng(12)
    h, w = 97, 333  # 4 w mod 64 != 0
    yy, xx = np.mgrid[0:h, 0:w]
    col = ((np.sin(xx * 0.05)[..., None] * np.cos(yy * 0.03)[..., None] * 90 + 128) + rng.integers(-3, 4, (h, w, 3))).clip(0, 255).astype(np.uint8)
    alpha = ((xx * 255) // (w - 1)).astype(np.uint8)
    smooth = np.ascontiguousarray(np.dstack([col, alpha]))
    mixed = smooth.copy()
    mixed[20:40, :, :3] = 77
    mixed[60:, 100:200, :3] = (0, 0, 255)
    mixed[5:15, 30:300] = 0     # alpha 0 over zero colour: runs that cross pixels
    mixed[70:90, 220:330] = 0
    const = np.empty((h, w, 4), np.uint8)
    const[..., :3] = (10, 200, 30)
    const[..., 3] = (alpha.astype(np.int32) + rng.integers(0, 3, (h, w))).clip(0, 255)
    flat = np.zeros((50, 4000, 4), np.uint8)  # rows wider than one 3072-pixel tile
    flat[:] = (10, 200, 30, 255)
    return {"smooth": smooth, "mixed": mixed, "const_colour": const, "noise": rng.integers(0, 256, (64, 200, 4), dtype=np.uint8), "flat": flat,
            "one_pixel": np.array([[[9, 8, 7, 6]]], np.uint8), "one_column": rng.integers(0, 256, (300, 1, 4), dtype=np.uint8),
            "one_row": smooth[:1].copy()}


@pytest.mark.parametrize("name", list(cases4()))
def test_rgba_decodes_to_the_input(ctx, name):
    a = cases4()[name]
    png = ctx.encode_png(a)
    rows, nb = decode_check4(png, a)
    if name == "flat":
        assert len(png) < a.size // 20
    if name == "noise":
        assert len(png) <= a.size + a.shape[0] + 17 * nb + 200


@pytest.mark.parametrize("band_rows", [1, 3, 7, 1000])
def test_rgba_band_heights(ctx, band_rows):
    rng = np.random.default_rng(band_rows)
    a = np.repeat(rng.integers(0, 256, (40, 31, 4), dtype=np.uint8), 3, axis=1)  # 40 x 93
    os.environ["S360_PNG_BAND_ROWS"] = str(band_rows)
    try:
        png = ctx.encode_png(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check4(png, a)
    assert rows == min(band_rows, 40) and nb == -(-40 // rows)


def test_rgba_length_limit(ctx):
    """The Fibonacci-frequency image of test_gpu_png.py::test_length_limit at 4 bytes per pixel, one band: the code is limited to
    15 bits and complete (zlib refuses over-subscribed and incomplete codes)."""
    fib = [1, 1]
    while len(fib) < 26:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(c, 3 + 2 * i, np.uint8) for i, c in enumerate(fib)])
    rng = np.random.default_rng(2)
    rng.shuffle(vals)
    w = 1500
    h = len(vals) // (4 * w)
    a = image_from_filtered4(vals[:h * 4 * w], h, w)
    os.environ["S360_PNG_BAND_ROWS"] = str(h)
    try:
        png = ctx.encode_png(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check4(png, a)
    assert nb == 1
    assert len(png) < 0.45 * a.size


def test_rgba_size_is_zlib_rle_size_on_frame_sized_bands(ctx):
    """Bands of the size an 8K frame has (8 rows of 6144 B,G,R,A pixels = 196 KB): within 1 % of zlib's Z_RLE output."""
    rng = np.random.default_rng(5)
    h, w = 64, 6144
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.empty((h, w, 4), np.uint8)
    a[..., :3] = ((np.sin(xx * 0.01)[..., None] * np.cos(yy * 0.13)[..., None] * 90 + 128) + rng.normal(0, 2.0, (h, w, 3))).clip(0, 255)
    a[..., 3] = 255
    a[10:14, 1000:3000] = 0
    os.environ["S360_PNG_BAND_ROWS"] = "8"
    try:
        png = ctx.encode_png(a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]
    rows, nb = decode_check4(png, a)
    assert rows == 8 and nb == 8
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    ref = len(c.compress(filtered_scanlines4(a).tobytes()) + c.flush())
    print("rgba size: device %d bytes, zlib Z_RLE %d bytes" % (len(png), ref))
    assert len(png) < 1.01 * ref + 2048, (len(png), ref)


def test_our_file_reader_reads_rgba_on_both_paths(ctx, tmp_path):
    """host/png_io.hpp with keep_alpha: the parallel band path ("sbNd") and the sequential one give back the input bytes."""
    src = tmp_path / "rd.cpp"
    src.write_text(r'''
#include "png_io.hpp"
int main(int argc, char** argv) {  // argv: in.png out.raw threads
  pngio::g_read_threads = std::atoi(argv[3]);
  pngio::Image im = pngio::read(argv[1], true);
  FILE* f = std::fopen(argv[2], "wb");
  std::fwrite(im.px.data(), 1, im.px.size(), f);
  std::fclose(f);
  return im.c == 4 ? 0 : 1;
}
''')
    exe = str(tmp_path / "rd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "host"), "-o", exe, str(src), "-lz", "-lpthread"])
    a = cases4()["mixed"]
    p = tmp_path / "m.png"
    p.write_bytes(ctx.encode_png(a))
    for threads in ("3", "-1"):
        subprocess.check_call([exe, str(p), str(tmp_path / "m.raw"), threads])
        assert np.array_equal(np.fromfile(str(tmp_path / "m.raw"), np.uint8).reshape(a.shape), a), threads


def test_bad_channel_count_is_refused(ctx):
    a = np.zeros((4, 4, 4), np.uint8)
    for ch in (0, 1, 2, 5):
        assert R.lib().s360_png_bound_c(4, 4, ch) == 0
        with pytest.raises(R.S360Error):
            ctx.encode_png_c(a, channels=ch)
    decode_check4(ctx.encode_png(a), a)


def test_rgb_files_are_byte_for_byte_what_they_were(ctx):
    """SHA-256 of the 3-channel files against the digests recorded in front of the change, through both entry points."""
    with open(os.path.join(ROOT, "tests", "golden", "png_rgb_digests.json")) as f:
        want = json.load(f)
    cs = T.cases()
    assert sorted(want) == ["flat", "mixed", "one_pixel", "smooth"]
    for name, dig in want.items():
        assert hashlib.sha256(ctx.encode_png(cs[name])).hexdigest() == dig, name
        assert hashlib.sha256(ctx.encode_png_c(cs[name], 3)).hexdigest() == dig, name


def test_batch_equals_the_single_image_calls(ctx):
    rng = np.random.default_rng(3)
    c4, c3 = cases4(), T.cases()
    wide = np.zeros((5, 3100, 4), np.uint8)  # wider than one tile, two tiles per row
    wide[..., :3] = ((np.sin(np.arange(3100) * 0.01)[None, :, None] * 100 + 128) + rng.integers(-2, 3, (5, 3100, 3))).clip(0, 255)
    wide[..., 3] = 200
    imgs = [c4["smooth"], c4["one_pixel"], wide, c3["noise"], np.repeat(rng.integers(0, 256, (40, 31, 3), dtype=np.uint8), 3, axis=1)]
    assert [a.shape for a in imgs] == [(97, 333, 4), (1, 1, 4), (5, 3100, 4), (64, 200, 3), (40, 93, 3)]
    files = ctx.encode_png_batch(imgs)
    assert len(files) == len(imgs)
    for a, f in zip(imgs, files):
        assert f == ctx.encode_png(a), a.shape
        check_any(f, a)


def state_names(ctx):
    n_side = len(rigutil.frame_inputs(ctx.rig_path, CAM)[0])
    names = []
    for p in range(n_side):
        names += [("overlap_l", p), ("overlap_r", p)]
    return names + [("extended_side", i) for i in range(4)] + [("extended_fisheye", i) for i in range(4)]


def check_state(ctx, names):
    ctx.encode_state_pngs(names)
    for i, (n, k) in enumerate(names):
        decode_check4(ctx.download_state_png(i).tobytes(), ctx.get_u8(n, k))


def test_frame_state_images(ctx):
    """encode_state_pngs over every pair's overlaps and the pole stage's extended images: every file decodes to get_u8's pixels —
    one frame, a chained second frame, two frame slots, frame pipelining; what cannot be served is refused and harms nothing."""
    side, top, bottom = rigutil.frame_inputs(ctx.rig_path, CAM)
    side2 = [np.ascontiguousarray(s[:, ::-1]) for s in side]
    names = state_names(ctx)
    with pytest.raises(R.S360Error):
        ctx.download_state_png(0)  # nothing encoded yet
    ctx.upload_frame(side, top, bottom)
    ctx.render(False)
    check_state(ctx, names)
    first = ctx.download_state_png(0).tobytes()
    # refused: unknown name, pole removal not run, index out of range, a 1000-byte buffer, a 3-channel name
    for bad in ([("no_such_image", 0)], [("bottom_image", 0)], [("overlap_l", 0), ("overlap_l", 1000)], [("eye_l", 0)]):
        with pytest.raises(R.S360Error):
            ctx.encode_state_pngs(bad)
    with pytest.raises(R.S360Error):
        ctx.download_state_png(len(names))
    with pytest.raises(R.S360Error):
        ctx.download_state_png(-1)
    with pytest.raises(R.S360Error):
        ctx.download_state_png(0, np.empty(1000, np.uint8))
    assert ctx.download_state_png(0).tobytes() == first  # the batch in front of the refused calls is still there
    # a second, chained frame
    ctx.upload_frame(side2, top, bottom)
    ctx.render(True)
    check_state(ctx, names)
    assert ctx.download_state_png(0).tobytes() != first
    # two frame slots with different inputs, each selected in turn
    ctx.set_frame_slots(2)
    ctx.select_frame_slot(0)
    ctx.upload_frame(side2, top, bottom)
    ctx.select_frame_slot(1)
    ctx.upload_frame(side, top, bottom)
    ctx.render_batch(False)
    got = []
    for k in range(2):
        ctx.select_frame_slot(k)
        check_state(ctx, names)
        got.append(ctx.download_state_png(0).tobytes())
    assert got[1] == first and got[0] != got[1]
    ctx.select_frame_slot(0)
    ctx.set_frame_slots(1)
    # frame pipelining: the encode is ordered behind the finish stream on the device
    ctx.set_frame_pipelining(True)
    ctx.upload_frame(side, top, bottom)
    ctx.render(False)
    ctx.upload_frame(side2, top, bottom)
    ctx.render(True)
    check_state(ctx, names)
    ctx.set_frame_pipelining(False)
    ctx.upload_frame(side, top, bottom)
    ctx.render(False)
    check_state(ctx, names)
    assert ctx.download_state_png(0).tobytes() == first
