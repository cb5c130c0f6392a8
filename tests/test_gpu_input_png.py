"""Camera images as banded PNG files, 8- and 16-bit, decoded on the device (include/s360_input_png.h; k_png_unfilter's layout 6 and
its four stores in surround360_amd/csrc/png_decode.hip): the operator form s360_decode_input_png_batch and the frame-level
s360_frame_upload_png, which writes a frame's source slots straight from the files.

The decoders that are not ours: test_gpu_png16.decode16 (zlib + numpy) for all 16 bits of every sample, its `>> 8` for the high
byte a 16-bit file gives without keep16 (png_set_strip_16), PIL for 8-bit files. The files that exercise the general inflate are
made here with Python's zlib in the banded layout at depth 16. At frame level the oracle is the pixel upload: a frame rendered
after upload_frame_png must equal, byte for byte, the frame rendered after upload_frame of the pixels the independent decoder gives.
Replayed on the CPU emulation by tests/test_cpu_input_png.py."""
import os
import zlib

import numpy as np
import pytest

import rigutil
import test_gpu_png as T
import test_gpu_png16 as P16
import test_gpu_png_decode as D
import test_gpu_state_png as SP
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

DAMAGED = 3  # S360_PNG_DECODE_FAILURE_DAMAGED
WIDTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513)  # around the 64-lane scan and the 256-pixel tile carry
HEIGHTS = (1, 2, 41)
BAND_ROWS = (1, 3, 7, 1000)


@pytest.fixture(scope="module")
def rig_path(tmp_path_factory, rig_json, s360lib):
    d = tmp_path_factory.mktemp("rig_input_png")
    return rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), D.CAM / 2048.0)


@pytest.fixture(scope="module")
def ctx(rig_path):
    c = D.make_ctx(rig_path)
    yield c
    c.close()


def with_band_rows(band_rows, fn, *a):
    if band_rows is None:
        return fn(*a)
    os.environ["S360_PNG_BAND_ROWS"] = str(band_rows)
    try:
        return fn(*a)
    finally:
        del os.environ["S360_PNG_BAND_ROWS"]


def encode16(ctx, a, band_rows=None):
    return bytes(with_band_rows(band_rows, ctx.encode_png16, a))


def encode8(ctx, a, band_rows=None):
    return bytes(with_band_rows(band_rows, ctx.encode_png, a))


def decode16_quick(png):
    """decode16 for files whose rows all have filter type 0 or 1, without its per-pixel loop (zlib + a cumulative sum along the
    row): the B,G,R uint16 image. The frame fixtures decode 68 camera images; two of them also go through decode16 itself."""
    ch = T.chunks(png)
    w, h = int.from_bytes(ch[0][1][:4], "big"), int.from_bytes(ch[0][1][4:8], "big")
    assert ch[0][1][8:] == bytes([16, 2, 0, 0, 0])
    lines = np.frombuffer(zlib.decompress(b"".join(d for t, d in ch if t == b"IDAT")), np.uint8).reshape(h, 1 + 6 * w)
    assert (lines[:, 0] <= 1).all()
    b = lines[:, 1:].reshape(h, w, 6).astype(np.int64)
    b = np.where((lines[:, 0] == 1)[:, None, None], np.cumsum(b, axis=1) & 255, b).astype(np.uint16)
    return np.ascontiguousarray(((b[..., 0::2] << 8) | b[..., 1::2])[..., ::-1])


CONTENTS = ("smooth", "flat", "noise", "low_noise_high_flat", "high_noise_low_flat")


def content16(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        return P16.smooth16(h, w, rng, 3.0)
    if kind == "flat":
        return np.full((h, w, 3), 0x4D4D, np.uint16)
    n = rng.integers(0, 256, (h, w, 3)).astype(np.uint16)
    if kind == "noise":
        return (n << 8) | rng.integers(0, 256, (h, w, 3)).astype(np.uint16)
    # a store that keeps only the high byte lanes must still sum the Adler-32 over all six: one half of every sample is noise
    return (0x4D00 | n) if kind == "low_noise_high_flat" else ((n << 8) | 0x4D)


def shapes(full_band_rows=None):
    """(w, h, band_rows): every width at every height; full_band_rows: that band height at h = 41, else the four band heights
    cycle over the widths. Odd widths make a line of odd length, so a row's first pixel takes every offset mod 4 as rows go by."""
    out = []
    for i, w in enumerate(WIDTHS):
        for h in HEIGHTS:
            if h < 41:
                out.append((w, h, (1, 1000)[(i + h) & 1]))
            else:
                out.append((w, h, full_band_rows or BAND_ROWS[i % 4]))
    return out


def first_pixel_offsets(shape_list):
    return {(r * (1 + 6 * w) + 1) & 3 for w, h, _ in shape_list for r in range(h)}


def check_batch16(ctx, images, files):
    """The 16-bit files through one decode call with and without keep16, against decode16."""
    want = []
    for a, f in zip(images, files):
        ref, rows, bands = P16.decode16(f)
        assert np.array_equal(ref, a)
        want.append(ref)
        assert R.input_png_decodable(f) == (a.shape[1], a.shape[0], 3, 16, rows)
    nb = sum(D.nbands(f) for f in files)
    for keep16 in (1, 0):
        got = ctx.decode_input_png_batch(files, keep16=keep16)
        fast, general, stored, rounds = ctx.png_decode_stats()
        assert fast + general + stored == nb
        for g, w_ in zip(got, want):
            ref = w_ if keep16 else (w_ >> 8).astype(np.uint8)
            assert g.dtype == ref.dtype and g.shape == ref.shape
            assert np.array_equal(g, ref), "keep16 %d, %s: %d samples differ" % (keep16, ref.shape, int((g != ref).sum()))
    return fast, general, stored


@pytest.mark.parametrize("kind", CONTENTS)
def test_round_trip_of_device_encoded_16_bit_files(ctx, kind):
    sh = shapes()
    assert first_pixel_offsets(sh) == {0, 1, 2, 3}
    images = [content16(kind, h, w, 1000 * k + w) for k, (w, h, _) in enumerate(sh)]
    files = [encode16(ctx, a, br) for a, (_, _, br) in zip(images, sh)]
    fast, general, stored = check_batch16(ctx, images, files)
    print("%s: fast %d general %d stored %d" % (kind, fast, general, stored))
    assert general == 0
    if kind == "noise":
        assert stored > 0
    if kind in ("smooth", "flat"):
        assert fast > 0


@pytest.mark.parametrize("band_rows", BAND_ROWS)
def test_every_band_height_at_every_width(ctx, band_rows):
    sh = [s for s in shapes(band_rows) if s[1] == 41]
    images = [content16("smooth", h, w, 7 * w + band_rows) for w, h, _ in sh]
    files = [encode16(ctx, a, br) for a, (_, _, br) in zip(images, sh)]
    for f in files:
        assert D.nbands(f) == -(-41 // min(band_rows, 41))
    check_batch16(ctx, images, files)


def test_8_bit_files_through_the_input_decoder(ctx):
    """encode_png files, 3 and 4 channels: the same bytes as decode_png_batch gives, and as PIL decodes; keep16 changes nothing."""
    rng = np.random.default_rng(8)
    files, want = [], []
    for k, (w, h, br) in enumerate(shapes()):
        c = 3 + (k & 1)
        a = np.ascontiguousarray(D.smooth_image(c)[:h, :w]) if w <= 257 else rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        files.append(encode8(ctx, a, br))
        want.append(a)
        assert R.input_png_decodable(files[-1]) == R.png_decodable(files[-1])[:3] + (8, R.png_decodable(files[-1])[3])
    old = ctx.decode_png_batch(files)
    for keep16 in (0, 1):
        got = ctx.decode_input_png_batch(files, keep16=keep16)
        for g, o, a, f in zip(got, old, want, files):
            assert g.dtype == np.uint8 and np.array_equal(g, a) and np.array_equal(g, o) and np.array_equal(g, D.pil_pixels(f))


# ---- files made with Python's zlib in the banded layout, depth 16 -------------------------------------------------------------
def filtered16(a, ftype):
    if ftype == 1:
        return P16.filtered_scanlines16(a)
    return np.concatenate([np.zeros((a.shape[0], 1), np.uint8), P16.png_bytes16(a)], axis=1)


def zlib_banded16(a, band_rows, level, strategy, pieces=1, ftype=1):
    """test_gpu_png_decode.zlib_banded at depth 16: a compressobj per band, Z_SYNC_FLUSH behind every band but the last; pieces > 1:
    Z_FULL_FLUSH between the pieces of a band (several blocks per band)."""
    f = filtered16(a, ftype)
    h, w = a.shape[:2]
    segs = []
    for y0 in range(0, h, band_rows):
        raw = f[y0:y0 + band_rows].tobytes()
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        z, step = b"", -(-len(raw) // pieces)
        for k in range(pieces):
            z += co.compress(raw[k * step:(k + 1) * step])
            if k + 1 < pieces:
                z += co.flush(zlib.Z_FULL_FLUSH)
        z += co.flush(zlib.Z_FINISH if y0 + band_rows >= h else zlib.Z_SYNC_FLUSH)
        segs.append(z)
    ihdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([16, 2, 0, 0, 0])
    return (D.SIG + D.chunk(b"IHDR", ihdr) + D.chunk(b"sbNd", band_rows.to_bytes(4, "big")) + D.chunk(b"IDAT", b"\x78\x01") +
            b"".join(D.chunk(b"IDAT", s) for s in segs) + D.chunk(b"IDAT", zlib.adler32(f.tobytes()).to_bytes(4, "big")) + D.chunk(b"IEND", b""))


def repeated16():
    rng = np.random.default_rng(61)
    return np.repeat(rng.integers(0, 65536, (40, 31, 3), dtype=np.uint16), 3, axis=1)  # 40 x 93, every pixel three times


def zlib_cases16():
    rep = repeated16()
    smo = P16.smooth16(48, 257, np.random.default_rng(62), 3.0)
    return {"repeated_rle1": (rep, zlib_banded16(rep, 5, 1, zlib.Z_RLE)),
            "smooth_rle1": (smo, zlib_banded16(smo, 16, 1, zlib.Z_RLE)),
            "repeated_level9": (rep, zlib_banded16(rep, 10, 9, zlib.Z_DEFAULT_STRATEGY)),           # distances above 1
            "repeated_level9_none": (rep, zlib_banded16(rep, 10, 9, zlib.Z_DEFAULT_STRATEGY, ftype=0)),  # filter type 0 rows
            "smooth_full_flush": (smo, zlib_banded16(smo, 16, 6, zlib.Z_DEFAULT_STRATEGY, pieces=3)),    # several blocks in a band
            "smooth_rle_full_flush": (smo, zlib_banded16(smo, 16, 1, zlib.Z_RLE, pieces=4))}


@pytest.mark.parametrize("name", list(zlib_cases16()))
def test_zlib_made_16_bit_files(ctx, name):
    a, png = zlib_cases16()[name]
    if name == "repeated_level9":
        assert any(D.dynamic_code_lengths(T.chunks(png)[3][1])[1][1:])  # the file has what it claims: distance codes above distance 1
    fast, general, stored = check_batch16(ctx, [a], [png])
    print("%s: fast %d general %d stored %d" % (name, fast, general, stored))
    assert fast + general + stored == D.nbands(png)
    if "level9" in name or "full_flush" in name:
        assert general > 0


def test_one_batch_of_8_bit_and_16_bit_files_of_differing_sizes(ctx):
    c8 = D.all_cases()
    c16 = P16.cases16()
    files = [encode8(ctx, c8["smooth_4"]), encode16(ctx, c16["mixed"]), encode8(ctx, c8["noise_3"]), encode16(ctx, c16["one_pixel"]),
             zlib_cases16()["repeated_level9"][1], encode8(ctx, c8["one_column_3"]), encode16(ctx, c16["one_column"]), encode8(ctx, c8["one_row_4"])]
    for keep16 in (0, 1):
        single = [ctx.decode_input_png_batch([f], keep16=keep16)[0] for f in files]
        got = ctx.decode_input_png_batch(files, keep16=keep16)
        fast, general, stored, _ = ctx.png_decode_stats()
        assert general > 0 and fast + general + stored == sum(D.nbands(f) for f in files)
        for g, s in zip(got, single):
            assert g.dtype == s.dtype and g.shape == s.shape and np.array_equal(g, s)
        assert [g.dtype == np.uint16 for g in got] == [False, bool(keep16), False, bool(keep16), bool(keep16), False, bool(keep16), False]
    assert np.array_equal(ctx.decode_input_png_batch(files, keep16=1)[1], c16["mixed"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def with_ihdr(png, **kw):
    """The file with bytes of its IHDR replaced: depth, ctype, interlace."""
    ch = T.chunks(png)
    d = bytearray(ch[0][1])
    for k, at in (("depth", 8), ("ctype", 9), ("interlace", 12)):
        if k in kw:
            d[at] = kw[k]
    return D.SIG + D.chunk(b"IHDR", bytes(d)) + png[33:]


def not_ours16(ctx):
    a = P16.cases16()["one_row"]
    good16, good8 = encode16(ctx, a), encode8(ctx, SP.cases4()["one_row"])
    return {"sixteen_bit_rgba": with_ihdr(good16, ctype=6), "sixteen_bit_grey": with_ihdr(good16, ctype=0),
            "pil_16": D.pil_file((np.arange(64, dtype=np.uint16) * 900).reshape(8, 8)), "interlaced_16": with_ihdr(good16, interlace=1),
            "interlaced_8": with_ihdr(good8, interlace=1), "eight_bit_made_16_rgba": with_ihdr(good8, depth=16),
            "pil_8": D.pil_file(SP.cases4()["one_row"][..., [2, 1, 0, 3]]), "empty": b"", "truncated": good16[:40]}


def test_files_this_decoder_does_not_take_are_refused(ctx):
    a = P16.cases16()["one_row"]
    good = encode16(ctx, a)
    for nm, f in not_ours16(ctx).items():
        assert R.input_png_decodable(f) is None, nm
        assert "not a banded PNG file" in R.lib().s360_last_error(None).decode(), nm
        out = [np.full(a.nbytes, 0xA5, np.uint8), np.full(1 << 16, 0xA5, np.uint8)]
        with pytest.raises(R.S360Error, match="image 1"):
            ctx.decode_input_png_batch([good, f], keep16=1, caps=[o.size for o in out], outs=out)
        assert (out[0] == 0xA5).all() and (out[1] == 0xA5).all(), nm  # nothing was written
        assert ctx.png_decode_failure() == (1, 1), nm
    assert np.array_equal(ctx.decode_input_png_batch([good], keep16=1)[0], a)
    assert ctx.png_decode_failure() == (-1, 0)


def test_the_8_bit_entry_points_still_refuse_every_16_bit_file(ctx):
    files = [encode16(ctx, a) for a in (P16.cases16()["one_row"], P16.cases16()["one_pixel"], content16("noise", 5, 9, 3))]
    files += [png for _, png in zlib_cases16().values()]
    good = encode8(ctx, SP.cases4()["one_row"])
    for f in files:
        assert R.input_png_decodable(f) is not None
        assert R.png_decodable(f) is None
        assert "not a banded PNG file" in R.lib().s360_last_error(None).decode()
        with pytest.raises(R.S360Error, match="image 1.*not a banded PNG file"):
            ctx.decode_png_batch([good, f], outs=[np.empty(1 << 16, np.uint8), np.empty(1 << 16, np.uint8)])
        assert ctx.png_decode_failure() == (1, 1)


@pytest.mark.parametrize("keep16", [0, 1])
def test_a_buffer_one_byte_short_is_refused(ctx, keep16):
    a = P16.cases16()["mixed"]
    png = encode16(ctx, a)
    size = a.size * (2 if keep16 else 1)
    out = [np.full(size, 0xA5, np.uint8)]
    with pytest.raises(R.S360Error, match="image 0.*too small"):
        ctx.decode_input_png_batch([png], keep16=keep16, caps=[size - 1], outs=out)
    assert (out[0] == 0xA5).all() and ctx.png_decode_failure() == (0, 2)
    got = ctx.decode_input_png_batch([png], keep16=keep16, caps=[size], outs=out)[0]
    assert np.array_equal(got, a if keep16 else (a >> 8).astype(np.uint8))
    assert ctx.png_decode_failure() == (-1, 0)


def rebuild(ch):
    return D.SIG + b"".join(D.chunk(t, d) for t, d in ch)


def damaged_files16(ctx):
    noise = content16("noise", 24, 50, 77)  # stored bands
    good = encode16(ctx, noise, 8)
    ch = T.chunks(good)
    assert len(ch) == 5 + 3
    out = {}
    c = list(ch)
    c[-2] = (b"IDAT", bytes([c[-2][1][0] ^ 1]) + c[-2][1][1:])
    out["adler_changed"] = rebuild(c)
    c = list(ch)
    d = bytearray(c[3][1])
    assert (d[0] >> 1) & 3 == 0 and d[5] == 1  # a stored block: 5 bytes of header, then the first row's filter byte
    d[7] ^= 0x10  # the first sample's low byte: a store that keeps the high bytes does not see it, the Adler-32 does
    c[3] = (b"IDAT", bytes(d))
    out["low_byte_changed"] = rebuild(c)
    d = bytearray(ch[3][1])
    d[5] = 2  # the filter type alone is wrong: the Adler-32 is made to fit
    f = bytearray(P16.filtered_scanlines16(noise).tobytes())
    f[0] = 2
    c = list(ch)
    c[3] = (b"IDAT", bytes(d))
    c[-2] = (b"IDAT", zlib.adler32(bytes(f)).to_bytes(4, "big"))
    out["filter_type_2"] = rebuild(c)
    # sbNd rewritten: 16 rows per band announced for bands that hold 8 each
    c = list(ch)
    c[1] = (b"sbNd", (16).to_bytes(4, "big"))
    out["band_inflates_short"] = rebuild(c[:3] + c[3:5] + c[-2:])
    return out


@pytest.mark.parametrize("keep16", [0, 1])
def test_damaged_files_are_errors_that_name_the_image(ctx, keep16):
    g0, g2 = P16.cases16()["one_row"], SP.cases4()["one_column"]
    f0, f2 = encode16(ctx, g0), encode8(ctx, g2)
    for nm, f in damaged_files16(ctx).items():
        assert R.input_png_decodable(f) is not None, nm  # well-formed: only the device finds out
        with pytest.raises(R.S360Error, match="image 1") as e:
            ctx.decode_input_png_batch([f0, f, f2], keep16=keep16)
        print(nm, "->", e.value)
        assert ctx.png_decode_failure() == (1, DAMAGED), nm
        want = {"filter_type_2": "unsupported filter", "band_inflates_short": "less output"}.get(nm, "Adler-32")
        assert want in str(e.value), nm
        got = ctx.decode_input_png_batch([f0, f2], keep16=1)  # the other images decode in a following call
        assert np.array_equal(got[0], g0) and np.array_equal(got[1], g2), nm


# ---- frame level --------------------------------------------------------------------------------------------------------------
def as16(img, seed):
    """An 8-bit camera image as the high bytes of 16-bit samples with noise below: what the pixel upload must get is img."""
    low = np.random.default_rng(seed).integers(0, 256, img.shape).astype(np.uint16)
    return (img.astype(np.uint16) << 8) | low


@pytest.fixture(scope="module", params=list(D.RIGS))
def frames(request, tmp_path_factory, rig_json, s360lib):
    """Two frames' camera images, and both frames rendered through the pixel uploads (the second chained with render(True)).
    The small rig's 128-row cameras are below 2 x side_alpha_feather_size (the two alpha ramps overlap), the other's 256 above."""
    cam, eqr = D.RIGS[request.param]
    rig_path = rigutil.scaled_rig_json(rig_json, str(tmp_path_factory.mktemp("rig_in_" + request.param) / "rig.json"), cam / 2048.0)
    mk = lambda: D.make_ctx(rig_path, eqr)  # noqa: E731
    inputs = [rigutil.frame_inputs(rig_path, cam), rigutil.frame_inputs(rig_path, cam, yaw_deg=1.5)]
    c = mk()
    feather = 100
    assert (cam < 2 * feather) == (request.param == "small")
    npairs = len(inputs[0][0])
    want = []
    for k, (side, top, bottom) in enumerate(inputs):
        c.upload_frame(side, top, bottom)
        c.render(k > 0)
        want.append(D.result_of(c, npairs))
    assert not np.array_equal(want[0]["equirect"], want[1]["equirect"])
    # the files, written by the device encoders; what the independent decoders make of them is what was uploaded above
    files = {}
    for depth in (16, 8):
        per_frame = []
        for k, (side, top, bottom) in enumerate(inputs):
            fs = []
            for j, img in enumerate(list(side) + [top, bottom]):
                assert img.dtype == np.uint8 and img.shape[2] == 3
                if depth == 16:
                    f = encode16(c, as16(img, 100 * k + j))
                    assert np.array_equal((decode16_quick(f) >> 8).astype(np.uint8), img)
                    if k == 0 and j in (0, len(side)):  # one side camera, the top camera
                        assert np.array_equal(P16.decode16(f)[0], decode16_quick(f))
                else:
                    f = encode8(c, img)
                    assert np.array_equal(D.pil_pixels(f), img)
                fs.append(f)
            per_frame.append(fs)
        files[depth] = per_frame
    c.close()
    return dict(mk=mk, inputs=inputs, want=want, files=files, npairs=npairs, cams=list(range(npairs)) + [-1, -2])


@pytest.mark.parametrize("depth", [16, 8])
def test_frames_from_files_equal_frames_from_pixels(frames, depth):
    c = frames["mk"]()
    try:
        for k in range(2):
            fs = frames["files"][depth][k]
            c.upload_frame_png(frames["cams"], fs)
            fast, general, stored, _ = c.png_decode_stats()
            assert general == 0 and fast > 0 and fast + stored == sum(D.nbands(f) for f in fs)
            assert c.png_decode_failure() == (-1, 0)
            c.render(k > 0)
            assert D.same(D.result_of(c, frames["npairs"]), frames["want"][k]), "frame %d" % k
    finally:
        c.close()


def test_cameras_in_several_calls_and_mixed_with_pixel_uploads(frames):
    """Sides, top and bottom in calls of their own, in any order, one side camera as pixels: the same frame."""
    c = frames["mk"]()
    try:
        fs, n = frames["files"][16][0], frames["npairs"]
        side = frames["inputs"][0][0]
        c.upload_frame_png([-2], [fs[n + 1]])
        c.upload_frame_png(list(range(n - 1, 0, -1)), [fs[i] for i in range(n - 1, 0, -1)])
        R.check(R.lib().s360_frame_upload_side(c.h, 0, R._p(side[0]), side[0].shape[1], side[0].shape[0], 3), c.h)
        c.upload_frame_png([-1], [frames["files"][8][0][n]])
        c.render(False)
        assert D.same(D.result_of(c, n), frames["want"][0])
    finally:
        c.close()


def test_frame_level_refusals(frames):
    c = frames["mk"]()
    try:
        fs, n, cams = frames["files"][16][0], frames["npairs"], frames["cams"]
        side, top, bottom = frames["inputs"][0]
        for bad_cam in (n, -3, 1000):
            with pytest.raises(R.S360Error, match="camera index out of range"):
                c.upload_frame_png([bad_cam], [fs[0]])
        with pytest.raises(R.S360Error, match="named twice"):
            c.upload_frame_png([0, 0], [fs[0], fs[0]])
        rgba = encode8(c, np.ascontiguousarray(np.dstack([top, np.full(top.shape[:2], 255, np.uint8)])))
        with pytest.raises(R.S360Error, match="image 0.*colour type 2"):
            c.upload_frame_png([-1], [rgba])
        assert c.png_decode_failure() == (0, 2)
        with pytest.raises(R.S360Error, match="image 1.*not a banded PNG file"):
            c.upload_frame_png([0, 1], [fs[0], D.pil_file(side[1][..., ::-1])])
        assert c.png_decode_failure() == (1, 1)
        other = encode16(c, as16(side[0][:-2], 5))
        with pytest.raises(R.S360Error, match="image 1.*side image size changed"):  # within one call
            c.upload_frame_png([0, 1], [fs[0], other])
        with pytest.raises(R.S360Error):
            c.render(False)  # nothing has been marked as uploaded by any of the refused calls
        # a damaged file: the error names it, nothing is marked
        ch = T.chunks(fs[3])
        ch[-2] = (b"IDAT", bytes(4))
        with pytest.raises(R.S360Error, match="image 3.*Adler-32"):
            c.upload_frame_png(cams, fs[:3] + [rebuild(ch)] + fs[4:])
        assert c.png_decode_failure() == (3, DAMAGED)
        with pytest.raises(R.S360Error, match="not uploaded"):
            c.render(False)
        # ... and the frame renders from a following pixel upload to the same bytes as without the failed call
        c.upload_frame(side, top, bottom)
        c.render(False)
        assert D.same(D.result_of(c, n), frames["want"][0])
        with pytest.raises(R.S360Error, match="image 0.*side image size changed"):  # against the frame before
            c.upload_frame_png([0], [other])
        assert c.png_decode_failure() == (0, 2)
        c.upload_frame_png(cams, frames["files"][8][1])
        c.render(True)
        assert D.same(D.result_of(c, n), frames["want"][1])
    finally:
        c.close()
