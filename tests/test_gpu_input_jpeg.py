"""Camera images as baseline JPEG files decoded on the device (include/s360_input_jpeg.h, surround360_amd/csrc/jpeg_decode.hip): the
operator form s360_decode_input_jpeg_batch, the test tap, and the frame-level s360_frame_upload_jpeg, which writes a frame's source
slots straight from the files.

Every comparison is byte equality; there is no tolerance. The decoders that are not ours: host/jpeg_io.hpp's jpegio::decode_any
(tools/jpeg_host_decode) and PIL. The writers: PIL with optimize on and off at three samplings, the host writer
(tools/jpeg_host_encode) and the device encoder (surround360_amd.jpeg). At frame level the oracle is the pixel upload: a frame
rendered after upload_jpeg must equal, byte for byte, the frame rendered after upload_frame of jpegio's pixels.
Replayed on the CPU emulation by tests/test_cpu_input_jpeg.py."""
import numpy as np
import pytest

import input_jpeg_cases as IJ
import jpeg_cases as JC
import rigutil
import test_gpu_png_decode as D
from surround360_amd import jpeg as J
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

NOT_DECODABLE, MISMATCH, BAD_CODE, BAD_RUN, SHORT, BLOCKS, LEFT_OVER, MARKER = 1, 2, 3, 4, 5, 6, 7, 8  # S360_JPEG_DECODE_FAILURE_*
NOT_MSG = "not a JPEG file of this decoder"


@pytest.fixture(scope="module")
def rig_path(tmp_path_factory, rig_json, s360lib):
    d = tmp_path_factory.mktemp("rig_input_jpeg")
    return rigutil.scaled_rig_json(rig_json, str(d / "rig_small.json"), D.CAM / 2048.0)


@pytest.fixture(scope="module")
def ctx(rig_path):
    c = D.make_ctx(rig_path)
    yield c
    c.close()


def differing(got, want, names):
    return ["%s: %d bytes differ" % (n, int((g != w).sum()) if g.shape == w.shape else -1) for g, w, n in zip(got, want, names)
            if g.shape != w.shape or not np.array_equal(g, w)]


def test_tap_equals_the_host_writers_coefficients(ctx):
    """Host-written files: the entropy stage's coefficients (emission order, absolute DC, dummy blocks) are jpeg_cases.host_case's."""
    for case in IJ.host_writer_cases():
        f, coef, _ = JC.host_case(case)
        got = ctx.debug_input_jpeg_blocks(f)
        assert got.shape == coef.shape, case
        assert np.array_equal(got, coef), "%s: %d coefficients differ" % (case, int((got != coef).sum()))


def test_operator_batch_of_mixed_files_in_shuffled_order(ctx):
    """PIL's files of every size, content, quality, sampling and optimize setting in ONE call, shuffled so that a small file follows
    a large one in the tables and scratch: jpegio's pixels, and PIL's. A second decode gives the same bytes."""
    cases, want = IJ.pil_cases(), IJ.pil_case_pixels()
    order = np.random.default_rng(7).permutation(len(cases))
    files = [cases[i][1] for i in order]
    names = [cases[i][0] for i in order]
    for k, f in zip(names, files):
        hs, vs = {2: (2, 2), 1: (2, 1), 0: (1, 1)}[k[4]]
        assert R.input_jpeg_decodable(f) == (k[0], k[1], 3, hs, vs, len(IJ.scan_of(f)[1])), k
    got = ctx.decode_input_jpeg_batch(files)
    s = ctx.jpeg_decode_stats()
    assert s["files"] == len(files) and s["rounds"] >= 1 and ctx.jpeg_decode_failure() == (-1, 0)
    assert s["subsequences"] == sum(max(1, -(-IJ.unstuffed_bits(f) // IJ.SUB_BITS)) for f in files)
    assert not differing(got, [want[i] for i in order], names)
    assert not differing(got, [IJ.pil_decode(f) for f in files], names)
    again = ctx.decode_input_jpeg_batch(files)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_host_writer_and_device_encoder_files_round_trip(ctx):
    """The host writer's files decode to jpegio's and PIL's pixels; encoding on the device with JpegEncoder and decoding on the
    device equals PIL's decode of that file."""
    cases = IJ.host_writer_cases()
    host_files = [JC.host_case(c)[0] for c in cases]
    encoders = {}
    dev_files = []
    for c in cases:
        if c[3] not in encoders:
            encoders[c[3]] = J.JpegEncoder(1030, 304, c[3])
        dev_files.append(encoders[c[3]].encode(JC.case_image(c)))
    for e in encoders.values():
        e.close()
    assert dev_files == host_files  # (the device encoder's contract; tests/test_gpu_jpeg.py owns it)
    got = ctx.decode_input_jpeg_batch(dev_files)
    assert not differing(got, [IJ.pil_decode(f) for f in dev_files], cases)
    assert not differing(got, IJ.host_decode(host_files), cases)


def constant_case():
    """The constant 4:2:0 image whose decoder in the wrong block phase never falls into step: at least 8 subsequences of scan."""
    f = IJ.pil_encode(IJ.image(2048, 304, "constant"), 95, 2, False)
    assert IJ.unstuffed_bits(f) >= 8 * IJ.SUB_BITS
    return f


def test_propagation_rounds_ran(ctx):
    """More than one decode pass for the constant 4:2:0 case: the exit states did travel from subsequence to subsequence on the
    hardware. The round counts of every PIL case are printed."""
    f = constant_case()
    got = ctx.decode_input_jpeg_batch([f])
    s = ctx.jpeg_decode_stats()
    print("constant 2048 x 304 4:2:0: %s" % s)
    assert np.array_equal(got[0], IJ.pil_decode(f))
    assert s["file_rounds"] == [s["most_file_rounds"]] and s["most_file_rounds"] > 1 and s["subsequences"] >= 8
    cases = IJ.pil_cases()
    ctx.decode_input_jpeg_batch([f for _, f in cases])
    s = ctx.jpeg_decode_stats()
    print("launches %d, subsequences %d, entropy %.3f ms, pixels %.3f ms" % (s["rounds"], s["subsequences"], s["ms_entropy"], s["ms_pixels"]))
    for (k, f), r in zip(cases, s["file_rounds"]):
        print("  %-50s %6d subsequences %5d rounds" % (k, max(1, -(-IJ.unstuffed_bits(f) // IJ.SUB_BITS)), r))
    assert all(r >= 1 for r in s["file_rounds"])


def with_scan(f, scan):
    at, old = IJ.scan_of(f)
    return f[:at] + bytes(scan) + f[at + len(old):]


def test_refusals_and_damaged_files(ctx):
    from PIL import Image
    import io
    a = IJ.image(64, 64, "photo")
    good = IJ.pil_encode(a, 95, 2, False)
    want = IJ.pil_decode(good)

    def pil_file(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()
    ex = Image.Exif()
    ex[0x0112] = 6
    rgb = np.ascontiguousarray(a[..., ::-1])
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "PNG")
    png = b.getvalue()
    not_ours = {"progressive": pil_file(rgb, progressive=True), "greyscale": pil_file(rgb[..., 0]), "restarts": pil_file(rgb, restart_marker_blocks=3),
                "orientation 6": pil_file(rgb, exif=ex), "truncated header": good[:200], "png": png}
    assert R.input_jpeg_decodable(b"") is None and NOT_MSG.encode() in R.lib().s360_last_error(None)
    for name, f in not_ours.items():
        assert R.input_jpeg_decodable(f) is None, name
        assert NOT_MSG.encode() in R.lib().s360_last_error(None)
        outs = [np.full(want.size, 0xA5, np.uint8), np.full(want.size, 0xA5, np.uint8)]
        with pytest.raises(R.S360Error, match="image 1.*" + NOT_MSG):
            ctx.decode_input_jpeg_batch([good, f], caps=[want.size, want.size], outs=outs)
        assert ctx.jpeg_decode_failure() == (1, NOT_DECODABLE), name
        assert all((o == 0xA5).all() for o in outs), name  # nothing written, not even the good file's pixels
    # a buffer one byte short
    outs = [np.full(want.size, 0xA5, np.uint8)]
    with pytest.raises(R.S360Error, match="image 0.*output buffer too small"):
        ctx.decode_input_jpeg_batch([good], caps=[want.size - 1], outs=outs)
    assert ctx.jpeg_decode_failure() == (0, MISMATCH) and (outs[0] == 0xA5).all()
    # damaged files: ordinary inputs of a bounded decoder (tools/fuzz/jpeg_decode_sweep runs these kinds under sanitizers first)
    _, scan = IJ.scan_of(good)
    noise = IJ.pil_encode(IJ.image(64, 64, "noise"), 95, 0, False)
    _, nscan = IJ.scan_of(noise)
    # twenty-four 1-bits (no Huffman code is all ones); 0xFF 0xD0: RST0 in a file without DRI. The reason of each is what
    # input_jpeg_cases.expected_failure — a serial walk of the tokens, independent of the library — gives for that file, and for the
    # invalid code also what jpegio says of it.
    damaged = [("truncated", with_scan(good, scan[:len(scan) // 2]), None), ("marker", with_scan(good, scan[:100] + b"\xff\xd0" + scan[100:]), MARKER),
               ("appended", with_scan(good, scan + bytes(40)), None),
               ("invalid code", with_scan(noise, nscan[:300].rstrip(b"\xff") + b"\xff\x00\xff\x00\xff\x00" + nscan[306:]), BAD_CODE)]
    assert IJ.expected_failure(good) == 0 and IJ.expected_failure(noise) == 0
    assert "bad Huffman code" in IJ.host_decode([damaged[3][1]])[0]
    seen = set()
    for name, f, reason in damaged:
        assert R.input_jpeg_decodable(f) is not None, name
        want_reason = IJ.expected_failure(f)
        assert want_reason >= BAD_CODE and reason in (None, want_reason), (name, want_reason)
        with pytest.raises(R.S360Error, match="image 2"):
            ctx.decode_input_jpeg_batch([good, good, f, good])
        img, why = ctx.jpeg_decode_failure()
        print("%s: reason %d" % (name, why))
        assert (img, why) == (2, want_reason), (name, why, want_reason)
        seen.add(why)
    assert len(seen) == 4  # four different faults
    # ... and a good file in a later call still decodes
    assert np.array_equal(ctx.decode_input_jpeg_batch([good])[0], want)
    assert ctx.jpeg_decode_failure() == (-1, 0)


# ---- frame level --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(tmp_path_factory, rig_json, s360lib):
    """Two frames' camera images as JPEG files of mixed samplings and writers, jpegio's pixels of them, and both frames rendered
    through the pixel uploads (the second chained with render(True)); the tiny geometry of test_gpu_input_png.py's frames fixture."""
    cam, eqr = D.RIGS["small"]
    rig_path = rigutil.scaled_rig_json(rig_json, str(tmp_path_factory.mktemp("rig_in_jpeg") / "rig.json"), cam / 2048.0)
    mk = lambda: D.make_ctx(rig_path, eqr)  # noqa: E731
    inputs = [rigutil.frame_inputs(rig_path, cam), rigutil.frame_inputs(rig_path, cam, yaw_deg=1.5)]
    npairs = len(inputs[0][0])
    files, pixels = [], []
    for k, (side, top, bottom) in enumerate(inputs):
        fs = []
        for j, img in enumerate(list(side) + [top, bottom]):
            assert img.dtype == np.uint8 and img.shape[2] == 3
            fs.append(IJ.pil_encode(img, (95, 75, 100)[j % 3], SAMPLING_OF(j), bool(j & 1)) if j % 4 else JC.host_encode(img, 95)[0])
        px = IJ.host_decode(fs)
        assert not differing(px, [IJ.pil_decode(f) for f in fs], range(len(fs)))
        files.append(fs)
        pixels.append(px)
    c = mk()
    want = []
    for k, px in enumerate(pixels):
        c.upload_frame(px[:npairs], px[npairs], px[npairs + 1])
        c.render(k > 0)
        want.append(D.result_of(c, npairs))
    c.close()
    assert not np.array_equal(want[0]["equirect"], want[1]["equirect"])
    return dict(mk=mk, files=files, pixels=pixels, want=want, npairs=npairs, cams=list(range(npairs)) + [-1, -2])


def SAMPLING_OF(j):
    return IJ.SAMPLINGS[j % 3]


def test_frames_from_files_equal_frames_from_pixels(frames):
    c = frames["mk"]()
    try:
        for k in range(2):
            c.upload_jpeg(frames["cams"], frames["files"][k])
            s = c.jpeg_decode_stats()
            assert s["files"] == len(frames["cams"]) and c.jpeg_decode_failure() == (-1, 0)
            c.render(k > 0)
            assert D.same(D.result_of(c, frames["npairs"]), frames["want"][k]), "frame %d" % k
    finally:
        c.close()


def test_cameras_in_several_calls_and_mixed_with_pixel_uploads(frames):
    """Sides, top and bottom in calls of their own, in any order, one side camera as pixels: the same frame."""
    c = frames["mk"]()
    try:
        fs, px, n = frames["files"][0], frames["pixels"][0], frames["npairs"]
        c.upload_jpeg([-2], [fs[n + 1]])
        c.upload_jpeg(list(range(n - 1, 0, -1)), [fs[i] for i in range(n - 1, 0, -1)])
        R.check(R.lib().s360_frame_upload_side(c.h, 0, R._p(px[0]), px[0].shape[1], px[0].shape[0], 3), c.h)
        c.upload_jpeg([-1], [fs[n]])
        c.render(False)
        assert D.same(D.result_of(c, n), frames["want"][0])
    finally:
        c.close()


def test_frame_level_refusals(frames):
    from PIL import Image
    import io
    c = frames["mk"]()
    try:
        fs, px, n, cams = frames["files"][0], frames["pixels"][0], frames["npairs"], frames["cams"]
        for bad_cam in (n, -3, 1000):
            with pytest.raises(R.S360Error, match="camera index out of range"):
                c.upload_jpeg([bad_cam], [fs[0]])
        with pytest.raises(R.S360Error, match="named twice"):
            c.upload_jpeg([0, 0], [fs[0], fs[0]])
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(px[1][..., ::-1])).save(b, "JPEG", progressive=True)
        with pytest.raises(R.S360Error, match="image 1.*" + NOT_MSG):
            c.upload_jpeg([0, 1], [fs[0], b.getvalue()])
        assert c.jpeg_decode_failure() == (1, NOT_DECODABLE)
        other = IJ.pil_encode(px[0][:-2], 95, 2, False)
        with pytest.raises(R.S360Error, match="image 1.*side image size changed"):  # within one call
            c.upload_jpeg([0, 1], [fs[0], other])
        assert c.jpeg_decode_failure() == (1, MISMATCH)
        with pytest.raises(R.S360Error):
            c.render(False)  # nothing has been marked as uploaded by any of the refused calls
        # a damaged file: the error names it, nothing is marked
        at, scan = IJ.scan_of(fs[3])
        with pytest.raises(R.S360Error, match="image 3"):
            c.upload_jpeg(cams, fs[:3] + [with_scan(fs[3], scan[:len(scan) // 3])] + fs[4:])
        assert c.jpeg_decode_failure()[0] == 3 and c.jpeg_decode_failure()[1] >= BAD_CODE
        with pytest.raises(R.S360Error, match="not uploaded"):
            c.render(False)
        # ... and the frame renders from a following pixel upload to the same bytes as without the failed call
        c.upload_frame(px[:n], px[n], px[n + 1])
        c.render(False)
        assert D.same(D.result_of(c, n), frames["want"][0])
        with pytest.raises(R.S360Error, match="image 0.*side image size changed"):  # against the frame before
            c.upload_jpeg([0], [other])
        assert c.jpeg_decode_failure() == (0, MISMATCH)
        c.upload_jpeg(cams, frames["files"][1])
        c.render(True)
        assert D.same(D.result_of(c, n), frames["want"][1])
    finally:
        c.close()
