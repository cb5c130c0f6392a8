"""Pole removal on the device input paths with the pole masks resident per context (include/s360_pole_inputs.h): s360_set_pole_masks,
s360_frame_upload_bottom2 and S360_CAMERA_BOTTOM2 in the raw, packed, PNG and JPEG uploads; k_pole_removal_inputs and
k_pole_removal_merge on the frame path.

Every comparison is byte equality; there is no tolerance. The resident path's oracle is the per-frame path
(s360_frame_upload_pole_removal) on a context of its own — the equirect, flow_bottom_secondary, the state images and the reference's
four debug images of the stage — and, for the plain case, the CPU oracle's frame. Inputs and helpers: tests/pole_inputs_cases.py.
Replayed on the CPU emulation by tests/test_cpu_pole_inputs.py."""
import numpy as np
import pytest

import input_jpeg_cases as IJ
import isputil
import pole_inputs_cases as PC
from surround360_amd import isp as I
from surround360_amd import render as R

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_STATE = R._capi.ERR_INVALID_ARG, R._capi.ERR_STATE
NOT_UPLOADED = "secondary bottom image / pole masks not uploaded"


@pytest.fixture(scope="module")
def rigs(tmp_path_factory, s360lib):
    d = tmp_path_factory.mktemp("rig_pole_inputs")
    golden = PC.small_rig(d)
    return {"golden": golden, "turned": PC.turned_rig(golden, str(d / "rig_turned.json"))}


@pytest.fixture(scope="module")
def two_frames(rigs):
    """Per rig: two frames (the world turned by 1.5 degrees between them) and their results on the per-frame path, the second chained
    with use_prev, the debug images on. Computed once per rig, on first use; nothing changes them."""
    cache = {}

    def get(name):
        if name not in cache:
            frames = [PC.inputs(rigs[name], yaw) for yaw in (0.0, 1.5)]
            cache[name] = (frames, PC.render_per_frame(rigs[name], frames, debug=True))
        return cache[name]
    return get


def code_of(excinfo):
    return excinfo.value.code


# ---- 1, 2: the resident path is the per-frame path is the oracle; both values of flip180 ----------------------------------------
def test_resident_path_equals_per_frame_path_and_oracle(rigs, two_frames, oracle):
    frames, want = two_frames("golden")
    got = PC.render_resident(rigs["golden"], frames, debug=True)
    for k in range(2):
        assert not PC.differing(got[k], want[k]), "frame %d" % k
    assert not np.array_equal(got[0]["equirect"], got[1]["equirect"])
    # the oracle's frames, as tests/test_gpu_frame.py::test_pole_removal_two_frames builds them
    cams, ids = oracle.load_rig(rigs["golden"])
    of = oracle.Frame(cams, oracle.make_params(**PC.FLAGS))
    for k, fr in enumerate(frames):
        of.set_pole_removal(fr["bottom2"], fr["m1"], fr["m2"])
        eqr, _ = of.render(fr["side"], None, fr["bottom"], use_prev=k > 0)
        for res in (got[k], want[k]):
            assert np.array_equal(res["equirect"], eqr), "frame %d: %d bytes differ from the oracle" % (k, int((res["equirect"] != eqr).sum()))
            assert np.array_equal(res["flow_bottom_secondary"], of.get_f32("flow_bottom_secondary").view(np.uint32))
            for n in PC.STATE:
                assert np.array_equal(res[n], of.get_u8(n)), n


def test_a_frame_whose_bottom_flow_is_not_zero(tmp_path):
    """At 256 x 256 the flow between these synthetic bottom images is zero everywhere (the oracle's too), so the merge above warps
    nothing. One frame pair at the size of tests/test_gpu_frame.py::test_pole_removal_two_frames, 512 x 512 with an equirect of
    1008 x 504, where that test finds a flow above half a pixel: the merge reads a warped secondary image."""
    rig = PC.small_rig(tmp_path, 512)
    frames = [PC.inputs(rig, yaw, 512) for yaw in (0.0, 1.5)]
    want = PC.render_per_frame(rig, frames, debug=True, eqr_width=1008, eqr_height=504)
    got = PC.render_resident(rig, frames, debug=True, eqr_width=1008, eqr_height=504)
    assert np.abs(got[1]["flow_bottom_secondary"].view(np.float32)).max() > 0.5
    assert not np.array_equal(got[1]["bottomWarp2.png"], got[1]["bottomImage2.png"])
    for k in range(2):
        assert not PC.differing(got[k], want[k]), "frame %d" % k


def test_both_values_of_flip180(rigs, two_frames):
    signs = set()
    for name in ("golden", "turned"):
        signs.add(PC.up_sign(rigs[name]))
        frames, want = two_frames(name)
        got = PC.render_resident(rigs[name], frames, debug=True)
        for k in range(2):
            assert not PC.differing(got[k], want[k]), "%s rig, frame %d" % (name, k)
    assert signs == {1, -1}
    # (the turned rig is another frame: its secondary image is read the other way round)
    assert not np.array_equal(two_frames("golden")[1][0]["bottomImage2.png"], two_frames("turned")[1][0]["bottomImage2.png"])


# ---- 3: sizes of the two bottom cameras -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig_name", ["golden", "turned"])
@pytest.mark.parametrize("size", PC.SIZES[1:], ids=lambda s: "%dx%d" % s)  # (256 x 256: the tests above)
def test_sizes_of_the_bottom_cameras(rigs, size, rig_name):
    """A whole frame from bottom cameras of w x h through the pixel uploads (the side cameras stay 256 x 256): the golden rig flips
    the secondary image, the turned one does not."""
    fr = PC.cropped(PC.inputs(rigs[rig_name]), size)
    assert fr["bottom"].shape == (size[1], size[0], 3) and (size[0] * size[1] % 4 != 0) == (size == (253, 251))
    want = PC.render_per_frame(rigs[rig_name], [fr], debug=True)[0]
    got = PC.render_resident(rigs[rig_name], [fr], debug=True)[0]
    assert got["bottomImage.png"].shape == (size[1], size[0], 4) and got["equirect"].std() > 5
    assert not PC.differing(got, want)


# ---- 4: masks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["no_red", "all_red_1", "corners", "near_reds"])
def test_masks(rigs, name):
    m1, m2 = PC.mask_cases(PC.CAM, PC.CAM)[name]
    fr = dict(PC.inputs(rigs["golden"]), m1=m1, m2=m2)
    want = PC.render_per_frame(rigs["golden"], [fr], debug=True)[0]
    got = PC.render_resident(rigs["golden"], [fr], debug=True)[0]
    assert not PC.differing(got, want)
    a1 = got["bottomImage.png"][..., 3]
    if name == "all_red_1":
        assert not a1.any()  # A1 = 0 everywhere: every pixel of the merge comes from the secondary camera
    if name == "near_reds":  # none of them counts: the planes of the mask without any red
        white = PC.mask_cases(PC.CAM, PC.CAM)["no_red"]
        plain = PC.render_resident(rigs["golden"], [dict(fr, m1=white[0], m2=white[1])], debug=True)[0]
        assert not PC.differing(got, plain)
    if name == "corners":
        assert a1[PC.CAM // 2, PC.CAM // 2] == 255


# ---- 5: the secondary camera through each input path, in one batch with the other cameras ------------------------------------------
def resident_from_pixels(rig_path, side, bottom, bottom2, m1, m2):
    return PC.render_resident(rig_path, [dict(side=side, bottom=bottom, bottom2=bottom2, m1=m1, m2=m2)])[0]


@pytest.mark.parametrize("bits", [12, 8])
def test_secondary_camera_from_packed_sensor_bytes(rigs, bits):
    fr = PC.inputs(rigs["golden"])
    n = len(fr["side"])
    cams = list(range(n)) + [-2, PC.BOTTOM2]
    raws = [isputil.bayer_frame(PC.CAM, PC.CAM, seed=300 + k, pattern="GRBG") for k in range(n + 2)]
    packed = [isputil.pack_frame(r, bits) for r in raws]
    cfg = I.config_from_json(isputil.CONFIG_GRBG_NOSHARP, 16)
    host, feeder = I.CameraIsp(cfg), I.CameraIsp(cfg)
    c = PC.make_ctx(rigs["golden"])
    try:
        px = [(host.get_image_packed(p, bits, PC.CAM, PC.CAM) >> 8).astype(np.uint8) for p in packed]  # s360_isp_process_packed, high byte
        want = resident_from_pixels(rigs["golden"], px[:n], px[n], px[n + 1], fr["m1"], fr["m2"])
        c.set_pole_masks(fr["m1"], fr["m2"])
        for cam, p in zip(cams, packed):
            c.upload_packed(feeder, cam, p, bits, PC.CAM, PC.CAM)
        c.render()
        assert not PC.differing(PC.result_of(c), want)
        if bits == 12:  # ... and s360_frame_upload_raw of the unpacked samples
            for cam, r in zip(cams, raws):
                v = r >> 4
                c.upload_raw(feeder, cam, (v << 4) | (v >> 8))  # (as the device widens 12-bit samples)
            c.render()
            assert not PC.differing(PC.result_of(c), want)
    finally:
        c.close()
        host.close()
        feeder.close()


@pytest.mark.parametrize("depth", [16, 8])
def test_secondary_camera_from_a_banded_png_file(rigs, depth):
    fr = PC.inputs(rigs["golden"])
    n = len(fr["side"])
    imgs = list(fr["side"]) + [fr["bottom"], fr["bottom2"]]
    want = resident_from_pixels(rigs["golden"], imgs[:n], imgs[n], imgs[n + 1], fr["m1"], fr["m2"])
    c = PC.make_ctx(rigs["golden"])
    try:
        rng = np.random.default_rng(5)
        if depth == 16:  # the pixels are the high bytes; the low bytes are noise
            files = [bytes(c.encode_png16((a.astype(np.uint16) << 8) | rng.integers(0, 256, a.shape, dtype=np.uint16))) for a in imgs]
        else:
            files = [bytes(c.encode_png(a)) for a in imgs]
        c.set_pole_masks(fr["m1"], fr["m2"])
        c.upload_frame_png(list(range(n)) + [-2, PC.BOTTOM2], files)
        c.render()
        assert not PC.differing(PC.result_of(c), want)
    finally:
        c.close()


@pytest.mark.parametrize("sampling", [2, 0], ids=["420", "444"])
def test_secondary_camera_from_a_jpeg_file(rigs, sampling):
    fr = PC.inputs(rigs["golden"])
    n = len(fr["side"])
    files = [IJ.pil_encode(a, 95, sampling, False) for a in list(fr["side"]) + [fr["bottom"], fr["bottom2"]]]
    px = [IJ.pil_decode(f) for f in files]
    want = resident_from_pixels(rigs["golden"], px[:n], px[n], px[n + 1], fr["m1"], fr["m2"])
    c = PC.make_ctx(rigs["golden"])
    try:
        c.set_pole_masks(fr["m1"], fr["m2"])
        c.upload_frame_jpeg(list(range(n)) + [-2, PC.BOTTOM2], files)
        c.render()
        assert not PC.differing(PC.result_of(c), want)
    finally:
        c.close()


# ---- 6, 7: two slots; masks replaced -------------------------------------------------------------------------------------------------
def test_two_frame_slots_share_the_masks(rigs, two_frames):
    frames, _ = two_frames("golden")
    solo = [PC.render_resident(rigs["golden"], [fr])[0] for fr in frames]
    c = PC.make_ctx(rigs["golden"])
    try:
        c.set_frame_slots(2)
        c.set_pole_masks(frames[0]["m1"], frames[0]["m2"])
        for k, fr in enumerate(frames):
            c.select_frame_slot(k)
            PC.feed_resident(c, fr)
        c.render_batch()
        for k in range(2):
            c.select_frame_slot(k)
            assert not PC.differing(PC.result_of(c), solo[k]), "slot %d" % k
        assert PC.differing(solo[0], solo[1])
    finally:
        c.close()


def test_masks_replaced_between_two_frames(rigs, two_frames):
    frames, _ = two_frames("golden")
    other = PC.mask_cases(PC.CAM, PC.CAM)["corners"]
    frames = [frames[0], dict(frames[1], m1=other[0], m2=other[1])]
    want = PC.render_per_frame(rigs["golden"], frames)
    got = PC.render_resident(rigs["golden"], frames, masks_of=[(fr["m1"], fr["m2"]) for fr in frames])
    for k in range(2):
        assert not PC.differing(got[k], want[k]), "frame %d" % k
    base = two_frames("golden")[1][1]
    assert PC.differing(want[1], {k: base[k] for k in want[1]})  # the new masks changed the frame


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(rigs, two_frames):
    frames, want = two_frames("golden")
    fr = frames[0]
    n = len(fr["side"])
    cfg = I.config_from_json(isputil.CONFIG_GRBG_NOSHARP, 16)
    isp = I.CameraIsp(cfg)
    plain = PC.make_ctx(rigs["golden"], enable_pole_removal=0)
    c = PC.make_ctx(rigs["golden"])
    try:
        png = bytes(c.encode_png(fr["bottom2"]))
        jpg = IJ.pil_encode(fr["bottom2"], 95, 2, False)
        raw = isputil.bayer_frame(PC.CAM, PC.CAM, seed=1, pattern="GRBG")
        # -3 on a context without enable_pole_removal, in all four upload calls; the masks on such a context
        for call in (lambda: plain.upload_raw(isp, PC.BOTTOM2, raw), lambda: plain.upload_packed(isp, PC.BOTTOM2, isputil.pack_frame(raw, 12), 12, PC.CAM, PC.CAM),
                     lambda: plain.upload_frame_png([PC.BOTTOM2], [png]), lambda: plain.upload_frame_jpeg([PC.BOTTOM2], [jpg])):
            with pytest.raises(R.S360Error, match="camera index out of range"):
                call()
        with pytest.raises(R.S360Error) as e:
            plain.set_pole_masks(fr["m1"], fr["m2"])
        assert code_of(e) == ERR_STATE
        for bad in (-4, n):
            with pytest.raises(R.S360Error, match="camera index out of range"):
                c.upload_frame_png([bad], [png])
        # masks and bottom images of different sizes
        c.set_pole_masks(fr["m1"], fr["m2"])
        small = np.ascontiguousarray(fr["bottom"][:-2])
        for call in (lambda: c.upload_frame(fr["side"], None, small), lambda: c.upload_bottom2(small),
                     lambda: c.upload_frame_png([PC.BOTTOM2], [bytes(c.encode_png(small))]),
                     lambda: c.upload_frame_jpeg([-2, PC.BOTTOM2], [jpg, IJ.pil_encode(small, 95, 2, False)])):
            with pytest.raises(R.S360Error) as e:
                call()
            assert code_of(e) == ERR_INVALID_ARG
        # the per-frame entry point while masks are resident; accepted again after clearing
        with pytest.raises(R.S360Error) as e:
            c.upload_pole_removal(fr["bottom2"], fr["m1"], fr["m2"])
        assert code_of(e) == ERR_STATE
        c.set_pole_masks()
        c.upload_frame(fr["side"], None, fr["bottom"])
        c.upload_pole_removal(fr["bottom2"], fr["m1"], fr["m2"])
        c.render()
        assert not PC.differing(PC.result_of(c), {k: want[0][k] for k in ("equirect", "flow_bottom_secondary") + PC.STATE})
    finally:
        c.close()
    c = PC.make_ctx(rigs["golden"])
    try:
        # masks but no secondary image: today's message
        c.set_pole_masks(fr["m1"], fr["m2"])
        c.upload_frame(fr["side"], None, fr["bottom"])
        with pytest.raises(R.S360Error, match=NOT_UPLOADED) as e:
            c.render()
        assert code_of(e) == ERR_STATE
        # a camera named twice, -3 included
        with pytest.raises(R.S360Error, match="named twice"):
            c.upload_frame_png([PC.BOTTOM2, 0, PC.BOTTOM2], [png, png, png])
        with pytest.raises(R.S360Error, match="named twice"):
            c.upload_frame_jpeg([PC.BOTTOM2, PC.BOTTOM2], [jpg, jpg])
        # a failing batch that contains -3 marks nothing as uploaded, the secondary included
        at, scan = IJ.scan_of(jpg)
        cut = jpg[:at] + scan[:len(scan) // 3] + jpg[at + len(scan):]
        with pytest.raises(R.S360Error, match="image 1"):
            c.upload_frame_jpeg([-2, PC.BOTTOM2], [IJ.pil_encode(fr["bottom"], 95, 2, False), cut])
        with pytest.raises(R.S360Error, match=NOT_UPLOADED):
            c.render()
        damaged = bytearray(png)
        damaged[len(damaged) // 2] ^= 0x5A
        with pytest.raises(R.S360Error, match="image 0"):
            c.upload_frame_png([PC.BOTTOM2, -2], [bytes(damaged), bytes(c.encode_png(fr["bottom"]))])
        with pytest.raises(R.S360Error, match=NOT_UPLOADED):
            c.render()
        # ... and the frame renders from a following upload to the bytes it has without the failed calls
        c.upload_bottom2(fr["bottom2"])
        c.render()
        assert not PC.differing(PC.result_of(c), {k: want[0][k] for k in ("equirect", "flow_bottom_secondary") + PC.STATE})
    finally:
        c.close()
        plain.close()
        isp.close()
