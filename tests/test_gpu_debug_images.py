"""The reference's debug images through the library (include/s360_debug_images.h, surround360_amd/debug_images.py): frames of the
cases of tests/debug_images_cases.py rendered with s360_set_debug_images on. The list of images — names, order-independent key set,
sizes — is the key set of tests/golden/debug_images_golden.json (the REFERENCE'S OWN PROGRAM's files) for each flag combination; the
pixels of s360_frame_get_debug_image digest to the golden; the files of the device PNG batch, decoded by PIL, are those pixels; a
frame rendered with the switch on equals the same frame with it off in equirect, flows and state images, byte for byte; pole
removal as an operator digests to the golden's four images. Replayed on the CPU emulation by tests/test_cpu_debug_images.py."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import debug_images_cases as D
import refprog
from surround360_amd import _capi, debug_images as DI, render as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig_path(tmp_path_factory, s360lib):
    return D.small_rig(tmp_path_factory.mktemp("rig_debug_images"))


def params_of(name):
    _, flags, w, h, _ = D.CASES[name]
    kw = dict(eqr_width=w, eqr_height=h, final_eqr_width=refprog.FINAL, final_eqr_height=refprog.FINAL,
              enable_top=int("--enable_top" in flags), enable_bottom=int("--enable_bottom" in flags),
              enable_pole_removal=int("--enable_pole_removal" in flags))
    for key in ("sharpening", "side_flow_alg"):
        if "--" + key in flags:
            v = flags[flags.index("--" + key) + 1]
            kw[key] = float(v) if key == "sharpening" else v
    return R.make_params(**kw)


def masks_of(rig_path):
    _, _, bottoms = refprog.rig_ids(rig_path)
    return {cid: refprog.pole_mask(refprog.CAM, 10 - j, 20) for j, cid in enumerate(bottoms)}


def upload(ctx, rig_path, name, k):
    """Frame k of a case's inputs, as the program reads them from imgs_dir."""
    p = ctx.params
    imgs = refprog.frame_images(rig_path, k)
    side, _, _ = refprog.rig_ids(rig_path)
    ctx.upload_frame([imgs[c] for c in side], imgs[ctx.rig.get_top_camera_id()] if p.enable_top else None,
                     imgs[ctx.rig.get_bottom_camera_id()] if p.enable_bottom else None)
    if p.enable_pole_removal:
        m = masks_of(rig_path)
        ctx.upload_pole_removal(imgs[ctx.rig.get_bottom_camera2_id()], m[ctx.rig.get_bottom_camera_id()], m[ctx.rig.get_bottom_camera2_id()])


def file_order(a):
    return a[:, :, [2, 1, 0, 3]] if a.shape[2] == 4 else a[:, :, ::-1]


@pytest.mark.parametrize("name", list(D.CASES))
def test_list_pixels_and_files_are_the_reference_programs(rig_path, name):
    ctx = R.Context(R.RigDescription(rig_path), params_of(name))
    try:
        DI.set_debug_images(ctx, True)
        with pytest.raises(_capi.S360Error) as e:  # nothing rendered yet
            DI.debug_image_list(ctx)
        assert e.value.code == _capi.ERR_STATE
        golden = D.golden()[name]
        for k, f in enumerate(D.CASES[name][0]):
            upload(ctx, rig_path, name, k)
            ctx.render(use_prev=k > 0)
            want = {key.split("/", 1)[1]: v for key, v in golden.items() if key.startswith(f + "/")}
            lst = DI.debug_image_list(ctx)
            assert len({n for n, _, _, _ in lst}) == len(lst) and {n for n, _, _, _ in lst} == set(want), sorted({n for n, _, _, _ in lst} ^ set(want))
            assert all(len(n) < 96 for n in want)
            px = []
            for i, (n, w, h, c) in enumerate(lst):
                assert [h, w, c] == want[n]["shape"], n
                a = DI.get_debug_image(ctx, i)
                assert D.pixels_digest(file_order(a)) == want[n]["sha256"], "%s frame %s" % (n, f)
                px.append(a)
            if k == 0:
                with pytest.raises(_capi.S360Error) as e:  # no batch encoded yet
                    DI.download_debug_png(ctx, 0, np.empty(1 << 20, np.uint8))
                assert e.value.code == _capi.ERR_STATE and DI.debug_png_bound(ctx, 0) == 0
            DI.encode_debug_pngs(ctx)
            for i, (n, w, h, c) in enumerate(lst):
                assert DI.debug_png_bound(ctx, i) >= w * h * c
                png = DI.download_debug_png(ctx, i).tobytes()
                im = Image.open(io.BytesIO(png))
                assert im.mode == ("RGBA" if c == 4 else "RGB") and np.array_equal(np.asarray(im), file_order(px[i])), n
            with pytest.raises(_capi.S360Error) as e:  # too small a buffer is refused, not overrun
                DI.download_debug_png(ctx, 0, np.empty(64, np.uint8))
            assert e.value.code == _capi.ERR_INVALID_ARG
            for i in (-1, len(lst)):
                with pytest.raises(_capi.S360Error) as e:
                    DI.get_debug_image(ctx, i)
                assert e.value.code == _capi.ERR_INVALID_ARG and DI.debug_png_bound(ctx, i) == 0
    finally:
        ctx.close()


def frame_outputs(ctx):
    """Equirect, every flow and every state image of the latest frame."""
    p = ctx.params
    out = {"equirect": ctx.download_equirect().copy()}
    for i in range(ctx.rig.get_side_camera_count()):
        for n in ("overlap_l", "overlap_r"):
            out["%s_%d" % (n, i)] = ctx.get_u8(n, i)
        for n in ("flow_l_to_r", "flow_r_to_l"):
            out["%s_%d" % (n, i)] = ctx.get_f32(n, i)
    for u in range(4):
        if p.enable_top if u < 2 else p.enable_bottom:
            out["extended_side_%d" % u] = ctx.get_u8("extended_side", u)
            out["extended_fisheye_%d" % u] = ctx.get_u8("extended_fisheye", u)
            out["flow_pole_%d" % u] = ctx.get_f32("flow_pole", u)
    if p.enable_pole_removal:
        for n in ("bottom_image", "bottom_image2"):
            out[n] = ctx.get_u8(n)
        out["flow_bottom_secondary"] = ctx.get_f32("flow_bottom_secondary")
    return out


@pytest.mark.parametrize("name", ["sharpen_cubemap_search", "pole_removal"])
def test_the_switch_changes_no_output(rig_path, name):
    """Two chained frames with the switch off, then the same two with it on (a context each): every output byte for byte."""
    res = []
    for on in (False, True):
        ctx = R.Context(R.RigDescription(rig_path), params_of(name))
        try:
            if on:
                DI.set_debug_images(ctx, True)
            frames = []
            for k in range(2):
                upload(ctx, rig_path, name, k)
                ctx.render(use_prev=k > 0)
                frames.append(frame_outputs(ctx))
                if not on:
                    with pytest.raises(_capi.S360Error) as e:
                        DI.debug_image_list(ctx)
                    assert e.value.code == _capi.ERR_STATE
            res.append(frames)
        finally:
            ctx.close()
    for k in range(2):
        assert set(res[0][k]) == set(res[1][k]) and len(res[0][k]) > 50
        for n in res[0][k]:
            assert res[0][k][n].dtype == res[1][k][n].dtype and np.array_equal(res[0][k][n].view(np.uint8), res[1][k][n].view(np.uint8)), (k, n)


def test_one_frame_at_a_time_is_enforced(rig_path):
    ctx = R.Context(R.RigDescription(rig_path), params_of("odd_490x245"))
    try:
        ctx.set_frame_pipelining(True)
        DI.set_debug_images(ctx, True)  # ends the pipelining
        for call in (lambda: ctx.set_frame_pipelining(True), lambda: ctx.set_frame_slots(2)):
            with pytest.raises(_capi.S360Error) as e:
                call()
            assert e.value.code == _capi.ERR_STATE
        upload(ctx, rig_path, "odd_490x245", 0)
        ctx.render()
        n = len(DI.debug_image_list(ctx))
        assert n == len(D.golden()["odd_490x245"])
        DI.set_debug_images(ctx, False)
        with pytest.raises(_capi.S360Error) as e:
            DI.debug_image_list(ctx)
        assert e.value.code == _capi.ERR_STATE
        ctx.set_frame_slots(2)
        with pytest.raises(_capi.S360Error) as e:
            DI.set_debug_images(ctx, True)
        assert e.value.code == _capi.ERR_STATE
    finally:
        ctx.close()


def test_pole_removal_as_an_operator(rig_path):
    """s360_pole_removal_combine on the inputs of case pole_removal, frame 000000, on a context whose flags describe no renderable
    frame: the four images are the golden's, the flow is the one the reference's program writes for that frame."""
    rig = R.RigDescription(rig_path)
    ctx = R.Context(rig, R.make_params(eqr_width=7, eqr_height=3))
    try:
        imgs = refprog.frame_images(rig_path, 0)
        m = masks_of(rig_path)
        b1, b2 = rig.get_bottom_camera_id(), rig.get_bottom_camera2_id()
        cam = rig.bottom_camera()
        cam2 = [c for c in rig.rig if c.id.decode() == b2][0]
        radius = [_capi.lib().s360_camera_usable_pixels_radius(C.byref(c)) for c in (cam, cam2)]
        flip180 = float(np.dot(list(cam.rotation)[3:6], list(cam2.rotation)[3:6])) < 0
        out = DI.pole_removal_combine(ctx, imgs[b1], imgs[b2], m[b1], m[b2], radius[0], radius[1], flip180, 31, "pixflow_low")
        want = D.golden()["pole_removal"]
        for n in ("bottomImage", "bottomImage2", "bottomWarp2", "_bottomCombined"):
            assert out[n].shape == (refprog.CAM, refprog.CAM, 4)
            assert D.pixels_digest(file_order(out[n])) == want["000000/%s.png" % n]["sha256"], n
        # ... and the flow is the one the reference's program leaves for the next frame (saveFlowToFile: rows, cols, the floats)
        import hashlib
        import json
        flow_file = np.array(out["flow"].shape[:2], np.int32).tobytes() + out["flow"].tobytes()
        assert hashlib.sha256(flow_file).hexdigest() == json.load(open(refprog.GOLDEN))["pole_removal"]["000000/flow_bottom_secondary.bin"]
        for bad in (dict(feather_size=30), dict(feather_size=33), dict(flow_alg="pixflow_high")):
            kw = dict(feather_size=31, flow_alg="pixflow_low")
            kw.update(bad)
            with pytest.raises(_capi.S360Error):
                DI.pole_removal_combine(ctx, imgs[b1], imgs[b2], m[b1], m[b2], radius[0], radius[1], flip180, **kw)
    finally:
        ctx.close()
