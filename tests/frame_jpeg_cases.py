"""Cases of the frame JPEG tests (include/s360_frame_jpeg.h): tests/test_gpu_frame_jpeg.py runs them on the GPU,
tests/test_cpu_frame_jpeg.py the same file on the emulated library. The specification is one line — the file is
jpegio::encode(pixels, w, h, quality) of the pixels the library itself downloads for the same frame — so every check is byte
equality against tools/jpeg_host_encode (jpeg_cases.host_encode) and against PIL's save(quality=q, subsampling=2), which writes the
same file (tests/test_cpu_jpeg_device.py pins that over jpeg_cases' case set). No tolerance anywhere.

The frames are those of tests/test_gpu_png.py: the 17-camera rig at 1/16 scale, eyes of 252 x 126. Output shapes, each for a way
the encoder can go wrong behind a frame:
  "m16"  240 x 224, width and height multiples of 16; video cubemap of 96 x 100 faces (288 x 400: height no multiple of 16)
  "odd"  250 x 214, neither a multiple of 16 nor of 8 (dummy luma blocks in the last MCU column and row); photo cubemap of
         100 x 96 faces (100 x 1152: a dummy column all the way down)
Qualities 95 (cv::imwrite's), 1 and 100 (the clamped tables: every divisor 255 / every divisor 1, the longest codes).

Through the tap (include/s360_debug_frame_jpeg.h), with jpeg_cases' constants: 64 x 48 noise at quality 100 for the capacity rule;
1030 x 304 noise at quality 95 — 7410 blocks = 7 x JPEG_SCAN_ITEMS + 242, a scan of many JPEG_STUFF_TILEs and no multiple — for the
index arithmetic of more than one workgroup per kernel; 8192 x 8192 once (marked fullsize)."""
import ctypes as C
import threading

import numpy as np

import jpeg_cases as JC
import rigutil
from surround360_amd import _capi
from surround360_amd import render as R

CAM, EQR_W, EQR_H = 128, 252, 126
SHAPES = {"m16": dict(final=(240, 224), cube=(96, 100, "video")), "odd": dict(final=(250, 214), cube=(100, 96, "photo"))}
QUALITIES = (95, 1, 100)
HEADER = 623
MCU_BYTES = 768  # JPEG_FRAME_MCU_BYTES: a slot's scan buffer holds this much per MCU of 16 x 16 pixels


def scan_cap(w, h):
    return MCU_BYTES * ((w + 15) // 16) * ((h + 15) // 16)


def oracle(px, quality):
    """jpegio::encode of px; PIL's file is the same file."""
    f = JC.host_encode(px, quality)[0]
    assert f == JC.pil_encode(px, quality), "the two oracles differ"
    return f


def same(got, want, what):
    got = bytes(got)
    n = min(len(got), len(want))
    first = next((i for i in range(n) if got[i] != want[i]), n)
    assert got == want, "%s: %d bytes, the host writer's file has %d; the first difference is at byte %d" % (what, len(got), len(want), first)


def small_rig(tmp_dir, rig_json):
    path = rigutil.scaled_rig_json(rig_json, str(tmp_dir / "rig_small.json"), CAM / 2048.0)
    inputs = [rigutil.frame_inputs(path, CAM, yaw_deg=y) for y in (0.0, 2.0, 4.0)]
    a = inputs[0]
    inputs += [([np.ascontiguousarray(s[:, ::-1]) for s in a[0]], a[1], a[2]), (a[0], a[2], a[1]),
               ([np.ascontiguousarray(s[::-1]) for s in a[0]], a[1], a[2])]
    return dict(path=path, rig=R.RigDescription(path), inputs=inputs)


def context(env, shape="m16", **flags):
    fw, fh = SHAPES[shape]["final"]
    return R.Context(env["rig"], R.make_params(**dict(dict(eqr_width=EQR_W, eqr_height=EQR_H, enable_top=1, enable_bottom=1, final_eqr_width=fw,
                                                       final_eqr_height=fh, sharpening=0.25), **flags)))


def equirect_slot(ctx, slot, age):
    g = ctx.geometry
    out = np.empty((g.out_height, g.out_width, 3), np.uint8)
    ctx._ck(R.lib().s360_frame_download_equirect_slot(ctx.h, int(slot), int(age), out.ctypes.data_as(C.c_void_p)))
    return out


# ---- small frames ---------------------------------------------------------------------------------------------------------
def check_small_frames(env, shape):
    """Equirect and cubemap of one frame at the three qualities == the oracle's files of the downloaded pixels."""
    ctx = context(env, shape)
    try:
        fw, fh, fmt = SHAPES[shape]["cube"]
        ctx.set_cubemap_output(fw, fh, fmt)
        g = ctx.geometry
        assert (g.out_width, g.out_height) == SHAPES[shape]["final"]
        cw, ch, _ = ctx.cubemap_size()
        assert ctx.jpeg_bound() == HEADER + scan_cap(g.out_width, g.out_height) + 2
        assert ctx.cubemap_jpeg_bound() == HEADER + scan_cap(cw, ch) + 2
        ctx.upload_frame(*env["inputs"][0])
        files = {}
        for q in QUALITIES:
            ctx.set_jpeg_encode(True, q)
            ctx.render(False)
            eq, cube = ctx.download_equirect(), ctx.download_cubemap()
            assert eq.std() > 5 and cube.std() > 5
            files[q] = ctx.download_jpeg().tobytes()
            print("%s quality %d: equirect %d bytes of %d, cubemap" % (shape, q, len(files[q]), ctx.jpeg_bound()), end=" ")
            same(files[q], oracle(eq, q), "%s equirect at quality %d" % (shape, q))
            cf = ctx.download_cubemap_jpeg().tobytes()
            print("%d of %d" % (len(cf), ctx.cubemap_jpeg_bound()))
            same(cf, oracle(cube, q), "%s cubemap at quality %d" % (shape, q))
        assert len(files[1]) < len(files[95]) < len(files[100])
        # a quality outside 1..100 is clamped as s360_jpeg_create clamps it; the pixels of a frame do not depend on the switch
        ctx.set_jpeg_encode(True, 150)
        ctx.render(False)
        same(ctx.download_jpeg(), files[100], "quality 150")
    finally:
        ctx.close()


# ---- PNG and JPEG both on ---------------------------------------------------------------------------------------------------
def check_png_and_jpeg(env):
    ctx = context(env, "odd")
    try:
        ctx.set_cubemap_output(*SHAPES["odd"]["cube"])
        ctx.upload_frame(*env["inputs"][1])
        ctx.set_png_encode(True)
        ctx.render(False)
        png, cube_png = ctx.download_png().tobytes(), ctx.download_cubemap_png().tobytes()
        with_jpeg_off = ctx.download_equirect()
        ctx.set_jpeg_encode(True, 95)
        ctx.render(False)
        eq, cube = ctx.download_equirect(), ctx.download_cubemap()
        assert np.array_equal(eq, with_jpeg_off)
        assert ctx.download_png().tobytes() == png and ctx.download_cubemap_png().tobytes() == cube_png, "the PNG bytes changed with the JPEG switch on"
        same(ctx.download_jpeg(), oracle(eq, 95), "equirect beside the PNG")
        same(ctx.download_cubemap_jpeg(), oracle(cube, 95), "cubemap beside the PNG")
        ctx.set_png_encode(False)
        ctx.render(False)
        same(ctx.download_jpeg(), oracle(eq, 95), "equirect, PNG off again")
        try:
            ctx.download_png()
            raise AssertionError("a PNG of a frame rendered with the PNG switch off")
        except R.S360Error as e:
            assert e.code == _capi.ERR_STATE
    finally:
        ctx.close()


# ---- two slots, three frames each ---------------------------------------------------------------------------------------------
def check_slots_and_ages(env):
    """Frame k's file is frame k's pixels: age 0 and age 1 of each slot after every enqueue; then the fetch of age 1 (frame 0) of
    slot 0 runs while a second thread enqueues frame 2 of both slots into the buffers frame 0 lies in."""
    ctx = context(env, "m16")
    try:
        ctx.set_frame_slots(2)
        ctx.set_output_double_buffer(True)
        ctx.set_cubemap_output(*SHAPES["m16"]["cube"])
        ctx.set_jpeg_encode(True, 95)
        want, want_cube = {}, {}

        def enqueue(k):
            for s in range(2):
                ctx.select_frame_slot(s)
                ctx.upload_frame(*env["inputs"][2 * k + s])
            ctx.render_batch(False)

        def learn(k):  # the pixels of frame k of both slots, while it is the latest frame
            for s in range(2):
                want[s, k] = oracle(equirect_slot(ctx, s, 0), 95)
                want_cube[s, k] = oracle(ctx.download_cubemap(slot=s), 95)

        def check(k):
            for s in range(2):
                same(ctx.download_jpeg_slot(s, 0), want[s, k], "slot %d frame %d at age 0" % (s, k))
                same(ctx.download_cubemap_jpeg_slot(s, 0), want_cube[s, k], "slot %d frame %d cubemap at age 0" % (s, k))
                if k:
                    same(ctx.download_jpeg_slot(s, 1), want[s, k - 1], "slot %d frame %d at age 1" % (s, k - 1))
                    same(ctx.download_cubemap_jpeg_slot(s, 1), want_cube[s, k - 1], "slot %d frame %d cubemap at age 1" % (s, k - 1))

        enqueue(0)
        learn(0)
        check(0)
        enqueue(1)
        learn(1)
        check(1)
        assert len({want[s, k] for s in range(2) for k in range(2)}) == 4
        # the feeder: frame 2 of both slots, from the moment the fetch below is called
        go, failed = threading.Event(), []

        def feeder():
            try:
                go.wait()
                enqueue(2)
            except Exception as e:  # noqa: BLE001
                failed.append(e)

        t = threading.Thread(target=feeder)
        t.start()
        buf = R.pinned_empty((ctx.jpeg_bound(),))
        go.set()
        got = ctx.download_jpeg_slot(1, 1, buf).tobytes()
        t.join()
        assert not failed, failed
        same(got, want[1, 0], "slot 1 frame 0 at age 1 with frame 2 enqueued meanwhile")
        learn(2)
        check(2)
        assert want[0, 2] not in (want[0, 0], want[0, 1])
    finally:
        ctx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def check_refusals(env):
    ctx = context(env, "odd")
    try:
        ctx.upload_frame(*env["inputs"][0])
        ctx.render(False)
        try:
            ctx.download_jpeg()
            raise AssertionError("a JPEG of a frame rendered before the switch")
        except R.S360Error as e:
            assert e.code == _capi.ERR_STATE and "s360_set_jpeg_encode" in str(e)
        ctx.set_jpeg_encode(True, 95)
        ctx.render(False)
        want = oracle(ctx.download_equirect(), 95)
        short = np.full(len(want) - 1, 0xEE, np.uint8)
        try:
            ctx.download_jpeg(0, short)
            raise AssertionError("cap one byte short was accepted")
        except R.S360Error as e:
            assert e.code == _capi.ERR_INVALID_ARG and ctx.jpeg_size_needed == len(want)
        assert (short == 0xEE).all(), "a refused call wrote into the buffer"
        exact = np.full(len(want), 0xEE, np.uint8)
        same(ctx.download_jpeg(0, exact), want, "cap exactly the file")
        try:
            ctx.download_cubemap_jpeg()
            raise AssertionError("a cubemap of a frame rendered without s360_set_cubemap_output")
        except R.S360Error as e:
            assert e.code == _capi.ERR_STATE
        ctx.set_jpeg_encode(False)
        ctx.render(False)
        try:
            ctx.download_jpeg()
            raise AssertionError("a JPEG of a frame rendered after the switch went off")
        except R.S360Error as e:
            assert e.code == _capi.ERR_STATE
    finally:
        ctx.close()
    # a context whose flags describe no frame: as s360_frame_download_png
    bad = context(env, "odd", final_eqr_height=1)
    try:
        out, n = np.empty(4096, np.uint8), C.c_size_t(0)
        p = out.ctypes.data_as(C.c_void_p)
        L = R.lib()
        assert L.s360_set_png_encode(bad.h, 1) == L.s360_set_jpeg_encode(bad.h, 1, 95) == 0
        rc_png = L.s360_frame_download_png(bad.h, 0, p, C.c_size_t(out.size), C.byref(n))
        msg_png = L.s360_last_error(bad.h)
        rc_jpg = L.s360_frame_download_jpeg(bad.h, 0, p, C.c_size_t(out.size), C.byref(n))
        assert rc_png == rc_jpg == _capi.ERR_INVALID_ARG and L.s360_last_error(bad.h) == msg_png and msg_png
        assert L.s360_frame_download_cubemap_jpeg_slot(bad.h, 0, 0, p, C.c_size_t(out.size), C.byref(n)) == _capi.ERR_INVALID_ARG
    finally:
        bad.close()


# ---- through the tap ------------------------------------------------------------------------------------------------------------
def check_capacity(env):
    """64 x 48 noise at quality 100: a capacity of exactly the scan's size gives the file; one byte less, or none at all, an error
    that names the size, with nothing stored and the guard region behind the buffer untouched."""
    ctx = context(env)
    try:
        ctx.set_jpeg_encode(True, 100)
        px = JC.image(64, 48, "noise", seed=5)
        want = oracle(px, 100)
        scan = len(want) - HEADER - 2
        print("64 x 48 noise at quality 100: scan %d bytes; %d per MCU in a slot's buffer would hold %d" % (scan, MCU_BYTES, scan_cap(64, 48)))
        got, info = ctx.debug_frame_jpeg(px, scan)
        assert info["rc"] == 0 and info["guard_touched"] == 0 and info["stored"] == scan, info
        same(got, want, "capacity exactly the scan")
        for cap in (scan - 1, 0):
            got, info = ctx.debug_frame_jpeg(px, cap, cap=len(want))
            assert got is None and info["rc"] == _capi.ERR_STATE, info
            assert str(scan) in info["message"] and info["n_out"] == len(want), info
            assert info["stored"] == 0 and info["guard_touched"] == 0, info
        got, info = ctx.debug_frame_jpeg(px, scan + 1000, cap=len(want) - 1)  # the host buffer's rule, as in s360_frame_download_jpeg
        assert got is None and info["rc"] == _capi.ERR_INVALID_ARG and info["n_out"] == len(want), info
        ctx.set_jpeg_encode(True, 95)  # the tap follows the switch's quality
        got, info = ctx.debug_frame_jpeg(px, scan_cap(64, 48))
        same(got, oracle(px, 95), "quality 95 after 100")
    finally:
        ctx.close()


def check_large_index(env):
    w, h = 1030, 304
    ctx = context(env)
    try:
        ctx.set_jpeg_encode(True, 95)
        px = JC.image(w, h, "noise")
        want, _, bits = JC.host_encode(px, 95)
        assert want == JC.pil_encode(px, 95)
        nbytes = (int(bits.astype(np.int64).sum()) + 7) // 8
        assert JC.n_blocks(w, h) > 7 * JC.SCAN_ITEMS and JC.n_blocks(w, h) % JC.SCAN_ITEMS
        assert nbytes > 8 * JC.STUFF_TILE and nbytes % JC.STUFF_TILE
        got, info = ctx.debug_frame_jpeg(px, scan_cap(w, h))
        assert info["rc"] == 0 and info["guard_touched"] == 0, info
        same(got, want, "1030 x 304 noise")
        small = JC.image(17, 9, "noise")  # a small image after a large one: stale scratch would show
        same(ctx.debug_frame_jpeg(small, scan_cap(17, 9))[0], oracle(small, 95), "17 x 9 after 1030 x 304")
    finally:
        ctx.close()


def smooth_8k():
    n = 8192
    x = np.arange(n, dtype=np.float32)
    rows = np.sin(x * 0.0031)[None, :], np.cos(x * 0.0017)[:, None]
    rng = np.random.default_rng(8)
    px = np.empty((n, n, 3), np.uint8)
    for c in range(3):
        plane = rows[0] * rows[1] * (90 - 10 * c) + 128 + 9 * c
        px[..., c] = (plane + rng.integers(-2, 3, (n, n), dtype=np.int8)).clip(0, 255).astype(np.uint8)
    return px


def check_8k(env):
    """8192 x 8192, the 8K preset's stereo frame: 262 144 MCUs, 1 572 864 blocks (1536 scan groups), the only case whose block and
    tile counts are in the millions and tens of thousands."""
    ctx = context(env)
    try:
        ctx.set_jpeg_encode(True, 95)
        px = smooth_8k()
        want = JC.host_encode(px, 95)[0]
        got, info = ctx.debug_frame_jpeg(px, scan_cap(8192, 8192))
        print("8192 x 8192: file %d bytes, device encode %.3f ms" % (len(want), info["ms"]))
        assert info["rc"] == 0 and info["guard_touched"] == 0, info
        same(got, want, "8192 x 8192")
    finally:
        ctx.close()
