"""The preview object (include/s360_preview.h, surround360_amd/preview.py) and host/TestHyperPreview on the GPU against the numpy
restatement of the reference's TestHyperPreview (tests/preview_oracle.py, pinned by tests/golden/preview_golden.npz), stage by
stage through the test taps of include/s360_debug_preview.h: the warp maps, the developed float4 layers, the remapped layers and
the final B,G,R bytes on caller-made maps, then the whole object on its own maps, gamma 2.2, layer persistence, the asynchronous
pair, and the program on a two-file capture. Shapes, contents and maps: tests/preview_cases.py.

Tolerances. Everything is bit for bit except: (1) the maps — sees() and pixel() run in double on the device with the device's
sqrt / atan2, so seen entries may differ by 1e-3 px (the allowance test_spherical_warp_map has, for the same reason), masks must be
equal; (2) the whole object on its own maps — a map entry that differs in its last bits can land on the other side of a 1/32-pixel
rounding tie, so a pixel may be left out if an oracle map entry x 32 of it lies within 0.032 (= 1e-3 px x 32) of a tie AND the
device's entry quantises differently there, at most 1 % of the pixels; (3) gamma 2.2 — pow in double on the device instead of
glibc's powf: +-1 level on at most 1 % of the pixels (a last-place error moves a value of at most 255 by under 1e-4 levels, so it
can only flip a rounding tie, and about 2e-4 of uniformly placed values lie that close to one)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import preview_cases as PC
import preview_oracle as PO

pytestmark = pytest.mark.gpu

ROOT = PC.ROOT
SHAPES = list(PC.SHAPES)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rig_files(shape):
    import tempfile
    d = tempfile.mkdtemp(prefix="s360_preview_rig_")
    return PC.write_rig(PC.small_rig(shape), os.path.join(d, "rig_%s.json" % shape))


@functools.lru_cache(maxsize=None)
def oracle_maps(shape):
    """(maps, double pixels, seen masks) of the three rescaled pole cameras; computed once, never written to."""
    _, _, W, H, _, _ = PC.SHAPES[shape]
    cams = [PO.rescaled_camera_json(c) for c in PC.pole_cameras(PC.small_rig(shape))]
    out = [PO.warp_map(c, W, H, with_pixels=True) for c in cams]
    for o in out:
        for a in o:
            a.setflags(write=False)
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


@functools.lru_cache(maxsize=None)
def oracle_developed(shape, bits, content, gamma=1.0):
    raw_w, raw_h = PC.SHAPES[shape][:2]
    d = [PO.develop(f, bits, raw_w, raw_h, l, gamma) for l, f in enumerate(PC.frames(shape, content, bits))]
    for a in d:
        a.setflags(write=False)
    return d


def make_preview(shape, gamma=1.0, coef=30.0):
    from surround360_amd import render as R
    from surround360_amd.preview import Preview
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    rig = R.RigDescription(rig_files(shape))
    return Preview(rig.rig, raw_w, raw_h, W, H, gamma, coef), rig


def near_tie(m, window=0.032):
    """Per pixel: does a coordinate of a seen entry, x 32, lie within `window` of k + 0.5?"""
    v = m.astype(np.float64) * 32.0
    d = np.abs(v - np.floor(v) - 0.5)
    return ((d <= window) & (m != -1.0)).any(axis=-1)


def quantised(m):
    return np.rint(m.astype(np.float32) * np.float32(32.0)).astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES)
def test_map(shape):
    """k_preview_map against precomputeProjectionWarp restated: equal seen / unseen masks, seen entries within 1e-3 px. First, on
    the oracle alone: no point of these shapes lies within a relative 1e-9 of the fov or the resolution boundary of sees(), so a
    last-bit difference in double cannot flip a mask."""
    maps, pix, seen = oracle_maps(shape)
    pv, rig = make_preview(shape)
    _, _, W, H, _, _ = PC.SHAPES[shape]
    assert [rig.rig[i].id.decode() for i in pv.camera_indices()] == list(PC.POLE_IDS)
    pts = PO.world_points(W, H)
    for l in range(3):
        cam = pv.debug_camera(l)
        want = PO.rescaled_camera_json(PC.pole_cameras(PC.small_rig(shape))[l])
        assert [cam.resolution[0], cam.resolution[1]] == want["resolution"]
        assert [cam.principal[0], cam.principal[1], cam.focal[0], cam.focal[1]] == want["principal"] + want["focal"]
        # the boundaries of sees() (Camera.h:157-180) on the oracle's numbers
        v = pts - np.array(list(cam.position))
        back = np.array(list(cam.rotation)[6:9])
        dot = -(v @ back)
        lhs, rhs = dot * np.abs(dot), cam.fov_threshold * (v * v).sum(-1)
        assert cam.fov_threshold not in (-1.0, 0.0)
        assert (np.abs(lhs - rhs) > 1e-9 * np.maximum(np.abs(lhs), np.abs(rhs))).all()
        inside_fov = lhs > rhs
        for k in range(2):
            p, res = pix[l][..., k][inside_fov], cam.resolution[k]
            assert (np.abs(p) > 1e-9 * res).all() and (np.abs(p - res) > 1e-9 * res).all()
        got = pv.debug_map(l)
        got_seen = ~((got[..., 0] == -1.0) & (got[..., 1] == -1.0))
        assert np.array_equal(got_seen, seen[l]), "layer %d: %d mask differences" % (l, (got_seen != seen[l]).sum())
        assert seen[l].any() and not seen[l].all()
        err = np.abs(got.astype(np.float64) - maps[l].astype(np.float64))[seen[l]]
        print("layer %d: seen %d of %d, max map error %.3g px" % (l, seen[l].sum(), seen[l].size, err.max()))
        assert err.max() <= 1e-3
    if shape == "portrait":  # the narrowed cameras: a band nobody sees, and the resolution test of sees() decides somewhere
        assert (~seen[0] & ~seen[1] & ~seen[2]).any()
        cam = pv.debug_camera(0)
        p = pix[0]
        inside = (p[..., 0] >= 0) & (p[..., 0] < cam.resolution[0]) & (p[..., 1] >= 0) & (p[..., 1] < cam.resolution[1])
        v = pts - np.array(list(cam.position))
        dot = -(v @ np.array(list(cam.rotation)[6:9]))
        assert ((dot * np.abs(dot) > cam.fov_threshold * (v * v).sum(-1)) & ~inside).any()


@pytest.mark.parametrize("content", PC.CONTENTS)
@pytest.mark.parametrize("bits", PC.BITS)
@pytest.mark.parametrize("shape", SHAPES)
def test_develop(shape, bits, content):
    """k_preview_develop at gamma 1: the float4 layers bit for bit (unpacking, demosaic taps and constants, alpha, both fades)."""
    pv, _ = make_preview(shape)
    pv.render_packed(*PC.frames(shape, content, bits), bits)
    want = oracle_developed(shape, bits, content)
    for l in range(3):
        got = pv.debug_developed(l)
        assert got.shape == want[l].shape
        assert np.array_equal(u32(got), u32(want[l])), "layer %d: %d of %d words differ" % (l, (u32(got) != u32(want[l])).sum(), got.size)
    if content == "max":
        assert want[0][..., :3].max() == np.float32(65535.0) / np.float32(13.0) * np.float32(29.0)


@pytest.mark.parametrize("content,bits", [("spread", 12), ("spread", 8), ("zeros", 12), ("max", 12), ("checker", 12), ("checker", 8)])
@pytest.mark.parametrize("maps_name", ["oracle", "hand"])
@pytest.mark.parametrize("shape", SHAPES)
def test_compose_on_caller_made_maps(shape, maps_name, content, bits):
    """k_preview_compose on uploaded maps — the oracle's own, and hand-made ones with exact 1/32 ties, -1 entries, the last column
    and row, entries just outside and far outside: remapped layers and final B,G,R bytes bit for bit; the band no layer sees exists
    and is 0 (0 * NaN through cvRound and the saturation)."""
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    if maps_name == "oracle":
        maps = oracle_maps(shape)[0]
    else:
        maps = [PC.hand_made_map(W, H, raw_w // 2, raw_h // 2, l) for l in range(3)]
        v = np.stack(maps).astype(np.float64) * 32
        assert ((v - np.floor(v) == 0.5) & (np.stack(maps) != -1)).sum() > 100  # exact ties are present
    pv, _ = make_preview(shape)
    pv.debug_set_maps(maps)
    got = pv.render_packed(*PC.frames(shape, content, bits), bits)
    dev = oracle_developed(shape, bits, content)
    rem, want = PO.compose(dev, maps)
    for l in range(3):
        g = pv.debug_remapped(l)
        assert np.array_equal(u32(g), u32(rem[l])), "remapped layer %d: %d words differ" % (l, (u32(g) != u32(rem[l])).sum())
    assert np.array_equal(got, want), "%d of %d bytes differ" % ((got != want).sum(), got.size)
    unseen = np.all([(m[..., 0] == -1) & (m[..., 1] == -1) for m in maps], axis=0)
    if maps_name == "hand" or shape == "portrait":
        assert unseen.any() and not got[unseen].any()
    if content == "checker":  # the cubic overshoot reaches both clamps
        assert got.min() == 0 and got.max() == 255
    if content == "spread":
        assert (got[~unseen] < 255).mean() > 0.5 and len(np.unique(got)) > 100


@pytest.mark.parametrize("content,bits", [("spread", 12), ("spread", 8), ("max", 8), ("checker", 12)])
@pytest.mark.parametrize("shape", SHAPES)
def test_whole_object_on_its_own_maps(shape, content, bits):
    """create + render_packed with nothing uploaded in between. Bit for bit, except where the device's map entry quantises to another
    1/32-pixel step than the oracle's AND the oracle's entry x 32 lies within 0.032 of a rounding tie; at most 1 % of the pixels.
    (The window alone covers far more than 1 % of the pixels — 6.4 % per coordinate — so it is the pixels actually left out that
    the cap counts.)"""
    pv, _ = make_preview(shape)
    got = pv.render_packed(*PC.frames(shape, content, bits), bits)
    maps = oracle_maps(shape)[0]
    want = PO.compose(oracle_developed(shape, bits, content), maps)[1]
    left_out = np.zeros(got.shape[:2], bool)
    for l in range(3):
        left_out |= near_tie(maps[l]) & (quantised(pv.debug_map(l)) != quantised(maps[l])).any(axis=-1)
    print("left out: %d of %d pixels" % (left_out.sum(), left_out.size))
    assert left_out.mean() <= 0.01
    bad = (got != want).any(axis=-1) & ~left_out
    assert not bad.any(), "%d pixels differ outside the tie allowance" % bad.sum()


@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_2_2(shape):
    pv, _ = make_preview(shape, gamma=2.2)
    got = pv.render_packed(*PC.frames(shape, "dark", 12), 12)
    want = PO.compose(oracle_developed(shape, 12, "dark", 2.2), oracle_maps(shape)[0])[1]
    d = np.abs(got.astype(int) - want.astype(int))
    print("gamma 2.2: max difference %d, %d of %d pixels differ" % (d.max(), d.any(axis=-1).sum(), d.shape[0] * d.shape[1]))
    assert d.max() <= 1 and d.any(axis=-1).mean() <= 0.01
    assert len(np.unique(want)) > 50 and (want < 255).mean() > 0.3  # (the content is one that gamma 2.2 does not saturate)


def test_layer_persistence_and_first_frame():
    """Layers start as raw images of zeros; a None layer keeps its previous raw image (also across a change of packing)."""
    shape = "landscape"
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    pv, _ = make_preview(shape)
    maps = oracle_maps(shape)[0]
    pv.debug_set_maps(maps)
    ref = PO.Renderer(PC.pole_cameras(PC.small_rig(shape)), raw_w, raw_h, W, H, maps=maps)
    a, b = PC.frames(shape, "spread", 12), PC.frames(shape, "checker", 8)
    steps = [((a[0], None, None), 12), ((None, a[1], None), 12), ((None, None, b[2]), 8), ((b[0], None, None), 8), ((None, None, None), 12),
             ((a[0], a[1], a[2]), 12)]
    seen = []
    for fr, bits in steps:
        got, want = pv.render_packed(*fr, bits), ref.render(*fr, bits)
        assert np.array_equal(got, want)
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and np.array_equal(seen[3], seen[4]) and not np.array_equal(seen[4], seen[5])


def test_submit_and_fetch():
    """The asynchronous pair: two frames in flight come back in order and equal the synchronous call's; a third submit and a fetch
    of nothing are refused with S360_ERR_STATE, as are bad packings with S360_ERR_INVALID_ARG."""
    from surround360_amd import _capi
    shape = "portrait"
    pv, _ = make_preview(shape)
    a, b = PC.frames(shape, "spread", 12), PC.frames(shape, "checker", 12)
    wa, wb = pv.render_packed(*a, 12), pv.render_packed(*b, 12)
    pv.submit_packed(*a, 12)
    pv.submit_packed(*b, 12)
    with pytest.raises(_capi.S360Error) as e:
        pv.submit_packed(*a, 12)
    assert e.value.code == _capi.ERR_STATE and "waiting to be fetched" in str(e.value)
    with pytest.raises(_capi.S360Error) as e:
        pv.render_packed(*a, 12)
    assert e.value.code == _capi.ERR_STATE
    assert np.array_equal(pv.fetch(), wa) and np.array_equal(pv.fetch(), wb)
    with pytest.raises(_capi.S360Error) as e:
        pv.fetch()
    assert e.value.code == _capi.ERR_STATE
    with pytest.raises(_capi.S360Error) as e:
        pv.render_packed(a[0], None, None, 10)
    assert e.value.code == _capi.ERR_INVALID_ARG
    d, c = pv.last_times()
    assert d >= 0 and c >= 0


# ---- the program ----------------------------------------------------------------------------------------------------------
def pil_roundtrip(bgr):
    """What PIL decodes from its own save(quality=95, subsampling=2) of the pixels."""
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=95, subsampling=2)
    return np.array(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))


def run_program(exe, tmp_path, shape, bits, ext=None, more=()):
    cap = tmp_path / "capture"
    dest = tmp_path / ("out_%s_%d" % (ext or "default", len(more)))
    if not cap.exists():
        cap.mkdir()
        PC.write_capture(str(cap), shape, bits)
    _, _, W, H, _, _ = PC.SHAPES[shape]
    rig = PC.write_rig(PC.small_rig(shape), str(tmp_path / "rig.json"))
    cmd = [exe, "--logbuflevel", "-1", "--stderrthreshold", "0", "--v", "0", "--log_dir", str(tmp_path / "logs"), "--rig_json_file", rig,
           "--binary_prefix", str(cap), "--preview_dest", str(dest), "--eqr_width", str(W), "--eqr_height", str(H), "--gamma", "1.0",
           "--file_count", "2"] + (["--preview_ext", ext] if ext else []) + list(more)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return dest, r.stderr


def check_program(exe, tmp_path, shape="landscape", bits=12):
    """preview.py's command line (plus the equirect size of the small case) on a two-file capture of 17 cameras x 3 frames whose
    serial numbers sort differently as strings and as numbers: --preview_ext png holds the restatement's pixels, frame by frame,
    with the right cameras picked; the default .jpg files decode to what PIL decodes from its own encoding of those pixels;
    --start_frame 1 --frame_count 1 writes 000001 only."""
    from PIL import Image
    raw_w, raw_h, W, H, _, _ = PC.SHAPES[shape]
    fr = PC.capture_frames(shape, bits)
    ref = PO.Renderer(PC.pole_cameras(PC.small_rig(shape)), raw_w, raw_h, W, H, maps=oracle_maps(shape)[0])
    want = [ref.render(*[fr[f][c] for c in PC.CAPTURE_POLES], bits) for f in range(PC.CAPTURE_FRAMES)]
    assert not np.array_equal(want[0], want[1]) and len(np.unique(want[0])) > 100
    dest, log = run_program(exe, tmp_path, shape, bits, "png")
    assert sorted(os.listdir(dest)) == ["%06d.png" % f for f in range(PC.CAPTURE_FRAMES)]
    assert all("Rendering frame %d..." % f in log for f in range(PC.CAPTURE_FRAMES))
    maps = oracle_maps(shape)[0]
    for f in range(PC.CAPTURE_FRAMES):
        got = np.array(Image.open(os.path.join(dest, "%06d.png" % f)).convert("RGB"))[..., ::-1]
        # (the tie allowance of test_whole_object_on_its_own_maps: the program builds its maps on the device)
        differ = (got != want[f]).any(axis=-1)
        assert differ.mean() <= 0.01 and not (differ & ~np.any([near_tie(m) for m in maps], axis=0)).any(), "frame %d: %d pixels differ" % (f, differ.sum())
    dest, _ = run_program(exe, tmp_path, shape, bits)
    assert sorted(os.listdir(dest)) == ["%06d.jpg" % f for f in range(PC.CAPTURE_FRAMES)]
    pngs = tmp_path / "out_png_0"
    for f in range(PC.CAPTURE_FRAMES):
        px = np.array(Image.open(os.path.join(pngs, "%06d.png" % f)).convert("RGB"))[..., ::-1]
        im = Image.open(os.path.join(dest, "%06d.jpg" % f))
        assert im.format == "JPEG" and im.size == (W, H)
        assert np.array_equal(np.array(im.convert("RGB")), pil_roundtrip(px)), "frame %d" % f
    dest, log = run_program(exe, tmp_path, shape, bits, "png", ["--start_frame", "1", "--frame_count", "1"])
    assert os.listdir(dest) == ["000001.png"] and "Rendering frame 0..." not in log
    got = np.array(Image.open(os.path.join(dest, "000001.png")).convert("RGB"))[..., ::-1]
    # frame 1 alone: every layer is frame 1's (nothing persists from a frame 0 that was not read)
    assert np.array_equal(got, np.array(Image.open(os.path.join(pngs, "000001.png")).convert("RGB"))[..., ::-1])


def test_program(tmp_path):
    check_program(os.path.join(ROOT, "host", "TestHyperPreview"), tmp_path)
