"""Host-side mirror of the reference's operator interface for the stereo-panorama path, over the
C ABI of libs360 (include/s360.h). Names follow the reference:

  RigDescription                      SR/render/RigDescription.h:27-59
  make_optical_flow_by_name           SR/optical_flow/OpticalFlowFactory.h:23-64
  OpticalFlow.compute_optical_flow    SR/optical_flow/OpticalFlowInterface.h:34-41
  NovelViewGeneratorAsymmetricFlow    SR/optical_flow/NovelView.h:160-190
  bicubic_remap_to_spherical          SR/render/ImageWarper.h:59-66
  flatten_layers_deghost_prefer_base, offset_horizontal_wrap, feather_alpha_channel   SR/util/CvUtil.h
  StereoPanoramaRenderer.render       renderStereoPanorama, SR/test/TestRenderStereoPanorama.cpp:716-972

Everything computes on the GPU through libs360; numpy arrays are the cv::Mat stand-ins
(H x W x C uint8, H x W x 2 float32 for flow).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import HINT, S360_CAMERA_BOTTOM2, Camera, Geometry, Params, S360Error, check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def pinned_empty(shape, dtype=np.uint8):
    """A numpy array in page-locked host memory (s360_host_alloc): images uploaded from such an array are sent in place (and
    must stay untouched until Context.uploads_complete() has returned), a download into one is a single DMA transfer.
    Freed with the array."""
    import weakref
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib().s360_host_alloc(max(n, 1))
    if not p:
        raise MemoryError("s360_host_alloc(%d) failed: %s" % (n, lib().s360_last_error(None).decode()))
    raw = (C.c_uint8 * max(n, 1)).from_address(p)
    arr = np.frombuffer(raw, np.uint8, n).view(dtype).reshape(shape)
    weakref.finalize(raw, lib().s360_host_free, p)
    return arr


class VrCamException(S360Error):
    """The reference's exception type for bad arguments / unknown algorithms (VrCamException.h:18-23)."""


class RigDescription:
    """RigDescription(filename): rig JSON -> cameras; rig_side_only = cameras whose group contains 'side'."""

    MAX_CAMS = 64

    def __init__(self, filename):
        arr = (Camera * self.MAX_CAMS)()
        n = check(lib().s360_rig_load_json(str(filename).encode(), arr, self.MAX_CAMS))
        self.rig = (Camera * n)(*arr[:n])
        self.rig_side_only = [c for c in self.rig if c.is_side]
        if not self.rig_side_only:
            raise VrCamException(_capi.ERR_INVALID_ARG, "rig has no side cameras")
        self.top_index = lib().s360_rig_find_top(self.rig, n)
        self.bottom_index = lib().s360_rig_find_bottom(self.rig, n)

    def get_side_camera_count(self):
        return len(self.rig_side_only)

    def get_side_camera_id(self, idx):
        return self.rig_side_only[idx].id.decode()

    def get_top_camera_id(self):
        return self.rig[self.top_index].id.decode()

    def get_bottom_camera2_id(self):
        return self.rig[lib().s360_rig_find_bottom2(self.rig, len(self.rig))].id.decode()

    def get_bottom_camera_id(self):
        return self.rig[self.bottom_index].id.decode()

    def top_camera(self):
        return self.rig[self.top_index]

    def bottom_camera(self):
        return self.rig[self.bottom_index]


def make_params(**kw):
    """The gflags defaults of TestRenderStereoPanorama.cpp:44-70."""
    p = Params()
    p.interpupilary_dist = 6.4
    p.zero_parallax_dist = 10000.0
    p.sharpening = 0.0
    p.side_alpha_feather_size = 100
    p.std_alpha_feather_size = 31
    p.enable_top = 0
    p.enable_bottom = 0
    p.eqr_width = 256
    p.eqr_height = 128
    p.final_eqr_width = 3480
    p.final_eqr_height = 960
    p.side_flow_alg = b"pixflow_low"
    p.polar_flow_alg = b"pixflow_low"
    p.enable_pole_removal = 0
    p.poleremoval_flow_alg = b"pixflow_low"
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown flag: " + k)
        setattr(p, k, v.encode() if isinstance(v, str) else v)
    return p


class Context:
    """One s360_ctx: one GPU, its stream and its persistent HBM buffers."""

    def __init__(self, rig, params=None, device=0):
        self.rig = rig
        self.params = params if params is not None else make_params()
        h = C.c_void_p()
        check(lib().s360_create(C.byref(h), int(device), rig.rig, len(rig.rig), C.byref(self.params)))
        self.h = h
        g = Geometry()
        check(lib().s360_get_geometry(self.h, C.byref(g)), self.h)
        self.geometry = g

    def close(self):
        if getattr(self, "h", None):
            lib().s360_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        return check(rc, self.h)

    def synchronize(self):
        self._ck(lib().s360_synchronize(self.h))

    @property
    def stream(self):
        return lib().s360_stream(self.h)

    # ---- operators --------------------------------------------------------------------------
    def compute_optical_flow(self, i0, i1, alg="pixflow_low", hint="UNKNOWN", prev_flow=None, prev_i0=None,
                             prev_i1=None):
        i0, i1 = _u8(i0), _u8(i1)
        batched = i0.ndim == 4
        b = i0.shape[0] if batched else 1
        h, w = i0.shape[-3], i0.shape[-2]
        flow = np.empty(i0.shape[:-1] + (2,), np.float32)
        pf = np.ascontiguousarray(prev_flow, np.float32) if prev_flow is not None else None
        p0 = _u8(prev_i0) if prev_i0 is not None else None
        p1 = _u8(prev_i1) if prev_i1 is not None else None
        rc = lib().s360_compute_optical_flow_batch(self.h, alg.encode(), b, _p(i0), _p(i1), w, h, _p(pf), _p(p0), _p(p1),
                                                   HINT[hint], _p(flow))
        if rc == _capi.ERR_UNKNOWN_ALG:
            raise VrCamException(rc, "unrecognized flow algorithm name: " + alg)
        self._ck(rc)
        return flow

    def debug_flow_levels(self, i0, i1, alg="pixflow_low", hint="UNKNOWN"):
        i0, i1 = _u8(i0), _u8(i1)
        h, w = i0.shape[:2]
        cap = w * h * 8
        buf = np.empty(cap, np.float32)
        n = C.c_int()
        self._ck(lib().s360_debug_flow_levels(self.h, alg.encode(), _p(i0), _p(i1), w, h, HINT[hint], _p(buf),
                                              C.c_size_t(cap), C.byref(n)))
        return buf, n.value

    def debug_entry_downscale(self, src, dw, dh, generic=False, keep_down=True):
        """PixFlow's entry on a stack of BGRA images: (resized images or None, grey planes, alpha planes, tiled kernel taken)."""
        src = _u8(src)
        b, sh, sw = src.shape[:3]
        down = np.empty((b, dh, dw, 4), np.uint8) if keep_down else None
        gray = np.empty((b, dh, dw), np.float32)
        alpha = np.empty((b, dh, dw), np.float32)
        tiled = C.c_int()
        self._ck(lib().s360_debug_entry_downscale(self.h, _p(src), sw, sh, b, dw, dh, 1 if generic else 0, _p(down), _p(gray),
                                                  _p(alpha), C.byref(tiled)))
        return down, gray, alpha, bool(tiled.value)

    def debug_upscale_blur(self, src_flow, dw, dh, post_scale, generic=False):
        """PixFlow's final step on a stack of flows (b x sh x sw x 2): (resized, scaled and blurred flows, tiled kernel taken)."""
        src = np.ascontiguousarray(src_flow, np.float32)
        b, sh, sw = src.shape[:3]
        out = np.empty((b, dh, dw, 2), np.float32)
        tiled = C.c_int()
        self._ck(lib().s360_debug_upscale_blur(self.h, _p(src), sw, sh, b, dw, dh, C.c_float(post_scale), 1 if generic else 0,
                                               _p(out), C.byref(tiled)))
        return out, bool(tiled.value)

    def debug_flow_level(self, gray, alpha, i0, i1, initial_flow=None, alg="pixflow_low", hint="UNKNOWN", prev_flow=None, motion=None,
                         prev_scale=1.0, want=None):
        """One pyramid level of the flow engine (include/s360_debug_flow_level.h) on N grey and N alpha planes (N x h x w) for the
        flows i0[b] -> i1[b], in the context's sweep mode. Returns ({stage: array}, {info name: int}); `want` names the stages
        to hand out (default: all that exist for the call — no "diffused" with previous state)."""
        gray, alpha = np.ascontiguousarray(gray, np.float32), np.ascontiguousarray(alpha, np.float32)
        n, h, w = gray.shape
        assert alpha.shape == gray.shape
        i0, i1 = np.ascontiguousarray(i0, np.int32), np.ascontiguousarray(i1, np.int32)
        b = len(i0)
        f32 = lambda a, shape: None if a is None else np.ascontiguousarray(a, np.float32).reshape(shape)  # noqa: E731
        init, prev, mo = f32(initial_flow, (b, h, w, 2)), f32(prev_flow, (b, h, w, 2)), f32(motion, (n, h, w))
        shapes = {"gradients": ((n, h, w, 2), np.float32), "updated": ((b, h, w), np.uint8), "row_flags": ((b, h), np.uint32)}
        names = [f[0] for f in _capi.FlowLevelOut._fields_]
        if want is None:
            want = [k for k in names if not (k == "diffused" and prev is not None)]
        out = {k: np.empty(*shapes.get(k, ((b, h, w, 2), np.float32))) for k in want}
        o = _capi.FlowLevelOut(**{k: _p(v) for k, v in out.items()})
        info = np.zeros(_capi.FLOW_LEVEL_INFO_COUNT, np.int32)
        self._ck(lib().s360_debug_flow_level(self.h, _p(gray), _p(alpha), n, w, h, _p(i0), _p(i1), b, _p(init), alg.encode(), HINT[hint],
                                             _p(prev), _p(mo), C.c_float(prev_scale), C.byref(o), _p(info)))
        return out, dict(zip(_capi.FLOW_LEVEL_INFO, (int(v) for v in info)))

    def debug_flow_prepare(self, images, i0, i1, prev_images=None, prev_flows=None, alg="pixflow_low", fill=0xFF, max_levels=64):
        """The flow engine's preparation (include/s360_debug_flow_pyramid.h) on N BGRA images (N x h x w x 4) for the flows
        i0[b] -> i1[b], optionally with N previous images and B previous flows (B x h x w x 2). Returns {"sizes": [(w, h)] finest
        first, "gray", "alpha": per level N x h x w}, and with previous state {"prev": per level B x h x w x 2 (before the level's
        factor), "motion": per level N x h x w, "factors": float32 per level}. fill: the byte every engine buffer the preparation
        writes holds before it runs (None: left as the last call left them)."""
        images = _u8(images)
        n, h, w = images.shape[:3]
        assert images.shape == (n, h, w, 4)
        i0, i1 = np.ascontiguousarray(i0, np.int32), np.ascontiguousarray(i1, np.int32)
        b = len(i0)
        assert len(i1) == b
        use_prev = prev_images is not None or prev_flows is not None
        pim = _u8(prev_images).reshape(n, h, w, 4) if prev_images is not None else None
        pfl = np.ascontiguousarray(prev_flows, np.float32).reshape(b, h, w, 2) if prev_flows is not None else None
        # room for any pyramid of x0.9 levels: sum of 0.81^l < 5.3, plus the roundings up of max_levels levels
        cap = 6 * max(w // 2, 1) * max(h // 2, 1) + 2 * max_levels * (w // 2 + h // 2 + 1)
        lw, lh = np.zeros(max_levels, np.int32), np.zeros(max_levels, np.int32)
        nl = C.c_int()
        factors = np.zeros(max_levels, np.float32)
        byte = 0 if fill is None else fill
        pyr = np.full(2 * n * cap * 4, byte, np.uint8).view(np.float32)
        prev = np.full(b * cap * 8, byte, np.uint8).view(np.float32) if use_prev else None
        motion = np.full(n * cap * 4, byte, np.uint8).view(np.float32) if use_prev else None
        o = _capi.FlowPrepareOut(max_levels, cap, _p(lw), _p(lh), C.cast(C.byref(nl), C.c_void_p), _p(factors), _p(pyr), _p(prev), _p(motion))
        self._ck(lib().s360_debug_flow_prepare(self.h, _p(images), n, w, h, _p(i0), _p(i1), b, _p(pim), _p(pfl), alg.encode(),
                                               -1 if fill is None else fill, C.byref(o)))
        sizes = [(int(lw[k]), int(lh[k])) for k in range(nl.value)]
        out = {"sizes": sizes, "gray": [], "alpha": []}
        if use_prev:
            out.update(prev=[], motion=[], factors=factors[:nl.value].copy())
        off = 0
        for a, c in sizes:
            px = a * c
            lvl = pyr[2 * n * off:2 * n * (off + px)].reshape(2, n, c, a)
            out["gray"].append(lvl[0])
            out["alpha"].append(lvl[1])
            if use_prev:
                out["prev"].append(prev[2 * b * off:2 * b * (off + px)].reshape(b, c, a, 2))
                out["motion"].append(motion[n * off:n * (off + px)].reshape(n, c, a))
            off += px
        return out

    def debug_resize_linear_f32(self, src, dw, dh, post_scale=1.0, do_scale=False, fill=0xFF):
        """The pyramids' INTER_LINEAR resize (include/s360_debug_flow_pyramid.h) of B planes (B x sh x sw: one channel, or
        B x sh x sw x 2: two interleaved) through the engine's launcher: (result, tiled kernel taken). Every byte of the result
        is `fill` before the launch."""
        src = np.ascontiguousarray(src, np.float32)
        b, sh, sw = src.shape[:3]
        cn = 1 if src.ndim == 3 else src.shape[3]
        dst = np.full((b, dh, dw) + src.shape[3:], fill * 0x01010101, np.uint32).view(np.float32)
        tiled = C.c_int()
        self._ck(lib().s360_debug_resize_linear_f32(self.h, _p(src), sw, sh, cn, b, dw, dh, C.c_float(post_scale), 1 if do_scale else 0,
                                                    _p(dst), C.cast(C.byref(tiled), C.c_void_p)))
        return dst, bool(tiled.value)

    def debug_resize_linear_f32_kernel(self, sw, sh, dw, dh, cn=1):
        """True if the launcher takes the tiled kernel for the shape; nothing is launched."""
        tiled = C.c_int(-1)
        self._ck(lib().s360_debug_resize_linear_f32(self.h, None, sw, sh, cn, 1, dw, dh, C.c_float(1.0), 0, None,
                                                    C.cast(C.byref(tiled), C.c_void_p)))
        return bool(tiled.value)

    def debug_resize_cubic_flow(self, src, dw, dh, post_scale=1.0, through_table=False, fill=0xFF):
        """The flows' INTER_CUBIC resize and scalar multiply (include/s360_debug_flow_pyramid.h) of B flows (B x sh x sw x 2) through
        the engine's launcher, the sources as one array or as one allocation each behind a pointer table: (result, tiled kernel
        taken). Every byte of the result is `fill` before the launch."""
        src = np.ascontiguousarray(src, np.float32)
        b, sh, sw = src.shape[:3]
        assert src.shape == (b, sh, sw, 2)
        dst = np.full((b, dh, dw, 2), fill * 0x01010101, np.uint32).view(np.float32)
        tiled = C.c_int()
        self._ck(lib().s360_debug_resize_cubic_flow(self.h, _p(src), sw, sh, b, dw, dh, C.c_float(post_scale), 1 if through_table else 0,
                                                    _p(dst), C.cast(C.byref(tiled), C.c_void_p)))
        return dst, bool(tiled.value)

    def debug_resize_cubic_flow_kernel(self, sw, sh, dw, dh, through_table=False):
        """True if the launcher takes the tiled kernel for the shape; nothing is launched."""
        tiled = C.c_int(-1)
        self._ck(lib().s360_debug_resize_cubic_flow(self.h, None, sw, sh, 1, dw, dh, C.c_float(1.0), 1 if through_table else 0, None,
                                                    C.cast(C.byref(tiled), C.c_void_p)))
        return bool(tiled.value)

    def debug_remap_packed(self, src, mp, alpha_mode=0, y_feather_start=0, feather_size=1, weights=0, fill=0):
        """The frame's packed bicubic remap (include/s360_debug_remap.h) of B BGRA sources (B x sh x sw x 4) through B maps
        (B x dh x dw x 2). Returns (images B x dh x dw x 4, packed dwords B x dh x dw, tile records B x ty x tx x 4); every byte of
        the three is `fill` before the launches."""
        src, mp = _u8(src), np.ascontiguousarray(mp, np.float32)
        b, sh, sw = src.shape[:3]
        dh, dw = mp.shape[1:3]
        assert src.shape == (b, sh, sw, 4) and mp.shape == (b, dh, dw, 2)
        dst = np.full((b, dh, dw, 4), fill, np.uint8)
        packed = np.full((b, dh, dw), fill * 0x01010101, np.uint32)
        tiles = np.full((b, -(-dh // 16), -(-dw // 64), 4), fill * 0x01010101, np.uint32).view(np.int32)
        self._ck(lib().s360_debug_remap_packed(self.h, _p(src), sw, sh, _p(mp), dw, dh, b, alpha_mode, y_feather_start, feather_size,
                                               weights, _p(dst), _p(packed), _p(tiles)))
        return dst, packed, tiles

    def debug_pole_warp_packed(self, ext_fisheye, flow, pole_camera_radius, phi_ramp_start, phi_mid, phi_ramp_end, fill=0):
        """poleToSideFlow's ramped warp of an extended fisheye image (rows x extW x 4) by a flow (rows x extW x 2) through the
        frame's launcher: (warped image, packed dwords, tile records), pre-filled as in debug_remap_packed."""
        src, fl = _u8(ext_fisheye), np.ascontiguousarray(flow, np.float32)
        rows, ext_w = src.shape[:2]
        assert src.shape == (rows, ext_w, 4) and fl.shape == (rows, ext_w, 2)
        dst = np.full((rows, ext_w, 4), fill, np.uint8)
        packed = np.full((rows, ext_w), fill * 0x01010101, np.uint32)
        tiles = np.full((-(-rows // 16), -(-ext_w // 64), 4), fill * 0x01010101, np.uint32).view(np.int32)
        self._ck(lib().s360_debug_pole_warp_packed(self.h, _p(src), ext_w, rows, _p(fl), pole_camera_radius, phi_ramp_start, phi_mid,
                                                   phi_ramp_end, _p(dst), _p(packed), _p(tiles)))
        return dst, packed, tiles

    def debug_remap_by_flow(self, src, flow, fill=0):
        """Pole removal's warp: the BGRA image (h x w x 4) sampled at (x, y) + flow (h x w x 2); the output pre-filled with `fill`."""
        src, fl = _u8(src), np.ascontiguousarray(flow, np.float32)
        h, w = src.shape[:2]
        assert src.shape == (h, w, 4) and fl.shape == (h, w, 2)
        dst = np.full((h, w, 4), fill, np.uint8)
        self._ck(lib().s360_debug_remap_by_flow(self.h, _p(src), w, h, _p(fl), _p(dst)))
        return dst

    def debug_cubemap_tiles(self, eyes, fw, fh, fmt="video", lds_pixels=4096, fill=0):
        """The cubemap of every frame (include/s360_debug_cubemap.h) of S pairs of BGRA eyes (S x 2 x sh x sw x 4) through the
        frame's map construction and launchers. Returns (stacked BGR cubemaps S x oh x ow x 3, face maps 6 x fh x fw x 2, packed
        dwords of one eye's half oh / 2 x ow, tile records 6 x ty x tx x 4); every byte of the four is `fill` before the launches."""
        eyes = _u8(eyes)
        s, two, sh, sw = eyes.shape[:4]
        assert eyes.shape == (s, 2, sh, sw, 4)
        video = {"video": 1, "photo": 0}[fmt]
        ow, oh = (3 * fw, 4 * fh) if video else (fw, 12 * fh)
        out = np.full((s, oh, ow, 3), fill, np.uint8)
        maps = np.full((6, fh, fw, 2), fill * 0x01010101, np.uint32).view(np.float32)
        packed = np.full((oh // 2, ow), fill * 0x01010101, np.uint32)
        tiles = np.full((6, -(-fh // 16), -(-fw // 16), 4), fill * 0x01010101, np.uint32).view(np.int32)
        self._ck(lib().s360_debug_cubemap_tiles(self.h, _p(eyes), s, sw, sh, fw, fh, video, lds_pixels, _p(out), _p(maps), _p(packed),
                                                _p(tiles)))
        return out, maps, packed, tiles

    def debug_cubemap(self, eyes, fw, fh, fmt="video", fill=0):
        """The on-demand cubemap kernel (one thread per pixel) on the same eyes and maps: (stacked BGR cubemaps, face maps)."""
        eyes = _u8(eyes)
        s, two, sh, sw = eyes.shape[:4]
        assert eyes.shape == (s, 2, sh, sw, 4)
        video = {"video": 1, "photo": 0}[fmt]
        ow, oh = (3 * fw, 4 * fh) if video else (fw, 12 * fh)
        out = np.full((s, oh, ow, 3), fill, np.uint8)
        maps = np.full((6, fh, fw, 2), fill * 0x01010101, np.uint32).view(np.float32)
        self._ck(lib().s360_debug_cubemap(self.h, _p(eyes), s, sw, sh, fw, fh, video, _p(out), _p(maps)))
        return out, maps

    def spherical_warp_map(self, cam, dw, dh, l, r, t, b):
        m = np.empty((dh, dw, 2), np.float32)
        self._ck(lib().s360_spherical_warp_map(self.h, _p(m), dw, dh, C.byref(cam), C.c_float(l), C.c_float(r),
                                               C.c_float(t), C.c_float(b)))
        return m

    def bicubic_remap_to_spherical(self, src, cam, dw, dh, dc, l, r, t, b):
        src = _u8(src)
        dst = np.empty((dh, dw, dc), np.uint8)
        self._ck(lib().s360_bicubic_remap_to_spherical(self.h, _p(dst), dw, dh, dc, _p(src), src.shape[1], src.shape[0],
                                                       src.shape[2], C.byref(cam), C.c_float(l), C.c_float(r),
                                                       C.c_float(t), C.c_float(b)))
        return dst

    def combine_lazy_novel_views(self, image_l, image_r, flow_l_to_r, flow_r_to_l):
        g = self.geometry
        w = self.params.eqr_width // self.rig.get_side_camera_count()
        cl = np.empty((g.cam_image_height, w, 4), np.uint8)
        cr = np.empty_like(cl)
        self._ck(lib().s360_combine_lazy_novel_views(
            self.h, _p(_u8(image_l)), _p(_u8(image_r)), _p(np.ascontiguousarray(flow_l_to_r, np.float32)),
            _p(np.ascontiguousarray(flow_r_to_l, np.float32)), _p(cl), _p(cr)))
        return cl, cr

    def generate_novel_views(self, img_l, img_r, flow_l_to_r, flow_r_to_l, shifts, want_sides=False):
        """generateNovelView (NovelView.cpp:156-172) for every shift_from_left in `shifts`: merged views [n][h][w][4], and with
        want_sides also the two warped images (merged, from_l, from_r)."""
        il, ir = _u8(img_l), _u8(img_r)
        h, w = il.shape[:2]
        sh = np.ascontiguousarray(np.atleast_1d(shifts), np.float64)
        n = sh.shape[0]
        merged = np.empty((n, h, w, 4), np.uint8)
        fl, fr = (np.empty_like(merged), np.empty_like(merged)) if want_sides else (None, None)
        self._ck(lib().s360_generate_novel_views(
            self.h, _p(il), _p(ir), _p(np.ascontiguousarray(flow_l_to_r, np.float32)),
            _p(np.ascontiguousarray(flow_r_to_l, np.float32)), w, h, _p(sh), n, _p(merged), _p(fl), _p(fr)))
        return (merged, fl, fr) if want_sides else merged

    def interpolate_views(self, img_l, img_r, shifts, alg="pixflow_low", want_sides=False, want_flows=False):
        """NovelViewGeneratorAsymmetricFlow::prepare + generateNovelView per shift, flows kept on the device in between.
        Returns merged, then (from_l, from_r) with want_sides, then (flow_l_to_r, flow_r_to_l) with want_flows."""
        il, ir = _u8(img_l), _u8(img_r)
        h, w = il.shape[:2]
        sh = np.ascontiguousarray(np.atleast_1d(shifts), np.float64)
        n = sh.shape[0]
        merged = np.empty((n, h, w, 4), np.uint8)
        fl, fr = (np.empty_like(merged), np.empty_like(merged)) if want_sides else (None, None)
        flr, frl = (np.empty((h, w, 2), np.float32), np.empty((h, w, 2), np.float32)) if want_flows else (None, None)
        rc = lib().s360_interpolate_views(self.h, alg.encode(), _p(il), _p(ir), w, h, _p(sh), n, _p(merged), _p(fl), _p(fr),
                                          _p(flr), _p(frl))
        if rc == _capi.ERR_UNKNOWN_ALG:
            raise VrCamException(rc, "unrecognized flow algorithm name: " + alg)
        self._ck(rc)
        out = (merged,) + ((fl, fr) if want_sides else ()) + ((flr, frl) if want_flows else ())
        return out if len(out) > 1 else merged

    def flatten_layers_deghost_prefer_base(self, bottom_layer, top_layer):
        b, t = _u8(bottom_layer), _u8(top_layer)
        out = np.empty_like(b)
        self._ck(lib().s360_flatten_layers_deghost_prefer_base(self.h, _p(b), _p(t), b.shape[1], b.shape[0], _p(out)))
        return out

    def offset_horizontal_wrap(self, src, offset):
        s = _u8(src)
        out = np.empty_like(s)
        self._ck(lib().s360_offset_horizontal_wrap(self.h, _p(s), s.shape[1], s.shape[0], s.shape[2], C.c_float(offset),
                                                   _p(out)))
        return out

    def feather_alpha_channel(self, src, erode_size):
        s = _u8(src)
        out = np.empty_like(s)
        self._ck(lib().s360_feather_alpha_channel(self.h, _p(s), s.shape[1], s.shape[0], int(erode_size), _p(out)))
        return out

    def pole_to_side_flow(self, side, pole, want_flow=False):
        side, pole = _u8(side), _u8(pole)
        out = np.empty_like(side)
        rows = pole.shape[0]
        fl = None
        if want_flow:
            fl = np.empty((rows, int(np.float32(side.shape[1]) * np.float32(1.2)), 2), np.float32)
        self._ck(lib().s360_pole_to_side_flow(self.h, _p(side), _p(pole), rows, _p(out), _p(fl)))
        return (out, fl) if want_flow else out

    def sharpen(self, bgr, sharpening):
        b = _u8(bgr).copy()
        self._ck(lib().s360_sharpen(self.h, _p(b), b.shape[1], b.shape[0], C.c_float(sharpening)))
        return b

    # ---- frame level -----------------------------------------------------------------------
    def upload_frame(self, side, top=None, bottom=None):
        for i, s in enumerate(side):
            s = _u8(s)
            self._ck(lib().s360_frame_upload_side(self.h, i, _p(s), s.shape[1], s.shape[0], s.shape[2]))
        if top is not None:
            t = _u8(top)
            self._ck(lib().s360_frame_upload_top(self.h, _p(t), t.shape[1], t.shape[0]))
        if bottom is not None:
            b = _u8(bottom)
            self._ck(lib().s360_frame_upload_bottom(self.h, _p(b), b.shape[1], b.shape[0]))

    def upload_raw(self, isp, camera, raw16):
        """A camera's raw Bayer frame (H x W uint16) through `isp` (surround360_amd.isp.CameraIsp, output_bpp 16) into
        this frame's source slot on the device. camera: side index, -1 top, -2 bottom, -3 (S360_CAMERA_BOTTOM2, on a context with
        enable_pole_removal) the secondary bottom camera."""
        r = np.ascontiguousarray(raw16, np.uint16)
        self._ck(lib().s360_frame_upload_raw(self.h, isp.h, int(camera), _p(r), r.shape[1], r.shape[0]))

    def upload_packed(self, isp, camera, frame, bits, w, h):
        """The same from the sensor's packed bytes of one w x h frame (8 or 12 bits per pixel, as in a capture's .bin container)."""
        fr = np.ascontiguousarray(frame, np.uint8)
        self._ck(lib().s360_frame_upload_packed(self.h, isp.h, int(camera), _p(fr), int(bits), int(w), int(h)))

    def upload_pole_removal(self, bottom2, mask, mask2):
        """Secondary bottom camera image + the two red pole masks (BGR) for enable_pole_removal (PoleRemoval.cpp:48-66)."""
        b2, m1, m2 = _u8(bottom2), _u8(mask), _u8(mask2)
        assert b2.shape == m1.shape == m2.shape and b2.shape[2] == 3
        self._ck(lib().s360_frame_upload_pole_removal(self.h, _p(b2), _p(m1), _p(m2), b2.shape[1], b2.shape[0]))

    def upload_bottom2(self, bottom2):
        """s360_frame_upload_bottom2: the secondary bottom camera's image (BGR) alone; the masks are the context's (set_pole_masks)."""
        b2 = _u8(bottom2)
        assert b2.ndim == 3 and b2.shape[2] == 3
        self._ck(lib().s360_frame_upload_bottom2(self.h, _p(b2), b2.shape[1], b2.shape[0]))

    def set_pole_masks(self, mask=None, mask2=None):
        """s360_set_pole_masks: the two red pole masks (BGR) as state of the context, shared by its frame slots; pole removal's alpha
        planes are computed once. No arguments: the masks are cleared."""
        if mask is None and mask2 is None:
            self._ck(lib().s360_set_pole_masks(self.h, None, None, 0, 0))
            return
        m1, m2 = _u8(mask), _u8(mask2)
        assert m1.shape == m2.shape and m1.ndim == 3 and m1.shape[2] == 3
        self._ck(lib().s360_set_pole_masks(self.h, _p(m1), _p(m2), m1.shape[1], m1.shape[0]))

    # ---- frame slots: several independent frames through one launch sequence ----
    def set_frame_slots(self, n):
        self._ck(lib().s360_set_frame_slots(self.h, int(n)))

    def select_frame_slot(self, k):
        self._ck(lib().s360_select_frame_slot(self.h, int(k)))

    def render_batch(self, use_prev=False):
        self._ck(lib().s360_frame_render_batch(self.h, int(use_prev)))

    def render_slots(self, slots, use_prev=False):
        """s360_frame_render_slots: the given frame slots (ascending) as one batch."""
        arr = (C.c_int * len(slots))(*slots)
        self._ck(lib().s360_frame_render_slots(self.h, arr, len(slots), int(use_prev)))

    def render(self, use_prev=False):
        self._ck(lib().s360_frame_render(self.h, int(use_prev)))

    def render_pairs(self, p0, p1, use_prev=False):
        self._ck(lib().s360_frame_render_pairs(self.h, p0, p1, int(use_prev)))

    def finish(self, pole_mask=15, use_prev=False):
        self._ck(lib().s360_frame_finish(self.h, pole_mask, int(use_prev)))

    # ---- multi-GPU: sharded frame + native RCCL strip gather (s360.h, "multi-GPU") ----
    @staticmethod
    def comm_get_unique_id():
        buf = C.create_string_buffer(128)
        check(lib().s360_comm_get_unique_id(buf))
        return buf.raw

    @staticmethod
    def comm_library_path():
        """The file the RCCL entry points were resolved from (None: no librccl could be loaded)."""
        p = lib().s360_comm_library_path()
        return p.decode() if p else None

    def comm_init_rank(self, unique_id, rank, nranks):
        self._ck(lib().s360_comm_init_rank(self.h, C.c_char_p(unique_id), int(rank), int(nranks)))

    def comm_destroy(self):
        self._ck(lib().s360_comm_destroy(self.h))

    def comm_size(self):
        """ncclCommCount of the context's communicator (0: it has none)."""
        n = lib().s360_comm_size(self.h)
        if n < 0:
            self._ck(-1)
        return n

    def comm_rank(self):
        return lib().s360_comm_rank(self.h)

    def comm_stats(self, which):
        """{calls, bytes_sent, bytes_received} of exchange `which` (0 strips, 1 pole layers) since the communicator was made."""
        out = (C.c_ulonglong * 3)()
        self._ck(lib().s360_comm_stats(self.h, int(which), out))
        return {"calls": int(out[0]), "bytes_sent": int(out[1]), "bytes_received": int(out[2])}

    def gather_strips(self, bounds, root=0):
        arr = (C.c_int * len(bounds))(*bounds)
        self._ck(lib().s360_frame_gather_strips(self.h, arr, int(root)))

    def exchange_strips(self, bounds, need_mask):
        b = (C.c_int * len(bounds))(*bounds)
        n = (C.c_int * len(need_mask))(*need_mask)
        self._ck(lib().s360_frame_exchange_strips(self.h, b, n))

    def pole_units(self, pole_mask, use_prev=False):
        self._ck(lib().s360_frame_pole_units(self.h, int(pole_mask), int(bool(use_prev))))

    def gather_pole_layers(self, owner, root=0):
        o = (C.c_int * 4)(*owner)
        self._ck(lib().s360_frame_gather_pole_layers(self.h, o, int(root)))

    def composite(self, pole_mask=15):
        self._ck(lib().s360_frame_composite(self.h, int(pole_mask)))

    def comm_loopback(self, src_pair, dst_pair):
        self._ck(lib().s360_comm_loopback(self.h, int(src_pair), int(dst_pair)))

    def set_partition(self, p0, p1):
        self._ck(lib().s360_frame_set_partition(self.h, int(p0), int(p1)))

    def strip_ptr(self, eye):
        p = C.c_void_p()
        n = C.c_size_t()
        self._ck(lib().s360_frame_strip_ptr(self.h, eye, C.byref(p), C.byref(n)))
        return p.value, n.value

    def equirect_dev(self):
        p = C.c_void_p()
        n = C.c_size_t()
        self._ck(lib().s360_frame_equirect_dev(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def download_equirect(self):
        g = self.geometry
        out = np.empty((g.out_height, g.out_width, 3), np.uint8)
        self._ck(lib().s360_frame_download_equirect(self.h, _p(out)))
        return out

    def download_equirect_of(self, age, out=None):
        """age 0: the frame enqueued last; 1: the one before (fetched while the last one still renders). `out`: a buffer to
        fetch into (pinned_empty: one DMA transfer); the context's lock is released while the call waits for the frame."""
        g = self.geometry
        if out is None:
            out = np.empty((g.out_height, g.out_width, 3), np.uint8)
        assert out.shape == (g.out_height, g.out_width, 3) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        self._ck(lib().s360_frame_download_equirect_of(self.h, int(age), _p(out)))
        return out

    # ---- the equirect as a PNG file, encoded on the device (s360.h; replaces imwriteExceptionOnFail, TRSP:938-961) ----
    def set_output_double_buffer(self, on=True):
        """Two output buffers per slot without frame pipelining: a batch host enqueues step k+1, then fetches step k (age 1)."""
        self._ck(lib().s360_set_output_double_buffer(self.h, int(bool(on))))

    def set_png_encode(self, on=True):
        self._ck(lib().s360_set_png_encode(self.h, int(bool(on))))

    def download_png(self, age=0, out=None):
        """The finished frame as the bytes of a complete PNG file (rendered with set_png_encode(True)). `out`: a uint8 buffer of at
        least s360_frame_png_bound bytes (pinned_empty: one DMA transfer); returns a view of the file's bytes in it."""
        cap = int(lib().s360_frame_png_bound(self.h))
        if out is None:
            out = np.empty(cap, np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0)
        self._ck(lib().s360_frame_download_png(self.h, int(age), _p(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    def encode_png(self, bgr):
        """Operator form: an (h, w, 3) uint8 B,G,R image -> the bytes of a PNG file (8-bit RGB), or an (h, w, 4) B,G,R,A image ->
        an 8-bit RGBA file (alpha kept), encoded on the device."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        h, w = bgr.shape[:2]
        if bgr.shape == (h, w, 4):
            return self.encode_png_c(bgr)
        assert bgr.shape == (h, w, 3)
        out = np.empty(int(lib().s360_png_bound(w, h)), np.uint8)
        n = C.c_size_t(0)
        self._ck(lib().s360_encode_png(self.h, _p(bgr), w, h, _p(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value].tobytes()

    def encode_png_c(self, px, channels=None):
        """s360_encode_png_c: the same encoder with the channel count spelled out (3 or 4; the default is the array's)."""
        px = np.ascontiguousarray(px, np.uint8)
        h, w = px.shape[:2]
        ch = int(px.shape[2] if channels is None else channels)
        cap = int(lib().s360_png_bound_c(w, h, ch))
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_size_t(0)
        self._ck(lib().s360_encode_png_c(self.h, _p(px), w, h, ch, _p(out), C.c_size_t(cap), C.byref(n)))
        return out[:n.value].tobytes()

    def encode_png16(self, bgr16, cap=None):
        """s360_encode_png16: an (h, w, 3) uint16 B,G,R image -> the bytes of a 16-bit RGB PNG file, encoded on the device. `cap`: the
        buffer size to offer instead of s360_png_bound_16 (a smaller one is refused)."""
        px = np.ascontiguousarray(bgr16, np.uint16)
        h, w = px.shape[:2]
        assert px.shape == (h, w, 3)
        bound = int(lib().s360_png_bound_16(w, h))
        cap = bound if cap is None else int(cap)
        out = np.empty(max(bound, cap, 1), np.uint8)
        n = C.c_size_t(0)
        self._ck(lib().s360_encode_png16(self.h, _p(px), w, h, _p(out), C.c_size_t(cap), C.byref(n)))
        return out[:n.value].tobytes()

    def encode_png_batch(self, images):
        """s360_encode_png_batch: a list of (h, w, 3) / (h, w, 4) uint8 images of any sizes -> the list of their PNG files, encoded
        by one launch sequence on the device."""
        imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
        k = len(imgs)
        assert k > 0 and all(a.ndim == 3 and a.shape[2] in (3, 4) for a in imgs)
        outs = [np.empty(int(lib().s360_png_bound_c(a.shape[1], a.shape[0], a.shape[2])), np.uint8) for a in imgs]
        ints = lambda v: (C.c_int * k)(*v)  # noqa: E731
        n = (C.c_size_t * k)()
        self._ck(lib().s360_encode_png_batch(
            self.h, k, (C.c_void_p * k)(*[a.ctypes.data for a in imgs]), ints([a.shape[1] for a in imgs]), ints([a.shape[0] for a in imgs]),
            ints([a.shape[2] for a in imgs]), (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*[o.size for o in outs]), n))
        return [o[:n[i]].tobytes() for i, o in enumerate(outs)]

    def encode_state_pngs(self, names_idx):
        """s360_frame_encode_state_pngs: enqueues the batched encode of the named 4-channel intermediates of the selected slot's
        latest frame — a list of (name, idx) with the names of get_u8 — behind that frame's kernels. Waits for nothing; the files
        are fetched with download_state_png(i), i the position in this list."""
        k = len(names_idx)
        names = (C.c_char_p * k)(*[n.encode() for n, _ in names_idx])
        self._ck(lib().s360_frame_encode_state_pngs(self.h, k, names, (C.c_int * k)(*[int(i) for _, i in names_idx])))

    def download_state_png(self, i, out=None):
        """File i of the last encode_state_pngs call: a view of its bytes in `out` (a uint8 buffer; default: one of the file's bound)."""
        if out is None:
            out = np.empty(max(int(lib().s360_frame_state_png_bound(self.h, int(i))), 1), np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0)
        self._ck(lib().s360_frame_download_state_png(self.h, int(i), _p(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    def decode_png_batch(self, files, caps=None, outs=None):
        """s360_decode_png_batch: a list of banded PNG files (bytes) -> the list of their images, (h, w, 3) B,G,R or (h, w, 4)
        B,G,R,A uint8 arrays, decoded by one launch sequence on the device. `caps`: output buffer sizes to offer instead of the
        images' own (a smaller one is refused); `outs`: uint8 buffers to decode into (default: new ones of those sizes)."""
        k = len(files)
        assert k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        whc = []
        for f in bufs:
            d = png_decodable(f)
            whc.append(d[:3] if d else (0, 0, 0))
        sizes = [w * h * c for w, h, c in whc] if caps is None else [int(v) for v in caps]
        if outs is None:
            outs = [np.empty(max(n, 1), np.uint8) for n in sizes]
        got = (C.c_int * (3 * k))()
        self._ck(lib().s360_decode_png_batch(
            self.h, k, (C.c_void_p * k)(*[b.ctypes.data for b in bufs]), (C.c_size_t * k)(*[b.size for b in bufs]),
            (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*sizes), got))
        return [o[:got[3 * i] * got[3 * i + 1] * got[3 * i + 2]].reshape(got[3 * i + 1], got[3 * i], got[3 * i + 2]) for i, o in enumerate(outs)]

    def png_decode_stats(self):
        """s360_png_decode_stats: (fast-path bands, general-path bands, stored-only bands, most speculation rounds) of the last
        decode call on this context."""
        v = (C.c_uint64 * 4)()
        self._ck(lib().s360_png_decode_stats(self.h, v))
        return tuple(int(x) for x in v)

    def png_decode_round_histogram(self):
        """hist[r] = fast-path bands of the last decode call whose slowest window took r speculation rounds (66 entries)."""
        v = (C.c_uint64 * 66)()
        self._ck(lib().s360_png_decode_round_histogram(self.h, v))
        return [int(x) for x in v]

    def png_decode_failure(self):
        """s360_png_decode_failure: (image index or -1, reason) of the last decode call — reason 0 none, 1 not a file of this decoder,
        2 size / channels / buffer mismatch, 3 damaged."""
        image, reason = C.c_int(-1), C.c_int(0)
        self._ck(lib().s360_png_decode_failure(self.h, C.byref(image), C.byref(reason)))
        return image.value, reason.value

    def set_prev_images_png(self, names_idx, files):
        """s360_frame_set_prev_images_png: banded PNG files decoded straight into the previous-state image buffers. names_idx: a
        list of (name, idx) with the names of encode_state_pngs; files: their bytes."""
        k = len(names_idx)
        assert k == len(files) and k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        names = (C.c_char_p * k)(*[n.encode() for n, _ in names_idx])
        self._ck(lib().s360_frame_set_prev_images_png(
            self.h, k, names, (C.c_int * k)(*[int(i) for _, i in names_idx]), (C.c_void_p * k)(*[b.ctypes.data for b in bufs]),
            (C.c_size_t * k)(*[b.size for b in bufs])))

    def decode_input_png_batch(self, files, keep16=False, caps=None, outs=None):
        """s360_decode_input_png_batch: a list of banded PNG files (bytes), 8-bit or 16-bit RGB, -> the list of their images decoded
        by one launch sequence on the device: (h, w, c) uint8 B,G,R(,A); a 16-bit file gives (h, w, 3) uint16 B,G,R if `keep16`, else
        its samples' high bytes as uint8. `caps`: output buffer sizes in bytes to offer instead of the images' own (a smaller one is
        refused); `outs`: uint8 buffers to decode into (default: new ones of those sizes)."""
        k = len(files)
        assert k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        sizes = []
        for f in bufs:
            d = input_png_decodable(f)
            sizes.append(d[0] * d[1] * d[2] * (2 if d[3] == 16 and keep16 else 1) if d else 0)
        if caps is not None:
            sizes = [int(v) for v in caps]
        if outs is None:
            outs = [np.empty(max(n + (n & 1), 2), np.uint8) for n in sizes]
        got = (C.c_int * (5 * k))()
        self._ck(lib().s360_decode_input_png_batch(
            self.h, k, (C.c_void_p * k)(*[b.ctypes.data for b in bufs]), (C.c_size_t * k)(*[b.size for b in bufs]),
            (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*sizes), 1 if keep16 else 0, got))
        res = []
        for i, o in enumerate(outs):
            w, h, c, depth = got[5 * i:5 * i + 4]
            if depth == 16 and keep16:
                res.append(o[:w * h * c * 2].view(np.uint16).reshape(h, w, c))
            else:
                res.append(o[:w * h * c].reshape(h, w, c))
        return res

    def upload_frame_png(self, cameras, files):
        """s360_frame_upload_png: camera images from their banded PNG files (bytes; colour type 2, 8- or 16-bit), decoded on the
        device straight into the frame's source slots. cameras: side indices, -1 (top), -2 (bottom), -3 (S360_CAMERA_BOTTOM2 with
        enable_pole_removal). Synchronous."""
        k = len(cameras)
        assert k == len(files) and k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        self._ck(lib().s360_frame_upload_png(
            self.h, k, (C.c_int * k)(*[int(v) for v in cameras]), (C.c_void_p * k)(*[b.ctypes.data if b.size else None for b in bufs]),
            (C.c_size_t * k)(*[b.size for b in bufs])))

    def decode_input_jpeg_batch(self, files, caps=None, outs=None):
        """s360_decode_input_jpeg_batch: a list of baseline JPEG files (bytes) -> the list of their images, (h, w, 3) uint8 B,G,R,
        decoded by one launch sequence on the device. `caps`: output buffer sizes in bytes to offer instead of the images' own (a
        smaller one is refused); `outs`: uint8 buffers to decode into (default: new ones of those sizes)."""
        k = len(files)
        assert k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        sizes = []
        for f in bufs:
            d = input_jpeg_decodable(f)
            sizes.append(d[0] * d[1] * 3 if d else 0)
        if caps is not None:
            sizes = [int(v) for v in caps]
        if outs is None:
            outs = [np.empty(max(n, 1), np.uint8) for n in sizes]
        got = (C.c_int * (6 * k))()
        self._ck(lib().s360_decode_input_jpeg_batch(
            self.h, k, (C.c_void_p * k)(*[b.ctypes.data if b.size else None for b in bufs]), (C.c_size_t * k)(*[b.size for b in bufs]),
            (C.c_void_p * k)(*[o.ctypes.data for o in outs]), (C.c_size_t * k)(*sizes), got))
        return [o[:got[6 * i] * got[6 * i + 1] * 3].reshape(got[6 * i + 1], got[6 * i], 3) for i, o in enumerate(outs)]

    def upload_jpeg(self, cameras, files):
        """s360_frame_upload_jpeg: camera images from their baseline JPEG files (bytes), decoded on the device straight into the
        frame's source slots. cameras: side indices, -1 (top), -2 (bottom), -3 (S360_CAMERA_BOTTOM2 with enable_pole_removal).
        Synchronous."""
        k = len(cameras)
        assert k == len(files) and k > 0
        bufs = [np.frombuffer(bytes(f), np.uint8) for f in files]
        self._ck(lib().s360_frame_upload_jpeg(
            self.h, k, (C.c_int * k)(*[int(v) for v in cameras]), (C.c_void_p * k)(*[b.ctypes.data if b.size else None for b in bufs]),
            (C.c_size_t * k)(*[b.size for b in bufs])))

    upload_frame_jpeg = upload_jpeg  # an alias beside upload_frame_png; upload_jpeg is the method's name

    def jpeg_decode_stats(self):
        """s360_jpeg_decode_stats of the last JPEG decode call on this context: a dict with files, subsequences, rounds (the
        synchronisation launches), most_file_rounds, ms_entropy, ms_pixels and file_rounds (a list, one entry per file)."""
        counts, ms = (C.c_uint64 * 4)(), (C.c_double * 2)()
        self._ck(lib().s360_jpeg_decode_stats(self.h, counts, ms, None, 0))
        k = int(counts[0])
        fr = (C.c_uint32 * max(k, 1))()
        self._ck(lib().s360_jpeg_decode_stats(self.h, counts, ms, fr, k))
        return {"files": k, "subsequences": int(counts[1]), "rounds": int(counts[2]), "most_file_rounds": int(counts[3]),
                "ms_entropy": float(ms[0]), "ms_pixels": float(ms[1]), "file_rounds": [int(v) for v in fr[:k]]}

    def jpeg_decode_failure(self):
        """s360_jpeg_decode_failure: (image index or -1, reason) of the last JPEG decode call — reason 0 none, 1 not a file of this
        decoder, 2 size / buffer mismatch, 3 invalid code, 4 run past 63, 5 scan ends short, 6 blocks missing, 7 bits left over, 8
        marker inside the scan."""
        image, reason = C.c_int(), C.c_int()
        self._ck(lib().s360_jpeg_decode_failure(self.h, C.byref(image), C.byref(reason)))
        return image.value, reason.value

    def debug_input_jpeg_blocks(self, file):
        """s360_debug_input_jpeg_blocks (test tap): the quantised coefficients the entropy stage left for `file`, (blocks, 64) int16 in
        emission order, natural order inside a block, absolute DC, dummy blocks included."""
        b = np.frombuffer(bytes(file), np.uint8)
        d = input_jpeg_decodable(b)
        n = (-(-d[0] // (8 * d[3]))) * (-(-d[1] // (8 * d[4]))) * (d[3] * d[4] + 2) if d else 1
        out = np.zeros((n, 64), np.int16)
        got = C.c_size_t()
        self._ck(lib().s360_debug_input_jpeg_blocks(self.h, b.ctypes.data if b.size else None, C.c_size_t(b.size), out.ctypes.data, C.c_size_t(n),
                                                    C.byref(got)))
        return out[:got.value]

    def set_prev_flow(self, name, idx, flow):
        """s360_frame_set_prev_flow: one previous-frame flow (the names of get_f32) as (h, w, 2) float32."""
        flow = np.ascontiguousarray(flow, np.float32)
        self._ck(lib().s360_frame_set_prev_flow(self.h, name.encode(), int(idx), _p(flow)))

    def uploads_complete(self):
        """Blocks until every upload enqueued so far has left its host buffer (needed for buffers from pinned_empty only)."""
        self._ck(lib().s360_frame_uploads_complete(self.h))

    def set_sweep_mode(self, mode):
        """'latency' (default) or 'throughput' — which sweep kernel PixFlow uses (bit-identical results)."""
        self._ck(lib().s360_set_sweep_mode(self.h, mode.encode()))

    def set_frame_pipelining(self, on=True):
        """One video stream: overlap the pole stage of frame k with the side stage of frame k+1 (same results)."""
        self._ck(lib().s360_set_frame_pipelining(self.h, 1 if on else 0))

    def cubemap(self, face_width, face_height, fmt="video"):
        """Stereo cubemap of the last rendered frame (TestRenderStereoPanorama.cpp:917-935), BGR."""
        whc = (C.c_int * 3)()
        self._ck(lib().s360_frame_cubemap(self.h, int(face_width), int(face_height), fmt.encode(), whc, None))
        out = np.empty((whc[1], whc[0], 3), np.uint8)
        self._ck(lib().s360_frame_cubemap(self.h, int(face_width), int(face_height), fmt.encode(), whc, _p(out)))
        return out

    # ---- the stereo cubemap of every frame of a stream or batch (s360_set_cubemap_output) ----
    def set_cubemap_output(self, face_width, face_height, fmt="video"):
        """Every frame rendered from now on also leaves its stereo cubemap (face size 0 = off); fetched per frame and slot
        with download_cubemap / download_cubemap_png under the equirect's age contract."""
        self._ck(lib().s360_set_cubemap_output(self.h, int(face_width), int(face_height), fmt.encode()))

    def cubemap_size(self):
        """(width, height, 3) of the stacked cubemap the next frame will leave."""
        whc = (C.c_int * 3)()
        self._ck(lib().s360_frame_cubemap_size(self.h, whc))
        return whc[0], whc[1], whc[2]

    def download_cubemap(self, age=0, slot=None, out=None):
        """The cubemap rendered with the frame (age 0: enqueued last, 1: the one before) of the selected or the named slot, BGR.
        The buffer is sized by the CURRENT setting; a frame rendered under another size has to be fetched before the change."""
        w, h, _ = self.cubemap_size()
        if out is None:
            out = np.empty((h, w, 3), np.uint8)
        assert out.shape == (h, w, 3) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        if slot is None:
            self._ck(lib().s360_frame_download_cubemap(self.h, int(age), _p(out)))
        else:
            self._ck(lib().s360_frame_download_cubemap_slot(self.h, int(slot), int(age), _p(out)))
        return out

    def download_cubemap_png(self, age=0, slot=None, out=None):
        """The same cubemap as the bytes of a complete PNG file (frames rendered with set_png_encode(True))."""
        cap = int(lib().s360_frame_cubemap_png_bound(self.h))
        if out is None:
            out = np.empty(cap, np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0)
        if slot is None:
            self._ck(lib().s360_frame_download_cubemap_png(self.h, int(age), _p(out), C.c_size_t(out.size), C.byref(n)))
        else:
            self._ck(lib().s360_frame_download_cubemap_png_slot(self.h, int(slot), int(age), _p(out), C.c_size_t(out.size), C.byref(n)))
        return out[:n.value]

    # ---- the equirect and the cubemap as JPEG files, encoded on the device (include/s360_frame_jpeg.h) ----
    def set_jpeg_encode(self, on=True, quality=95):
        """Frames enqueued from now on are also encoded as baseline JPEG (quality 1..100, clamped); independent of set_png_encode."""
        self._ck(lib().s360_set_jpeg_encode(self.h, int(bool(on)), int(quality)))

    def jpeg_bound(self):
        return int(lib().s360_frame_jpeg_bound(self.h))

    def cubemap_jpeg_bound(self):
        return int(lib().s360_frame_cubemap_jpeg_bound(self.h))

    def _download_jpeg(self, stem, bound, age, slot, out):
        if out is None:
            out = np.empty(max(bound, 1), np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0)
        if slot is None:
            rc = getattr(lib(), stem)(self.h, int(age), _p(out), C.c_size_t(out.size), C.byref(n))
        else:
            rc = getattr(lib(), stem + "_slot")(self.h, int(slot), int(age), _p(out), C.c_size_t(out.size), C.byref(n))
        self.jpeg_size_needed = n.value  # (what a refused call says the file needs)
        self._ck(rc)
        return out[:n.value]

    def download_jpeg(self, age=0, out=None):
        """The finished frame as the bytes of a complete JPEG file (rendered with set_jpeg_encode(True)): jpegio::encode of the
        pixels download_equirect_of returns. `out`: a uint8 buffer, jpeg_bound() bytes hold every file (pinned_empty: one DMA
        transfer); returns a view of the file's bytes in it."""
        return self._download_jpeg("s360_frame_download_jpeg", self.jpeg_bound(), age, None, out)

    def download_jpeg_slot(self, slot, age=0, out=None):
        return self._download_jpeg("s360_frame_download_jpeg", self.jpeg_bound(), age, slot, out)

    def download_cubemap_jpeg(self, age=0, out=None):
        """The frame's cubemap (set_cubemap_output) as the bytes of a complete JPEG file."""
        return self._download_jpeg("s360_frame_download_cubemap_jpeg", self.cubemap_jpeg_bound(), age, None, out)

    def download_cubemap_jpeg_slot(self, slot, age=0, out=None):
        return self._download_jpeg("s360_frame_download_cubemap_jpeg", self.cubemap_jpeg_bound(), age, slot, out)

    def debug_frame_jpeg(self, bgr, scan_cap, cap=None):
        """include/s360_debug_frame_jpeg.h: `bgr` through the context's frame encoder into a device buffer of scan_cap bytes.
        Returns (file bytes or None, dict(rc, message, n_out, stored, guard_touched, ms))."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        h, w = bgr.shape[:2]
        if cap is None:
            cap = 623 + int(scan_cap) + 2
        out = np.empty(max(int(cap), 1), np.uint8)
        n, stored, guard = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        ms = C.c_float(0)
        rc = lib().s360_debug_frame_jpeg(self.h, _p(bgr), w, h, C.c_size_t(int(scan_cap)), _p(out), C.c_size_t(int(cap)), C.byref(n),
                                         C.byref(stored), C.byref(guard), C.byref(ms))
        msg = lib().s360_last_error(self.h) if rc < 0 else b""
        info = dict(rc=rc, message=msg.decode() if msg else "", n_out=n.value, stored=stored.value, guard_touched=guard.value, ms=ms.value)
        return (out[:n.value].tobytes() if rc == 0 else None), info

    def set_sharpening(self, sharpening):
        """FLAGS_sharpening for the frames rendered from now on (TRSP:56, :901)."""
        self._ck(lib().s360_set_sharpening(self.h, C.c_double(sharpening)))

    def keep_intermediates(self, on=True):
        self._ck(lib().s360_set_keep_intermediates(self.h, int(on)))

    def get_u8(self, name, idx=0):
        whc = (C.c_int * 3)()
        self._ck(lib().s360_frame_get_u8(self.h, name.encode(), idx, whc, None))
        d = np.empty((whc[1], whc[0], whc[2]), np.uint8)
        self._ck(lib().s360_frame_get_u8(self.h, name.encode(), idx, whc, _p(d)))
        return d

    def get_f32(self, name, idx=0):
        whc = (C.c_int * 3)()
        self._ck(lib().s360_frame_get_f32(self.h, name.encode(), idx, whc, None))
        d = np.empty((whc[1], whc[0], whc[2]), np.float32)
        self._ck(lib().s360_frame_get_f32(self.h, name.encode(), idx, whc, _p(d)))
        return d

    # ---- measurement ------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._ck(lib().s360_profile_enable(self.h, int(on)))

    def profile_get(self):
        names = C.create_string_buffer(4096)
        ms = (C.c_float * 64)()
        cnt = (C.c_int * 64)()
        n = self._ck(lib().s360_profile_get(self.h, names, 4096, ms, cnt, 64))
        ns = names.value.decode().split(";") if n else []
        return {ns[i]: (ms[i], cnt[i]) for i in range(n)}


def save_flow_to_file(flow, filename):
    """saveFlowToFile (CvUtil.cpp:159-177)."""
    f = np.ascontiguousarray(flow, np.float32)
    check(lib().s360_save_flow_to_file(str(filename).encode(), _p(f), f.shape[1], f.shape[0]))


def read_flow_from_file(filename):
    """readFlowFromFile (CvUtil.cpp:179-199) -> H x W x 2 float32."""
    w, h = C.c_int(), C.c_int()
    check(lib().s360_read_flow_from_file(str(filename).encode(), None, C.byref(w), C.byref(h), C.c_size_t(0)))
    out = np.empty((h.value, w.value, 2), np.float32)
    check(lib().s360_read_flow_from_file(str(filename).encode(), _p(out), C.byref(w), C.byref(h), C.c_size_t(out.size)))
    return out


# ---- reference-shaped operator objects ----------------------------------------------------------
class OpticalFlow:
    """OpticalFlowInterface implementation returned by make_optical_flow_by_name."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name

    def compute_optical_flow(self, i0_bgra, i1_bgra, prev_flow=None, prev_i0_bgra=None, prev_i1_bgra=None,
                             hint="UNKNOWN"):
        return self.ctx.compute_optical_flow(i0_bgra, i1_bgra, self.name, hint, prev_flow, prev_i0_bgra, prev_i1_bgra)


def make_optical_flow_by_name(ctx, flow_alg_name):
    if flow_alg_name not in ("pixflow_low", "pixflow_search_20"):
        raise VrCamException(_capi.ERR_UNKNOWN_ALG, "unrecognized flow algorithm name: " + flow_alg_name)
    return OpticalFlow(ctx, flow_alg_name)


class NovelViewGeneratorAsymmetricFlow:
    """prepare() computes flowLtoR / flowRtoL (NovelView.cpp:270-299); combine_lazy_novel_views renders the
    left/right eye chunks of the pair (NovelView.cpp:226-268)."""

    def __init__(self, ctx, flow_alg_name):
        self.ctx, self.flow_alg_name = ctx, flow_alg_name
        self.image_l = self.image_r = self.flow_l_to_r = self.flow_r_to_l = None

    def prepare(self, color_image_l, color_image_r, prev_flow_l_to_r=None, prev_flow_r_to_l=None,
                prev_color_image_l=None, prev_color_image_r=None):
        alg = make_optical_flow_by_name(self.ctx, self.flow_alg_name)
        self.image_l, self.image_r = _u8(color_image_l).copy(), _u8(color_image_r).copy()
        self.flow_l_to_r = alg.compute_optical_flow(self.image_l, self.image_r, prev_flow_l_to_r, prev_color_image_l,
                                                    prev_color_image_r, "LEFT")
        self.flow_r_to_l = alg.compute_optical_flow(self.image_r, self.image_l, prev_flow_r_to_l, prev_color_image_r,
                                                    prev_color_image_l, "RIGHT")

    def get_flow_l_to_r(self):
        return self.flow_l_to_r

    def get_flow_r_to_l(self):
        return self.flow_r_to_l

    def combine_lazy_novel_views(self):
        return self.ctx.combine_lazy_novel_views(self.image_l, self.image_r, self.flow_l_to_r, self.flow_r_to_l)


class StereoPanoramaRenderer:
    """renderStereoPanorama for one rig + flag set; frames are uploaded, rendered and downloaded explicitly."""

    def __init__(self, rig_json_file, device=0, **flags):
        self.rig = RigDescription(rig_json_file)
        self.params = make_params(**flags)
        if self.params.eqr_width % self.rig.get_side_camera_count() != 0:
            raise VrCamException(_capi.ERR_INVALID_ARG,
                                 "eqr_width must be evenly divisible by the number of cameras")
        self.ctx = Context(self.rig, self.params, device)

    def render(self, side_images, top_image=None, bottom_image=None, use_prev=False):
        self.ctx.upload_frame(side_images, top_image, bottom_image)
        self.ctx.render(use_prev)
        return self.ctx.download_equirect()


def png_decodable(file):
    """s360_png_decodable (host only): (w, h, channels, band_rows) if `file` (bytes) is a banded PNG the device decoder takes, else
    None."""
    b = np.frombuffer(bytes(file), np.uint8) if not isinstance(file, np.ndarray) else file
    whc = (C.c_int * 3)()
    rows = C.c_int(0)
    if lib().s360_png_decodable(b.ctypes.data if b.size else None, C.c_size_t(b.size), whc, C.byref(rows)) != 0:
        return None
    return whc[0], whc[1], whc[2], rows.value


def input_jpeg_decodable(file):
    """s360_input_jpeg_decodable (host only): (w, h, 3, luma h sampling, luma v sampling, scan bytes) if `file` (bytes) is a baseline
    JPEG the device decoder takes, else None."""
    b = np.frombuffer(bytes(file), np.uint8)
    info = (C.c_int * 6)()
    if lib().s360_input_jpeg_decodable(b.ctypes.data if b.size else None, C.c_size_t(b.size), info) != 0:
        return None
    return tuple(int(v) for v in info)


def input_png_decodable(file):
    """s360_input_png_decodable (host only): (w, h, channels, bits per sample, band_rows) if `file` (bytes) is a banded PNG the
    camera-image decoder takes (what png_decodable takes, or 16-bit RGB), else None."""
    b = np.frombuffer(bytes(file), np.uint8) if not isinstance(file, np.ndarray) else file
    info = (C.c_int * 5)()
    if lib().s360_input_png_decodable(b.ctypes.data if b.size else None, C.c_size_t(b.size), info) != 0:
        return None
    return tuple(info)
