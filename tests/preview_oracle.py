"""A numpy restatement of the reference's hyper preview (SR/test/TestHyperPreview.cpp:77-185 and what it calls in
SR/util/CvUtil.cpp:312-360, SR/render/ImageWarper.cpp:179-196, SR/render/Camera.cpp:273-289), the yardstick of
tests/test_cpu_preview.py and tests/test_gpu_preview.py. TEST INFRASTRUCTURE ONLY.

Built from what oracle/liboracle.so already exports — orc_camera_sees, orc_camera_pixel, orc_remap_cubic_f32 — plus float32
numpy arithmetic (IEEE: +, -, *, /, sqrt round as the reference's SSE2 build does) and the HOST'S libm through ctypes for
sinf, cosf, expf and powf (numpy's float32 transcendentals are not glibc's). It needs no reference checkout: the recorded
outputs of the reference's own functions (tests/golden/preview_golden.npz, written by tests/golden/make_preview_golden.py,
which also asserts that this file gives the same bits) pin it."""
import ctypes as C
import ctypes.util

import numpy as np

import oracle_lib as O

F = np.float32
_libm = None


def libm():
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for n in ("sinf", "cosf", "expf"):
            getattr(_libm, n).restype = C.c_float
            getattr(_libm, n).argtypes = [C.c_float]
        _libm.powf.restype = C.c_float
        _libm.powf.argtypes = [C.c_float, C.c_float]
    return _libm


def _map1(fn, a):
    """fn (a libm float function of one argument) over a float32 array, once per distinct bit pattern."""
    a = np.ascontiguousarray(a, F)
    bits, inv = np.unique(a.view(np.uint32).reshape(-1), return_inverse=True)
    vals = np.array([fn(float(v)) for v in bits.view(F)], F)
    return vals[inv].reshape(a.shape)


def sinf(a):
    return _map1(libm().sinf, a)


def cosf(a):
    return _map1(libm().cosf, a)


def expf(a):
    return _map1(libm().expf, a)


def powf(a, e):
    e = float(F(e))
    return _map1(lambda v: libm().powf(v, e), a)


# ---- cameras -------------------------------------------------------------------------------------------------------
def rescaled_camera_json(j, scale=0.5):
    """Camera::createRescaledCamera (Camera.cpp:273-289) on a camera's JSON object: int() of the scaled resolution, FLOAT scale
    factors applied to the double principal point and focal length."""
    scale = float(F(scale))
    res = [float(v) for v in j["resolution"]]
    new = [float(int(res[0] * scale)), float(int(res[1] * scale))]
    sx, sy = float(F(new[0] / res[0])), float(F(new[1] / res[1]))
    pr = j.get("principal", [res[0] / 2, res[1] / 2])
    out = dict(j)
    out["resolution"] = new
    out["principal"] = [float(pr[0]) * sx, float(pr[1]) * sy]
    out["focal"] = [float(j["focal"][0]) * sx, float(j["focal"][1]) * sy]
    return out


def angles(W, H):
    """theta per column, phi per row (TestHyperPreview.cpp:121-122): `2.0f * M_PI * (1.0 - (x + 0.5f) / float(W))` — the
    quotient is float, the rest double — and `M_PI * (y + 0.5f) / float(H)`, double throughout; each rounded to float once."""
    x = np.arange(W, dtype=F)
    q = (x + F(0.5)) / F(W)
    theta = (2.0 * np.pi * (1.0 - q.astype(np.float64))).astype(F)
    y = np.arange(H, dtype=F)
    phi = (np.pi * (y + F(0.5)).astype(np.float64) / float(F(H))).astype(F)
    return theta, phi


def directions(W, H):
    """projectEquirectToCam's sphericalDir per pixel, float products (ImageWarper.cpp:185-188): H x W x 3 float32."""
    theta, phi = angles(W, H)
    ct, st, sp, cp = cosf(theta), sinf(theta), sinf(phi), cosf(phi)
    d = np.empty((H, W, 3), F)
    d[..., 0] = sp[:, None] * ct[None, :]
    d[..., 1] = sp[:, None] * st[None, :]
    d[..., 2] = np.broadcast_to(cp[:, None], (H, W))
    return d


def world_points(W, H):
    """depth * sphericalDir with depth = float(Camera::kNearInfinity) = 1e6, in double."""
    return 1000000.0 * directions(W, H).astype(np.float64)


def warp_map(cam_json, W, H, with_pixels=False):
    """precomputeProjectionWarp (TestHyperPreview.cpp:117-129) of an (already rescaled) camera: H x W x 2 float32, the pixel where
    the camera sees the point and (-1, -1) elsewhere. with_pixels: also the double pixels of every point and the sees() mask."""
    cam = O.camera_from_json(cam_json)
    L = O.lib()
    pts = np.ascontiguousarray(world_points(W, H).reshape(-1, 3))
    pix = np.empty((W * H, 2), np.float64)
    seen = np.empty(W * H, bool)
    p3, p2 = (C.c_double * 3)(), (C.c_double * 2)()
    for i in range(W * H):
        p3[0], p3[1], p3[2] = pts[i]
        seen[i] = bool(L.orc_camera_sees(C.byref(cam), p3))
        L.orc_camera_pixel(C.byref(cam), p3, p2)
        pix[i] = p2[0], p2[1]
    m = np.where(seen[:, None], pix, -1.0).astype(F).reshape(H, W, 2)
    if with_pixels:
        return m, pix.reshape(H, W, 2), seen.reshape(H, W)
    return m


# ---- frames --------------------------------------------------------------------------------------------------------
def unpack(frame, bits, w, h):
    """The .bin container's packed bytes -> 16-bit samples, the value replicated to 16 bits (TestHyperPreview.cpp:374-397)."""
    b = np.ascontiguousarray(frame, np.uint8).reshape(-1).astype(np.uint32)
    if bits == 8:
        return (b[:w * h] * 0x101).astype(np.uint16).reshape(h, w)
    t = b[:h * (3 * w // 2)].reshape(h, w // 2, 3)
    even = t[..., 0] << 4 | (t[..., 1] & 0xF)
    odd = t[..., 2] << 4 | t[..., 1] >> 4
    u = np.stack([even, odd], axis=-1).reshape(h, w)
    return ((u << 4 | u >> 8) & 0xFFFF).astype(np.uint16)


def simple_demosaic(raw16, gamma=1.0):
    """simpleDemosaic (TestHyperPreview.cpp:163-184): (h / 2) x (w / 2) x 3 float32, B,G,R. kMaxValue16 and kMaxValue32 there are
    `2^16-1` and `2^32-1`, C++ XOR expressions: 13 and 29."""
    k16, k32 = F(2 ^ 16 - 1), F(2 ^ 32 - 1)
    assert (k16, k32) == (13, 29)
    h, w = raw16.shape
    hh, hw = h // 2, w // 2
    r = raw16[:2 * hh, :2 * hw].astype(F)
    g1 = r[0::2, 0::2] / k16
    g2 = r[1::2, 1::2] / k16
    b = r[0::2, 1::2] / k16
    rr = r[1::2, 0::2] / k16
    g = (g1 + g2) / F(2.0)
    rr, g, b = powf(rr, gamma), powf(g, gamma), powf(b, gamma)
    return np.stack([b * k32, g * k32, rr * k32], axis=-1)


def top_down_alpha_fade(img):
    """topDownAlphaFade (CvUtil.cpp:326-334), in place on an H x W x 4 float32 image."""
    rows = img.shape[0]
    img[..., 3] *= (np.arange(rows, dtype=F) / F(rows))[:, None]
    return img


def radial_alpha_fade(img):
    """radialAlphaFade (CvUtil.cpp:312-324), in place."""
    rows, cols = img.shape[:2]
    dx = np.arange(cols, dtype=F) - F(cols) / F(2.0)
    dy = np.arange(rows, dtype=F) - F(rows) / F(2.0)
    r = np.sqrt(dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None]) / F(F(min(rows, cols)) / F(2.0))
    img[..., 3] *= np.maximum(F(0.0), F(1.0) - r)
    return img


def develop(frame, bits, w, h, layer, gamma=1.0):
    """One layer as render() prepares it (TestHyperPreview.cpp:146-153): demosaic, alpha 1, the fades. (h / 2) x (w / 2) x 4."""
    bgr = simple_demosaic(unpack(frame, bits, w, h), gamma)
    img = np.concatenate([bgr, np.ones(bgr.shape[:2] + (1,), F)], axis=-1)
    if layer > 0:
        top_down_alpha_fade(img)
    return radial_alpha_fade(img)


def remap(layer_img, mp):
    """cv::remap INTER_CUBIC, BORDER_CONSTANT(0) of a 32FC4 image (projectToEquirect, :131-141)."""
    return O.remap_cubic_f32(np.ascontiguousarray(layer_img, F), np.ascontiguousarray(mp, F))


def flatten_layers_alpha_softmax(layers, softmax_coef=30.0):
    """flattenLayersAlphaSoftmax (CvUtil.cpp:336-360): H x W x 3 float32; Vec3f / float multiplies by 1.f / sumAlpha, so a pixel
    whose layers all have alpha 0 is 0 * inf = NaN."""
    coef = F(softmax_coef)
    sum_alpha = np.zeros(layers[0].shape[:2], F)
    sum_color = np.zeros(layers[0].shape[:2] + (3,), F)
    with np.errstate(all="ignore"):
        for img in layers:
            a = expf(coef * img[..., 3]) - F(1.0)
            sum_color = sum_color + a[..., None] * img[..., :3]
            sum_alpha = sum_alpha + a
        return sum_color * (F(1.0) / sum_alpha)[..., None]


K_NORM_16_TO_8 = F(255.0) / F(65535.0)


def to_u8(flat):
    """`eqrImage * kNorm16to8` (a float multiply) and imwrite's conversion of a float image: saturate_cast<uchar> = cvRound
    (round half to even; INT_MIN for NaN and for what does not fit an int) clamped to 0..255."""
    with np.errstate(all="ignore"):
        v = flat * K_NORM_16_TO_8
        ok = (v >= F(-2147483648.0)) & (v < F(2147483648.0))
        r = np.where(ok, np.rint(np.where(ok, v, F(0))).astype(np.int64), -2147483648)
    return np.clip(r, 0, 255).astype(np.uint8)


def compose(developed, maps, softmax_coef=30.0):
    """(remapped layers, B,G,R bytes) of three developed layers through three maps."""
    rem = [remap(d, m) for d, m in zip(developed, maps)]
    return rem, to_u8(flatten_layers_alpha_softmax(rem, softmax_coef))


class Renderer:
    """PreviewRenderer: three rescaled cameras' maps, raw images that persist between frames (zeros at first)."""

    def __init__(self, cams_json, raw_w, raw_h, eqr_w, eqr_h, gamma=1.0, softmax_coef=30.0, maps=None):
        """cams_json: the top, bottom and secondary bottom camera's JSON objects, NOT yet rescaled."""
        self.w, self.h, self.gamma, self.coef = raw_w, raw_h, gamma, softmax_coef
        self.cams = [rescaled_camera_json(j, 0.5) for j in cams_json]
        self.maps = maps if maps is not None else [warp_map(c, eqr_w, eqr_h) for c in self.cams]
        zero = np.zeros(raw_w * raw_h, np.uint8)
        self.developed = [develop(zero, 8, raw_w, raw_h, l, gamma) for l in range(3)]

    def render(self, top, bottom, bottom2, bits):
        for l, f in enumerate((top, bottom, bottom2)):
            if f is not None:
                self.developed[l] = develop(f, bits, self.w, self.h, l, self.gamma)
        return compose(self.developed, self.maps, self.coef)[1]
